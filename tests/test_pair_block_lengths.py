"""GPU (-m gpu): the rows of tests/pair_cases.py through bf_das_device -- the four two-frame kernels at all 32 block lengths they take
(the lerp kernels' power-pass drains by every exit, with and without a trip of the loop before it; the staging masks at every length),
the neighbouring lengths at which the route leaves them, a table whose sweep order is not the identity, and the microphone counts at which a kernel takes the ids of the halves or
chunks beyond the 64th from memory, or wraps to half 0 somewhere else.

Every row: the family (bf_last_das_variant) and the row layout (bf_last_das_rows) written beside it; every frame's map equal to the
CPU oracle's bit for bit, over the shard [3, D - 2) and over the full range; the shard written into image rows 5 columns wider than it
with a spare row, the frames inside a NaN-guarded allocation: the padding, the spare row and the guards are NaN afterwards.

Teeth: the lerp length rows were run once against a build whose add_in_order_linear missed exit 4 (BF_L_DONE(4) never taken, so round 1
summed on to its eighth quad).  The five cell rows that leave by exit 4 failed -- N = 144, 176, 208, 240 with three frames and 144 with
two, all 272 directions of every map -- and the other 87 passed: none of the lengths the suite had before (132, 200, 252, 256) takes
that exit."""
import numpy as np
import pytest

import batched_cases as BC
import pair_cases as PC
import util
from support import nat
from util import ALGOS

pytestmark = pytest.mark.gpu

PAD_COLS = 5
GUARD = 64      # NaN floats in front of and behind the frames on the device

_LOADERS = {"pad": ("load_coefficients_pad", "iptr"), "lerp": ("load_coefficients_lerp", "fptr"), "hybrid": ("load_coefficients_convolve_hybrid", "fptr"),
            "fir_naive": ("load_coefficients_convolve", "fptr"), "fir_vec": ("load_coefficients_convolve", "fptr")}


def _das(nat, c, algo, d_sig, mics, lo, hi, stride, spare_rows):
    torch = util.torch_gpu()
    F = d_sig.shape[0]
    out = torch.full((F + spare_rows, stride), float("nan"), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_device(ALGOS[algo], d_sig.data_ptr(), c.M_total, out.data_ptr(), stride, F, nat.iptr(mics), mics.size, lo, hi,
                                 torch.cuda.current_stream().cuda_stream) == 0, nat.check()
    torch.cuda.synchronize()
    return out.cpu().numpy(), nat.lib.bf_last_das_variant(), nat.lib.bf_last_das_rows()


def _row_matches(nat, oracle_lib, row):
    torch = util.torch_gpu()
    from interface import config
    c, d = PC.BY_NAME[row.case], BC.data(row.case)
    algo = row.algo
    D, F = c.X * c.Y, c.F
    lo, hi = BC.shard(c)
    W = hi - lo
    want = BC.want(oracle_lib, row.case, algo)
    mics = d.mics.copy()
    try:
        config.configure(N_MICROPHONES=c.M_total, N_SAMPLES=c.N, MAX_RES_X=c.X, MAX_RES_Y=c.Y, N_TAPS=c.T)
        loader, ptr = _LOADERS[algo]
        t = np.ascontiguousarray(BC.table(row.case, algo)).ravel()
        getattr(nat.lib, loader)(getattr(nat, ptr)(t), t.size)
        nat.check()

        buf = torch.full((GUARD + d.frames.size + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        d_sig = buf[GUARD:GUARD + d.frames.size].view(F, c.M_total, c.N)
        d_sig.copy_(torch.from_numpy(d.frames.copy()))
        full, family, rows = _das(nat, c, algo, d_sig, mics, 0, D, D, 0)
        got, family_s, rows_s = _das(nat, c, algo, d_sig, mics, lo, hi, W + PAD_COLS, 1)
        differ = [util.bits_differ(full[f], want[f]) for f in range(F)] + [util.bits_differ(got[f, :W], want[f, lo:hi]) for f in range(F)]
        print("%s %s (N %d, %d of %d microphones, %d frames): family %d rows %d (shard: %d, %d), %d of %d maps differ from the oracle"
              % (row.case, algo, c.N, c.n, c.M_total, F, family, rows, family_s, rows_s, sum(1 for w in differ if w), 2 * F))

        assert (family, rows) == (row.family, row.rows) == (family_s, rows_s)
        for f in range(F):
            assert not differ[f], "%s %s family %d rows %d, frame %d of the full range: %s" % (row.case, algo, family, rows, f, differ[f])
            assert not differ[F + f], "%s %s family %d rows %d, frame %d of the shard: %s" % (row.case, algo, family, rows, f, differ[F + f])
        assert np.isfinite(full).all() and np.isfinite(got[:F, :W]).all()
        assert np.isnan(got[:F, W:]).all()
        assert np.isnan(got[F]).all()
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()
    finally:
        util.configure("cfg1")


@pytest.mark.parametrize("row", PC.BLOCK_LENGTHS, ids=["%s-%s" % (r.case, r.algo) for r in PC.BLOCK_LENGTHS])
def test_block_length_row_matches_the_oracle(nat, oracle_lib, row):
    _row_matches(nat, oracle_lib, row)


@pytest.mark.parametrize("row", PC.MANY_MICS, ids=["%s-%s" % (r.case, r.algo) for r in PC.MANY_MICS])
def test_microphone_count_row_matches_the_oracle(nat, oracle_lib, row):
    _row_matches(nat, oracle_lib, row)
