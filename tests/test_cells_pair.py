"""GPU (-m gpu): das_pair2_cells_kernel (csrc/das_cells.hip), the lerp pair kernel on rows of 16-byte cells, through bf_das_device:
every map compared bit for bit with the CPU oracle (oracle/das_oracle: mimo_lerp's arithmetic over a direction range), and
bf_last_das_rows() == 2 says that this kernel ran and not das_pair2_kernel.

The kernel takes microphone counts that are a multiple of 32.  What the cases are for -- each the smallest shape at which a path of
the kernel can go wrong:
  * halves2_f2: 32 microphones of 40, rows out of order, N = 256, 2 frames, 272 directions.  Two halves of 16: the fetch that follows
    the first staging already wraps to half 0; a wrong mic id shows at once.
  * halves4_f3_masked_from_5: 64 of 70, N = 252, 3 frames, directions [5, 272).  Lanes 60..63 of the fourth register load the row's
    last sample again and stage zero cells, D[251] is masked, the last workgroup row computes its frame twice, and neither the first
    direction nor the image origin is 0.
  * halves6_f3 and halves6_n132_f3: 96 of 100, N = 256 and 132, 3 frames.  Six halves (the mic id of half h + 2 is loaded a half
    ahead, five times), 96 is no power of two (the means are true divisions), and at N = 132 round 1 of the power pass is one quad
    and the third and fourth registers are all but empty.
  * tile_of_137_from_5: 32 of 40, 20 x 20 directions [5, 398), 169 frames.  With many frames a tile is two groups of 128: tiles of
    256 and 137, the second group of the second tile partial and staged from the fetch of half 0 that the first group's last half
    issued.
  * grid_17x16_f3: 64 microphones, the 17 x 16 grid's own delays (lib.directions.calculate_delays), 3 frames: a real table, whose
    delays change at many microphones at once.  Its rows of 16 directions are two runs of 8, so the sweep-order rule gains nothing
    there and keeps the identity;
  * grid_order_13x21_f3: the same on the 13 x 21 grid, whose rows of 21 directions no run of 8 divides: the digest then carries a
    sweep order (bf_sweep_order is not the identity for this grid: asserted), and the four summing waves store through it.

Drawn delays are smooth, c_m + s_m d / D in [0, 54.75] as in tests/test_pair2_staging.py (so that the sweep runs and not the
direction-outer kernel), with column 0 all 0 and column 1 all 54.75, the largest delay the 56-cell zero prefix admits.  Column 1
reads the wiped prefix at every output sample below 55.  With delays spread over 0..54 every output sample k reads cell k - p - 1
of some microphone, so all of D[63], D[127] and D[191] -- the lane-63 seams, where a difference takes lane 0 of the next register
-- are read in every case, by the microphones whose delay leaves k - p - 1 = 63, 127, 191 inside the block: column 0 reads them at
k = 64, 128, 192.

Teeth: halves2_f2 was run once against a build whose seam was deliberately wrong (lane 63 of the first three registers kept
D = s[i] - s[i] = 0 instead of taking lane 0 of the next register): both of its maps differed from the oracle.
"""
import collections

import numpy as np
import pytest

import util
from support import nat
from util import ALGOS

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "name M_total n N X Y F lo hi grid")
CASES = [
    Case("halves2_f2", 40, 32, 256, 17, 16, 2, 0, 272, False),
    Case("halves4_f3_masked_from_5", 70, 64, 252, 17, 16, 3, 5, 272, False),
    Case("halves6_f3", 100, 96, 256, 17, 16, 3, 0, 272, False),
    Case("halves6_n132_f3", 100, 96, 132, 17, 16, 3, 0, 272, False),
    Case("tile_of_137_from_5", 40, 32, 256, 20, 20, 169, 5, 398, False),
    Case("grid_17x16_f3", 64, 64, 256, 17, 16, 3, 0, 272, True),
    Case("grid_order_13x21_f3", 64, 64, 256, 13, 21, 3, 0, 273, True),
]
PMAX = 54.9


def data(c):
    """frames float32 [F, M_total, N], mics int32 [n] (descending rows), delays float32 [D, n]; a grid case takes the array's own
    delays for its grid and every microphone in order."""
    D = c.X * c.Y
    rng = np.random.default_rng(sum(map(ord, c.name)))
    frames = (rng.standard_normal((c.F, c.M_total, c.N)) * 0.25).astype(np.float32)
    if c.grid:
        from interface import config
        from lib import directions
        config.configure(N_MICROPHONES=c.M_total, ACTIVE_TILES=1, N_SAMPLES=c.N, MAX_RES_X=c.X, MAX_RES_Y=c.Y, N_TAPS=8)
        assert c.n == c.M_total
        return frames, np.arange(c.n, dtype=np.int32), np.float32(directions.calculate_delays()).reshape(D, c.n)
    mics = np.ascontiguousarray(np.sort(rng.choice(c.M_total, c.n, replace=False))[::-1]).astype(np.int32)
    span = min(D / 8.0, PMAX / 2.0)
    c_m = rng.uniform(0, PMAX - span, size=c.n)
    s_m = rng.uniform(-span, span, size=c.n)
    delays = np.maximum(c_m[None, :] + s_m[None, :] * (np.arange(D)[:, None] / D), 0.0)
    delays[:, 0] = 0.0
    delays[:, 1] = 54.75
    delays = np.float32(delays)
    assert delays.min() == 0.0 and delays.max() == 54.75
    return frames, mics, delays


def maps_and_rows(nat, oracle_lib, c, rows):
    """Runs the case; asserts family 8, the row layout `rows` and every map bit-equal to the oracle."""
    import torch
    from interface import config
    D, W = c.X * c.Y, c.hi - c.lo
    try:
        frames, mics, delays = data(c)
        if c.name.startswith("grid_order"):
            whole = np.ascontiguousarray(np.floor(delays).astype(np.int32))
            order = np.empty(W, dtype=np.int32)
            assert nat.lib.bf_sweep_order(nat.iptr(whole), D, c.n, c.lo, c.hi, 8, nat.iptr(order)) == 0, nat.check()
            assert sorted(order) == list(range(c.lo, c.hi)) and (order != np.arange(c.lo, c.hi)).any()     # the sweep order is in use
        orc = oracle_lib.Oracle(c.N, c.X, c.Y, 8)
        orc.load(ALGOS["lerp"], delays.reshape(c.X, c.Y, c.n))
        want = np.stack([orc.mimo_range(ALGOS["lerp"], frames[f], mics, c.lo, c.hi) for f in range(c.F)])

        config.configure(N_MICROPHONES=c.M_total, N_SAMPLES=c.N, MAX_RES_X=c.X, MAX_RES_Y=c.Y, N_TAPS=8)
        t = np.ascontiguousarray(delays).ravel()
        nat.lib.load_coefficients_lerp(nat.fptr(t), t.size)
        nat.check()
        d_sig = torch.from_numpy(frames).cuda()
        out = torch.full((c.F, W), float("nan"), dtype=torch.float32, device="cuda")
        assert nat.lib.bf_das_device(ALGOS["lerp"], d_sig.data_ptr(), c.M_total, out.data_ptr(), W, c.F, nat.iptr(mics), mics.size, c.lo, c.hi,
                                     torch.cuda.current_stream().cuda_stream) == 0, nat.check()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        family, layout = nat.lib.bf_last_das_variant(), nat.lib.bf_last_das_rows()
        differ = [f for f in range(c.F) if got[f].tobytes() != want[f].tobytes()]
        print("%s: family %d, rows %d, %d of %d maps differ from the oracle" % (c.name, family, layout, len(differ), c.F))
        assert family == 8 and layout == rows
        assert np.isfinite(got).all()
        assert not differ, differ[:8]
    finally:
        util.configure("cfg1")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lerp_cell_row_maps_are_the_oracles_bit_for_bit(nat, oracle_lib, case):
    maps_and_rows(nat, oracle_lib, case, 2)
