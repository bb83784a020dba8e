"""GPU (-m gpu): the k-ordered mean-power pass of das_pair2_kernel (csrc/das_pair.hip), lerp through bf_das_device, every map
compared byte for byte with the CPU oracle (oracle/das_oracle: mimo_lerp's arithmetic over a direction range).

The pass sums both frames of a workgroup at once in two rounds -- samples 0..127, then 128..N-1 -- on four waves, a lane keeping its
running sum between the rounds.  The cases are the smallest shapes at which that can go wrong:
  * N = 256 (round 1 is four trips of eight quads), 252 (124 samples: three trips and seven quads), 192 (two trips), 160 (exactly
    one trip: the drain alone), 132 (one quad).  16 microphones of 20, 272 directions, 2 and 3 frames: with few frames plan_das
    gives tiles of 8 directions -- one busy wave, fifteen that park zeros, a workgroup whose summing waves mask all but 8 lanes --
    and with 3 the last workgroup row computes its frame twice and must store it once.
  * 48 microphones of 56 (not a power of two: the means are true divisions) at N = 256 and 252, 3 frames.
  * many frames, where a tile is two groups of 128: 377 directions x 174 frames (tiles of 256 and 121) and directions [5, 398) x 169
    frames (tiles of 256 and 137: the second group is partial, dir_begin and the image origin are not 0, the frame count is odd).
  * a rectangular grid's own delays (64 microphones, 17 x 16, lib.directions.calculate_delays): the digest then carries a sweep
    order, and the four summing waves store through it.

That the comparison has teeth is shown on the CPU first: for one case, the float32 sum of the oracle's squared block taken as
(sum of k < 128) + (sum of k >= 128) differs in bits from the k-ordered sum for at least one direction -- a pass that added two
partial sums instead of carrying one would not pass.
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
    Case("n256_f2", 20, 16, 256, 17, 16, 2, 0, 272, False),
    Case("n256_f3", 20, 16, 256, 17, 16, 3, 0, 272, False),
    Case("n252_f2", 20, 16, 252, 17, 16, 2, 0, 272, False),
    Case("n252_f3", 20, 16, 252, 17, 16, 3, 0, 272, False),
    Case("n192_f2", 20, 16, 192, 17, 16, 2, 0, 272, False),
    Case("n192_f3", 20, 16, 192, 17, 16, 3, 0, 272, False),
    Case("n160_f2", 20, 16, 160, 17, 16, 2, 0, 272, False),
    Case("n160_f3", 20, 16, 160, 17, 16, 3, 0, 272, False),
    Case("n132_f2", 20, 16, 132, 17, 16, 2, 0, 272, False),
    Case("n132_f3", 20, 16, 132, 17, 16, 3, 0, 272, False),
    Case("mics48_n256_f3", 56, 48, 256, 17, 16, 3, 0, 272, False),
    Case("mics48_n252_f3", 56, 48, 252, 17, 16, 3, 0, 272, False),
    Case("tile_of_121", 20, 16, 256, 29, 13, 174, 0, 377, False),
    Case("tile_of_137_from_5", 40, 32, 256, 20, 20, 169, 5, 398, False),
    Case("grid_order_f3", 64, 64, 256, 17, 16, 3, 0, 272, True),
]
TEETH = "n256_f2"
PMAX = 54.9


def _data(c):
    """frames float32 [F, M_total, N], mics int32 [n] (descending rows), delays float32 [D, n].  Drawn delays are smooth as
    tests/batched_cases.py draws them (c_m + s_m d / D, so that the sweep kernel runs and not the direction-outer one); a grid case
    takes the array's own delays for its grid and every microphone in order."""
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
    delays = np.float32(np.maximum(c_m[None, :] + s_m[None, :] * (np.arange(D)[:, None] / D), 0.0))
    return frames, mics, delays


def _split_sum_differs(orc, c, frames, mics, delays, want0):
    """Directions of frame 0 (of the first 64) whose float32 power differs in bits between the k-ordered sum and the sum of the two
    halves' sums.  The k-ordered restatement must be the oracle's own value, or it shows nothing."""
    differ = []
    for d in range(c.lo, min(c.hi, c.lo + 64)):
        block = orc.miso_lerp(frames[0], delays.reshape(c.X, c.Y, c.n), mics, d * c.n)
        o = block / np.float32(c.n)
        sq = (o * o).astype(np.float32)
        ordered = np.cumsum(sq, dtype=np.float32)[-1]                     # (cumsum adds front to back, one float32 rounding per sample)
        assert (ordered / np.float32(c.N)).tobytes() == want0[d - c.lo].tobytes(), d
        halves = np.float32(np.cumsum(sq[:128], dtype=np.float32)[-1] + np.cumsum(sq[128:], dtype=np.float32)[-1])
        if halves.tobytes() != ordered.tobytes():
            differ.append(d)
    return differ


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lerp_pair_power_pass_maps_are_the_oracles_byte_for_byte(nat, oracle_lib, case):
    import torch
    from interface import config
    c = case
    D, W = c.X * c.Y, c.hi - c.lo
    try:
        frames, mics, delays = _data(c)
        orc = oracle_lib.Oracle(c.N, c.X, c.Y, 8)
        orc.load(ALGOS["lerp"], delays.reshape(c.X, c.Y, c.n))
        want = np.stack([orc.mimo_range(ALGOS["lerp"], frames[f], mics, c.lo, c.hi) for f in range(c.F)])
        if c.name == TEETH:
            differ = _split_sum_differs(orc, c, frames, mics, delays, want[0])
            print("%s: the sum of two half sums differs from the k-ordered sum in %d of 64 directions" % (c.name, len(differ)))
            assert differ
            orc.load(ALGOS["lerp"], delays.reshape(c.X, c.Y, c.n))

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
        family = nat.lib.bf_last_das_variant()
        differ = [f for f in range(c.F) if got[f].tobytes() != want[f].tobytes()]
        print("%s: family %d, %d of %d maps differ from the oracle" % (c.name, family, len(differ), c.F))
        assert family == 8
        assert np.isfinite(got).all()
        assert not differ, differ[:8]
    finally:
        util.configure("cfg1")
