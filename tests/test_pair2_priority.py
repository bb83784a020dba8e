"""GPU (-m gpu): das_pair2_kernel (csrc/das_pair.hip) with its wave priorities, lerp through bf_das_device, every map compared bit
for bit with the CPU oracle (oracle/das_oracle: mimo_lerp's arithmetic over a direction range) -- and das_pair_kernel, which has
the ladder at the grain of its three-mic trips (3, 1, 0), on the same cases with pad (the whole-sample delays of the same tables).

A priority decides which wave of a SIMD issues next and can change no bit of any map; what can go wrong is the code around it.
The ladder (3 from a half's barrier on, 2, 1, 0 at mics 2, 4, 6, 0 again behind the half loop) restarts at every barrier, a wave
without directions keeps 3 from barrier to barrier and must still meet every barrier, and every wave enters the power pass at 0.
The cases are the smallest shapes at which those lines run differently, after the pattern of tests/test_pair2_staging.py:
  * 16 and 32 microphones (two and four halves of 8), N = 256 and N = 132, 2 and 3 frames (an odd count computes the last frame
    twice).  With few frames plan_das gives tiles of 8 directions: one sweeping wave per workgroup, fifteen that skip the sweep.
  * 48 microphones of 56: the division path of the power pass behind the same loop.
  * 171 frames, where a tile is two groups of 128: directions [3, 392) are the tiles [3, 259) and [259, 392), the second one full
    group and a group of five directions in which fifteen waves skip the sweep.
  * the tables are the array's own delays for a 20 x 20 grid (lib.directions.calculate_delays, 64 microphones, of which a case
    takes its columns), so the launch takes the sweep and not the direction-outer kernel; bf_last_das_variant() == 8 says so
    (5 for pad's pair kernel).

The pair kernel runs at 256 directions or more (plan_das: a narrower launch gets 8-wave workgroups of the one-frame kernel), so the
range [3, 136) -- one full group and one of five directions -- cannot be a launch of its own and is the second tile of [3, 392).
"""
import collections

import numpy as np
import pytest

import util
from support import nat
from util import ALGOS

pytestmark = pytest.mark.gpu

X, Y, M_ARRAY = 20, 20, 64
Case = collections.namedtuple("Case", "name M_total n N F lo hi")
CASES = [
    Case("halves2_f2", 64, 16, 256, 2, 3, 392),
    Case("halves2_n132_f3", 64, 16, 132, 3, 3, 392),
    Case("halves4_f3", 64, 32, 256, 3, 3, 392),
    Case("halves4_n132_f2", 64, 32, 132, 2, 3, 392),
    Case("mics48_of_56_f3", 56, 48, 256, 3, 3, 392),
    Case("group_of_5_f171", 64, 16, 256, 171, 3, 392),
]


@pytest.fixture(scope="module")
def array_delays(nat):
    """float32 [X * Y, 64]: the delays of the 64-microphone array for the grid, computed once and left unchanged"""
    from interface import config
    from lib import directions
    config.configure(N_MICROPHONES=M_ARRAY, ACTIVE_TILES=1, N_SAMPLES=256, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=8)
    d = np.float32(directions.calculate_delays()).reshape(X * Y, M_ARRAY)
    d.setflags(write=False)
    return d


def _data(c, array_delays):
    """frames float32 [F, M_total, N], mics int32 [n] (rows of the frames, descending), delays float32 [D, n] (their columns)"""
    rng = np.random.default_rng(sum(map(ord, c.name)))
    frames = (rng.standard_normal((c.F, c.M_total, c.N)) * 0.25).astype(np.float32)
    mics = np.ascontiguousarray(np.sort(rng.choice(c.M_total, c.n, replace=False))[::-1]).astype(np.int32)
    return frames, mics, np.ascontiguousarray(array_delays[:, mics])


FAMILY = {"lerp": 8, "pad": 5}       # bf_last_das_variant: das_pair2_kernel, das_pair_kernel


@pytest.mark.parametrize("algo", ["lerp", "pad"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_pair_maps_with_priorities_are_the_oracles_bit_for_bit(nat, oracle_lib, array_delays, case, algo):
    import torch
    from interface import config
    c = case
    try:
        W = c.hi - c.lo
        frames, mics, delays = _data(c, array_delays)
        if algo == "pad":
            delays = np.ascontiguousarray(delays.astype(int).astype(np.int32))      # the reference's truncation
        orc = oracle_lib.Oracle(c.N, X, Y, 8)
        orc.load(ALGOS[algo], delays.reshape(X, Y, c.n))
        want = np.stack([orc.mimo_range(ALGOS[algo], frames[f], mics, c.lo, c.hi) for f in range(c.F)])

        config.configure(N_MICROPHONES=c.M_total, N_SAMPLES=c.N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=8)
        t = np.ascontiguousarray(delays).ravel()
        if algo == "pad":
            nat.lib.load_coefficients_pad(nat.iptr(t), t.size)
        else:
            nat.lib.load_coefficients_lerp(nat.fptr(t), t.size)
        nat.check()
        d_sig = torch.from_numpy(frames).cuda()
        out = torch.full((c.F, W), float("nan"), dtype=torch.float32, device="cuda")
        assert nat.lib.bf_das_device(ALGOS[algo], d_sig.data_ptr(), c.M_total, out.data_ptr(), W, c.F, nat.iptr(mics), mics.size, c.lo, c.hi,
                                     torch.cuda.current_stream().cuda_stream) == 0, nat.check()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        family = nat.lib.bf_last_das_variant()
        differ = [f for f in range(c.F) if got[f].tobytes() != want[f].tobytes()]
        print("%s %s: family %d, %d of %d maps differ from the oracle" % (c.name, algo, family, len(differ), c.F))
        assert family == FAMILY[algo]
        assert np.isfinite(got).all()
        assert not differ, differ[:8]
    finally:
        util.configure("cfg1")      # (the module's fixture and cases leave the array, the grid and N configured)
