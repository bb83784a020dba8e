"""GPU (-m gpu): the staging and table addressing of das_pair2_kernel (csrc/das_pair.hip), lerp through bf_das_device, every map
compared bit for bit with the CPU oracle (oracle/das_oracle: mimo_lerp's arithmetic over a direction range).

What the cases are for -- each the smallest shape at which a path of the kernel's staging can go wrong:
  * 16 / 32 / 64 microphones: 2, 4 and 8 halves of 8.  With two halves the fetch that follows the first staging already wraps to
    half 0; with more, the mic id of half h + 2 is loaded a half ahead.
  * N = 256 (every lane loads its own quad) and N = 252 (lane 63 loads the row's last quad again and stages zeros).
  * 2 and 3 frames: with 3, the last workgroup row computes its frame twice.
  * m_total > n with the rows out of order: a wrong mic id shows at once.
  * delays from 0 (column 0) to 54.75 (column 1), the largest the fixed 56-sample prefix admits: 54.75 reads the wiped prefix at
    every output sample below 55.

The pair kernel needs 16 waves, hence 256 directions or more in a launch.  plan_das gives a launch with few frames tiles of 8
directions -- one busy wave, one group per workgroup -- so the group loop is reached by two launches of many frames, where a tile is
two groups of 128:
  * 377 directions: tiles of 256 and 121 (121: one partial group);
  * directions [5, 398): tiles of 256 and 137 (137: two groups, the second partial, staged from the fetch of half 0 that the first
    group's last but one half issued), with an odd frame count.
"""
import collections

import numpy as np
import pytest

from support import nat
from util import ALGOS

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "name M_total n N X Y F lo hi")
CASES = [
    Case("halves2_f2", 20, 16, 256, 17, 16, 2, 0, 272),
    Case("halves2_f3_masked", 20, 16, 252, 17, 16, 3, 0, 272),
    Case("halves4_f3_masked", 40, 32, 252, 17, 16, 3, 0, 272),
    Case("halves4_f2", 40, 32, 256, 17, 16, 2, 3, 270),
    Case("halves8_f3", 70, 64, 256, 17, 16, 3, 5, 272),
    Case("halves8_f2_masked", 64, 64, 252, 17, 16, 2, 0, 272),
    Case("tile_of_121", 20, 16, 256, 29, 13, 174, 0, 377),
    Case("tile_of_137_from_5", 40, 32, 256, 20, 20, 169, 5, 398),
]
PMAX = 54.9


def _data(c):
    """frames float32 [F, M_total, N], mics int32 [n] (descending rows), delays float32 [D, n]: smooth as tests/batched_cases.py
    draws them (c_m + s_m d / D, so that the sweep kernel runs and not the direction-outer one), column 0 all 0, column 1 all 54.75."""
    D = c.X * c.Y
    rng = np.random.default_rng(sum(map(ord, c.name)))
    frames = (rng.standard_normal((c.F, c.M_total, c.N)) * 0.25).astype(np.float32)
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


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lerp_pair_maps_are_the_oracles_bit_for_bit(nat, oracle_lib, case):
    import torch
    from interface import config
    c = case
    D, W = c.X * c.Y, c.hi - c.lo
    frames, mics, delays = _data(c)
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
    family = nat.lib.bf_last_das_variant()
    differ = [f for f in range(c.F) if got[f].tobytes() != want[f].tobytes()]
    print("%s: family %d, %d of %d maps differ from the oracle" % (c.name, family, len(differ), c.F))
    assert family == 8
    assert np.isfinite(got).all()
    assert not differ, differ[:8]
