"""GPU (-m gpu): bf_das_device on frame batches that reach every kernel family plan_das routes to (tests/batched_cases.py), with
what the one-frame tests never combine: several frames, more frame rows than active microphones (m_total > n, rows out of order in
one case per family), a direction shard [3, D - 2) and an image stride wider than the shard.

Every kernel derives its frame from the workgroup id: the signals of frame f start at f * m_total * N and its image row at
f * image_stride.  So every case asserts
  * the family that ran (bf_last_das_variant) -- the case then means what its comment says,
  * every frame against the CPU oracle within REL_TOL, frame by frame (a wrong frame base shows as frame f != 0 failing),
  * the padding columns of every image row and one spare row still NaN (nothing written outside [f * stride, f * stride + hi - lo)),
  * frame F - 1 bit-identical to the host-pointer one-frame call where that call ran the same family (only the frame walk differs),
  * the shard bit-identical to the same columns of a full-range call with image_stride = D.
The digest cache (four slots per table, least recently used evicted) then sees six direction ranges and returns to the first two."""
import ctypes as C

import numpy as np
import pytest

import batched_cases as BC
import sweep_order_np as SO
from test_gpu_parity import run_product
from util import ALGOS, REL_TOL, max_rel

pytestmark = pytest.mark.gpu

PAD_COLS = 5


@pytest.fixture(scope="module")
def nat(native):
    assert native.gpu_available(), "these tests need the MI355X"
    return native


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _configure(c):
    from interface import config
    config.configure(N_MICROPHONES=c.M_total, N_SAMPLES=c.N, MAX_RES_X=c.X, MAX_RES_Y=c.Y, N_TAPS=c.T)


def _das(nat, c, algo, d_sig, mics, lo, hi, stride=None, spare_rows=0):
    """bf_das_device on the frames of d_sig over directions [lo, hi) -> float32 [frames + spare_rows, stride], NaN where nothing was written."""
    torch = _torch()
    F = d_sig.shape[0]
    stride = hi - lo if stride is None else stride
    out = torch.full((F + spare_rows, stride), float("nan"), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_device(ALGOS[algo], d_sig.data_ptr(), c.M_total, out.data_ptr(), stride, F, nat.iptr(mics), mics.size, lo, hi,
                                 torch.cuda.current_stream().cuda_stream) == 0, nat.check()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case,algo", BC.PARAMS)
def test_batch_reaches_its_family_and_matches_the_oracle(nat, oracle_lib, case, algo):
    torch = _torch()
    c, d = BC.BY_NAME[case], BC.data(case)
    D, F = c.X * c.Y, c.F
    lo, hi = BC.shard(c)
    W = hi - lo
    want = BC.want(oracle_lib, case, algo)
    mics = d.mics.copy()
    _configure(c)

    # 1. load the table; frame F - 1 through the host-pointer call (its frame has max(mics) + 1 rows, its image D columns)
    one = run_product(nat, algo, BC.table(case, algo), d.frames[F - 1], mics)
    one_family = nat.lib.bf_last_das_variant()

    # 2. the batch: a direction shard into image rows 5 columns wider than it, one spare row behind the last frame
    d_sig = torch.from_numpy(d.frames.copy()).cuda()
    got = _das(nat, c, algo, d_sig, mics, lo, hi, stride=W + PAD_COLS, spare_rows=1)
    family = nat.lib.bf_last_das_variant()
    err = [max_rel(got[f, :W], want[f, lo:hi]) if np.isfinite(got[f, :W]).all() else float("nan") for f in range(F)]
    print("%s %s: family %d (one frame: %d), max rel err per frame %s" % (case, algo, family, one_family, " ".join("%.3g" % e for e in err)))

    # 3. the family the case is written for
    assert family == BC.family_of(c, algo)
    # 4. every frame against the oracle
    for f in range(F):
        assert np.isfinite(got[f, :W]).all(), f
        assert err[f] <= REL_TOL, f
    # 5. nothing outside the frames' own columns
    assert np.isnan(got[:F, W:]).all()
    assert np.isnan(got[F]).all()
    # 6. the one-frame call, where it ran the same family
    assert max_rel(one[:D], want[F - 1]) <= REL_TOL
    if one_family == family:
        assert got[F - 1, :W].tobytes() == one[lo:hi].tobytes()
    # 7. the full range, image rows back to back
    full = _das(nat, c, algo, d_sig, mics, 0, D)
    assert full[:, lo:hi].tobytes() == got[:F, :W].tobytes()
    for f in range(F):
        assert max_rel(full[f], want[f]) <= REL_TOL, f


def _reloads(nat):
    """(return code, changes, steps) of bf_last_das_reloads; a launch that counted nothing reports (-1, -1, 0) and an error text."""
    ch, st = C.c_longlong(-2), C.c_longlong(-2)
    rc = nat.lib.bf_last_das_reloads(C.byref(ch), C.byref(st))
    nat.lib.bf_clear_error()
    return rc, ch.value, st.value


@pytest.mark.parametrize("algo", ["pad", "lerp", "hybrid"])
def test_digest_cache_eviction(nat, oracle_lib, algo):
    """Six direction ranges through the four digest slots of one table, then the first two again (both evicted by then) and a
    one-frame call: every result is the matching slice of the full maps bit for bit, and a rebuilt digest counts the re-reads it
    counted the first time."""
    torch = _torch()
    case = BC.EVICT_PLAIN if algo in BC.PLAIN else BC.EVICT_FIR
    c, d = BC.BY_NAME[case], BC.data(case)
    D, F = c.X * c.Y, c.F
    want = BC.want(oracle_lib, case, algo)
    mics = d.mics.copy()
    _configure(c)
    run_product(nat, algo, BC.table(case, algo), d.frames[0], mics)         # loads the table (and takes a slot for its one-frame geometry)
    d_sig = torch.from_numpy(d.frames.copy()).cuda()
    pair = {"pad": 5, "lerp": 8, "hybrid": 7}[algo]

    full = _das(nat, c, algo, d_sig, mics, 0, D)
    assert nat.lib.bf_last_das_variant() == pair
    for f in range(F):
        assert max_rel(full[f], want[f]) <= REL_TOL, f

    shards = [(0, D), (0, 130), (130, D), (5, D - 3), (64, 200), (1, 9)]
    seen = {}
    for lo, hi in shards + shards[:2]:
        part = _das(nat, c, algo, d_sig, mics, lo, hi)
        fam, counted = nat.lib.bf_last_das_variant(), _reloads(nat)
        print("%s [%d, %d): family %d, re-reads (rc, changes, steps) %s" % (algo, lo, hi, fam, counted))
        assert part.tobytes() == np.ascontiguousarray(full[:, lo:hi]).tobytes(), (lo, hi)
        if (lo, hi) in seen:
            assert (fam, counted) == seen[(lo, hi)], (lo, hi)               # the rebuilt digest is the one built first
        seen[(lo, hi)] = (fam, counted)
    if algo in BC.PLAIN:
        # Shards under 256 directions take the 8-wave sweep (2), which counts no re-reads: bf_last_das_reloads reports (-1, -1, 0) for
        # them both times.  The 16-wave pair launches do count -- what NumPy counts in the order the launch sweeps.
        w = BC.whole(case, algo)
        for lo, hi in ((0, D), (5, D - 3)):
            order, info = SO.sweep_order(w, lo, hi)
            assert seen[(lo, hi)] == (pair, (0, info["changes"], -(-(hi - lo) // SO.DPW) * (SO.DPW - 1) * c.n)), (lo, hi)
        for lo, hi in ((0, 130), (130, D), (64, 200), (1, 9)):
            assert seen[(lo, hi)] == (2, (-1, -1, 0)), (lo, hi)
    one = _das(nat, c, algo, d_sig[:1], mics, 0, D)
    assert nat.lib.bf_last_das_variant() == {"pad": 2, "lerp": 2, "hybrid": 4}[algo]
    assert one.tobytes() == full[:1].tobytes()
