"""GPU (-m gpu): bf_das_device on frame batches that reach every kernel family plan_das routes to (tests/batched_cases.py), with
what the one-frame tests never combine: several frames, more frame rows than active microphones (m_total > n, rows out of order in
one case per family), a direction shard [3, D - 2) and an image stride wider than the shard.

Every kernel derives its frame from the workgroup id: the signals of frame f start at f * m_total * N and its image row at
f * image_stride.  So every case asserts
  * the family that ran (bf_last_das_variant) -- the case then means what its comment says,
  * every frame against the CPU oracle within REL_TOL and then bit for bit, frame by frame (a wrong frame base shows as frame f != 0
    failing; a wrong order of the microphones or of the power sum shows only in the bits),
  * the padding columns of every image row and one spare row still NaN (nothing written outside [f * stride, f * stride + hi - lo)),
  * frame F - 1 bit-identical to the host-pointer one-frame call where that call ran the same family (only the frame walk differs),
  * the shard bit-identical to the same columns of a full-range call with image_stride = D.
test_hostile_frames_match_the_oracle then puts seven frames through the same cases that a kernel can get wrong while every N(0, 0.25)
frame passes (BC.hostile: subnormal maps, NaN that only some directions read, overflow, signed zeros, NaN wherever the oracle never reads).
The digest cache (four slots per table, least recently used evicted) then sees six direction ranges and returns to the first two."""
import ctypes as C

import numpy as np
import pytest

import batched_cases as BC
import sweep_order_np as SO
import util
from support import nat
from test_gpu_parity import run_product
from util import ALGOS, REL_TOL, max_rel

pytestmark = pytest.mark.gpu

PAD_COLS = 5


def _configure(c):
    from interface import config
    config.configure(N_MICROPHONES=c.M_total, N_SAMPLES=c.N, MAX_RES_X=c.X, MAX_RES_Y=c.Y, N_TAPS=c.T)


def _das(nat, c, algo, d_sig, mics, lo, hi, stride=None, spare_rows=0):
    """bf_das_device on the frames of d_sig over directions [lo, hi) -> float32 [frames + spare_rows, stride], NaN where nothing was written."""
    torch = util.torch_gpu()
    F = d_sig.shape[0]
    stride = hi - lo if stride is None else stride
    out = torch.full((F + spare_rows, stride), float("nan"), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_device(ALGOS[algo], d_sig.data_ptr(), c.M_total, out.data_ptr(), stride, F, nat.iptr(mics), mics.size, lo, hi,
                                 torch.cuda.current_stream().cuda_stream) == 0, nat.check()
    torch.cuda.synchronize()
    return out.cpu().numpy()


# (case, algo) of BC.PARAMS whose maps are not the oracle's bit for bit, each with its cause, the number of differing entries and the
# largest distance in float32 steps as measured.  Empty: all 56 are held to bits, on plain frames and on the hostile ones.  An entry
# has to bring its own bound with it: the kernel's distance from a float64 evaluation of the same sum at most twice the oracle's own,
# both measured and written beside the entry.
NOT_BIT_IDENTICAL = {}


def _same_bits(got, want, what):
    """The oracle is the definition: same microphone order, same operation order, same k-ordered power sum -- the same bits."""
    assert not NOT_BIT_IDENTICAL, "no exception is implemented: see the comment at NOT_BIT_IDENTICAL"
    why = util.bits_differ(got, want)
    assert not why, "%s: %s" % (what, why)


@pytest.mark.parametrize("case,algo", BC.PARAMS)
def test_batch_reaches_its_family_and_matches_the_oracle(nat, oracle_lib, case, algo):
    torch = util.torch_gpu()
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
    family, layout = nat.lib.bf_last_das_variant(), nat.lib.bf_last_das_rows()
    err = [max_rel(got[f, :W], want[f, lo:hi]) if np.isfinite(got[f, :W]).all() else float("nan") for f in range(F)]
    print("%s %s: family %d rows %d (one frame: %d), max rel err per frame %s" % (case, algo, family, layout, one_family, " ".join("%.3g" % e for e in err)))

    # 3. the family the case is written for, and for lerp's pair sweep the kernel: rows of sample pairs (1) or of cells (2)
    assert family == BC.family_of(c, algo)
    assert layout == BC.rows_of(c, algo)
    # 4. every frame against the oracle
    for f in range(F):
        assert np.isfinite(got[f, :W]).all(), f
        assert err[f] <= REL_TOL, f
        _same_bits(got[f, :W], want[f, lo:hi], "%s %s family %d, frame %d of the shard" % (case, algo, family, f))
    # 5. nothing outside the frames' own columns
    assert np.isnan(got[:F, W:]).all()
    assert np.isnan(got[F]).all()
    # 6. the one-frame call, where it ran the same family
    assert max_rel(one[:D], want[F - 1]) <= REL_TOL
    _same_bits(one[:D], want[F - 1], "%s %s family %d, the one-frame call" % (case, algo, one_family))
    if one_family == family:
        assert got[F - 1, :W].tobytes() == one[lo:hi].tobytes()
    # 7. the full range, image rows back to back
    full = _das(nat, c, algo, d_sig, mics, 0, D)
    assert nat.lib.bf_last_das_rows() == layout
    assert full[:, lo:hi].tobytes() == got[:F, :W].tobytes()
    for f in range(F):
        assert max_rel(full[f], want[f]) <= REL_TOL, f
        _same_bits(full[f], want[f], "%s %s family %d, frame %d of the full range" % (case, algo, family, f))


GUARD = 64      # NaN floats in front of and behind the hostile batch on the device


def _hostile_frame_matches(got, want, what):
    """NaN where and only where the oracle's map is NaN; every other entry -- +inf and subnormals included -- equal in bits."""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if not np.array_equal(nan_g, nan_w):
        d = int(np.flatnonzero(nan_g != nan_w)[0])
        return ["%s: NaN in %d entries, the oracle in %d; first at flat direction %d: got %r, want %r"
                % (what, nan_g.sum(), nan_w.sum(), d, float(got[d]), float(want[d]))]
    why = util.bits_differ(got, want, nan_is_nan=True)
    return ["%s: %s" % (what, why)] if why else []


@pytest.mark.parametrize("case,algo", BC.PARAMS)
def test_hostile_frames_match_the_oracle(nat, oracle_lib, case, algo):
    """The seven frames of BC.hostile -- subnormal maps, one NaN that half of the directions read, partners that are loud, saturated
    or signed zeros, NaN in every sample and row the oracle never reads -- inside a NaN-filled allocation: the batched call over the
    shard and over the full range and the host-pointer one-frame call give the oracle's NaNs and the oracle's bits, frame by frame."""
    torch = util.torch_gpu()
    c, d = BC.BY_NAME[case], BC.data(case)
    h = BC.hostile(case, algo)
    D, F = c.X * c.Y, BC.HOSTILE_FRAMES
    lo, hi = BC.shard(c)
    W = hi - lo
    mics = d.mics.copy()
    _configure(c)

    # the one-frame calls first (they load the table): the frame trimmed to the rows the call copies
    rows = int(mics.max()) + 1
    ones = [run_product(nat, algo, BC.table(case, algo), np.ascontiguousarray(h.frames[f, :rows]), mics) for f in range(F)]
    one_family = nat.lib.bf_last_das_variant()

    buf = torch.full((GUARD + h.frames.size + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    d_sig = buf[GUARD:GUARD + h.frames.size].view(F, c.M_total, c.N)
    d_sig.copy_(torch.from_numpy(h.frames.copy()))
    got = _das(nat, c, algo, d_sig, mics, lo, hi, stride=W + PAD_COLS, spare_rows=1)
    family, layout = nat.lib.bf_last_das_variant(), nat.lib.bf_last_das_rows()
    full = _das(nat, c, algo, d_sig, mics, 0, D, stride=D)
    assert (nat.lib.bf_last_das_variant(), nat.lib.bf_last_das_rows()) == (family, layout)
    print("%s %s: family %d rows %d (one frame: %d), quiet * 2^%d, loud * 2^%d, NaN at %s, %d samples poisoned"
          % (case, algo, family, layout, one_family, h.info["e_quiet"], h.info["e_loud"], h.info["bad"], h.info["poisoned"]))

    assert family == BC.family_of(c, algo)
    assert layout == BC.rows_of(c, algo)
    wrong = []                                                  # every frame is compared before any fails: the kinds tell the cause apart
    for f, kind in enumerate(BC.KINDS):
        what = "%s %s, frame %d (%s)" % (case, algo, f, kind)
        wrong += _hostile_frame_matches(got[f, :W], h.want[f, lo:hi], what + ", shard, family %d" % family)
        wrong += _hostile_frame_matches(full[f], h.want[f], what + ", full range, family %d" % family)
        wrong += _hostile_frame_matches(ones[f][:D], h.want[f], what + ", one-frame call, family %d" % one_family)
    assert not wrong, "\n".join(wrong)
    assert np.isnan(got[:F, W:]).all()
    assert np.isnan(got[F]).all()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()


def _reloads(nat):
    """(return code, changes, steps) of bf_last_das_reloads; a launch that counted nothing reports (-1, -1, 0) and an error text."""
    ch, st = C.c_longlong(-2), C.c_longlong(-2)
    rc = nat.lib.bf_last_das_reloads(C.byref(ch), C.byref(st))
    nat.lib.bf_clear_error()
    return rc, ch.value, st.value


@pytest.mark.parametrize("algo,case", [("pad", BC.EVICT_PLAIN), ("lerp", BC.EVICT_PLAIN), ("hybrid", BC.EVICT_FIR), ("lerp", BC.EVICT_CELLS)],
                         ids=["pad", "lerp", "hybrid", "lerp_cells"])
def test_digest_cache_eviction(nat, oracle_lib, algo, case):
    """Six direction ranges through the four digest slots of one table, then the first two again (both evicted by then) and a
    one-frame call: every result is the matching slice of the full maps bit for bit, and a rebuilt digest counts the re-reads it
    counted the first time.  lerp_cells: the pair launches run on cell rows, whose summing waves store through the digest's sweep order."""
    torch = util.torch_gpu()
    c, d = BC.BY_NAME[case], BC.data(case)
    D, F = c.X * c.Y, c.F
    want = BC.want(oracle_lib, case, algo)
    mics = d.mics.copy()
    _configure(c)
    run_product(nat, algo, BC.table(case, algo), d.frames[0], mics)         # loads the table (and takes a slot for its one-frame geometry)
    d_sig = torch.from_numpy(d.frames.copy()).cuda()
    pair, layout = {"pad": 5, "lerp": 8, "hybrid": 7}[algo], BC.rows_of(c, algo)

    full = _das(nat, c, algo, d_sig, mics, 0, D)
    assert (nat.lib.bf_last_das_variant(), nat.lib.bf_last_das_rows()) == (pair, layout)
    for f in range(F):
        assert max_rel(full[f], want[f]) <= REL_TOL, f

    shards = [(0, D), (0, 130), (130, D), (5, D - 3), (64, 200), (1, 9)]
    seen = {}
    for lo, hi in shards + shards[:2]:
        part = _das(nat, c, algo, d_sig, mics, lo, hi)
        fam, counted = nat.lib.bf_last_das_variant(), _reloads(nat)
        assert nat.lib.bf_last_das_rows() == (layout if fam == pair else 0), (lo, hi)
        print("%s %s [%d, %d): family %d rows %d, re-reads (rc, changes, steps) %s" % (case, algo, lo, hi, fam, nat.lib.bf_last_das_rows(), counted))
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
