"""CPU: bf_lcmv_design_device without a device -- filtersum.design_slots (the host statement of the call, and the oracle of
tests/test_lcmv_design.py) against design_lcmv, the restatement with intermediates the GPU tests use (tests/lcmv_np.py) against
design_slots, every refusal that sits before device bring-up (fake pointers, as tests/test_filter_sum_host.py), and the binding."""
import ctypes as C

import numpy as np
import pytest

import filtersum_np as fsn
import lcmv_np
import util
from support import FAKE, grid_tau as tau


SCENE = [fsn.LOOK, fsn.INTERFERER, fsn.NEAR, (5, 3)]


# ------------------------------------------------------------------ design_slots

def test_all_slots_valid_is_the_cross_null_design(native, tau):
    """cross_null's own arguments to design_lcmv (it needs a device to build its listener; tests/test_lcmv_design.py compares with
    cross_null itself): with every slot a source the slots are the compacted beams."""
    import filtersum
    M = 64
    dirs = [fsn.flat(c) for c in SCENE]
    offsets = np.array(dirs, dtype=np.int32) * M
    taps, kept, status = filtersum.design_slots(tau, offsets, M, n_taps=65, band=fsn.BAND, fs=fsn.FS)
    nulls = [[d for j, d in enumerate(dirs) if j != i] for i in range(4)]
    want, want_kept = filtersum.design_lcmv(tau, dirs, nulls, n_taps=65, band=fsn.BAND, fs=fsn.FS)
    K = filtersum.band_bins(65, fsn.BAND, fsn.FS).size
    assert taps.dtype == np.float32 and taps.shape == (4, M, 65) and kept.dtype == np.int32 and kept.shape == (4, K, 4) and status.dtype == np.int32
    assert np.array_equal(util.bits(taps), util.bits(want)) and (status == 0).all()
    for i in range(4):
        others = [j for j in range(4) if j != i]
        assert np.array_equal(kept[i][:, others], want_kept[i].astype(np.int32))        # column j of kept is SLOT j, not position j of the list
        assert (kept[i, :, i] == 0).all()
    # NEAR and LOOK cannot be told apart at the two lowest in-band bins: each is dropped as the other's null there, and for the two other
    # beams LOOK (the earlier slot) is kept and NEAR dropped against it.  76 of the 84 decisions are kept
    off_diagonal = [(i, j) for i in range(4) for j in range(4) if i != j]
    assert {(i, j) for i, j in off_diagonal if not kept[i, :, j].all()} == {(0, 2), (2, 0), (1, 2), (3, 2)}
    for i, j in ((0, 2), (2, 0), (1, 2), (3, 2)):
        assert kept[i, :, j].tolist() == [0, 0, 1, 1, 1, 1, 1]
    assert kept.sum() == 76


def test_slots_that_are_no_source(native, tau):
    import filtersum
    M, D = 64, tau.shape[0]
    look, null = fsn.flat(fsn.LOOK), fsn.flat(fsn.INTERFERER)
    assert filtersum.slot_directions([look * M, -1, null * M + 7, D * M, (D - 1) * M, 0], M, D) == [look, -1, -1, -1, D - 1, 0]
    # -1, a non-multiple and a direction past the table: silent beams that are nobody's null, and the other slots keep THEIR index
    offsets = np.array([-1, look * M, null * M + 7, D * M, null * M], dtype=np.int32)
    taps, kept, status = filtersum.design_slots(tau, offsets, M, n_taps=33, band=fsn.BAND, fs=fsn.FS)
    want, want_kept = filtersum.design_lcmv(tau, [look, null], [[null], [look]], n_taps=33, band=fsn.BAND, fs=fsn.FS)
    assert status.tolist() == [1, 0, 1, 1, 0]
    assert np.array_equal(util.bits(taps[[1, 4]]), util.bits(want)) and not taps[[0, 2, 3]].any()
    assert want_kept.all() and (kept[1, :, 4] == 1).all() and (kept[4, :, 1] == 1).all() and kept.sum() == 2 * kept.shape[1]
    # no source at all: every beam silent, nothing designed
    taps, kept, status = filtersum.design_slots(tau, [-1, 3], M, n_taps=33, band=fsn.BAND, fs=fsn.FS)
    assert not taps.any() and not kept.any() and status.tolist() == [1, 1] and taps.shape == (2, M, 33)
    with pytest.raises(ValueError):
        filtersum.design_slots(tau, [], M)
    with pytest.raises(ValueError):
        filtersum.design_slots(tau, [0], 0)
    with pytest.raises(ValueError):
        filtersum.design_slots(tau[:, :3], [0, 3, 6, 9], 3)          # more slots than microphones: the device call refuses it too
    with pytest.raises(ValueError):
        filtersum.design_slots(tau, [0], M, rho=0.0)
    with pytest.raises(ValueError):
        filtersum.design_slots(tau, [0], M, n_taps=9, band=(100.0, 200.0), fs=fsn.FS)


def test_a_duplicated_direction_is_dropped_as_a_null_everywhere(native, tau):
    """Two slots on one direction: coherence 1 > rho, so each is dropped as the other's null, and a third beam keeps the first of
    them (slot order) and drops the second against it.  Both still get their beam: the same taps."""
    import filtersum
    M = 64
    look, null = fsn.flat(fsn.LOOK), fsn.flat(fsn.INTERFERER)
    taps, kept, status = filtersum.design_slots(tau, np.array([look, null, look]) * M, M, n_taps=33, band=fsn.BAND, fs=fsn.FS)
    assert (status == 0).all()
    assert not kept[0, :, 2].any() and not kept[2, :, 0].any()
    assert kept[1, :, 0].all() and not kept[1, :, 2].any()
    assert kept[0, :, 1].all() and kept[2, :, 1].all()
    assert np.array_equal(util.bits(taps[0]), util.bits(taps[2]))
    want, _ = filtersum.design_lcmv(tau, [look, null], [[null], [look]], n_taps=33, band=fsn.BAND, fs=fsn.FS)
    assert np.array_equal(util.bits(taps[:2]), util.bits(want))


@pytest.mark.parametrize("n,S,T,band,rho,seed", lcmv_np.TABLE)
def test_the_restatement_with_intermediates_is_design_slots(native, n, S, T, band, rho, seed):
    """What the GPU test compares the device's gains with is tests/lcmv_np.slot_gains; here it is tied to design_slots: the same kept
    entries and status, and its gains through irfft are design_slots' taps bit for bit."""
    import filtersum
    tau_r = lcmv_np.table_tau(n, S, T, seed)
    step = lcmv_np.offset_per_dir(n)
    for name, row in lcmv_np.offset_rows(n, S, T, seed):
        taps, kept, status = filtersum.design_slots(tau_r, row, step, n_taps=T, band=band, rho=rho, fs=lcmv_np.FS)
        r = lcmv_np.slot_gains(tau_r, row, step, T, band, rho)
        assert np.array_equal(kept, r["kept"]) and np.array_equal(status, r["status"]), name
        assert np.array_equal(util.bits(taps), util.bits(lcmv_np.taps_of(r["gains"], r["bins"], T))), name
        silent = status == 1
        assert not r["gains"][silent].any() and not kept[silent].any() and not kept[:, :, silent].any()


# ------------------------------------------------------------------ refusals before device bring-up

DIRS, N_MICS, SRC, STEP, TAPS, LO, HI = 12, 16, 4, 16, 9, 1, 3
K = HI - LO + 1
D_TAU, D_OFF, D_GAINS, D_TAPS, D_KEPT, D_STATUS = (FAKE + i * 0x100000 for i in range(6))
TAU_BYTES, OFF_BYTES = DIRS * N_MICS * 8, SRC * 4
GAINS_BYTES, TAPS_BYTES, KEPT_BYTES, STATUS_BYTES = SRC * K * N_MICS * 16, SRC * N_MICS * TAPS * 4, SRC * K * SRC * 4, SRC * 4
W = "bf_lcmv_design_device: "


def _call(native, d_tau=D_TAU, dirs=DIRS, n=N_MICS, d_offsets=D_OFF, sources=SRC, offset_per_dir=STEP, n_taps=TAPS, bin_lo=LO, bin_hi=HI, rho=0.95,
          d_gains=D_GAINS, d_taps=D_TAPS, d_kept=D_KEPT, d_status=D_STATUS):
    return native.lib.bf_lcmv_design_device(d_tau, dirs, n, d_offsets, sources, offset_per_dir, n_taps, bin_lo, bin_hi, rho, d_gains, d_taps, d_kept, d_status, None)


@pytest.mark.parametrize("kw,text", [
    (dict(d_tau=None), "d_tau is null"),
    (dict(d_offsets=None), "d_offsets is null"),
    (dict(d_gains=None), "d_gains is null"),
    (dict(d_taps=None), "d_taps is null"),
    (dict(d_kept=None), "d_kept is null"),
    (dict(d_status=None), "d_status is null"),
    (dict(d_tau=None, d_status=None, n=0), "d_tau is null"),
    (dict(dirs=0), "dirs = 0 < 1"),
    (dict(n=0), "n = 0 < 1"),
    (dict(n=-2, sources=0), "n = -2 < 1"),
    (dict(sources=0), "sources = 0 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(n_taps=0), "n_taps = 0 < 1"),
    (dict(sources=9), "sources = 9 > 8"),
    (dict(sources=9, n=4), "sources = 9 > 8"),
    (dict(sources=4, n=3), "sources = 4 > n = 3 (more constraints than microphones make the system singular)"),
    (dict(sources=2, n=1), "sources = 2 > n = 1 (more constraints than microphones make the system singular)"),
    (dict(n_taps=1025, bin_hi=3), "n_taps = 1025 > 1024"),
    (dict(bin_lo=-1), "bins [-1, 3] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 4"),
    (dict(bin_lo=3, bin_hi=2), "bins [3, 2] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 4"),
    (dict(bin_hi=5), "bins [1, 5] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 4"),
    (dict(n_taps=1, bin_lo=0, bin_hi=1), "bins [0, 1] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 0"),
    (dict(rho=0.0), "rho = 0 is not in (0, 1]"),
    (dict(rho=-0.5), "rho = -0.5 is not in (0, 1]"),
    (dict(rho=1.5), "rho = 1.5 is not in (0, 1]"),
    (dict(rho=float("nan")), "rho = nan is not in (0, 1]"),
    (dict(rho=float("inf")), "rho = inf is not in (0, 1]"),
    # every output against both inputs and against the outputs behind it: the first and the last byte of a range
    (dict(d_gains=D_TAU + TAU_BYTES - 8), "d_gains overlaps d_tau"),
    (dict(d_tau=D_GAINS + GAINS_BYTES - 8), "d_gains overlaps d_tau"),
    (dict(d_offsets=D_GAINS), "d_gains overlaps d_offsets"),
    (dict(d_taps=D_GAINS + GAINS_BYTES - 4), "d_gains overlaps d_taps"),
    (dict(d_kept=D_GAINS - KEPT_BYTES + 4), "d_gains overlaps d_kept"),
    (dict(d_status=D_GAINS + 8), "d_gains overlaps d_status"),
    (dict(d_taps=D_TAU), "d_taps overlaps d_tau"),
    (dict(d_offsets=D_TAPS + TAPS_BYTES - 4), "d_taps overlaps d_offsets"),
    (dict(d_kept=D_TAPS + TAPS_BYTES - 4), "d_taps overlaps d_kept"),
    (dict(d_status=D_TAPS - STATUS_BYTES + 4), "d_taps overlaps d_status"),
    (dict(d_kept=D_TAU + TAU_BYTES - 4), "d_kept overlaps d_tau"),
    (dict(d_offsets=D_KEPT + KEPT_BYTES - 4), "d_kept overlaps d_offsets"),
    (dict(d_status=D_KEPT + KEPT_BYTES - 4), "d_kept overlaps d_status"),
    (dict(d_status=D_TAU), "d_status overlaps d_tau"),
    (dict(d_status=D_OFF), "d_status overlaps d_offsets"),
    (dict(d_offsets=D_STATUS + STATUS_BYTES - 4), "d_status overlaps d_offsets"),
])
def test_refusals(native, kw, text):
    lib = native.lib
    lib.bf_clear_error()
    assert _call(native, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(native):
    """Ranges that only touch, the largest sizes, sources == n, rho = 1, one bin at either end: all pass the argument checks, so without
    a GPU the one refusal left is the missing device (with one, fake pointers must not be launched: nothing is called)."""
    if native.gpu_available():
        return
    lib = native.lib
    for kw in (dict(), dict(d_gains=D_TAU + TAU_BYTES), dict(d_tau=D_GAINS + GAINS_BYTES), dict(d_taps=D_GAINS + GAINS_BYTES), dict(d_kept=D_GAINS - KEPT_BYTES),
               dict(d_status=D_TAPS - STATUS_BYTES), dict(d_offsets=D_STATUS + STATUS_BYTES), dict(d_offsets=D_TAU), dict(sources=8, n=8), dict(sources=1, n=1),
               dict(rho=1.0), dict(rho=1e-300), dict(bin_lo=0, bin_hi=0), dict(bin_lo=4, bin_hi=4), dict(n_taps=1024, bin_lo=0, bin_hi=512),
               dict(n_taps=1, bin_lo=0, bin_hi=0), dict(dirs=1, offset_per_dir=2 ** 31 - 1)):
        lib.bf_clear_error()
        assert _call(native, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device"), kw
    lib.bf_clear_error()


def test_the_symbol_is_exported_and_bound(native):
    fn = native.lib.bf_lcmv_design_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 15 and fn.argtypes[9] is C.c_double
    assert [i for i, t in enumerate(fn.argtypes) if t is C.c_void_p] == [0, 3, 10, 11, 12, 13, 14]
    assert all(t is C.c_int for i, t in enumerate(fn.argtypes) if i in (1, 2, 4, 5, 6, 7, 8))
    import filtersum
    header = open(native.__file__.replace("zybo-rt-sampler-image-detection_amd/lib/_native.py", "include/beamformer_hip.h")).read()
    assert "#define BF_LCMV_MAX_SOURCES %d\n" % filtersum.MAX_SLOTS in header and "#define BF_LCMV_MAX_TAPS %d\n" % filtersum.MAX_DESIGN_TAPS in header
