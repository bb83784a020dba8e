"""CPU: bf_mvdr_design_device without a device -- filtersum.design_mvdr / design_mvdr_slots (the host statements of the call, and the
oracle of tests/test_mvdr_design.py), the restatement with intermediates the GPU tests use (tests/mvdr_np.py) against them, what the
design does on the scene with an interferer no slot names, every refusal that sits before device bring-up (fake pointers, as
tests/test_lcmv_design_host.py), and the binding."""
import ctypes as C

import numpy as np
import pytest

import filtersum_np as fsn
import lcmv_np
import mvdr_np
import util
from support import FAKE, scene_tau as tau, sized


# ------------------------------------------------------------------ the host design

@pytest.mark.parametrize("case", mvdr_np.TABLE, ids=mvdr_np.case_id)
def test_the_restatement_with_intermediates_is_design_mvdr_slots(native, case):
    """What the GPU test compares the device's stages with is tests/mvdr_np.slot_stages; here it is tied to design_mvdr_slots: the same
    fallback and status, and its gains through irfft are design_mvdr_slots' taps bit for bit.  Its stages hang together: the loaded
    matrix is L L^H, cond(R') <= n / loading + 1 <= 1e4, the case's rows are the ones its comment promises."""
    import filtersum
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window = case
    frames, mics, tau_r, win = mvdr_np.case_inputs(case)
    assert frames.shape == (F, m_total, N) and len(set(mics.tolist())) == n and seg_first + (segs - 1) * seg_hop + T <= N
    if (n, m_total) == (3, 5):
        assert mics.tolist() != sorted(mics.tolist())
    step = lcmv_np.offset_per_dir(n)
    for name, row in lcmv_np.offset_rows(n, S, T, 0):
        taps, fallback, status = filtersum.design_mvdr_slots(frames, mics, tau_r, row, step, n_taps=T, band=band, loading=loading, seg_first=seg_first,
                                                             seg_hop=seg_hop, segs=segs, window=win, fs=mvdr_np.FS)
        r = mvdr_np.slot_stages(frames, mics, tau_r, row, step, T, band, loading, seg_first, seg_hop, segs, win)
        assert np.array_equal(fallback, r["fallback"]) and not fallback.any() and np.array_equal(status, r["status"]), name
        assert taps.dtype == np.float32 and taps.shape == (S, n, T) and np.array_equal(util.bits(taps), util.bits(r["taps"])), name
        assert not taps[status == 1].any() and not r["gains"][status == 1].any() and all(taps[i].any() for i in np.flatnonzero(status == 0))
        assert r["conds"].max() <= n / loading + 1.0 + 1e-6 and r["conds"].max() <= 1e4
        L = r["chol"]
        err = np.abs(L @ L.conj().transpose(0, 2, 1) - r["loaded"])
        scale = np.sqrt(np.einsum("kaa,kbb->kab", r["loaded"].real, r["loaded"].real))
        assert (err <= 1e-12 * scale).all() and not np.triu(L, 1).any()
    look, _ = filtersum.design_mvdr(frames, mics, tau_r, [int(row[0]) // step for _, row in lcmv_np.offset_rows(n, S, T, 0)[:1]], n_taps=T, band=band,
                                    loading=loading, seg_first=seg_first, seg_hop=seg_hop, segs=segs, window=win, fs=mvdr_np.FS)
    first = filtersum.design_mvdr_slots(frames, mics, tau_r, lcmv_np.offset_rows(n, S, T, 0)[0][1], step, n_taps=T, band=band, loading=loading,
                                        seg_first=seg_first, seg_hop=seg_hop, segs=segs, window=win, fs=mvdr_np.FS)[0]
    assert np.array_equal(util.bits(look[0]), util.bits(first[0]))            # design_mvdr is the same design without the slot semantics


def test_silence_and_a_huge_loading_give_the_beam_without_nulls(native, tau):
    """Silent frames: every bin falls back, the taps are design_lcmv(nulls=None)'s to 2^-23 of the largest.  loading = 1e9 drowns the
    covariance: the same taps to 1e-6 of the largest."""
    import filtersum
    M, T = 64, 65
    look = [fsn.flat(fsn.LOOK), fsn.flat(fsn.NEAR)]
    want, _ = filtersum.design_lcmv(tau, look, None, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    K = filtersum.band_bins(T, fsn.BAND, fsn.FS).size
    silent = np.zeros((2, M, 256), dtype=np.float32)
    taps, fallback = filtersum.design_mvdr(silent, np.arange(M), tau, look, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    assert fallback.dtype == np.int32 and fallback.tolist() == [1] * K
    for b in range(2):
        assert (np.abs(taps[b].astype(np.float64) - want[b]) <= 2.0 ** -23 * np.abs(want[b]).max()).all()
    noisy = np.random.default_rng(5).standard_normal((2, M, 256)).astype(np.float32)
    taps, fallback = filtersum.design_mvdr(noisy, np.arange(M), tau, look, n_taps=T, band=fsn.BAND, loading=1e9, fs=fsn.FS)
    assert not fallback.any()
    for b in range(2):
        assert (np.abs(taps[b].astype(np.float64) - want[b]) <= 1e-6 * np.abs(want[b]).max()).all()
    bad = noisy.copy()
    bad[1, 7, 100] = np.nan                                           # one NaN sample: every bin's trace is NaN
    taps, fallback = filtersum.design_mvdr(bad, np.arange(M), tau, look, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    assert fallback.all() and np.isfinite(taps).all()
    for kw in (dict(loading=0.0), dict(loading=float("nan")), dict(seg_hop=0), dict(seg_first=-1), dict(segs=13), dict(n_taps=257), dict(window=np.ones(3)),
               dict(band=(100.0, 200.0))):
        with pytest.raises(ValueError):
            filtersum.design_mvdr(noisy, np.arange(M), tau, look, fs=fsn.FS, **kw)
    with pytest.raises(ValueError):
        filtersum.design_mvdr(noisy, np.arange(M), tau, [], fs=fsn.FS)
    with pytest.raises(ValueError):
        filtersum.design_mvdr(noisy, np.arange(M), tau, [tau.shape[0]], fs=fsn.FS)
    with pytest.raises(ValueError):
        filtersum.design_mvdr(noisy.astype(np.float64), np.arange(M), tau, look, fs=fsn.FS)
    with pytest.raises(ValueError):
        filtersum.design_mvdr(noisy, [0, 64], tau[:, :2], look, fs=fsn.FS)


def test_the_scene_an_interferer_no_slot_names(native, tau):
    """The scene of tests/mvdr_np.py, whole windows (design_mvdr's defaults): 8 x 8 microphones, look (20, 11), interferer (28, 14),
    sensor noise 0.05 RMS, 14 windows of 256 at hop 128, 65 taps, a segment every 16 samples, rectangular window, loading 0.1.
    Learned from interferer + noise the design passes the interferer at least 20 dB below delay-and-sum (the project's threshold in
    test_graph_retarget_then_listen; 26.0 dB measured), holds the look response to what float32 taps allow, and the three rows of the
    README's table are printed."""
    import filtersum
    M, T = mvdr_np.M, mvdr_np.T
    look = fsn.flat(fsn.LOOK)
    sc = mvdr_np.scene(tau)
    das, _ = filtersum.design_lcmv(tau, [look], None, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    lcmv, _ = filtersum.design_lcmv(tau, [look], [[fsn.flat(fsn.INTERFERER)]], n_taps=T, band=fsn.BAND, fs=fsn.FS)
    print("delay-and-sum (no slot for the interferer): interferer %.1f dB, white-noise gain %.1f dB, look %+.2f dB" % mvdr_np.row(sc, das[0]))
    print("design_lcmv, the interferer's direction GIVEN: interferer %.1f dB, white-noise gain %.1f dB, look %+.2f dB" % mvdr_np.row(sc, lcmv[0]))
    rows = []
    for name, train in mvdr_np.trainings(sc):
        frames, _ = mvdr_np.cut(train)
        taps, fallback = filtersum.design_mvdr(frames, np.arange(M), tau, [look], n_taps=T, band=fsn.BAND, loading=mvdr_np.LOADING, seg_hop=mvdr_np.SEG_HOP, fs=fsn.FS)
        assert not fallback.any()
        rows.append(mvdr_np.row(sc, taps[0]))
        print("design_mvdr, covariance from %s: interferer %.1f dB, white-noise gain %.1f dB, look %+.2f dB" % ((name,) + rows[-1]))
        bins = filtersum.band_bins(T, fsn.BAND, fsn.FS)
        w = 2.0 * np.pi * bins / T
        e = np.abs(filtersum.response(taps[0], tau[look], w) - np.exp(-1j * w * (T - 1) / 2.0))
        assert (e <= M * T * 2.0 ** -24 * float(np.abs(taps[0]).max())).all(), (name, float(e.max()))
    leak_das = mvdr_np.row(sc, das[0])[0]
    print("interferer + noise: %.1f dB below delay-and-sum" % (leak_das - rows[0][0]))
    assert leak_das - rows[0][0] >= 20.0
    assert abs(rows[0][2]) < 0.1                                       # and the look talker, absent from the covariance, passes unharmed


# ------------------------------------------------------------------ refusals before device bring-up

M_TOTAL, FRAMES, N_MICS, FIRST, SHOP, SEGS, DIRS, SRC, STEP, TAPS, LO, HI = 20, 3, 16, 4, 8, 5, 12, 4, 16, 9, 1, 3
K, P = HI - LO + 1, FRAMES * SEGS
D_SIG, D_WIN, D_TAU, D_OFF, D_SNAP, D_COV, D_CHOL, D_GAINS, D_TAPS, D_STATUS, D_FALL = (FAKE + i * 0x1000000 for i in range(11))
SIG_BYTES, WIN_BYTES, TAU_BYTES, OFF_BYTES = FRAMES * M_TOTAL * 256 * 4, TAPS * 8, DIRS * N_MICS * 8, SRC * 4
SNAP_BYTES, COV_BYTES, GAINS_BYTES, TAPS_BYTES, STATUS_BYTES, FALL_BYTES = P * K * N_MICS * 16, K * N_MICS * N_MICS * 16, SRC * K * N_MICS * 16, SRC * N_MICS * TAPS * 4, SRC * 4, K * 4
MICS = np.arange(N_MICS, dtype=np.int32)
W = "bf_mvdr_design_device: "


def _call(native, d_signals=D_SIG, m_total=M_TOTAL, frames=FRAMES, mics=MICS, n=N_MICS, seg_first=FIRST, seg_hop=SHOP, segs=SEGS, d_window=D_WIN, d_tau=D_TAU,
          dirs=DIRS, d_offsets=D_OFF, sources=SRC, offset_per_dir=STEP, n_taps=TAPS, bin_lo=LO, bin_hi=HI, loading=0.1, d_snap=D_SNAP, d_cov=D_COV, d_chol=D_CHOL,
          d_gains=D_GAINS, d_taps=D_TAPS, d_status=D_STATUS, d_fallback=D_FALL):
    return native.lib.bf_mvdr_design_device(d_signals, m_total, frames, None if mics is None else native.iptr(mics), n, seg_first, seg_hop, segs, d_window, d_tau,
                                            dirs, d_offsets, sources, offset_per_dir, n_taps, bin_lo, bin_hi, loading, d_snap, d_cov, d_chol, d_gains, d_taps,
                                            d_status, d_fallback, None)


BAD_ROW = MICS.copy()
BAD_ROW[5] = M_TOTAL
NEG_ROW = MICS.copy()
NEG_ROW[0] = -1


@pytest.mark.parametrize("kw,text", [
    (dict(d_signals=None), "d_signals is null"),
    (dict(mics=None), "adaptive_array is null"),
    (dict(d_tau=None), "d_tau is null"),
    (dict(d_offsets=None), "d_offsets is null"),
    (dict(d_snap=None), "d_snap is null"),
    (dict(d_cov=None), "d_cov is null"),
    (dict(d_chol=None), "d_chol is null"),
    (dict(d_gains=None), "d_gains is null"),
    (dict(d_taps=None), "d_taps is null"),
    (dict(d_status=None), "d_status is null"),
    (dict(d_fallback=None), "d_fallback is null"),
    (dict(d_signals=None, d_fallback=None, n=0), "d_signals is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(n=0), "n = 0 < 1"),
    (dict(segs=0), "segs = 0 < 1"),
    (dict(seg_hop=0), "seg_hop = 0 < 1"),
    (dict(dirs=0), "dirs = 0 < 1"),
    (dict(sources=0), "sources = 0 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(n_taps=0), "n_taps = 0 < 1"),
    (dict(seg_first=-1), "seg_first = -1 < 0"),
    (dict(seg_first=216), "seg_first + (segs - 1) * seg_hop + n_taps = 257 > N_SAMPLES = 256 (a segment would leave its window)"),
    (dict(segs=32), "seg_first + (segs - 1) * seg_hop + n_taps = 261 > N_SAMPLES = 256 (a segment would leave its window)"),
    (dict(seg_hop=2 ** 31 - 1, segs=2 ** 31 - 1), "seg_first + (segs - 1) * seg_hop + n_taps = 4611686011984936975 > N_SAMPLES = 256 (a segment would leave its window)"),
    (dict(n=257), "n = 257 > 256"),
    (dict(sources=9), "sources = 9 > 8"),
    (dict(n_taps=1025), "n_taps = 1025 > 1024"),                      # (before the segments: N_SAMPLES never exceeds 1024, it could not be told otherwise)
    (dict(bin_lo=-1), "bins [-1, 3] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 4"),
    (dict(bin_lo=3, bin_hi=2), "bins [3, 2] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 4"),
    (dict(bin_hi=5), "bins [1, 5] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 4"),
    (dict(loading=0.0), "loading = 0 is not finite and > 0"),
    (dict(loading=-0.5), "loading = -0.5 is not finite and > 0"),
    (dict(loading=float("nan")), "loading = nan is not finite and > 0"),
    (dict(loading=float("inf")), "loading = inf is not finite and > 0"),
    (dict(mics=BAD_ROW), "adaptive_array[5] = 20 is not a row of frames with m_total = 20 rows"),
    (dict(mics=NEG_ROW), "adaptive_array[0] = -1 is not a row of frames with m_total = 20 rows"),
    # every output against the outputs behind it and the four inputs: the first or the last byte of a range
    (dict(d_cov=D_SNAP + SNAP_BYTES - 8), "d_snap overlaps d_cov"),
    (dict(d_chol=D_SNAP), "d_snap overlaps d_chol"),
    (dict(d_gains=D_SNAP - GAINS_BYTES + 8), "d_snap overlaps d_gains"),
    (dict(d_taps=D_SNAP + 16), "d_snap overlaps d_taps"),
    (dict(d_status=D_SNAP + SNAP_BYTES - 4), "d_snap overlaps d_status"),
    (dict(d_fallback=D_SNAP), "d_snap overlaps d_fallback"),
    (dict(d_signals=D_SNAP + SNAP_BYTES - 4), "d_snap overlaps d_signals"),
    (dict(d_tau=D_SNAP), "d_snap overlaps d_tau"),
    (dict(d_offsets=D_SNAP), "d_snap overlaps d_offsets"),
    (dict(d_window=D_SNAP - WIN_BYTES + 8), "d_snap overlaps d_window"),
    (dict(d_chol=D_COV + COV_BYTES - 8), "d_cov overlaps d_chol"),
    (dict(d_gains=D_COV), "d_cov overlaps d_gains"),
    (dict(d_taps=D_COV), "d_cov overlaps d_taps"),
    (dict(d_status=D_COV), "d_cov overlaps d_status"),
    (dict(d_fallback=D_COV + COV_BYTES - 4), "d_cov overlaps d_fallback"),
    (dict(d_signals=D_COV - SIG_BYTES + 4), "d_cov overlaps d_signals"),
    (dict(d_tau=D_COV + COV_BYTES - 8), "d_cov overlaps d_tau"),
    (dict(d_offsets=D_COV), "d_cov overlaps d_offsets"),
    (dict(d_window=D_COV), "d_cov overlaps d_window"),
    (dict(d_gains=D_CHOL + COV_BYTES - 8), "d_chol overlaps d_gains"),
    (dict(d_taps=D_CHOL), "d_chol overlaps d_taps"),
    (dict(d_status=D_CHOL), "d_chol overlaps d_status"),
    (dict(d_fallback=D_CHOL), "d_chol overlaps d_fallback"),
    (dict(d_signals=D_CHOL), "d_chol overlaps d_signals"),
    (dict(d_tau=D_CHOL), "d_chol overlaps d_tau"),
    (dict(d_offsets=D_CHOL + COV_BYTES - 4), "d_chol overlaps d_offsets"),
    (dict(d_window=D_CHOL), "d_chol overlaps d_window"),
    (dict(d_taps=D_GAINS + GAINS_BYTES - 4), "d_gains overlaps d_taps"),
    (dict(d_status=D_GAINS), "d_gains overlaps d_status"),
    (dict(d_fallback=D_GAINS), "d_gains overlaps d_fallback"),
    (dict(d_signals=D_GAINS), "d_gains overlaps d_signals"),
    (dict(d_tau=D_GAINS - TAU_BYTES + 8), "d_gains overlaps d_tau"),
    (dict(d_offsets=D_GAINS), "d_gains overlaps d_offsets"),
    (dict(d_window=D_GAINS), "d_gains overlaps d_window"),
    (dict(d_status=D_TAPS + TAPS_BYTES - 4), "d_taps overlaps d_status"),
    (dict(d_fallback=D_TAPS), "d_taps overlaps d_fallback"),
    (dict(d_signals=D_TAPS), "d_taps overlaps d_signals"),
    (dict(d_tau=D_TAPS), "d_taps overlaps d_tau"),
    (dict(d_offsets=D_TAPS), "d_taps overlaps d_offsets"),
    (dict(d_window=D_TAPS + TAPS_BYTES - 8), "d_taps overlaps d_window"),
    (dict(d_fallback=D_STATUS + STATUS_BYTES - 4), "d_status overlaps d_fallback"),
    (dict(d_signals=D_STATUS), "d_status overlaps d_signals"),
    (dict(d_tau=D_STATUS), "d_status overlaps d_tau"),
    (dict(d_offsets=D_STATUS), "d_status overlaps d_offsets"),
    (dict(d_window=D_STATUS), "d_status overlaps d_window"),
    (dict(d_signals=D_FALL - SIG_BYTES + 4), "d_fallback overlaps d_signals"),
    (dict(d_tau=D_FALL), "d_fallback overlaps d_tau"),
    (dict(d_offsets=D_FALL + FALL_BYTES - 4), "d_fallback overlaps d_offsets"),
    (dict(d_window=D_FALL), "d_fallback overlaps d_window"),
])
def test_refusals(sized, kw, text):
    lib = sized.lib
    lib.bf_clear_error()
    assert _call(sized, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(sized):
    """Ranges that only touch, no window, the largest sizes, a segment that ends with its window, one bin at either end: all pass the
    argument checks, so without a GPU the one refusal left is the missing device (with one, fake pointers must not be launched:
    nothing is called)."""
    if sized.gpu_available():
        return
    lib = sized.lib
    big = np.arange(256, dtype=np.int32)
    for kw in (dict(), dict(d_window=None), dict(d_cov=D_SNAP + SNAP_BYTES), dict(d_chol=D_COV + COV_BYTES), dict(d_gains=D_CHOL - GAINS_BYTES),
               dict(d_status=D_TAPS + TAPS_BYTES), dict(d_fallback=D_STATUS + STATUS_BYTES), dict(d_signals=D_SNAP - SIG_BYTES), dict(d_window=D_SNAP - WIN_BYTES),
               dict(d_offsets=D_TAU), dict(d_window=D_TAU), dict(seg_first=215), dict(seg_first=0, seg_hop=1, segs=248), dict(n_taps=256, seg_first=0, segs=1, bin_lo=0, bin_hi=128),
               dict(mics=big, n=256, m_total=256, d_signals=FAKE + 0x20000000), dict(sources=8), dict(loading=1e-300), dict(loading=1e300),
               dict(bin_lo=0, bin_hi=0), dict(bin_lo=4, bin_hi=4), dict(n=1, mics=MICS[:1]), dict(dirs=1, offset_per_dir=2 ** 31 - 1)):
        lib.bf_clear_error()
        assert _call(sized, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device"), kw
    lib.bf_clear_error()


def test_the_symbol_is_exported_and_bound(native):
    fn = native.lib.bf_mvdr_design_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 26 and fn.argtypes[17] is C.c_double and fn.argtypes[3] is native.IP
    assert [i for i, t in enumerate(fn.argtypes) if t is C.c_void_p] == [0, 8, 9, 11, 18, 19, 20, 21, 22, 23, 24, 25]
    assert all(t is C.c_int for i, t in enumerate(fn.argtypes) if i in (1, 2, 4, 5, 6, 7, 10, 12, 13, 14, 15, 16))
    header = open(native.__file__.replace("zybo-rt-sampler-image-detection_amd/lib/_native.py", "include/beamformer_hip.h")).read()
    assert "#define BF_MVDR_MAX_MICS 256\n" in header and "int bf_mvdr_design_device(" in header
    import filtersum
    assert callable(filtersum.design_mvdr) and callable(filtersum.design_mvdr_slots) and callable(filtersum.FilterSumListener.adapt)
