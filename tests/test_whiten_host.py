"""CPU: bf_whiten_device without a device -- the restatement's own consistency (tests/whiten_np.py), whiten.Whitener's plumbing, every
refusal that sits before device bring-up, and the end-to-end claim the feature rests on, through the committed checker: under a hum
20 dB above it the plain band-pass map peaks on the hum, the whitened map of the same bins on the source.

Sizes of the refusals: 16 microphones, 64 samples, as tests/test_api_refusals_host.py."""
import ctypes as C

import numpy as np
import pytest

import util
import whiten_np as wn
from support import FAKE, entry, lib_16x64 as lib

M, N = 16, 64


def _hann(n):
    t = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * t / n)).astype(np.float32)


# ------------------------------------------------------------------ the restatement is consistent with itself

BANDS = dict(bins=[(1, 20), (0, 33), (7, 8), (-3, 99)], beta=[1.0, 0.5, 1.0, 0.0], gain=[2.0, 1.0, 64.0, -3.0])


@pytest.mark.parametrize("n", [32, 64, 1024])
def test_zero_rows_scaling_and_band_independence(n):
    rng = np.random.default_rng(n)
    x = wn.noise_rows(rng, (2, 3, n))
    x[..., :] += (np.cos(2 * np.pi * 7 * np.arange(n) / n) * np.abs(x).max(axis=-1, keepdims=True)).astype(np.float32)     # the one-bin band's bin
    x[1, 1] = 0.0
    w = _hann(n)
    out, tol = wn.whiten(x, w, with_tol=True, **BANDS)
    assert out.shape == (4, 2, 3, n) and np.isfinite(tol).all()
    assert not out[:, 1, 1].any() and not tol[:, 1, 1].any()                    # a row of zeros: zeros, for every beta, exactly
    assert not wn.whiten(np.zeros((1, n), np.float32), None, floor_abs=0.5, **BANDS).any()
    for b in range(4):                                                          # band b of a K-band call is the single-band call
        one = wn.whiten(x, w, [BANDS["bins"][b]], [BANDS["beta"][b]], [BANDS["gain"][b]])
        assert np.array_equal(one[0], out[b])
    scaled = wn.whiten((x * np.float32(2.0 ** -5)).astype(np.float32), w, **BANDS)
    live = np.ones((2, 3), bool)
    live[1, 1] = False
    for b, beta in enumerate(BANDS["beta"]):                                    # a power-of-two gain: nothing (beta 1) .. all of it (beta 0)
        want = out[b][live] * 2.0 ** (-5 * (1 - beta))
        assert np.abs(scaled[b][live] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("n", [32, 256])
def test_beta_0_rect_full_band_is_the_identity(n):
    rng = np.random.default_rng(n + 1)
    x = wn.noise_rows(rng, (5, n))
    out, tol = wn.whiten(x, None, [(0, n // 2 + 1)], [0.0], [3.0], with_tol=True)
    assert np.abs(out[0] - 3.0 * x.astype(np.float64)).max() < 1e-12 * np.abs(x).max()
    assert (tol > 0).all() and (tol.max(axis=-1) < 1e-2 * wn.row_rms(out)).all()
    one = wn.whiten(x, None, [(0, n // 2 + 1)], [1.0], [n / np.sqrt(n)])                   # the default gain: unit-RMS rows at beta = 1
    assert np.allclose(wn.row_rms(one), 1.0, rtol=1e-6)                                   # (the gain is a float32)


@pytest.mark.parametrize("n", [32, 256, 1024])
@pytest.mark.parametrize("floor_rel", [1e-3, 5e-2])
def test_a_float32_transform_sits_far_inside_the_tolerance_which_stays_small(n, floor_rel):
    """scipy's float32 transforms around the float32 weighting use under 0.05 of the tolerance; a bin shifted by one, or a conjugated
    spectrum, falls outside; and the tolerance is at most 0.05 of each row's RMS output."""
    import scipy.fft as sf
    rng = np.random.default_rng([n, int(floor_rel * 1e4)])
    x = wn.noise_rows(rng, (12, n))
    w = _hann(n)
    lo, hi = 1, n // 2
    gain = n / np.sqrt(2 * (hi - lo))
    want, tol = wn.whiten(x, w, [(lo, hi)], [1.0], [gain], floor_rel, with_tol=True)
    assert (tol.max(axis=-1) <= 0.05 * wn.row_rms(want)).all()
    X = sf.rfft(wn.windowed(x, w))
    assert X.dtype == np.complex64
    mag = np.abs(X)
    rms = np.sqrt((mag[:, lo:hi] ** 2).mean(axis=-1, dtype=np.float32))[:, None]
    Wk = np.zeros_like(X)
    Wk[:, lo:hi] = (X / np.maximum(mag, np.float32(floor_rel) * rms))[:, lo:hi]
    got = sf.irfft(Wk, n=n) * np.float32(gain)
    assert got.dtype == np.float32
    ratio = float((np.abs(got - want[0]) / tol[0]).max())
    print("N = %d, floor_rel = %g: scipy float32 error / tolerance %.4f; tolerance / row RMS at most %.4f" % (n, floor_rel, ratio, (tol.max(axis=-1) / wn.row_rms(want)).max()))
    assert ratio < 0.05
    for wrong in (sf.irfft(np.roll(Wk, 1, axis=-1), n=n), sf.irfft(np.conj(Wk), n=n)):
        assert (np.abs(wrong * np.float32(gain) - want[0]) > tol[0]).any()


# ------------------------------------------------------------------ Whitener's plumbing

def test_whitener_bins_gain_and_errors(native):
    import whiten
    from interface import config
    util.configure_small(256)
    try:
        fs = 48828.0
        wh = whiten.Whitener([(1000.0, 12000.0), (0.0, 1e9, 0.5), (-1.0, 500.0), (fs / 256, fs / 256)], fs=fs)
        # lo = ceil(f_lo N / fs), at least 1 unless f_lo < 0; hi = floor(f_hi N / fs) + 1, capped at N / 2 + 1
        assert wh.bins.tolist() == [[6, 63], [1, 129], [0, 3], [1, 2]] and wh.bins.dtype == np.int32
        assert wh.beta.tolist() == [1.0, 0.5, 1.0, 1.0] and wh.K == 4
        assert whiten.band_bins(1000.0, 12000.0, 256, fs) == (6, 63) and whiten.band_bins(0.0, 100.0, 256, fs) == (1, 1)
        assert [whiten.two_sided_bins(lo, hi, 256) for lo, hi in wh.bins] == [114, 255, 5, 2]
        assert np.array_equal(wh.gain, (256 / np.sqrt([114, 255, 5, 2])).astype(np.float32))
        assert wh.floor_rel == 1e-3 and wh.floor_abs == 0.0
        assert np.array_equal(wh.window, _hann(256)) and whiten.Whitener([(1000.0, 2000.0)], window="rect").window is None
        assert whiten.Whitener([(1000.0, 2000.0)], gain=2.0).gain.tolist() == [2.0]
        assert whiten.Whitener([(1000.0, 2000.0)], beta=0.25).beta.tolist() == [0.25]
        assert whiten.Whitener([(3000.0, 8000.0)]).fs == float(config.SAMPLE_RATE)
        for kw, text in ((dict(bands=[]), "bands, got 0"), (dict(bands=[(1.0, 2.0)] * 17), "bands, got 17"),
                         (dict(bands=[(8000.0, 3000.0)]), "holds no bin"), (dict(bands=[(0.0, 100.0)]), "holds no bin"),
                         (dict(bands=[(1000.0, 2000.0, 1.5)]), "beta must be in \\[0, 1\\], got 1.5"),
                         (dict(bands=[(1000.0, 2000.0)], beta=-0.5), "got -0.5"), (dict(bands=[(1000.0, 2000.0)], beta=float("nan")), "got nan"),
                         (dict(bands=[(1000.0,)]), "want \\(f_lo, f_hi\\)"), (dict(bands=[(1000.0, 2000.0)], window="kaiser"), "'kaiser'"),
                         (dict(bands=[(1000.0, 2000.0)], window=np.ones(100, np.float32)), "shape \\(100,\\)"),
                         (dict(bands=[(1000.0, 2000.0)], floor_rel=-1.0), "floor_rel must be finite and >= 0, got -1"),
                         (dict(bands=[(1000.0, 2000.0)], floor_abs=float("inf")), "floor_abs must be finite and >= 0, got inf"),
                         (dict(bands=[(1000.0, 2000.0)], gain=float("nan")), "gain must be finite"), (dict(bands=[(1000.0, 2000.0)], fs=0.0), "fs must be > 0")):
            with pytest.raises(ValueError, match=text):
                whiten.Whitener(**kw)
        util.configure_small(100)
        with pytest.raises(ValueError, match="N_SAMPLES = 100 is not a power of two"):
            whiten.Whitener([(1000.0, 2000.0)])
    finally:
        util.configure("cfg1")


def test_pipeline_has_whiten(native):
    import pipeline
    import whiten

    class Stub:
        def frames(self, x):
            return ("frames", x)
    assert pipeline.FusedPipeline.whiten(None, "x", Stub()) == ("frames", "x")
    for word in ("raw frames", "independently", "hop"):
        assert word in whiten.__doc__


# ------------------------------------------------------------------ refusals before device bring-up

BINS = np.array([[1, 20], [0, 33]] + [[2, 9]] * 15, dtype=np.int32)
BETA = np.array([1.0, 0.5] + [1.0] * 15, dtype=np.float32)
GAIN = np.ones(17, dtype=np.float32)
D_OUT, D_WINDOW = FAKE + 0x200000, FAKE + 0x100000
IN_BYTES = 2 * M * N * 4          # of _call's default batch
W = "bf_whiten_device: "

_call = entry("bf_whiten_device", d_signals=FAKE, rows=M, frames=2, d_window=D_WINDOW, bins=BINS.ctypes.data_as(C.POINTER(C.c_int)),
              beta=BETA.ctypes.data_as(C.POINTER(C.c_float)), gain=GAIN.ctypes.data_as(C.POINTER(C.c_float)), bands=2, floor_rel=1e-3, floor_abs=0.0,
              d_out=D_OUT)


def _ints(*v):
    a = np.array(v, dtype=np.int32)
    return a.ctypes.data_as(C.POINTER(C.c_int)), a


def _floats(*v):
    a = np.array(v, dtype=np.float32)
    return a.ctypes.data_as(C.POINTER(C.c_float)), a


@pytest.mark.parametrize("kw,text", [
    (dict(d_signals=None), "d_signals is null"),
    (dict(bins=None), "bins is null"),
    (dict(beta=None), "beta is null"),
    (dict(gain=None), "gain is null"),
    (dict(d_out=None), "d_out is null"),
    (dict(d_signals=None, d_out=None, rows=0), "d_signals is null"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(rows=-4, frames=0), "rows = -4 < 1"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(bands=0), "bands = 0 < 1"),
    (dict(bands=17), "bands = 17 > 16"),
    (dict(bins=_ints(1, 20, 5, 5)), "band 1: bins [5, 5) hold no bin of [0, N_SAMPLES / 2 + 1 = 33)"),
    (dict(bins=_ints(9, 4, 0, 33)), "band 0: bins [9, 4) hold no bin of [0, N_SAMPLES / 2 + 1 = 33)"),
    (dict(bins=_ints(33, 50, 0, 33)), "band 0: bins [33, 50) hold no bin of [0, N_SAMPLES / 2 + 1 = 33)"),
    (dict(bins=_ints(1, 20, -4, 0)), "band 1: bins [-4, 0) hold no bin of [0, N_SAMPLES / 2 + 1 = 33)"),
    (dict(beta=_floats(1.0, -0.5)), "beta[1] = -0.5 is not finite and >= 0"),
    (dict(beta=_floats(1.5, 1.0)), "beta[0] = 1.5 > 1"),
    (dict(beta=_floats(np.nan, 1.0)), "beta[0] = nan is not finite and >= 0"),
    (dict(beta=_floats(1.0, np.inf)), "beta[1] = inf is not finite and >= 0"),
    (dict(gain=_floats(1.0, np.nan)), "gain[1] = nan is not finite"),
    (dict(gain=_floats(-np.inf, 1.0)), "gain[0] = -inf is not finite"),
    (dict(floor_rel=-1.0), "floor_rel = -1 is not finite and >= 0"),
    (dict(floor_rel=float("nan")), "floor_rel = nan is not finite and >= 0"),
    (dict(floor_abs=-0.5), "floor_abs = -0.5 is not finite and >= 0"),
    (dict(floor_abs=float("inf")), "floor_abs = inf is not finite and >= 0"),
    (dict(d_out=FAKE), "d_out overlaps d_signals"),
    (dict(d_out=FAKE + IN_BYTES - 4), "d_out overlaps d_signals"),
    (dict(d_signals=D_OUT + 2 * IN_BYTES - 4), "d_out overlaps d_signals"),
    (dict(d_window=D_OUT - N * 4 + 4), "d_out overlaps d_window"),
    (dict(d_window=D_OUT + 2 * IN_BYTES - 4), "d_out overlaps d_window"),
])
def test_refusals(native, lib, kw, text):
    kw = {k: (v[0] if isinstance(v, tuple) else v) for k, v in kw.items()}          # (a tuple keeps its array alive in the parameter list)
    assert _call(native, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


@pytest.mark.parametrize("n", [100, 16, 96])
def test_n_samples_must_be_a_power_of_two_in_range(native, lib, n):
    assert lib.bf_configure(M, n, 5, 5, 8) == 0
    try:
        assert _call(native) == -1
        assert lib.bf_last_error().decode() == W + "N_SAMPLES = %d is not a power of two in [32, 4096]" % n
    finally:
        lib.bf_clear_error()
        assert lib.bf_configure(M, N, 5, 5, 8) == 0


def test_accepted_arguments_reach_the_device_check(native, lib):
    """Ranges that only touch, no window, 16 bands, bands clipped at both ends, beta 0 and 1, a floor of 0: all pass the argument checks,
    so without a GPU the one refusal left is the missing device (with one, fake pointers must not be launched: nothing is called)."""
    if native.gpu_available():
        return
    for kw in (dict(d_out=FAKE + IN_BYTES), dict(d_signals=D_OUT + 2 * IN_BYTES), dict(d_window=D_OUT - N * 4), dict(d_window=None, d_out=FAKE + IN_BYTES),
               dict(bands=16), dict(bins=_ints(-5, 1, 32, 99)), dict(beta=_floats(0.0, 1.0)), dict(floor_rel=0.0, floor_abs=0.0), dict(floor_abs=2.0),
               dict(gain=_floats(0.0, -3.0)), dict(bands=1, rows=1, frames=1)):
        kw = {k: (v[0] if isinstance(v, tuple) else v) for k, v in kw.items()}
        assert _call(native, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device")
        lib.bf_clear_error()


# ------------------------------------------------------------------ the end-to-end claim, through the committed checker

SEEDS = (0, 1, 2, 3)


def _lerp_map(oracle_lib, frame, delays, n):
    X, Y, mics = delays.shape
    orc = oracle_lib.Oracle(n, X, Y, 8)
    return orc.mimo_lerp(np.ascontiguousarray(frame, dtype=np.float32), np.float32(delays), np.arange(mics, dtype=np.int32))


@pytest.fixture(scope="module")
def hum_maps(oracle_lib):
    """Per seed: the committed checker's lerp maps of the hum scene's window band-passed (beta = 0) and whitened (beta = 1) over the same
    bins with a Hann window, by the restatement; computed once."""
    import directions_np as D
    s = wn.HUM
    delays = D.calculate_delays(s["X"], s["Y"], arrays=1)
    n, (lo, hi) = s["n"], s["bins"]
    gain = n / np.sqrt(2 * (hi - lo))
    maps = {}
    for seed in SEEDS:
        y = wn.whiten(wn.hum_frame(seed, delays, **s), _hann(n), [(lo, hi), (lo, hi)], [0.0, 1.0], [1.0, gain], 1e-3)
        maps[seed] = (_lerp_map(oracle_lib, y[0], delays, n), _lerp_map(oracle_lib, y[1], delays, n))
    return maps


@pytest.mark.parametrize("seed", SEEDS)
def test_whitening_finds_the_source_under_the_hum(hum_maps, seed):
    """The hum scene (wn.HUM: a 2-10 kHz source at cell (12, 8), a 1200 / 2400 / 3600 Hz hum 20 dB above it at (30, 15), Hann window,
    bins [5, 64)).  Confirmed with the committed checker before the seeds were fixed: the band-pass map peaks on the hum at (30, 15) with
    785 to 787 of the 943 cells within 3 dB; the whitened map peaks on (12, 8) in all four seeds with 117 to 125 cells within 3 dB (README)."""
    plain, white = hum_maps[seed]
    src, hum = wn.HUM["src"], wn.HUM["hum"]
    peak_plain, peak_white = wn.argmax2(plain), wn.argmax2(white)
    n_plain, n_white = wn.within_3db(plain), wn.within_3db(white)
    print("seed %d: band-pass argmax %s, %d cells within 3 dB; whitened argmax %s, %d cells" % (seed, peak_plain, n_plain, peak_white, n_white))
    assert peak_white == src, (peak_white, src)
    assert peak_plain != src and max(abs(peak_plain[0] - hum[0]), abs(peak_plain[1] - hum[1])) <= 1, peak_plain
    assert 2 * n_white <= n_plain, (n_white, n_plain)


@pytest.mark.parametrize("seed", SEEDS)
def test_whitening_finds_the_pink_source_with_no_band_chosen(oracle_lib, seed):
    """The 1/f + DC scene of test_band_filter_host.py, whitened over bins [1, 129) -- everything but DC, no band chosen: the peak is on
    the source at (12, 8) in all four seeds."""
    import directions_np as D
    delays = D.calculate_delays(41, 23, arrays=1)
    n = 256
    frame = wn.pink_frame(seed, delays, (12, 8), n, 48828.0)
    y = wn.whiten(frame, _hann(n), [(1, 129)], [1.0], [n / np.sqrt(255)], 1e-3)[0]
    raw, white = _lerp_map(oracle_lib, frame, delays, n), _lerp_map(oracle_lib, y, delays, n)
    print("seed %d: raw argmax %s, %d cells within 3 dB; whitened argmax %s, %d cells"
          % (seed, wn.argmax2(raw), wn.within_3db(raw), wn.argmax2(white), wn.within_3db(white)))
    assert wn.argmax2(white) == (12, 8)
