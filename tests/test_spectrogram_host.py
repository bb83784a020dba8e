"""CPU: bf_spectrogram_device without a device -- the symbols, bf_spectrogram_capacity, every refusal that sits before device bring-up,
the filterbank designers of features.py, the state arithmetic over ragged pushes, and the bound of tests/spectrogram_np.py itself: three
deliberately wrong restatements fall outside it and a float32 FFT of the same data falls inside."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import spectrogram_np as S
from support import FAKE, lib_clearing as lib


# ------------------------------------------------------------------ symbols

def test_symbols_are_exported_and_bound(native):
    cap, dev = native.lib.bf_spectrogram_capacity, native.lib.bf_spectrogram_device
    assert cap.restype is C.c_longlong and cap.argtypes == [C.c_longlong, C.c_int]
    assert dev.restype is C.c_int and len(dev.argtypes) == 20
    assert [i for i, a in enumerate(dev.argtypes) if a is C.c_float] == [14, 15]            # scale, floor_
    assert [i for i, a in enumerate(dev.argtypes) if a is C.c_void_p] == [0, 4, 5, 6, 7, 11, 12, 16, 18, 19]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "beamformer_hip.h")).read()
    for text in ("long long bf_spectrogram_capacity(long long len, int hop_s);", "int bf_spectrogram_device(const float *d_in, int rows, int in_stride, int len,",
                 "#define BF_SPECTROGRAM_MAX_BANDS 4096"):
        assert text in header


def test_capacity(native):
    cap = native.lib.bf_spectrogram_capacity
    for length, hop in [(0, 1), (0, 160), (1, 1), (1, 160), (159, 160), (160, 160), (161, 160), (126, 160), (4096, 1), (24320, 160), (1 << 40, 3),
                        ((1 << 62) + 1, (1 << 31) - 1)]:
        assert cap(length, hop) == S.capacity(length, hop) == -(-length // hop), (length, hop)
    for bad in [(-1, 1), (64, 0), (64, -3), (-5, 0)]:
        assert cap(*bad) == -1, bad


# ------------------------------------------------------------------ refusals before device bring-up


D_IN, D_LEN, D_HIST, D_STATE, D_WINDOW, D_BANK, D_SUPPORT, D_OUT, D_COUNT = (FAKE + i * 0x100000 for i in range(9))
IN_BYTES = ((3 - 1) * 64 + 64) * 4          # of _call's defaults: first float to the last one read
HIST_BYTES = 3 * 24 * 4
OUT_BYTES = ((3 - 1) * 4 + 4) * 10 * 4      # cap = ceil(64 / 16) = 4 frames of 10 bands
BANK_BYTES = 10 * 17 * 4


def _call(lib, d_in=D_IN, rows=3, in_stride=64, len=64, d_len=D_LEN, d_hist=D_HIST, d_state=D_STATE, d_window=D_WINDOW, n_win=25, n_fft=32, hop_s=16,
          d_bank=D_BANK, d_support=D_SUPPORT, n_bands=10, scale=1.0, floor_=1e-10, d_out=D_OUT, out_frames=4, d_count=D_COUNT):
    return lib.bf_spectrogram_device(d_in, rows, in_stride, len, d_len, d_hist, d_state, d_window, n_win, n_fft, hop_s, d_bank, d_support, n_bands, scale,
                                     floor_, d_out, out_frames, d_count, None)


W = "bf_spectrogram_device: "
POW2 = " is not a power of two in [32, 4096]"


@pytest.mark.parametrize("kw,text", [
    (dict(d_in=None), "d_in is null"),
    (dict(d_hist=None), "d_hist is null"),
    (dict(d_state=None), "d_state is null"),
    (dict(d_window=None), "d_window is null"),
    (dict(d_out=None), "d_out is null"),
    (dict(d_count=None), "d_count is null"),
    (dict(d_hist=None, d_count=None, rows=0), "d_hist is null"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(rows=-2, len=-1), "rows = -2 < 1"),
    (dict(len=-1), "len = -1 < 0"),
    (dict(in_stride=63), "in_stride = 63 < len = 64"),
    (dict(n_fft=16, n_win=16), "n_fft = 16" + POW2),
    (dict(n_fft=48), "n_fft = 48" + POW2),
    (dict(n_fft=0), "n_fft = 0" + POW2),
    (dict(n_fft=-32), "n_fft = -32" + POW2),
    (dict(n_fft=4097), "n_fft = 4097" + POW2),
    (dict(n_fft=8192), "n_fft = 8192" + POW2),
    (dict(n_win=0), "n_win = 0 < 1"),
    (dict(n_win=33), "n_win = 33 > n_fft = 32"),
    (dict(hop_s=0), "hop_s = 0 < 1"),
    (dict(hop_s=-160), "hop_s = -160 < 1"),
    (dict(n_bands=0), "n_bands = 0 < 1"),
    (dict(n_bands=4097), "n_bands = 4097 > 4096"),
    (dict(d_bank=None), "d_bank is null (the power spectrum) but n_bands = 10 != n_fft / 2 + 1 = 17"),
    (dict(d_bank=None, d_support=None, n_bands=16), "d_bank is null (the power spectrum) but n_bands = 16 != n_fft / 2 + 1 = 17"),
    (dict(out_frames=3), "out_frames = 3 < cap = 4"),
    (dict(hop_s=1, out_frames=63), "out_frames = 63 < cap = 64"),
    (dict(scale=float("nan")), "scale = nan is not finite"),
    (dict(scale=float("inf")), "scale = inf is not finite"),
    (dict(scale=float("-inf"), floor_=0.0), "scale = -inf is not finite"),
    (dict(floor_=0.0), "floor_ = 0 is not finite and > 0"),
    (dict(floor_=-1.0), "floor_ = -1 is not finite and > 0"),
    (dict(floor_=float("nan")), "floor_ = nan is not finite and > 0"),
    (dict(scale=10.0, floor_=float("inf")), "floor_ = inf is not finite and > 0"),
    (dict(d_out=D_IN), "d_out overlaps d_in"),
    (dict(d_out=D_IN + IN_BYTES - 4), "d_out overlaps d_in"),
    (dict(d_in=D_OUT + OUT_BYTES - 4), "d_out overlaps d_in"),
    (dict(d_out=D_HIST + HIST_BYTES - 4), "d_out overlaps d_hist"),
    (dict(d_hist=D_OUT + OUT_BYTES - 4), "d_out overlaps d_hist"),
    (dict(d_state=D_OUT - 12), "d_out overlaps d_state"),
    (dict(d_count=D_OUT + OUT_BYTES - 4), "d_out overlaps d_count"),
    (dict(d_len=D_OUT + OUT_BYTES - 4), "d_out overlaps d_len"),
    (dict(d_window=D_OUT - 25 * 4 + 4), "d_out overlaps d_window"),
    (dict(d_bank=D_OUT - BANK_BYTES + 4), "d_out overlaps d_bank"),
    (dict(d_support=D_OUT + OUT_BYTES - 4), "d_out overlaps d_support"),
    (dict(d_hist=D_IN + IN_BYTES - 4), "d_hist overlaps d_in"),
    (dict(d_in=D_HIST + HIST_BYTES - 4), "d_hist overlaps d_in"),
    (dict(d_state=D_HIST + HIST_BYTES - 4), "d_hist overlaps d_state"),
    (dict(d_window=D_HIST + 8), "d_hist overlaps d_window"),
    (dict(d_state=D_COUNT + 4), "d_state overlaps d_count"),
    (dict(d_state=D_COUNT - 12), "d_state overlaps d_count"),
    (dict(d_len=D_STATE + 12), "d_state overlaps d_len"),
    (dict(d_state=D_BANK + BANK_BYTES - 4), "d_state overlaps d_bank"),
    (dict(d_len=D_COUNT + 4), "d_count overlaps d_len"),
    (dict(d_count=D_IN + IN_BYTES - 4), "d_count overlaps d_in"),
    (dict(d_count=D_SUPPORT + 76), "d_count overlaps d_support"),
])
def test_refusals(lib, kw, text):
    assert _call(lib, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(native, lib):
    """Ranges that only touch, every optional argument left out, the limits themselves: all pass the argument checks, so without a GPU
    the one refusal left is the missing device (with one, fake pointers must not be launched: nothing is called)."""
    if native.gpu_available():
        return
    for kw in (dict(), dict(d_out=D_IN + IN_BYTES), dict(d_in=D_OUT + OUT_BYTES), dict(d_hist=D_OUT + OUT_BYTES), dict(d_state=D_COUNT - 16),
               dict(d_state=D_COUNT + 8), dict(d_len=D_STATE + 16), dict(d_len=None), dict(d_support=None), dict(d_bank=None, d_support=None, n_bands=17),
               dict(d_bank=None, n_bands=17), dict(scale=0.0, floor_=float("nan")), dict(scale=0.0, floor_=-1.0), dict(scale=-10.0), dict(len=0, out_frames=0),
               dict(len=0, in_stride=0, out_frames=0), dict(n_win=32), dict(n_win=1), dict(hop_s=1, out_frames=64), dict(hop_s=1 << 30), dict(in_stride=100),
               dict(n_fft=4096, n_win=4096, n_bands=4096, d_bank=FAKE + 0x10000000, d_out=FAKE + 0x20000000, d_hist=FAKE + 0x30000000), dict(out_frames=9)):
        assert _call(lib, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device"), (kw, lib.bf_last_error())
        lib.bf_clear_error()


# ------------------------------------------------------------------ the designers

def test_hann(native):
    import features
    for n in (1, 2, 25, 400, 4096):
        w = features.hann(n)
        t = np.arange(n, dtype=np.float64)
        assert w.dtype == np.float32 and w.shape == (n,)
        assert np.array_equal(w, (0.5 - 0.5 * np.cos(2 * np.pi * t / n)).astype(np.float32))
        assert w[0] == 0.0 and np.array_equal(w[1:], w[1:][::-1])                    # periodic: w[t] = w[n - t], no second zero
    assert features.hann(400).max() == 1.0
    with pytest.raises(ValueError):
        features.hann(0)


@pytest.mark.parametrize("htk", [False, True])
def test_mel_scale_and_centres(native, htk):
    import features
    f = np.array([0.0, 100.0, 999.0, 1000.0, 1001.0, 4000.0, 8000.0, 24414.0])
    assert np.allclose(features.mel_to_hz(features.hz_to_mel(f, htk), htk), f, rtol=1e-12, atol=1e-9)
    if htk:
        assert abs(features.hz_to_mel(1000.0, True) - 1000.0) < 0.05               # the scale's anchor: 1000 Hz is 1000 mel
    else:
        assert abs(features.hz_to_mel(1000.0) - 15.0) < 1e-12 and abs(features.hz_to_mel(6400.0) - 42.0) < 1e-12        # 27 mels per factor 6.4
        assert features.hz_to_mel(200.0) == pytest.approx(3.0, abs=1e-12)
    # the centres: where a fine grid of bins finds every triangle's peak, equally spaced on the mel scale to the grid's resolution
    sr, n_fft, n_mels = 16000.0, 4096, 20
    bank, support = features.design_mel(sr, n_fft, n_mels, htk=htk, norm=None)
    peak_hz = np.argmax(bank, axis=1) * sr / n_fft
    mel = features.hz_to_mel(peak_hz, htk)
    step = float(features.hz_to_mel(sr / 2, htk)) / (n_mels + 1)
    slope = float(features.hz_to_mel(1.0, htk))                                     # mel per Hz at 0 Hz, where both scales are steepest
    tol = slope * (sr / n_fft) / 2                                                  # a peak is found within half a bin
    assert np.abs(mel - step * np.arange(1, n_mels + 1)).max() <= tol, (mel, step)
    assert np.abs(np.diff(mel) - step).max() <= 2 * tol
    assert bank.max() <= 1.0 and bank.max(axis=1).min() > 0.95                     # unit peaks (the narrowest side is 84 Hz, half a bin 2 Hz)


@pytest.mark.parametrize("sr,n_fft,n_mels,f_lo,f_hi,htk,norm", [
    (16000, 512, 80, 0.0, None, False, "slaney"), (16000, 512, 80, 0.0, None, False, None), (16000, 512, 40, 20.0, 7600.0, True, None),
    (48828, 1024, 64, 0.0, None, False, "slaney"), (16000, 32, 6, 0.0, None, True, "slaney"), (48000, 4096, 128, 50.0, 20000.0, False, None),
    (16000, 64, 40, 0.0, None, False, None),            # more triangles than bins at the low end: some hold no bin at all
])
def test_mel_triangles(native, sr, n_fft, n_mels, f_lo, f_hi, htk, norm):
    import features
    bank, support = features.design_mel(sr, n_fft, n_mels, f_lo=f_lo, f_hi=f_hi, htk=htk, norm=norm)
    n_bins = n_fft // 2 + 1
    assert bank.dtype == np.float32 and bank.shape == (n_mels, n_bins) and support.dtype == np.int32 and support.shape == (n_mels, 2)
    assert (bank >= 0).all() and np.isfinite(bank).all()
    k = np.arange(n_bins)
    for b in range(n_mels):
        lo, hi = support[b]
        assert 0 <= lo <= hi <= n_bins
        assert not bank[b, :lo].any() and not bank[b, hi:].any()                     # zero outside the support
        if hi > lo:
            assert bank[b, lo] > 0 and bank[b, hi - 1] > 0                           # and the support is tight
            top = np.argmax(bank[b])
            assert (np.diff(bank[b, lo:top + 1]) >= 0).all() and (np.diff(bank[b, top:hi]) <= 0).all()      # one rise, one fall
    edges = features.mel_to_hz(np.linspace(features.hz_to_mel(f_lo, htk), features.hz_to_mel(sr / 2.0 if f_hi is None else f_hi, htk), n_mels + 2), htk)
    f = k * float(sr) / n_fft
    for b in range(n_mels):                                                          # the support is the open interval (f_b, f_b+2)
        want = np.flatnonzero((f > edges[b]) & (f < edges[b + 2]))
        got = np.arange(support[b, 0], support[b, 1])
        # (a bin within rounding of an edge may carry a weight that rounds to zero)
        assert set(got) <= set(want) and len(want) - len(got) <= 2
    if norm is None:
        interior = (f >= edges[1]) & (f <= edges[-2])                                # between the first and the last centre two triangles
        assert interior.sum() >= 1                                                   # overlap, a rising and a falling one: they sum to 1
        assert np.abs(bank[:, interior].astype(np.float64).sum(axis=0) - 1.0).max() < 4 * 2.0 ** -24
    else:
        unit, _ = features.design_mel(sr, n_fft, n_mels, f_lo=f_lo, f_hi=f_hi, htk=htk, norm=None)
        area = (2.0 / (edges[2:] - edges[:-2]))[:, None]
        assert np.allclose(bank, unit.astype(np.float64) * area, rtol=2.0 ** -22, atol=0)
    if n_fft == 64:
        assert (support[:, 0] == support[:, 1]).any()                                # the empty triangles are there


def test_design_mel_refusals(native):
    import features
    for kw in (dict(n_fft=48), dict(n_fft=8192), dict(n_mels=0), dict(f_lo=-1.0), dict(f_lo=4000.0, f_hi=4000.0), dict(f_hi=8001.0), dict(norm="area"),
               dict(sr=0)):
        args = dict(sr=16000, n_fft=512, n_mels=40)
        args.update(kw)
        with pytest.raises(ValueError):
            features.design_mel(**args)


def test_design_bands_partition_the_bins(native):
    import features
    sr, n_fft = 16000, 1024
    centres = 1000.0 * 2.0 ** (np.arange(-12, 9) / 3.0)                              # third-octave centres 62.5 Hz .. 6.35 kHz
    edges = np.concatenate([centres * 2.0 ** (-1 / 6.0), centres[-1:] * 2.0 ** (1 / 6.0)])
    bank, support = features.design_bands(sr, n_fft, edges)
    n_bins = n_fft // 2 + 1
    f = np.arange(n_bins) * sr / n_fft
    assert bank.shape == (len(edges) - 1, n_bins) and bank.dtype == np.float32 and support.dtype == np.int32
    assert set(np.unique(bank)) <= {0.0, 1.0}
    covered = (f >= edges[0]) & (f < edges[-1])
    assert np.array_equal(bank.sum(axis=0), covered.astype(np.float32))              # every bin between the outer edges in exactly one band
    for b in range(len(edges) - 1):
        want = np.flatnonzero((f >= edges[b]) & (f < edges[b + 1]))
        lo, hi = support[b]
        assert np.array_equal(np.arange(lo, hi), want) if want.size else lo == hi
    live = support[support[:, 0] < support[:, 1]]
    assert np.array_equal(live[1:, 0], live[:-1, 1])                                 # the bands follow each other without a gap
    # an edge on a bin: the bin belongs to the band that starts there
    bank, support = features.design_bands(16000, 32, [0.0, 1000.0, 2000.0, 8000.0])
    assert support.tolist() == [[0, 2], [2, 4], [4, 16]]
    for bad in ([100.0], [100.0, 100.0], [200.0, 100.0]):
        with pytest.raises(ValueError):
            features.design_bands(16000, 512, bad)


# ------------------------------------------------------------------ the state arithmetic

@pytest.mark.parametrize("n_win,hop", [(25, 10), (25, 25), (25, 28), (32, 1), (400, 160), (1, 1), (1, 7)])
def test_ragged_pushes_count_like_one_long_push(native, n_win, hop):
    import features
    rng = np.random.default_rng([n_win, hop])
    for _ in range(20):
        sizes = [int(v) for v in rng.integers(0, 3 * max(n_win, hop), size=rng.integers(1, 12))] + [0, 1, n_win - 1 if n_win > 1 else 1]
        s0, starts, pos = 0, [], 0
        for L in sizes:
            count, s1 = S.advance(s0, L, n_win, hop)
            assert features.advance_frames(s0, L, n_win, hop) == (count, s1)
            assert 0 <= count <= S.capacity(L, hop) and s1 >= -(n_win - 1)
            starts += [pos + s0 + j * hop for j in range(count)]
            assert all(s + n_win <= pos + L for s in starts)
            pos += L
            s0 = s1
        total = sum(sizes)
        count, s1 = S.advance(0, total, n_win, hop)
        assert len(starts) == count and s0 == s1                                     # and the frames are the same frames
        assert starts == [j * hop for j in range(count)]
        if count:
            assert (count - 1) * hop + n_win <= total < count * hop + n_win          # the next frame does not fit yet


def test_restatement_split_calls_equal_one_call():
    rng = np.random.default_rng(11)
    n_win, n_fft, hop, rows = 25, 32, 7, 2
    x = rng.standard_normal((rows, 300)).astype(np.float32)
    w = rng.standard_normal(n_win).astype(np.float32)
    whole = S.spectrogram(x, np.zeros((rows, n_win - 1), np.float32), 0, w, n_fft, hop)
    for cuts in ([150], [3, 20, 21, 100, 101, 290]):
        hist, s0, parts = np.zeros((rows, n_win - 1), np.float32), 0, []
        for a, b in zip([0] + cuts, cuts + [300]):
            got = S.spectrogram(x[:, a:b], hist, s0, w, n_fft, hop)
            parts.append(got["out"][:, :got["count"]])
            hist, s0 = got["hist"], got["s0"]
        joined = np.concatenate(parts, axis=1)
        assert joined.shape[1] == whole["count"] and np.array_equal(joined, whole["out"][:, :whole["count"]])
        assert s0 == whole["s0"] and np.array_equal(hist, whole["hist"])
    bad = S.spectrogram(x, np.zeros((rows, n_win - 1), np.float32), -n_win, w, n_fft, hop)
    assert bad["status"] == 1 and bad["count"] == 0 and bad["s0"] == -n_win and not bad["out"].any()


# ------------------------------------------------------------------ the bound means something

def _bound_case(native, which):
    import features
    rng = np.random.default_rng(5)
    if which == "speech":
        sr, n_fft, n_win, hop = 16000, 512, 400, 160
        bank, support = features.design_mel(sr, n_fft, 40)
    elif which == "small":
        sr, n_fft, n_win, hop = 16000, 32, 25, 10
        bank, support = features.design_bands(sr, n_fft, [0.0, 1000.0, 2500.0, 4000.0, 8000.0])
    else:
        sr, n_fft, n_win, hop = 16000, 1024, 1024, 300
        bank, support = None, None
    x = rng.standard_normal((3, 8 * hop + n_win)).astype(np.float32)
    return x, features.hann(n_win), n_fft, n_win, hop, bank, support


def _outside(got, want):
    """bool [rows, count, n_bands]: the values of the completed frames that miss the interval."""
    g = got.astype(np.float64)[:, :want["count"]]
    return ~((g >= want["lo"][:, :want["count"]]) & (g <= want["hi"][:, :want["count"]]))


@pytest.mark.parametrize("scale", [0.0, 1.0])
@pytest.mark.parametrize("which", ["speech", "small", "spectrum"])
def test_wrong_restatements_fall_outside_and_a_float32_fft_inside(native, which, scale):
    x, w, n_fft, n_win, hop, bank, support = _bound_case(native, which)
    hist = np.zeros((x.shape[0], n_win - 1), np.float32)
    floor = 1e-10
    want = S.spectrogram(x, hist, 0, w, n_fft, hop, bank, support, scale, floor)
    count = want["count"]
    assert count == 9
    Wt, _ = S._weights(bank, support, n_fft // 2 + 1)

    def outputs(u, roll=0):
        X = np.roll(S.spectrum(u, n_fft), -roll, axis=-1)                            # roll 1: bin k + 1 stands where bin k belongs
        out = np.zeros_like(want["out"])
        out[:, :count] = S.to_output((X.real ** 2 + X.imag ** 2) @ Wt.T, scale, floor)
        return out.astype(np.float32)

    frames = S.framed(x, hist, 0, x.shape[1], n_win, hop)
    right = outputs(S.windowed(frames, w))
    assert S.inside(right, want) == ""                                               # the float64 value, rounded once, is inside
    wrong = {"bin k + 1 for bin k": outputs(S.windowed(frames, w), roll=1),
             "the window one sample late": outputs(S.windowed(frames, np.roll(w, 1))),
             "the frames one sample late": outputs(S.windowed(S.framed(x, hist, 0, x.shape[1], n_win, hop, shift=1), w))}
    for name, got in wrong.items():
        assert S.inside(got, want) != "", name
        outside = _outside(got, want)
        print("%s, %s, scale %g: %.3f of the values outside the bound" % (which, name, scale, outside.mean()))
        # every frame of every row shows the mistake.  (Not every value: the bound is absolute in A = sum |u|, so a weak bin of a
        # long window moves less than it allows -- a window one sample late leaves 80 % of a 1024-point noise spectrum inside.)
        assert outside.any(axis=2).all(), name
    # a float32 FFT of the same u, float32 power, float32 bank sums
    u = S.windowed(frames, w)
    X32 = np.fft.rfft(u, n=n_fft, axis=-1).astype(np.complex64)
    P32 = (X32.real * X32.real + X32.imag * X32.imag).astype(np.float32)
    E32 = (P32 @ Wt.T.astype(np.float32)).astype(np.float32)
    got = np.zeros_like(want["out"], dtype=np.float32)
    got[:, :count] = E32 if scale == 0 else (np.float32(scale) * np.log10(np.maximum(E32, np.float32(floor)))).astype(np.float32)
    assert S.inside(got, want) == ""
    print("%s, scale %g: a float32 FFT uses %.4f of the bound" % (which, scale, S.worst_ratio(got, want)))


# ------------------------------------------------------------------ the Python layer

def test_pipeline_has_features(native):
    import features
    import pipeline

    class Pushed:
        def push_from(self, ao, out):
            return ("feat", ao, out)
    assert list(inspect.signature(pipeline.FusedPipeline.features).parameters) == ["self", "out", "ao", "bfeat"]
    assert pipeline.FusedPipeline.features(None, "beams", "ao", Pushed()) == ("feat", "ao", "beams")
    assert list(inspect.signature(features.BeamFeatures.push).parameters) == ["self", "d_audio", "length", "d_len"]
    assert list(inspect.signature(features.BeamFeatures.__init__).parameters)[:11] == ["self", "sr", "rows", "n_fft", "n_win", "hop", "bank", "support", "scale",
                                                                                      "floor", "max_len"]
