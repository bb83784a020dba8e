"""CPU: bf_band_filter_device without a device -- the restatement's own consistency (tests/band_np.py), the windowed-sinc design of
band.design, every refusal that sits before device bring-up, and the end-to-end claim the feature rests on: on this array a
broadband map of a 1/f source is nearly flat and peaks in the wrong place, the 3-8 kHz map of the same frame finds the source.

Sizes of the refusals: 16 microphones, 64 samples, as tests/test_api_refusals_host.py."""
import numpy as np
import pytest

import band_np
import util
from support import FAKE, lib_16x64 as lib

M, N, X, Y, T = 16, 64, 5, 5, 8


# ------------------------------------------------------------------ the restatement is consistent with itself

@pytest.mark.parametrize("n,taps,hop", [(64, 9, 8), (64, 9, 32), (64, 33, 32), (100, 9, 50), (256, 65, 64)])
def test_overlapping_windows_agree(n, taps, hop):
    rng = np.random.default_rng(n + taps + hop)
    F, R = 4, 3
    S = util.wild(rng, (R, hop * F + n))
    frames = np.stack([S[:, (f + 1) * hop:(f + 1) * hop + n] for f in range(F)])
    prev = np.ascontiguousarray(S[:, :n])
    h = util.wild(rng, (2, taps))
    y = band_np.band_filter(frames, h, hop, prev)
    assert taps - 1 <= hop < n
    for f in range(1, F):
        assert np.array_equal(util.bits(y[:, f, :, :n - hop]), util.bits(y[:, f - 1, :, hop:]))


@pytest.mark.parametrize("n,taps,hop,F,F1", [(64, 5, 16, 5, 2), (64, 64, 64, 3, 1), (100, 9, 100, 4, 3)])
def test_split_batch_equals_one_call(n, taps, hop, F, F1):
    rng = np.random.default_rng(7 * n + taps)
    R = 3
    S = util.wild(rng, (R, hop * F + n))
    frames = np.stack([S[:, (f + 1) * hop:(f + 1) * hop + n] for f in range(F)])
    prev = np.ascontiguousarray(S[:, :n])
    h = util.wild(rng, (3, taps))
    whole = band_np.band_filter(frames, h, hop, prev)
    a = band_np.band_filter(frames[:F1], h, hop, prev)
    b = band_np.band_filter(frames[F1:], h, hop, frames[F1 - 1])       # the carried window: the last frame of the first call
    assert np.array_equal(util.bits(whole), util.bits(np.concatenate([a, b], axis=1)))
    # and silence before the stream differs from a real history exactly in the first taps - 1 outputs of frame 0
    cold = band_np.band_filter(frames, h, hop, None)
    assert np.array_equal(util.bits(cold[:, 1:]), util.bits(whole[:, 1:])) and np.array_equal(util.bits(cold[:, 0, :, taps - 1:]), util.bits(whole[:, 0, :, taps - 1:]))
    assert not np.array_equal(util.bits(cold[:, 0, :, :taps - 1]), util.bits(whole[:, 0, :, :taps - 1]))


def test_identity_and_impulse():
    rng = np.random.default_rng(3)
    x = util.wild(rng, (2, 3, 64))
    one = band_np.band_filter(x, np.ones((1, 1), np.float32))
    assert np.array_equal(util.bits(one[0]), util.bits(x))                   # T = 1, h = [1]: the identity on the bits
    h = util.wild(rng, (3, 9))
    imp = np.zeros((1, 1, 64), np.float32)
    imp[0, 0, 0] = 1.0
    y = band_np.band_filter(imp, h)
    assert np.array_equal(util.bits(y[:, 0, 0, :9]), util.bits(h)) and not y[:, 0, 0, 9:].any()    # a unit impulse gives the taps back


# ------------------------------------------------------------------ the design

def test_design(native):
    import band
    fs = 48828.0
    h = band.design([(3000.0, 8000.0), (0.0, 4000.0), (6000.0, fs)], n_taps=65, fs=fs)
    assert h.dtype == np.float32 and h.shape == (3, 65)
    assert np.array_equal(util.bits(h), util.bits(h[:, ::-1]))                # symmetric: linear phase, one delay for every microphone and band
    # A Hamming-windowed low-pass ripples 53 dB under its pass band (0.0022) outside the transition band, which is 3.3 fs / T = 2.5 kHz
    # wide: DC lies 3 kHz below the edge.  A band-pass is the difference of two low-passes, so its stop band is bounded by twice that.
    stop = 2 * 10 ** (-53 / 20)
    assert abs(float(h[0].astype(np.float64).sum())) < stop
    assert abs(float(h[2].astype(np.float64).sum())) < stop                                  # the high-pass rejects DC as well
    assert abs(float(h[1].astype(np.float64).sum()) - 1.0) < 1e-6                            # low-pass: unit gain at DC
    m = np.arange(65) - 32
    for k, fc in ((0, 5500.0), (2, fs / 2)):
        assert abs(abs(np.sum(h[k].astype(np.float64) * np.exp(-2j * np.pi * fc / fs * m))) - 1.0) < 1e-6    # unit gain mid-band
    y = band_np.band_filter(np.eye(1, 256, dtype=np.float32)[None], h)
    assert np.array_equal(util.bits(y[:, 0, 0, :65]), util.bits(h))
    with pytest.raises(ValueError):
        band.design([(6000.0, fs)], n_taps=64, fs=fs)                # an even-length high-pass
    with pytest.raises(ValueError):
        band.design([(8000.0, 3000.0)], fs=fs)
    with pytest.raises(ValueError):
        band.design([(3000.0, 8000.0)], window="kaiser", fs=fs)


# ------------------------------------------------------------------ refusals before device bring-up


def _call(lib, d_signals=FAKE, rows=M, frames=2, hop=32, d_prev=None, d_taps=FAKE + 0x100000, n_taps=9, bands=2, d_out=FAKE + 0x200000):
    return lib.bf_band_filter_device(d_signals, rows, frames, hop, d_prev, d_taps, n_taps, bands, d_out, None)


IN_BYTES = 2 * M * N * 4          # of _call's default batch
W = "bf_band_filter_device: "


@pytest.mark.parametrize("kw,text", [
    (dict(d_signals=None), "d_signals is null"),
    (dict(d_taps=None), "d_taps is null"),
    (dict(d_out=None), "d_out is null"),
    (dict(d_signals=None, d_out=None, rows=0), "d_signals is null"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(rows=-4, frames=0), "rows = -4 < 1"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(bands=0), "bands = 0 < 1"),
    (dict(n_taps=0), "n_taps = 0 < 1"),
    (dict(n_taps=-1, hop=-1), "n_taps = -1 < 1"),
    (dict(bands=17), "bands = 17 > 16"),
    (dict(n_taps=65, hop=64), "n_taps = 65 > N_SAMPLES = 64"),
    (dict(hop=-1), "hop = -1 < 0"),
    (dict(hop=65), "hop = 65 > N_SAMPLES = 64 (the windows would leave gaps in the stream)"),
    (dict(hop=7), "the filter needs n_taps - 1 = 8 samples of history but hop = 7 (continuous mode wants n_taps - 1 <= hop)"),
    (dict(n_taps=64, hop=62), "the filter needs n_taps - 1 = 63 samples of history but hop = 62 (continuous mode wants n_taps - 1 <= hop)"),
    (dict(d_out=FAKE), "d_out overlaps d_signals (frame f - 1 is read while frame f is written)"),
    (dict(d_out=FAKE + IN_BYTES - 4), "d_out overlaps d_signals (frame f - 1 is read while frame f is written)"),
    (dict(d_signals=FAKE + 0x200000 + 2 * IN_BYTES - 4), "d_out overlaps d_signals (frame f - 1 is read while frame f is written)"),
    (dict(d_prev=FAKE + 0x200000 - M * N * 4 + 4), "d_out overlaps d_prev"),
    (dict(d_prev=FAKE + 0x200000 + 2 * IN_BYTES - 4), "d_out overlaps d_prev"),
])
def test_refusals(lib, kw, text):
    assert _call(lib, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(native, lib):
    """Ranges that only touch, hop = 0 with a long filter, hop = n_taps - 1, 16 bands: all pass the argument checks, so without a
    GPU the one refusal left is the missing device (with one, fake pointers must not be launched: nothing is called)."""
    if native.gpu_available():
        return
    for kw in (dict(d_out=FAKE + IN_BYTES), dict(d_signals=FAKE + 0x200000 + 2 * IN_BYTES), dict(d_prev=FAKE + 0x200000 - M * N * 4),
               dict(hop=0, n_taps=64), dict(hop=8), dict(bands=16), dict(hop=64, n_taps=64)):
        assert _call(lib, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device")
        lib.bf_clear_error()


# ------------------------------------------------------------------ the end-to-end claim

SCENE = dict(seed=0, X=41, Y=23, src=(12, 8), n=256, taps=65, band=(3000.0, 8000.0), fs=48828.0, noise=0.02, dc=0.05)


def scene_maps(oracle_lib, seed, X, Y, src, n, taps, band, fs, noise, dc):
    """One window of a seeded stream on the 8 x 8 array -- a plane wave from grid point `src` with a 1/f amplitude spectrum from
    100 Hz to 8 kHz (400 tones, random phases, unit RMS), microphone noise, a DC offset per microphone -- as the raw frame and as
    the restated band-pass of it, whose history is the taps - 1 stream samples before the window.  Returns the committed checker's
    lerp maps (raw, filtered), float32 [X, Y]."""
    import band as band_mod
    import directions_np as D
    rng = np.random.default_rng(seed)
    delays = D.calculate_delays(X, Y, arrays=1)                      # [X, Y, 64] in samples
    Mics = delays.shape[2]
    hop = taps - 1
    L = hop + n                                                       # the window starts `hop` samples into the stream
    f = np.linspace(100.0, 8000.0, 400)
    amp, ph = 1.0 / f, rng.uniform(0, 2 * np.pi, f.size)
    t = (np.arange(L, dtype=np.float64)[None, :] + delays[src[0], src[1]][:, None]) / fs           # microphone m leads by its delay
    s = np.zeros_like(t)
    for fi, ai, pi in zip(f, amp, ph):
        s += ai * np.sin(2 * np.pi * fi * t + pi)
    s /= np.sqrt(np.mean(s ** 2))
    S = (s + noise * rng.standard_normal((Mics, L)) + dc * rng.standard_normal((Mics, 1))).astype(np.float32)
    frame, prev = np.ascontiguousarray(S[:, hop:hop + n]), np.ascontiguousarray(S[:, :n])
    h = band_mod.design([band], n_taps=taps, fs=fs)
    filtered = band_np.band_filter(frame[None], h, hop, prev)[0, 0]
    orc = oracle_lib.Oracle(n, X, Y, 8)
    mics = np.arange(Mics, dtype=np.int32)
    d32 = np.float32(delays)
    return orc.mimo_lerp(frame, d32, mics), orc.mimo_lerp(filtered, d32, mics)


def within_3db(img):
    return int(np.count_nonzero(img >= img.max() * 10 ** -0.3))


def test_band_pass_finds_the_source_the_broadband_map_misses(native, oracle_lib):
    """This scene (seed 0, confirmed on the CPU before the seed was fixed): the raw lerp map peaks at (20, 11), 8 grid steps from the
    source at (12, 8), with all 943 cells within 3 dB of its maximum; the 3-8 kHz map of the same window, filtered by the restatement
    with the 64 stream samples before the window as history, peaks at (12, 8) with 186 cells within 3 dB."""
    raw, flt = scene_maps(oracle_lib, **SCENE)
    src = SCENE["src"]
    peak_raw = tuple(int(v) for v in np.unravel_index(np.argmax(raw), raw.shape))
    peak_flt = tuple(int(v) for v in np.unravel_index(np.argmax(flt), flt.shape))
    n_raw, n_flt = within_3db(raw), within_3db(flt)
    print("raw argmax %s, %d cells within 3 dB; filtered argmax %s, %d cells" % (peak_raw, n_raw, peak_flt, n_flt))
    assert peak_flt == src, (peak_flt, src)
    assert peak_raw != src, peak_raw
    assert 2 * n_flt <= n_raw, (n_flt, n_raw)
