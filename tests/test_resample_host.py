"""CPU: bf_resample_device without a device -- the restatement's own consistency (tests/resample_np.py: split calls, the closed-form
count and state against the definition's loop, the identity), the Kaiser design of audio_out.design_resampler (symmetry, DC gain,
tones through the restated converter), every refusal that sits before device bring-up, bf_resample_capacity, and rate_ratio and
AudioOut's host mirror of the state."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import resample_np as R
import util
from support import FAKE, lib_clearing as lib

RATIOS = [(2, 3, 4), (3, 2, 5), (7, 5, 8), (4000, 4069, 32)]


def _windows(rng, rows, n, hop, F):
    """A stream cut into F windows of n every `hop` samples (0: back to back), and the window before the first."""
    step = hop if hop > 0 else n
    S = util.wild(rng, (rows, step * F + n))
    frames = np.ascontiguousarray(np.stack([S[:, (f + 1) * step:(f + 1) * step + n] for f in range(F)]))
    return frames, np.ascontiguousarray(S[:, :n])


# ------------------------------------------------------------------ the restatement is consistent with itself

# (the call refuses a history longer than a window's share of the stream: 32 taps on a hop of 16)
@pytest.mark.parametrize("hop,L,M,T", [(hop, L, M, T) for hop in (0, 16, 33, 64) for L, M, T in RATIOS if T - 1 <= (hop or 64)])
def test_split_calls_equal_one_call(hop, L, M, T):
    n, F, F1, rows = 64, 5, 2, 3
    rng = np.random.default_rng([hop, L, M, T])
    x, prev = _windows(rng, rows, n, hop, F)
    h = util.wild(rng, (L, T))
    state = (1, L // 2)                     # the first output reads the history, for every T > 1 here
    whole = R.resample(x, h, L, M, state, hop, prev, gain=0.5)
    a = R.resample(x[:F1], h, L, M, state, hop, prev, gain=0.5)
    b = R.resample(x[F1:], h, L, M, a["state"], hop, x[F1 - 1], gain=0.5)       # the carried state and window
    assert a["count"] + b["count"] == whole["count"] and b["state"] == whole["state"] and whole["status"] == a["status"] == b["status"] == 0
    assert whole["count"] > 0 and a["count"] <= a["cap"] and whole["count"] <= whole["cap"]
    joined = np.concatenate([a["y"][:, :a["count"]], b["y"][:, :b["count"]]], axis=1)
    assert np.array_equal(util.bits(joined), util.bits(whole["y"][:, :whole["count"]]))
    joined = np.concatenate([a["pcm"][:a["count"]], b["pcm"][:b["count"]]], axis=0)
    assert joined.tobytes() == whole["pcm"][:whole["count"]].tobytes()
    assert np.array_equal(a["clipped"] + b["clipped"], whole["clipped"])
    assert not whole["y"][:, whole["count"]:].any() and not whole["pcm"][whole["count"]:].any()
    if T > 1:      # silence before the stream differs from the real history, and only where the history is read
        cold = R.resample(x, h, L, M, state, hop, None, gain=0.5)
        assert not np.array_equal(util.bits(cold["y"]), util.bits(whole["y"]))
        late = [k for k, (i, _) in enumerate(R.positions(state[0], state[1], F * (hop or n), L, M)) if i >= T - 1]
        assert np.array_equal(util.bits(cold["y"][:, late]), util.bits(whole["y"][:, late]))


def test_count_and_state_closed_form_against_the_loop():
    import audio_out
    for (L, M), S, o in itertools.product([(1, 1), (2, 3), (3, 2), (7, 5), (5, 1), (1, 4), (160, 441), (4000, 4069), (1, 200), (3, 192)],
                                          [1, 2, 63, 64, 100, 950], [0, 1, 5, 63, 64, 65, 200, 1000]):
        for phi in sorted({0, 1 % L, L // 2, L - 1}):
            pos = R.positions(o, phi, S, L, M)
            count, o2, phi2 = R.closed_form(o, phi, S, L, M)
            assert count == len(pos) and count <= R.capacity(S, L, M), (L, M, S, o, phi)
            a = phi + len(pos) * M              # the first output the loop did not emit is the next call's first
            assert (o2, phi2) == (o + a // L - S, a % L) and o2 >= 0 and 0 <= phi2 < L
            assert audio_out.advance_state(o, phi, S, L, M) == (count, o2, phi2)
            if o >= S:
                assert count == 0 and (o2, phi2) == (o - S, phi)
    # the sparse case: one output every 200 samples, windows of 64
    state, seen = (0, 0), []
    for _ in range(4):
        count, o, phi = R.closed_form(state[0], state[1], 64, 1, 200)
        assert count == len(R.positions(state[0], state[1], 64, 1, 200))
        state = (o, phi)
        seen.append((count, o))
    assert seen[:3] == [(1, 136), (0, 72), (0, 8)] and seen[3][0] == 1
    x = np.arange(1, 65, dtype=np.float32).reshape(1, 1, 64)
    one = np.ones((1, 1), np.float32)
    got = R.resample(x, one, 1, 200, (8, 0))
    assert got["count"] == 1 and got["cap"] == 1 and got["y"][0, 0] == 9.0 and got["state"] == (144, 0)
    assert R.resample(x, one, 1, 200, (72, 0))["count"] == 0


def test_identity_on_the_bits():
    rng = np.random.default_rng(3)
    x = util.wild(rng, (3, 2, 64))
    x[0, 0, :5] = [np.nan, np.inf, -np.inf, 1e-40, -1e-45]
    for hop in (0, 16, 64):
        got = R.resample(x, np.ones((1, 1), np.float32), 1, 1, (0, 0), hop)
        S = 3 * (hop or 64)
        assert got["count"] == got["cap"] == S and got["state"] == (0, 0)
        want = x[:, :, 64 - (hop or 64):].transpose(1, 0, 2).reshape(2, S)
        assert np.array_equal(util.bits(got["y"]), util.bits(want))
    # the one exception: the chain starts at +0.0f, and fmaf(1, -0, +0) is +0
    zero = R.resample(np.full((1, 1, 4), -0.0, np.float32), np.ones((1, 1), np.float32), 1, 1)
    assert np.array_equal(util.bits(zero["y"]), np.zeros((1, 4), np.uint32))


def test_corrupt_state_is_reported():
    x = np.ones((1, 2, 64), np.float32)
    for state in ((-1, 0), (0, 2), (0, -1)):
        got = R.resample(x, np.ones((2, 3), np.float32), 2, 3, state)
        assert got["status"] == 1 and got["count"] == 0 and got["state"] == state and not got["y"].any() and not got["pcm"].any()


def test_pcm_rounding():
    v = np.array([0.0, 1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 32767.5 / 32768, 32766.5 / 32768,
                  -32768.5 / 32768, -32769.0 / 32768, np.nan, np.inf, -np.inf, 3e38], dtype=np.float32)
    q, c = R.to_pcm(v)
    assert q.tolist() == [0, 32767, -32768, 0, 2, 2, 0, -2, 32767, 32766, -32768, -32768, 0, 32767, -32768, 32767]
    assert c.tolist() == [False, True, False, False, False, False, False, False, True, False, False, True, True, True, True, True]


# ------------------------------------------------------------------ the design

def test_design_symmetry_and_dc_gain(native):
    import audio_out
    for L, M, T in ((4000, 4069, 32), (3675, 4069, 32), (2, 3, 16), (3, 2, 16), (1, 1, 32), (160, 441, 24)):
        h = audio_out.design_resampler(L, M, T)
        assert h.dtype == np.float32 and h.shape == (L, T)
        g = h.T.reshape(-1)                                              # g[t * up + p] = h[p][t]
        assert np.array_equal(util.bits(g), util.bits(g[::-1]))                  # symmetric: linear phase, the delay is (Q - 1) / (2 up)
        # A phase's DC gain is the prototype's response at 0 plus its images at the multiples of the input rate, which lie in the stop
        # band: the pass-band ripple and two images of 80 dB each bound the error by 3e-4 for any design; the audio designs (rate
        # changes near 1 at 32 taps, whose images sit far down the stop band) keep it within 1e-4
        dc = np.abs(h.astype(np.float64).sum(axis=1) - 1.0).max()
        assert dc < (1e-4 if T == 32 else 3e-4), (L, M, T, dc)
    with pytest.raises(ValueError):
        audio_out.design_resampler(0, 1)
    with pytest.raises(ValueError):
        audio_out.design_resampler(2, 3, rolloff=1.5)


TONES = (440.0, 3000.0, 8000.0, 15000.0)


@pytest.mark.parametrize("rate_out", [48000, 44100])
def test_tones_keep_their_frequency(native, rate_out):
    """A tone of f Hz at 48828 Hz comes out as a tone of f Hz at rate_out: output k is the input at time k * down / up - delay input
    samples.  Bound: the design's 80 dB stop band and ripple less a 10 dB margin.  (A float64 run of this design gives 88-97 dB for
    48 kHz and 82-103 dB for 44.1 kHz over these tones; the float32 chain of the restatement, measured here, is printed.)"""
    import audio_out
    rate_in = 48828
    L, M = audio_out.rate_ratio(rate_out, rate_in)
    T, n = 32, 1280
    h = audio_out.design_resampler(L, M, T)
    delay = (L * T - 1) / (2.0 * L)
    s = np.arange(n, dtype=np.float64)
    x = np.stack([np.sin(2 * np.pi * f * s / rate_in) for f in TONES]).astype(np.float32)[None]      # [1, 4, n]: a flat stream, a tone per row
    got = R.resample(x, h, L, M)
    count = got["count"]
    assert count == R.capacity(n, L, M) and got["status"] == 0
    k = np.arange(count, dtype=np.float64)
    settled = k * M / L >= T                                             # outputs whose taps all lie in the stream
    assert settled.sum() > 1000
    for r, f in enumerate(TONES):
        ideal = np.sin(2 * np.pi * f * (k * M / L - delay) / rate_in)
        err = got["y"][r, :count].astype(np.float64) - ideal
        snr = 10 * np.log10(np.sum(ideal[settled] ** 2) / np.sum(err[settled] ** 2))
        y = got["y"][r, :count][settled].astype(np.float64)
        spec = np.abs(np.fft.rfft(y * np.hanning(y.size), 1 << 16))
        f_peak = np.argmax(spec) * rate_out / float(1 << 16)
        print("%d Hz -> %d Hz at %g Hz: SNR %.1f dB, spectral peak at %.1f Hz" % (rate_in, rate_out, f, snr, f_peak))
        assert abs(f_peak - f) < rate_out / float(y.size), (f, f_peak)   # within one bin of the unpadded transform
        assert snr >= 70.0, (rate_out, f, snr)


# ------------------------------------------------------------------ refusals before device bring-up


D_IN, D_TAPS, D_STATE, D_OUT, D_PCM, D_CLIP, D_COUNT = (FAKE + i * 0x100000 for i in range(7))
IN_BYTES = ((2 * 3 - 1) * 64 + 64) * 4      # of _call's default batch: first float to the last one read
CAP = 43                                    # ceil(2 * 32 * 2 / 3)
OUT_BYTES = (2 * 48 + CAP) * 4


def _call(lib, d_in=D_IN, rows=3, frames=2, n=64, in_stride=64, hop=32, d_prev=None, d_taps=D_TAPS, up=2, down=3, n_taps=4, d_state=D_STATE, gain=1.0,
          d_out=D_OUT, out_stride=48, d_pcm=D_PCM, d_clip=D_CLIP, d_count=D_COUNT):
    return lib.bf_resample_device(d_in, rows, frames, n, in_stride, hop, d_prev, d_taps, up, down, n_taps, d_state, gain, d_out, out_stride, d_pcm, d_clip,
                                  d_count, None)


W = "bf_resample_device: "
GAPS = " (the windows would leave gaps in the stream)"
HISTORY = "the filter needs n_taps - 1 = %d samples of history but a window adds %d to the stream (the history must be stream samples)"


@pytest.mark.parametrize("kw,text", [
    (dict(d_in=None), "d_in is null"),
    (dict(d_taps=None), "d_taps is null"),
    (dict(d_state=None), "d_state is null"),
    (dict(d_count=None), "d_count is null"),
    (dict(d_in=None, d_count=None, rows=0), "d_in is null"),
    (dict(d_out=None, d_pcm=None), "d_out and d_pcm are both null"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(rows=-2, frames=0), "rows = -2 < 1"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(n=0), "n = 0 < 1"),
    (dict(up=0), "up = 0 < 1"),
    (dict(down=0), "down = 0 < 1"),
    (dict(n_taps=0), "n_taps = 0 < 1"),
    (dict(up=16385), "up = 16385 > 16384"),
    (dict(n_taps=129), "n_taps = 129 > 128"),
    (dict(up=16384, n_taps=128), "up * n_taps = 2097152 > 1048576"),
    (dict(up=8193, n_taps=128), "up * n_taps = 1048704 > 1048576"),
    (dict(down=129), "down = 129 > 64 * up = 128"),
    (dict(up=1, down=65), "down = 65 > 64 * up = 64"),
    (dict(hop=-1), "hop = -1 < 0"),
    (dict(hop=65), "hop = 65 > n = 64" + GAPS),
    (dict(in_stride=63), "in_stride = 63 < n = 64"),
    (dict(n_taps=34), HISTORY % (33, 32)),
    (dict(n_taps=66, hop=0, out_stride=128), HISTORY % (65, 64)),
    (dict(frames=(1 << 24) + 1, hop=0, down=128), "frames * n = 1073741888 > 1073741823"),
    (dict(frames=(1 << 25), hop=32, down=128), "frames * hop = 1073741824 > 1073741823"),
    (dict(frames=1 << 23, hop=0, up=8, down=1), "cap = 4294967296 does not fit an int"),
    (dict(out_stride=42), "out_stride = 42 < cap = 43"),
    (dict(hop=0, out_stride=85), "out_stride = 85 < cap = 86"),
    (dict(gain=float("nan")), "gain = nan is not finite"),
    (dict(gain=float("inf")), "gain = inf is not finite"),
    (dict(gain=float("-inf")), "gain = -inf is not finite"),
    (dict(d_out=D_IN), "d_out overlaps d_in"),
    (dict(d_out=D_IN + IN_BYTES - 4), "d_out overlaps d_in"),
    (dict(d_in=D_OUT + OUT_BYTES - 4), "d_out overlaps d_in"),
    (dict(d_prev=D_OUT - 3 * 64 * 4 + 4), "d_out overlaps d_prev"),
    (dict(d_prev=D_OUT + OUT_BYTES - 4), "d_out overlaps d_prev"),
    (dict(d_taps=D_OUT + OUT_BYTES - 4), "d_out overlaps d_taps"),
    (dict(d_out=D_PCM + CAP * 3 * 2 - 2), "d_out overlaps d_pcm"),
    (dict(d_pcm=D_TAPS + 2 * 4 * 4 - 2), "d_pcm overlaps d_taps"),
    (dict(d_pcm=D_IN - CAP * 3 * 2 + 2), "d_pcm overlaps d_in"),
    (dict(d_clip=D_PCM + CAP * 3 * 2 - 2), "d_pcm overlaps d_clip"),
    (dict(d_clip=D_STATE + 12), "d_clip overlaps d_state"),
    (dict(d_clip=D_IN + 64), "d_clip overlaps d_in"),
    (dict(d_state=D_COUNT + 4), "d_state overlaps d_count"),
    (dict(d_state=D_COUNT - 12), "d_state overlaps d_count"),
    (dict(d_state=D_TAPS + 28), "d_state overlaps d_taps"),
    (dict(d_count=D_IN + IN_BYTES - 4), "d_count overlaps d_in"),
    (dict(d_count=D_OUT + OUT_BYTES - 4), "d_out overlaps d_count"),
    (dict(d_out=None, d_pcm=D_IN), "d_pcm overlaps d_in"),
])
def test_refusals(lib, kw, text):
    assert _call(lib, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(native, lib):
    """Ranges that only touch, either output alone, no meter, the limits themselves: all pass the argument checks, so without a GPU
    the one refusal left is the missing device (with one, fake pointers must not be launched: nothing is called)."""
    if native.gpu_available():
        return
    for kw in (dict(d_out=D_IN + IN_BYTES), dict(d_in=D_OUT + OUT_BYTES), dict(d_prev=D_OUT - 3 * 64 * 4), dict(d_state=D_COUNT - 16), dict(d_state=D_COUNT + 8),
               dict(d_clip=D_STATE + 16), dict(d_out=None), dict(d_pcm=None), dict(d_clip=None), dict(d_pcm=None, d_clip=None),
               dict(out_stride=43), dict(n_taps=33), dict(n_taps=65, hop=0, out_stride=128), dict(hop=64, out_stride=128), dict(down=128),
               dict(up=16384, n_taps=33, d_out=None, d_pcm=FAKE + 0x10000000, d_taps=FAKE + 0x20000000),      # a 2 MB table, 2 MB of PCM
               dict(in_stride=100)):
        assert _call(lib, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device"), (kw, lib.bf_last_error())
        lib.bf_clear_error()


def test_capacity(native):
    cap = native.lib.bf_resample_capacity
    for S, L, M in [(64, 2, 3), (64, 3, 2), (1, 1, 1), (0, 5, 7), (64, 1, 200), (128, 4000, 4069), (48828, 4000, 4069), (48828, 3675, 4069),
                    ((1 << 31) - 1, 16384, 1), (1 << 40, 16384, 3)]:
        assert cap(S, L, M) == R.capacity(S, L, M), (S, L, M)
    assert cap(48828, 4000, 4069) == 48000 and cap(48828, 3675, 4069) == 44100
    for bad in [(-1, 2, 3), (64, 0, 3), (64, 2, 0), (64, -1, 3), (64, 2, -3), (1 << 62, 16384, 1)]:
        assert cap(*bad) == -1, bad


# ------------------------------------------------------------------ rate_ratio and the host mirror

def test_rate_ratio_and_the_host_mirror(native):
    import audio_out
    from interface import config
    assert Fraction(config.SAMPLE_RATE) == 48828
    assert audio_out.rate_ratio(48000) == (4000, 4069)
    assert audio_out.rate_ratio(44100) == (3675, 4069)
    assert audio_out.rate_ratio(48000, 48828) == (4000, 4069) and audio_out.rate_ratio(48000.0, 48828.0) == (4000, 4069)
    assert audio_out.rate_ratio(16000, 48000) == (1, 3) and audio_out.rate_ratio(48000, 48000) == (1, 1)
    assert audio_out.rate_ratio(44100, Fraction(100000000, 2048)) == (14112, 15625)     # the divider's exact rate, as a Fraction
    assert audio_out.rate_ratio(Fraction(96000), 48000) == (2, 1)
    with pytest.raises(ValueError):
        audio_out.rate_ratio(0)
    # a stream of pushes: the mirror's integers are the restatement's state, call after call
    for (L, M), sizes in (((4000, 4069), [128] * 7 + [256, 128 * 190, 128]), ((3675, 4069), [128, 128, 640, 128]), ((1, 200), [64] * 8), ((3, 2), [1, 2, 3, 64])):
        mirror, state, total = (0, 0), (0, 0), 0
        for S in sizes:
            count, o, phi = audio_out.advance_state(mirror[0], mirror[1], S, L, M)
            assert count == len(R.positions(state[0], state[1], S, L, M))
            state = R.closed_form(state[0], state[1], S, L, M)[1:]
            mirror = (o, phi)
            assert mirror == state
            total += count
        assert total == len(R.positions(0, 0, sum(sizes), L, M))                           # and the calls together emit what one call would


def test_pipeline_has_audio_out(native):
    import inspect
    import pipeline

    class Pushed:
        def push(self, out):
            return ("audio", "pcm", out)
    assert list(inspect.signature(pipeline.FusedPipeline.audio_out).parameters) == ["self", "out", "ao"]
    assert pipeline.FusedPipeline.audio_out(None, "beams", Pushed()) == ("audio", "pcm", "beams")
