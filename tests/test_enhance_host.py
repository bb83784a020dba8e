"""CPU: bf_enhance_device without a device -- the symbols, bf_enhance_workspace, every refusal that sits before device bring-up, the
window designer of enhance.py, the frame bookkeeping against brute force, the restatement of tests/enhance_np.py itself (perfect
reconstruction at G = 1, split calls equal one call, its fmaf against libm's), and the acoustic figures of the README's tone scene."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import enhance_np as EN
from support import FAKE, lib_clearing as lib


# ------------------------------------------------------------------ symbols, workspace

def test_symbols_are_exported_and_bound(native):
    ws, dev = native.lib.bf_enhance_workspace, native.lib.bf_enhance_device
    assert ws.restype is C.c_longlong and ws.argtypes == [C.c_int, C.c_longlong, C.c_int, C.c_int]
    assert dev.restype is C.c_int and len(dev.argtypes) == 29
    assert [i for i, a in enumerate(dev.argtypes) if a is C.c_float] == [16, 17, 18, 19, 20]          # alpha, a_noise, g0, g1, g_min
    assert [i for i, a in enumerate(dev.argtypes) if a is C.c_void_p] == [0, 6, 7, 8, 9, 10, 11, 12, 15, 22, 23, 25, 26, 27, 28]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "beamformer_hip.h")).read()
    for text in ("long long bf_enhance_workspace(int rows, long long samples, int n_fft, int hop_s);",
                 "int bf_enhance_device(const float *d_in, int rows, int frames, int n, int in_stride, int hop,", "#define BF_ENHANCE_MAX_OVERLAP 8"):
        assert text in header


def test_workspace(native):
    ws = native.lib.bf_enhance_workspace
    for rows, samples, n_fft, hop_s in [(1, 1, 32, 32), (3, 120, 32, 4), (3, 120, 32, 16), (4, 128, 256, 128), (64, 24320, 256, 128), (1, 2500, 1024, 128),
                                        (2, 5, 4096, 512), (7, (2 ** 31 - 1) // 2, 4096, 4096), (65536, (2 ** 31 - 1) // 2, 4096, 512)]:
        want = 4 + rows * -(-samples // hop_s) * (4 * (n_fft // 2 + 1) + n_fft)
        assert ws(rows, samples, n_fft, hop_s) == EN.workspace(rows, samples, n_fft, hop_s) == want, (rows, samples, n_fft, hop_s)
    for bad in [(0, 64, 32, 16), (-1, 64, 32, 16), (1, 0, 32, 16), (1, -5, 32, 16), (1, (2 ** 31 - 1) // 2 + 1, 32, 16), (1, 64, 16, 16), (1, 64, 48, 16),
                (1, 64, 8192, 4096), (1, 64, 0, 1), (1, 64, 32, 0), (1, 64, 32, -16), (1, 64, 32, 5), (1, 64, 32, 64), (1, 64, 32, 2), (1, 64, 256, 16)]:
        assert ws(*bad) == EN.workspace(*bad) == -1, bad


# ------------------------------------------------------------------ refusals before device bring-up

D_IN, D_HIST, D_OLA, D_NOISE, D_PRIOR, D_STATE, D_WIN_A, D_WIN_S, D_GAIN_IN, D_WORK, D_OUT, D_POWER, D_GAIN, D_COUNT = (FAKE + i * 0x100000 for i in range(14))
# of _call's defaults: rows 3, frames 3 windows of 96 at hop 40 and stride 100 (S = 120), n_fft 32 at hop_s 16 (cap 8, 17 bins)
IN_BYTES = ((3 * 3 - 1) * 100 + 96) * 4
OUT_BYTES = ((3 - 1) * 120 + 120) * 4
CELL_BYTES = 3 * 8 * 17 * 4
WORK_BYTES = (4 + 3 * 8 * (4 * 17 + 32)) * 4
HIST_BYTES, OLA_BYTES, BIN_BYTES = 3 * 31 * 4, 3 * 32 * 4, 3 * 17 * 4


def _call(lib, d_in=D_IN, rows=3, frames=3, n=96, in_stride=100, hop=40, d_hist=D_HIST, d_ola=D_OLA, d_noise=D_NOISE, d_prior=D_PRIOR, d_state=D_STATE,
          d_win_a=D_WIN_A, d_win_s=D_WIN_S, n_fft=32, hop_s=16, d_gain_in=None, alpha=0.98, a_noise=0.9, g0=1.5, g1=5.0, g_min=0.1, n_init=8, d_work=D_WORK,
          d_out=D_OUT, out_stride=120, d_power_out=D_POWER, d_gain_out=D_GAIN, d_count=D_COUNT):
    return lib.bf_enhance_device(d_in, rows, frames, n, in_stride, hop, d_hist, d_ola, d_noise, d_prior, d_state, d_win_a, d_win_s, n_fft, hop_s, d_gain_in,
                                 alpha, a_noise, g0, g1, g_min, n_init, d_work, d_out, out_stride, d_power_out, d_gain_out, d_count, None)


W = "bf_enhance_device: "
POW2 = " is not a power of two in [32, 4096]"
NAN, INF = float("nan"), float("inf")


def _hop_s(hop_s, n_fft=32):
    return "hop_s = %d does not divide n_fft = %d into 1 .. 8 frames a sample" % (hop_s, n_fft)


REFUSALS = [
    (dict(d_in=None), "d_in is null"),
    (dict(d_hist=None), "d_hist is null"),
    (dict(d_ola=None), "d_ola is null"),
    (dict(d_state=None), "d_state is null"),
    (dict(d_win_a=None), "d_win_a is null"),
    (dict(d_win_s=None), "d_win_s is null"),
    (dict(d_work=None), "d_work is null"),
    (dict(d_out=None), "d_out is null"),
    (dict(d_count=None), "d_count is null"),
    (dict(d_noise=None), "d_noise is null"),
    (dict(d_prior=None), "d_prior is null"),
    (dict(d_hist=None, d_count=None, rows=0), "d_hist is null"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(frames=-3, n=0), "frames = -3 < 1"),
    (dict(n=0, hop=0), "n = 0 < 1"),
    (dict(hop=-1), "hop = -1 < 0"),
    (dict(hop=97), "hop = 97 > n = 96 (the windows would leave gaps in the stream)"),
    (dict(in_stride=95), "in_stride = 95 < n = 96"),
    (dict(n_fft=16, hop_s=16), "n_fft = 16" + POW2),
    (dict(n_fft=48), "n_fft = 48" + POW2),
    (dict(n_fft=0), "n_fft = 0" + POW2),
    (dict(n_fft=-32), "n_fft = -32" + POW2),
    (dict(n_fft=8192), "n_fft = 8192" + POW2),
    (dict(hop_s=0), "hop_s = 0 < 1"),
    (dict(hop_s=-16), "hop_s = -16 < 1"),
    (dict(hop_s=5), _hop_s(5)),
    (dict(hop_s=64), _hop_s(64)),
    (dict(hop_s=2), _hop_s(2)),
    (dict(n_fft=256, hop_s=16), _hop_s(16, 256)),
    (dict(frames=1 << 25, hop=40), "frames * hop = 1342177280 > 1073741823"),
    (dict(frames=1 << 24, hop=0, n=96), "frames * n = 1610612736 > 1073741823"),
    (dict(out_stride=119), "out_stride = 119 < S = 120"),
    (dict(hop=0, out_stride=287), "out_stride = 287 < S = 288"),
    (dict(alpha=1.0), "alpha = 1 >= 1"),
    (dict(alpha=-0.5), "alpha = -0.5 is not finite and >= 0"),
    (dict(alpha=NAN), "alpha = nan is not finite and >= 0"),
    (dict(a_noise=1.5), "a_noise = 1.5 >= 1"),
    (dict(a_noise=-1.0), "a_noise = -1 is not finite and >= 0"),
    (dict(a_noise=INF), "a_noise = inf is not finite and >= 0"),
    (dict(g0=-1.0), "g0 = -1 is not finite and >= 0"),
    (dict(g0=NAN), "g0 = nan is not finite and >= 0"),
    (dict(g1=INF), "g1 = inf is not finite"),
    (dict(g1=1.5), "g1 = 1.5 <= g0 = 1.5"),
    (dict(g1=1.0), "g1 = 1 <= g0 = 1.5"),
    (dict(g_min=-0.25), "g_min = -0.25 is not finite and >= 0"),
    (dict(g_min=1.5), "g_min = 1.5 > 1"),
    (dict(g_min=NAN), "g_min = nan is not finite and >= 0"),
    (dict(n_init=0), "n_init = 0 < 1"),
    (dict(d_out=D_IN + IN_BYTES - 4), "d_out overlaps d_in"),
    (dict(d_in=D_OUT + OUT_BYTES - 4), "d_out overlaps d_in"),
    (dict(d_work=D_OUT + OUT_BYTES - 4), "d_out overlaps d_work"),
    (dict(d_out=D_WORK + WORK_BYTES - 4), "d_out overlaps d_work"),
    (dict(d_power_out=D_OUT - CELL_BYTES + 4), "d_out overlaps d_power_out"),
    (dict(d_gain_out=D_OUT + OUT_BYTES - 4), "d_out overlaps d_gain_out"),
    (dict(d_hist=D_OUT - HIST_BYTES + 4), "d_out overlaps d_hist"),
    (dict(d_ola=D_OUT + 8), "d_out overlaps d_ola"),
    (dict(d_noise=D_OUT + OUT_BYTES - 4), "d_out overlaps d_noise"),
    (dict(d_prior=D_OUT - BIN_BYTES + 4), "d_out overlaps d_prior"),
    (dict(d_state=D_OUT - 12), "d_out overlaps d_state"),
    (dict(d_count=D_OUT + OUT_BYTES - 4), "d_out overlaps d_count"),
    (dict(d_win_a=D_OUT - 124), "d_out overlaps d_win_a"),
    (dict(d_win_s=D_OUT + OUT_BYTES - 4), "d_out overlaps d_win_s"),
    (dict(d_gain_in=D_OUT + OUT_BYTES - 4), "d_out overlaps d_gain_in"),
    (dict(d_power_out=D_WORK + WORK_BYTES - 4), "d_work overlaps d_power_out"),
    (dict(d_in=D_WORK + 16), "d_work overlaps d_in"),
    (dict(d_gain_out=D_POWER + CELL_BYTES - 4), "d_power_out overlaps d_gain_out"),
    (dict(d_gain_in=D_POWER - CELL_BYTES + 4), "d_power_out overlaps d_gain_in"),
    (dict(d_gain_in=D_GAIN), "d_gain_out overlaps d_gain_in"),
    (dict(d_ola=D_HIST + HIST_BYTES - 4), "d_hist overlaps d_ola"),
    (dict(d_in=D_HIST - IN_BYTES + 4), "d_hist overlaps d_in"),
    (dict(d_noise=D_OLA + OLA_BYTES - 4), "d_ola overlaps d_noise"),
    (dict(d_win_s=D_OLA + OLA_BYTES - 4), "d_ola overlaps d_win_s"),
    (dict(d_prior=D_NOISE + BIN_BYTES - 4), "d_noise overlaps d_prior"),
    (dict(d_state=D_PRIOR + BIN_BYTES - 4), "d_prior overlaps d_state"),
    (dict(d_count=D_STATE + 12), "d_state overlaps d_count"),
    (dict(d_state=D_COUNT + 4), "d_state overlaps d_count"),
    (dict(d_win_a=D_COUNT + 4), "d_count overlaps d_win_a"),
]


@pytest.mark.parametrize("kw,text", REFUSALS)
def test_refusals(lib, kw, text):
    assert _call(lib, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(native, lib):
    """Ranges that only touch, the optional arguments left out, the limits themselves, and with d_gain_in the recursion's parameters
    unchecked and its state optional: all pass the argument checks, so without a GPU the one refusal left is the missing device (with
    one, fake pointers must not be launched: nothing is called)."""
    if native.gpu_available():
        return
    for kw in (dict(), dict(d_out=D_IN + IN_BYTES), dict(d_in=D_OUT + OUT_BYTES), dict(d_work=D_OUT + OUT_BYTES), dict(d_power_out=None, d_gain_out=None),
               dict(d_gain_in=D_GAIN_IN), dict(d_gain_in=D_GAIN_IN, d_noise=None, d_prior=None), dict(d_gain_in=D_GAIN_IN, alpha=NAN, a_noise=2.0, g0=-1.0, g1=-2.0,
                                                                                                  g_min=7.0, n_init=0),
               dict(d_gain_in=D_GAIN_IN, d_noise=D_OUT, d_prior=D_OUT), dict(alpha=0.0, a_noise=0.0, g0=0.0, g_min=0.0), dict(g_min=1.0), dict(hop=0, out_stride=288),
               dict(hop=96, out_stride=288), dict(hop_s=32), dict(hop_s=4), dict(n_fft=4096, hop_s=512, d_work=FAKE + 0x10000000), dict(out_stride=1000),
               dict(in_stride=96), dict(frames=1, n=1, in_stride=1, hop=0, out_stride=1), dict(d_state=D_COUNT - 16), dict(d_state=D_COUNT + 8)):
        assert _call(lib, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device"), (kw, lib.bf_last_error())
        lib.bf_clear_error()


# ------------------------------------------------------------------ bookkeeping

def test_frame_bookkeeping_against_brute_force():
    """Walk the stream sample by sample: a frame ends whenever hop_s samples have passed since the last one."""
    for hop_s in (1, 4, 16, 128):
        for c in (range(hop_s) if hop_s <= 16 else (0, 1, 63, 127)):
            for S in (list(range(1, 3 * hop_s + 2)) if hop_s <= 16 else [1, 127, 128, 129, 255, 256, 300]) + [1000, 24320 // (129 - hop_s)]:
                since, ends = c, []
                for s in range(S):
                    since += 1
                    if since == hop_s:
                        ends.append(s)
                        since = 0
                count, c_new, cap = EN.advance(c, S, hop_s)
                assert (count, c_new) == (len(ends), since) and count <= cap == -(-S // hop_s), (hop_s, c, S)
                n_fft = 8 * hop_s
                assert [s + n_fft - 1 for s in EN.frame_starts(c, S, n_fft, hop_s)] == ends
                import enhance
                assert enhance.advance_frames(c, S, hop_s) == (count, c_new)
    assert EN.advance(0, 120, 32)[2] == 4 and EN.advance(31, 1, 32) == (1, 0, 1) and EN.advance(5, 3, 32) == (0, 8, 1)


def test_every_sample_is_covered_by_the_full_set_of_frames():
    for n_fft, hop_s, c in ((32, 4, 3), (32, 32, 0), (64, 16, 15), (256, 128, 1)):
        S = 5 * n_fft + 7
        cover = np.zeros(S + n_fft, int)                                 # index = position + n_fft
        for s in EN.frame_starts(c, S, n_fft, hop_s):
            assert -(n_fft - 1) <= s and s + n_fft <= S
            cover[s + n_fft:s + 2 * n_fft] += 1
        emitted = cover[n_fft - c:S]                                     # positions -c .. S - n_fft: every covering frame has ended
        assert (emitted == n_fft // hop_s).all() and (np.diff(cover[S:]) <= 0).all()


# ------------------------------------------------------------------ the windows

@pytest.mark.parametrize("kind", ["sqrt_hann", "hann"])
def test_design_cola(native, kind):
    import enhance
    for n_fft in (32, 256, 4096):
        for hop_s in (n_fft, n_fft // 2, n_fft // 4, n_fft // 8):
            wa, ws, dev = enhance.design_cola(n_fft, hop_s, kind)
            assert wa.dtype == ws.dtype == np.float32 and wa.shape == ws.shape == (n_fft,)
            total = (wa.astype(np.float64) * ws.astype(np.float64)).reshape(-1, hop_s).sum(axis=0)
            assert dev == np.abs(total - 1).max() and dev <= 4 * EN.EPS, (n_fft, hop_s, dev)
            if hop_s == n_fft:
                assert (wa == 1).all() and (ws == 1).all() and dev == 0.0
            elif kind == "sqrt_hann":
                assert np.allclose(wa.astype(np.float64) ** 2, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft), atol=1e-6)
                assert np.allclose(ws, wa / (n_fft / hop_s / 2), atol=1e-6)
    for bad in ((16, 8), (48, 16), (8192, 4096), (32, 0), (32, 5), (32, 64), (256, 16)):
        with pytest.raises(ValueError):
            enhance.design_cola(*bad)
    with pytest.raises(ValueError):
        enhance.design_cola(32, 16, "blackman")


def test_pipeline_has_enhance(native):
    import pipeline

    class En:
        def push(self, out):
            return ("pushed", out)
    assert pipeline.FusedPipeline.enhance(None, "beams", En()) == ("pushed", "beams")


# ------------------------------------------------------------------ the restatement itself

def test_fmaf_rounds_once():
    """Against libm's fmaf, on operands made to sit on float32 ties of the exact sum."""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))).astype(np.float32)
    a[:4] = np.float32(1 + 2.0 ** -12)
    b[:4] = np.float32(1 + 2.0 ** -12)
    c[:4] = np.float32([-(1 + 2.0 ** -11), 2.0 ** -60, -2.0 ** -60, 1.0])     # an exact cancellation, and a tie broken by a far-away addend
    a[4:8], b[4:8], c[4:8] = np.float32(3.0), np.float32(2.0 ** -24), np.float32([1.0, -1.0, 1 + 2.0 ** -23, 2.0])
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    got = EN.fmaf(a, b, c)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    print("fmaf: %d of %d operands round differently when rounded twice" % (np.count_nonzero(twice != want), want.size))


@pytest.mark.parametrize("n_fft,div", [(32, 1), (32, 2), (32, 4), (32, 8), (256, 2), (256, 8), (1024, 4)])
def test_unit_gains_return_the_input_delayed(native, n_fft, div):
    import enhance
    hop_s = n_fft // div
    wa, ws, dev = enhance.design_cola(n_fft, hop_s)
    rng = np.random.default_rng([n_fft, div])
    S = 5 * n_fft + 13
    x = (rng.standard_normal((2, S)) * np.exp2(rng.integers(-3, 4, (2, 1)))).astype(np.float32)
    zeros = lambda n: np.zeros((2, n), np.float32)
    count, _, cap = EN.advance(0, S, hop_s)
    got = EN.enhance(x, zeros(n_fft - 1), zeros(n_fft), 0, wa, ws, hop_s, G=np.ones((2, cap, n_fft // 2 + 1)))
    assert got["count"] == count and np.abs(got["out"][:, :n_fft]).max() < 1e-12
    delayed = np.concatenate([zeros(n_fft), x], axis=1)[:, :S]
    # the restatement's own float64 arithmetic, and the one float32 rounding of u = win_a * x: EPS |x| per covering frame
    err = np.abs(got["out"] - delayed)
    allowed = EN.cola_term(delayed, n_fft, dev) + div * EN.EPS * np.abs(delayed) * 1.01 + 1e-12
    assert (err <= allowed).all(), (err / allowed).max()
    print("n_fft %d hop_s %d: COLA deviation %.3g, worst |y - x| / allowed %.3f" % (n_fft, hop_s, dev, (err / allowed).max()))


def test_restatement_split_calls_equal_one_call(native):
    import enhance
    n_fft, hop_s = 32, 8
    wa, ws, _ = enhance.design_cola(n_fft, hop_s)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 200)).astype(np.float32)
    par = dict(alpha=0.9, a_noise=0.8, g0=1.5, g1=5.0, g_min=0.05, n_init=3)
    zeros = lambda n: np.zeros((2, n), np.float32)
    one = EN.enhance(x, zeros(31), zeros(32), 0, wa, ws, hop_s, track=dict(lam=zeros(17), prior=zeros(17), seen=0, **par), dtype=np.float32)
    st = dict(hist=zeros(31), ola=zeros(32), c=0, lam=zeros(17), prior=zeros(17), seen=0)
    outs, counts = [], []
    for a, b in ((0, 13), (13, 14), (14, 117), (117, 200)):
        r = EN.enhance(x[:, a:b], st["hist"], st["ola"], st["c"], wa, ws, hop_s, track=dict(lam=st["lam"], prior=st["prior"], seen=st["seen"], **par), dtype=np.float32)
        st = {k: r[k] for k in st}
        outs.append(r["out"])
        counts.append(r["count"])
    assert sum(counts) == one["count"] == 25 and st["c"] == one["c"] == 0 and st["seen"] == one["seen"] == 3
    assert np.allclose(np.concatenate(outs, axis=1), one["out"], rtol=0, atol=1e-12) and np.allclose(st["ola"], one["ola"], rtol=0, atol=1e-12)
    assert st["lam"].tobytes() == one["lam"].tobytes() and st["prior"].tobytes() == one["prior"].tobytes() and st["hist"].tobytes() == one["hist"].tobytes()


def test_gains_recursion_properties():
    """The first n_init frames average P; a steady P is its own noise and gets g_min; a jump far above the noise freezes the tracker and
    passes; a non-finite P leaves the bin's state alone; alpha = 0 against an overflowing prior / den stays finite."""
    P = np.full((1, 12, 3), 2.0, np.float32)
    P[0, :, 1] = np.arange(1, 13)
    G, lam, prior, seen = EN.gains(P[:, :4], np.zeros((1, 3)), np.zeros((1, 3)), 0, n_init=4)
    assert seen == 4 and lam[0].tolist() == [2.0, 2.5, 2.0] and (G[0, :, 0] >= np.float32(0.1)).all()
    G2, lam2, _, seen2 = EN.gains(P[:, 4:], lam, prior, seen, n_init=4)
    assert seen2 == 4 and lam2[0, 0] == 2.0 and G2[0, -1, 0] == np.float32(0.1)
    loud = np.full((1, 1, 3), 2000.0, np.float32)
    G3, lam3, _, _ = EN.gains(loud, lam2, np.zeros((1, 3)), 4, n_init=4)
    assert lam3.tobytes() == lam2.tobytes() and (G3 > 0.8).all()
    bad = np.array([[[np.nan, np.inf, 2.0]]], np.float32)
    G4, lam4, prior4, _ = EN.gains(bad, lam2, prior, 4, n_init=4)
    assert np.isnan(G4[0, 0, :2]).all() and np.isfinite(G4[0, 0, 2]) and lam4[0, :2].tobytes() == lam2[0, :2].tobytes() and prior4[0, :2].tobytes() == prior[0, :2].tobytes()
    G5, lam5, prior5, _ = EN.gains(np.full((1, 2, 1), 1e-30, np.float32), np.zeros((1, 1)), np.full((1, 1), 3e38), 9, alpha=0.0)
    assert np.isfinite(G5).all() and np.isfinite(lam5).all() and np.isfinite(prior5).all()


# ------------------------------------------------------------------ the acoustic figure

def test_the_tone_scene_improves(native):
    """Three gated tones in white noise at 6.6 dB (enhance_np.SCENE), the defaults of enhance.Enhancer, the restatement in float64.
    Measured, seeds 0-3: 6.73-6.84 dB in, 18.96-19.28 dB out (a spread of 0.32 dB, the slack of the device's figure in test_enhance.py),
    -19.3 to -20.3 dB of distortion, tracked / true noise power 0.68-0.73 (0.98-1.08 with g1 = 50); the README quotes them."""
    figs = [EN.host_scene(seed) for seed in range(4)]
    wide = [EN.host_scene(seed, g0=1.5, g1=50.0) for seed in range(4)]
    for seed, (f, w) in enumerate(zip(figs, wide)):
        print("seed %d: SNR over the active stretches %.2f dB in, %.2f dB out; distortion of the tones %.2f dB; tracked / true noise power %.3f (%.3f with g1 = 50)"
              % (seed, f["snr_in"], f["snr_out"], f["distortion"], f["noise_ratio"], w["noise_ratio"]))
        assert f["snr_out"] > f["snr_in"], f
    out = [f["snr_out"] for f in figs]
    print("spread of the SNR behind the filter over the seeds: %.2f dB" % (max(out) - min(out)))
