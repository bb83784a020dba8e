"""CPU: bf_postfilter_device without a device -- the symbols, bf_postfilter_workspace, every refusal that sits before device bring-up, the
restatement of tests/postfilter_np.py itself (the pair identity, the recursion's rules, split calls equal one call, the frame grid against
the Enhancer's), and the acoustic figures of the README's scenes."""
import ctypes as C
import os

import numpy as np
import pytest

import enhance_np as EN
import postfilter_np as PN
from support import FAKE, entry, lib_clearing as lib


# ------------------------------------------------------------------ symbols, workspace

def test_symbols_are_exported_and_bound(native):
    ws, dev = native.lib.bf_postfilter_workspace, native.lib.bf_postfilter_device
    assert ws.restype is C.c_longlong and ws.argtypes == [C.c_int, C.c_longlong, C.c_int, C.c_int]
    assert dev.restype is C.c_int and len(dev.argtypes) == 31
    assert [i for i, a in enumerate(dev.argtypes) if a is C.c_float] == [21, 22]                       # beta, g_min
    assert [i for i, a in enumerate(dev.argtypes) if a is C.c_void_p] == [0, 7, 9, 12, 13, 14, 15, 16, 23, 24, 25, 26, 27, 28, 29, 30]
    assert dev.argtypes[5] is native.IP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "beamformer_hip.h")).read()
    for text in ("long long bf_postfilter_workspace(int slots, long long samples, int n_fft, int hop_s);",
                 "int bf_postfilter_device(const float *d_signals, int m_total, int frames, int n_samples, int hop,", "#define BF_POSTFILTER_MAX_SLOTS 8"):
        assert text in header
    import __graft_entry__ as ge
    assert "postfilter.hip" in ge.SOURCES


def test_workspace(native):
    ws = native.lib.bf_postfilter_workspace
    for slots, samples, n_fft, hop_s in [(1, 1, 32, 32), (3, 120, 32, 4), (3, 120, 32, 16), (4, 128, 256, 128), (8, 24320, 256, 128), (1, 2500, 1024, 128),
                                         (2, 5, 4096, 512), (7, (2 ** 31 - 1) // 2, 4096, 4096), (8, (2 ** 31 - 1) // 2, 32, 4)]:
        want = 16 + slots * -(-samples // hop_s) * (1 + 2 * (n_fft // 2 + 1))
        assert ws(slots, samples, n_fft, hop_s) == PN.workspace(slots, samples, n_fft, hop_s) == want, (slots, samples, n_fft, hop_s)
    for bad in [(0, 64, 32, 16), (-1, 64, 32, 16), (9, 64, 32, 16), (1, 0, 32, 16), (1, -5, 32, 16), (1, (2 ** 31 - 1) // 2 + 1, 32, 16), (1, 64, 16, 16),
                (1, 64, 48, 16), (1, 64, 8192, 4096), (1, 64, 0, 1), (1, 64, 32, 0), (1, 64, 32, -16), (1, 64, 32, 5), (1, 64, 32, 64), (1, 64, 32, 2), (1, 64, 256, 16)]:
        assert ws(*bad) == PN.workspace(*bad) == -1, bad


# ------------------------------------------------------------------ refusals before device bring-up

(D_SIG, D_TAU, D_OFF, D_HIST, D_NUM, D_DEN, D_STATE, D_WIN, D_WORK, D_STEER, D_GAINS, D_NUM_OUT, D_DEN_OUT, D_STATUS, D_COUNT) = (FAKE + i * 0x100000 for i in range(15))
MICS = np.array([3, 0, 5, 1], dtype=np.int32)
MICS_PTR = MICS.ctypes.data_as(C.POINTER(C.c_int))
# of the defaults: 3 windows of 96 at hop 40 in frames of 6 rows (S = 120), 4 microphones, 5 directions, 3 slots, n_fft 32 at hop_s 16 (cap 8, 17 bins),
# lag 5 (H = 36)
SIG_BYTES = 3 * 6 * 96 * 4
TAU_BYTES, OFF_BYTES, WIN_BYTES = 5 * 4 * 8, 3 * 4, 32 * 4
HIST_BYTES, BIN_BYTES, STATE_BYTES = 4 * 36 * 4, 3 * 17 * 4, 5 * 4
WORK_BYTES = (16 + 3 * 8 * (1 + 2 * 17)) * 4
STEER_BYTES, CELL_BYTES, STATUS_BYTES = 3 * 4 * 17 * 2 * 4, 3 * 8 * 17 * 4, 3 * 4

_call = entry("bf_postfilter_device", d_signals=D_SIG, m_total=6, frames=3, n_samples=96, hop=40, adaptive_array=MICS_PTR, n=4, d_tau=D_TAU, dirs=5, d_offsets=D_OFF,
              slots=3, offset_per_dir=4, d_hist=D_HIST, d_num=D_NUM, d_den=D_DEN, d_state=D_STATE, d_window=D_WIN, n_fft=32, hop_s=16, lag=5, den_mode=0, beta=0.8,
              g_min=0.1, d_work=D_WORK, d_steer=D_STEER, d_gains=D_GAINS, d_num_out=D_NUM_OUT, d_den_out=D_DEN_OUT, d_status=D_STATUS, d_count=D_COUNT)

W = "bf_postfilter_device: "
POW2 = " is not a power of two in [32, 4096]"
NAN, INF = float("nan"), float("inf")
BAD_ROW = np.array([3, 0, 6, 1], dtype=np.int32)
NEG_ROW = np.array([3, -1, 5, 1], dtype=np.int32)
MANY = np.arange(257, dtype=np.int32)


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _hop_s(hop_s, n_fft=32):
    return "hop_s = %d does not divide n_fft = %d into 1 .. 8 frames a sample" % (hop_s, n_fft)


REFUSALS = [
    (dict(d_signals=None), "d_signals is null"),
    (dict(adaptive_array=None), "adaptive_array is null"),
    (dict(d_tau=None), "d_tau is null"),
    (dict(d_offsets=None), "d_offsets is null"),
    (dict(d_hist=None), "d_hist is null"),
    (dict(d_num=None), "d_num is null"),
    (dict(d_den=None), "d_den is null"),
    (dict(d_state=None), "d_state is null"),
    (dict(d_window=None), "d_window is null"),
    (dict(d_work=None), "d_work is null"),
    (dict(d_steer=None), "d_steer is null"),
    (dict(d_gains=None), "d_gains is null"),
    (dict(d_status=None), "d_status is null"),
    (dict(d_count=None), "d_count is null"),
    (dict(d_hist=None, d_count=None, frames=0), "d_hist is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(frames=-3, n_samples=0), "frames = -3 < 1"),
    (dict(n_samples=0, hop=0), "n_samples = 0 < 1"),
    (dict(hop=-1), "hop = -1 < 0"),
    (dict(hop=97), "hop = 97 > n_samples = 96 (the windows would leave gaps in the stream)"),
    (dict(n=1), "n = 1 < 2"),
    (dict(n=0), "n = 0 < 2"),
    (dict(n=257, adaptive_array=_ptr(MANY), m_total=300), "n = 257 > 256"),
    (dict(adaptive_array=_ptr(BAD_ROW)), "adaptive_array[2] = 6 is not a row of frames with m_total = 6 rows"),
    (dict(adaptive_array=_ptr(NEG_ROW)), "adaptive_array[1] = -1 is not a row of frames with m_total = 6 rows"),
    (dict(m_total=5), "adaptive_array[2] = 5 is not a row of frames with m_total = 5 rows"),
    (dict(m_total=0), "adaptive_array[0] = 3 is not a row of frames with m_total = 0 rows"),
    (dict(slots=0), "slots = 0 < 1"),
    (dict(slots=9), "slots = 9 > 8"),
    (dict(dirs=0), "dirs = 0 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(offset_per_dir=-4), "offset_per_dir = -4 < 1"),
    (dict(n_fft=16, hop_s=16), "n_fft = 16" + POW2),
    (dict(n_fft=48), "n_fft = 48" + POW2),
    (dict(n_fft=0), "n_fft = 0" + POW2),
    (dict(n_fft=8192), "n_fft = 8192" + POW2),
    (dict(hop_s=0), "hop_s = 0 < 1"),
    (dict(hop_s=-16), "hop_s = -16 < 1"),
    (dict(hop_s=5), _hop_s(5)),
    (dict(hop_s=64), _hop_s(64)),
    (dict(hop_s=2), _hop_s(2)),
    (dict(n_fft=256, hop_s=16), _hop_s(16, 256)),
    (dict(lag=-1), "lag = -1 < 0"),
    (dict(lag=33), "lag = 33 > 32"),
    (dict(den_mode=2), "den_mode = 2 is not 0 (the microphones' mean power) or 1 (the beam's power)"),
    (dict(den_mode=-1), "den_mode = -1 is not 0 (the microphones' mean power) or 1 (the beam's power)"),
    (dict(beta=1.0), "beta = 1 >= 1"),
    (dict(beta=-0.5), "beta = -0.5 is not finite and >= 0"),
    (dict(beta=NAN), "beta = nan is not finite and >= 0"),
    (dict(beta=INF), "beta = inf is not finite and >= 0"),
    (dict(g_min=-0.25), "g_min = -0.25 is not finite and >= 0"),
    (dict(g_min=1.5), "g_min = 1.5 > 1"),
    (dict(g_min=NAN), "g_min = nan is not finite and >= 0"),
    (dict(frames=1 << 25, hop=40), "frames * hop = 1342177280 > 1073741823"),
    (dict(frames=1 << 24, hop=0), "frames * n_samples = 1610612736 > 1073741823"),
    (dict(d_num_out=D_GAINS + CELL_BYTES - 4), "d_gains overlaps d_num_out"),
    (dict(d_den_out=D_GAINS - CELL_BYTES + 4), "d_gains overlaps d_den_out"),
    (dict(d_steer=D_GAINS + 8), "d_gains overlaps d_steer"),
    (dict(d_work=D_GAINS + CELL_BYTES - 4), "d_gains overlaps d_work"),
    (dict(d_gains=D_WORK + WORK_BYTES - 4), "d_gains overlaps d_work"),
    (dict(d_status=D_GAINS + 4), "d_gains overlaps d_status"),
    (dict(d_count=D_GAINS + CELL_BYTES - 4), "d_gains overlaps d_count"),
    (dict(d_hist=D_GAINS - HIST_BYTES + 4), "d_gains overlaps d_hist"),
    (dict(d_num=D_GAINS + CELL_BYTES - 4), "d_gains overlaps d_num"),
    (dict(d_den=D_GAINS - BIN_BYTES + 4), "d_gains overlaps d_den"),
    (dict(d_state=D_GAINS - STATE_BYTES + 4), "d_gains overlaps d_state"),
    (dict(d_signals=D_GAINS - SIG_BYTES + 4), "d_gains overlaps d_signals"),
    (dict(d_tau=D_GAINS + CELL_BYTES - 4), "d_gains overlaps d_tau"),
    (dict(d_offsets=D_GAINS - OFF_BYTES + 4), "d_gains overlaps d_offsets"),
    (dict(d_window=D_GAINS - WIN_BYTES + 4), "d_gains overlaps d_window"),
    (dict(d_den_out=D_NUM_OUT + CELL_BYTES - 4), "d_num_out overlaps d_den_out"),
    (dict(d_signals=D_DEN_OUT + 16), "d_den_out overlaps d_signals"),
    (dict(d_work=D_STEER + STEER_BYTES - 4), "d_steer overlaps d_work"),
    (dict(d_tau=D_STEER - TAU_BYTES + 4), "d_steer overlaps d_tau"),
    (dict(d_signals=D_WORK + WORK_BYTES - 4), "d_work overlaps d_signals"),
    (dict(d_count=D_STATUS + STATUS_BYTES - 4), "d_status overlaps d_count"),
    (dict(d_offsets=D_STATUS), "d_status overlaps d_offsets"),
    (dict(d_state=D_COUNT + 4), "d_count overlaps d_state"),
    (dict(d_num=D_HIST + HIST_BYTES - 4), "d_hist overlaps d_num"),
    (dict(d_signals=D_HIST - SIG_BYTES + 4), "d_hist overlaps d_signals"),
    (dict(d_den=D_NUM + BIN_BYTES - 4), "d_num overlaps d_den"),
    (dict(d_state=D_DEN + BIN_BYTES - 4), "d_den overlaps d_state"),
    (dict(d_window=D_STATE + STATE_BYTES - 4), "d_state overlaps d_window"),
]


@pytest.mark.parametrize("kw,text", REFUSALS)
def test_refusals(native, lib, kw, text):
    assert _call(native, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(native, lib):
    """Ranges that only touch, the observables left out, the limits themselves: all pass the argument checks, so without a GPU the one
    refusal left is the missing device (with one, fake pointers must not be launched: nothing is called)."""
    if native.gpu_available():
        return
    for kw in (dict(), dict(d_num_out=None, d_den_out=None), dict(d_num_out=D_GAINS + CELL_BYTES), dict(d_signals=D_GAINS + CELL_BYTES), dict(d_work=D_STEER + STEER_BYTES),
               dict(d_state=D_COUNT + 8), dict(d_state=D_COUNT - STATE_BYTES), dict(beta=0.0, g_min=0.0), dict(g_min=1.0), dict(den_mode=1), dict(lag=0), dict(lag=32),
               dict(hop=0), dict(hop=96), dict(hop_s=32), dict(hop_s=4), dict(slots=8, d_work=FAKE + 0x10000000), dict(slots=1), dict(dirs=1, offset_per_dir=1),
               dict(n=2), dict(n_fft=4096, hop_s=512, lag=4096, d_work=FAKE + 0x10000000, d_steer=FAKE + 0x20000000, d_hist=FAKE + 0x30000000),
               dict(n=256, adaptive_array=_ptr(MANY), m_total=256, d_steer=FAKE + 0x20000000, d_hist=FAKE + 0x30000000)):
        assert _call(native, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device"), (kw, lib.bf_last_error())
        lib.bf_clear_error()


# ------------------------------------------------------------------ the restatement itself

def test_the_pair_sum_needs_no_pair_loop():
    """(|sum Z|^2 - sum |Z|^2) / (n (n - 1)) is the mean over the n (n - 1) / 2 pairs of Re(Z_i conj Z_j)."""
    rng = np.random.default_rng(2)
    for n in (2, 3, 7, 64):
        X = rng.standard_normal((n, 3, 17)) + 1j * rng.standard_normal((n, 3, 17))
        ang = rng.uniform(0, 2 * np.pi, (2, n, 17))
        a = np.stack([np.cos(ang), -np.sin(ang)], axis=-1).astype(np.float32)
        r = PN.raw(X, a, 0)
        for b in range(2):
            want = PN.pair_mean(r["Z"][b])
            Zb = r["Z"][b]
            exact = (np.abs(Zb.sum(axis=0)) ** 2 - (np.abs(Zb) ** 2).sum(axis=0)) / (n * (n - 1))
            assert np.allclose(exact, want, rtol=0, atol=1e-12 * np.abs(r["Q"]).max()), n
            # the definition's Q sums |X|^2, not |a X|^2: the rounded steering has |a|^2 within sqrt 2 * 2^-24 of 1 (each component
            # within 2^-25), so num is the pair mean within 2 EPS Q / (n (n - 1))
            assert (np.abs(r["num"][b] - want) <= 2 * PN.EPS * r["Q"] / (n * (n - 1)) + 1e-12).all(), n
        # coherent microphones: num = den = the common power, in both modes; incoherent: num cancels against Q
        X1 = np.broadcast_to(X[:1], X.shape)
        ones = np.zeros((1, n, 17, 2), np.float32)
        ones[..., 0] = 1.0
        for mode in (0, 1):
            c = PN.raw(X1, ones, mode)
            assert np.allclose(c["num"], c["den"]) and np.allclose(c["den"][0], np.abs(X[0]) ** 2)


def test_frame_grid_is_the_enhancers():
    """lag = 0: the Enhancer's frames; a lag moves every frame that many samples back, and the history grows by it."""
    for n_fft, hop_s, c, S in ((32, 16, 0, 120), (32, 4, 3, 50), (256, 128, 127, 1), (64, 64, 5, 300)):
        assert PN.frame_starts(c, S, n_fft, hop_s, 0) == EN.frame_starts(c, S, n_fft, hop_s)
        for lag in (1, 5, n_fft):
            starts = PN.frame_starts(c, S, n_fft, hop_s, lag)
            assert starts == [s - lag for s in EN.frame_starts(c, S, n_fft, hop_s)]
            assert all(-(n_fft - 1 + lag) <= s and s + n_fft <= S - lag for s in starts)


def test_slot_rule():
    assert PN.slot_directions([0, 8, -1, 6, 20, 16, -4], 4, 5) == [0, 2, -1, -1, -1, 4, -1]


def _random_call(rng, n, S, n_fft, lag):
    scale = np.exp2(rng.integers(-3, 4, (n, 1)).astype(np.float64))
    return (rng.standard_normal((n, S)) * scale).astype(np.float32)


def test_restatement_split_calls_equal_one_call(native):
    import enhance
    n_fft, hop_s, lag, n = 32, 8, 5, 5
    win = enhance.design_cola(n_fft, hop_s)[0]
    rng = np.random.default_rng(3)
    tau = rng.uniform(0, 6, (4, n))
    x = _random_call(rng, n, 200, n_fft, lag)
    K = n_fft // 2 + 1
    fresh = lambda: dict(hist=np.zeros((n, n_fft - 1 + lag), np.float32), c=0, N=np.zeros((2, K), np.float32), D=np.zeros((2, K), np.float32), seen=[0, 0])
    run = lambda xs, st, offs: PN.postfilter(xs, st["hist"], st["c"], win, hop_s, lag, tau, offs, 3, 0, 0.7, 0.05, st["N"], st["D"], st["seen"], dtype=np.float32)
    one = run(x, fresh(), [3, 9])
    st, Gs = fresh(), []
    for a, b in ((0, 13), (13, 14), (14, 117), (117, 200)):
        r = run(x[:, a:b], st, [3, 9])
        st = {k: r[k] for k in st}
        Gs.append(r["G"])
    assert np.concatenate(Gs, axis=1).tobytes() == one["G"].tobytes() and one["count"] == 25
    assert st["N"].tobytes() == one["N"].tobytes() and st["D"].tobytes() == one["D"].tobytes() and st["hist"].tobytes() == one["hist"].tobytes()
    assert st["seen"] == one["seen"] == [1, 1] and st["c"] == one["c"] == 0


def test_recursion_rules():
    """The first finite frame is taken as it is; beta = 0 follows the frames; a frame with one non-finite bin is NaN in every bin and
    leaves the state; D = 0 gives g_min; a negative N gives g_min; a slot that is no source gets zeros, keeps N and D and loses `seen`."""
    num = np.array([[[1.0, 2.0], [3.0, 2.0], [np.nan, 1.0], [0.5, -4.0]]], np.float32)
    den = np.array([[[2.0, 2.0], [4.0, 0.0], [1.0, 1.0], [1.0, 8.0]]], np.float32)
    zero = np.zeros((1, 2), np.float32)
    G, N, D, seen = PN.recursion(num[:, :1], den[:, :1], zero + 9, zero + 9, [0], [True], 0.5, 0.1)
    assert G[0, 0].tolist() == [0.5, 1.0] and N[0].tolist() == [1.0, 2.0] and seen == [1]
    G, N, D, seen = PN.recursion(num[:, 1:], den[:, 1:], N, D, seen, [True], 0.5, 0.1)
    assert N[0].tolist() == [1.25, -1.0] and D[0].tolist() == [2.0, 4.5]            # bin 0: (1 + 3) / 2 = 2, then (2 + 0.5) / 2; the NaN frame skipped
    assert np.isnan(G[0, 1]).all() and G[0, 0, 0] == np.float32(2.0) / np.float32(3.0) and G[0, 2, 1] == np.float32(0.1)
    G0, N0, D0, _ = PN.recursion(num[:, :2], den[:, :2], zero, zero, [1], [True], 0.0, 0.1)
    assert N0[0].tolist() == [3.0, 2.0] and D0[0].tolist() == [4.0, 0.0] and G0[0, 1].tolist() == [0.75, np.float32(0.1)]
    G, N2, D2, seen = PN.recursion(num, den, N, D, [1], [False], 0.5, 0.1)
    assert not G.any() and seen == [0] and N2.tobytes() == N.tobytes() and D2.tobytes() == D.tobytes()
    bad = np.full((1, 3, 2), np.inf, np.float32)
    G, N3, D3, seen = PN.recursion(bad, bad, zero + 7, zero + 7, [0], [True], 0.5, 0.1)
    assert np.isnan(G).all() and seen == [0] and (N3 == 7).all() and (D3 == 7).all()


def test_zero_rows_give_the_floor(native):
    import enhance
    win = enhance.design_cola(32, 16)[0]
    tau = np.zeros((1, 3))
    r = PN.postfilter(np.zeros((3, 64), np.float32), np.zeros((3, 31), np.float32), 0, win, 16, 0, tau, [0], 1, 0, 0.8, 0.1, np.zeros((1, 17)), np.zeros((1, 17)),
                      [0], dtype=np.float32)
    assert (r["G"] == np.float32(0.1)).all() and not r["N"].any() and not r["D"].any() and r["seen"] == [1]


def test_pipeline_and_class(native):
    import pipeline
    import postfilter

    class Pf:
        def push(self, en, frames, out, offsets):
            return ("pushed", en, frames, out, offsets)
    assert pipeline.FusedPipeline.postfilter(None, "frames", "beams", "offsets", Pf(), "en") == ("pushed", "en", "frames", "beams", "offsets")
    assert postfilter.MAX_SLOTS == PN.MAX_SLOTS and postfilter.DEN_MODES == {"mics": 0, "beam": 1}
    assert callable(postfilter.SpatialPostFilter.for_listener) and callable(postfilter.SpatialPostFilter.gains)


# ------------------------------------------------------------------ the acoustic figures

def _row(name, f):
    extra = "".join(", %s %.1f dB" % (k, f[k]) for k in ("interferer", "noise") if k in f)
    return "%-44s SNR %.1f -> %.1f dB, tone distortion %.1f dB%s" % (name, f["snr_in"], f["snr_out"], f["distortion"], extra)


def test_the_scene_table(native):
    """The README's table: the scenes through the restatement in float64 (zero history: the edge frames are in).  Measured: microphone
    denominator, noise 0.2, seeds 0-3: 24.8 -> 36.0-36.3 dB, distortion -26.5 to -26.6 dB; beam denominator 24.8 -> 31.2 dB, -42.3 dB;
    noise 1.0: 10.9 -> 24.3 dB, -11.6 dB (microphones), 10.9 -> 19.4 dB, -29.7 dB (beam); with the interferer 8.7 -> 14.9 dB, interferer
    -6.4 dB (microphones), 8.7 -> 9.0 dB, interferer -0.3 dB (beam); beta = 0: 35.9 dB."""
    for seed in range(4):
        f = PN.host_scene(seed)
        print(_row("sensor noise 0.2, microphones, seed %d" % seed, f))
        assert f["snr_out"] - f["snr_in"] >= 9.0 and f["distortion"] <= -20.0, f
    beam = PN.host_scene(0, den_mode=1)
    print(_row("sensor noise 0.2, beam", beam))
    assert beam["distortion"] <= -35.0, beam
    print(_row("sensor noise 1.0, microphones", PN.host_scene(0, noise=1.0)))
    print(_row("sensor noise 1.0, beam", PN.host_scene(0, noise=1.0, den_mode=1)))
    mic_i = PN.host_scene(0, noise=PN.SCENE["interferer_noise"], interferer=True)
    print(_row("noise 0.05 + interferer 0.3, microphones", mic_i))
    assert mic_i["interferer"] <= -4.5, mic_i
    print(_row("noise 0.05 + interferer 0.3, beam", PN.host_scene(0, noise=PN.SCENE["interferer_noise"], interferer=True, den_mode=1)))
    print(_row("sensor noise 0.2, microphones, beta = 0", PN.host_scene(0, beta=0.0)))
