"""GPU (-m gpu): bf_enhance_device and enhance.Enhancer against the NumPy restatement of the definition (tests/enhance_np.py): the
synthesis path with given gains within the derived bound, the gain recursion bit for bit on the P the device reports, and the
definition's promises on the bytes: the cut of the stream into calls, the row count, the pointer alignment, a NaN's reach, a corrupt
state.  Every device output sits between canaries, which must survive, as must the floats of a d_out row past S.

Measured on an MI355X (the last test prints them): see DESIGN.md section 2."""
import numpy as np
import pytest

import enhance_np as EN
import util
from support import nat_restoring as nat

pytestmark = pytest.mark.gpu

CANARY = 64
CANARY_F = -1234.5
CANARY_I = 0x5A5A5A
PAR = dict(alpha=0.98, a_noise=0.9, g0=1.5, g1=5.0, g_min=0.1, n_init=8)
RATIOS = {}


def _canaried(a, off, value):
    """(buffer, lo): a device buffer of canaries with `a` at [lo, lo + a.size), off words past a 16-byte boundary."""
    torch = util.torch_gpu()
    a = np.ascontiguousarray(a).ravel()
    buf = torch.full((CANARY + 4 + a.size + CANARY,), value, dtype=torch.from_numpy(a).dtype, device="cuda")
    lo = CANARY + off
    buf[lo:lo + a.size].copy_(torch.from_numpy(a))
    assert buf[lo:].data_ptr() % 16 == 4 * off
    return buf, lo


def _inner(pair, size, value):
    buf, lo = pair
    host = buf.cpu().numpy()
    assert (host[:lo] == host.dtype.type(value)).all() and (host[lo + size:] == host.dtype.type(value)).all(), "a canary was overwritten"
    return host[lo:lo + size].copy()


def _design(n_fft, hop_s):
    import enhance
    return enhance.design_cola(n_fft, hop_s)


def _fresh(rows, n_fft):
    """The state at the start of a stream."""
    B = n_fft // 2 + 1
    z = lambda n: np.zeros((rows, n), np.float32)
    return dict(hist=z(n_fft - 1), ola=z(n_fft), noise=z(B), prior=z(B), words=np.zeros(4, np.int32))


def _run(nat, windows, n, hop, st, wa, ws, hop_s, gains=None, par=PAR, off=0, observe=True):
    """bf_enhance_device on device copies of windows [F, R, stride] and the state st -> dict(out [R, S], hist, ola, noise, prior, words, count,
    status, cap, P, G).  The canaries round d_out, d_work, the observables and the state are checked."""
    torch = util.torch_gpu()
    F, R, stride = windows.shape
    n_fft = wa.shape[0]
    B = n_fft // 2 + 1
    S = F * (hop if hop > 0 else n)
    cap = (hop_s - 1 + S) // hop_s
    words = nat.lib.bf_enhance_workspace(R, S, n_fft, hop_s)
    assert words == EN.workspace(R, S, n_fft, hop_s) > 0
    out_stride = S + 3
    d_x = util.place_words(windows, off)
    d_wa, d_ws = util.place_words(wa, off), util.place_words(ws, off)
    d_g = None if gains is None else util.place_words(gains.astype(np.float32), off)
    f32 = lambda a: _canaried(np.asarray(a, np.float32), off, CANARY_F)
    b_out = f32(np.full(R * out_stride, CANARY_F))
    b_work = f32(np.full(words, CANARY_F))
    b_p = f32(np.full(R * cap * B, CANARY_F)) if observe else None
    b_g = f32(np.full(R * cap * B, CANARY_F)) if observe else None
    b_hist, b_ola, b_noise, b_prior = f32(st["hist"]), f32(st["ola"]), f32(st["noise"]), f32(st["prior"])
    b_state = _canaried(np.asarray(st["words"], np.int32), off, CANARY_I)
    b_count = _canaried(np.array([-9, -9], np.int32), off, CANARY_I)
    ptr = lambda pair: None if pair is None else pair[0][pair[1]:].data_ptr()
    rc = nat.lib.bf_enhance_device(d_x.data_ptr(), R, F, n, stride, hop, ptr(b_hist), ptr(b_ola), ptr(b_noise), ptr(b_prior), ptr(b_state), d_wa.data_ptr(),
                                   d_ws.data_ptr(), n_fft, hop_s, None if d_g is None else d_g.data_ptr(), par["alpha"], par["a_noise"], par["g0"], par["g1"],
                                   par["g_min"], par["n_init"], ptr(b_work), ptr(b_out), out_stride, ptr(b_p), ptr(b_g), ptr(b_count),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, nat.lib.bf_last_error()
    out = _inner(b_out, R * out_stride, CANARY_F).reshape(R, out_stride)
    assert (out[:, S:] == np.float32(CANARY_F)).all(), "a float past S was written"
    _inner(b_work, words, CANARY_F)
    cnt = _inner(b_count, 2, CANARY_I)
    res = dict(out=out[:, :S].copy(), hist=_inner(b_hist, R * (n_fft - 1), CANARY_F).reshape(R, -1), ola=_inner(b_ola, R * n_fft, CANARY_F).reshape(R, -1),
               noise=_inner(b_noise, R * B, CANARY_F).reshape(R, B), prior=_inner(b_prior, R * B, CANARY_F).reshape(R, B), words=_inner(b_state, 4, CANARY_I),
               count=int(cnt[0]), status=int(cnt[1]), cap=cap)
    if observe:
        res["P"] = _inner(b_p, R * cap * B, CANARY_F).reshape(R, cap, B)
        res["G"] = _inner(b_g, R * cap * B, CANARY_F).reshape(R, cap, B)
        assert not res["P"][:, res["count"]:].any() and not res["G"][:, res["count"]:].any()
    return res


def _state_of(res):
    return {k: res[k] for k in ("hist", "ola", "noise", "prior", "words")}


def _windows(rng, F, R, n, stride, scale=None):
    """[F, R, stride]: windows of n samples with NaN behind them.  Overlapping windows (hop < n) need not agree: only the last hop
    samples of each are the stream."""
    w = np.full((F, R, stride), np.nan, np.float32)
    s = np.exp2(rng.integers(-6, 6, size=(1, R, 1)).astype(np.float64)) if scale is None else scale
    w[:, :, :n] = (rng.standard_normal((F, R, n)) * s).astype(np.float32)
    return w


def _same_state(a, b):
    for k in ("hist", "ola", "noise", "prior"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["words"].tolist() == b["words"].tolist()


# ------------------------------------------------------------------ 1. synthesis with given gains, to the derived bound

def _shape(n_fft):
    """(F, n, hop, stride): three windows of 96 at hop 40, 100 floats apart (S = 120); a flat stream of 2500 for n_fft = 1024."""
    return (1, 2500, 0, 2503) if n_fft == 1024 else (3, 96, 40, 100)


def _random_gains(rng, R, cap, B):
    g = rng.uniform(0.0, 1.0, (R, cap, B)).astype(np.float32)
    pick = rng.integers(0, 8, g.shape)
    g[pick == 0] = 0.0
    g[pick == 1] = 1.0
    return g


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("div", [1, 2, 8])
@pytest.mark.parametrize("n_fft", [32, 64, 512, 1024])
def test_given_gains_within_the_derived_bound(nat, n_fft, div, rows):
    """Two calls from a state in mid-stream (random history and partial sums, c > 0), so c wraps; every d_out element and the final d_ola
    within synthesis_bound of the float64 restatement of the whole stretch; P within its own bound; history and state exactly."""
    hop_s = n_fft // div
    wa, ws, _ = _design(n_fft, hop_s)
    F, n, hop, stride = _shape(n_fft)
    rng = np.random.default_rng([n_fft, div, rows])
    B = n_fft // 2 + 1
    st = _fresh(rows, n_fft)
    scale = np.exp2(rng.integers(-6, 6, size=(1, rows, 1)).astype(np.float64))
    st["hist"] = (rng.standard_normal((rows, n_fft - 1)) * scale[0]).astype(np.float32)
    st["ola"] = (rng.standard_normal((rows, n_fft)) * scale[0]).astype(np.float32)
    c0 = (2 * hop_s) // 3
    st["words"] = np.array([c0, 5, -7, 9], np.int32)                   # the reserved words are written 0, seen stays with given gains
    first = dict(st)
    xs, outs, Gs, c = [], [], [], c0
    for call in range(2):
        w = _windows(rng, F, rows, n, stride, scale)
        x = EN.stream(w[:, :, :n], n, hop)
        count, c_new, cap = EN.advance(c, x.shape[1], hop_s)
        g = _random_gains(rng, rows, cap, B)
        got = _run(nat, w, n, hop, st, wa, ws, hop_s, gains=g)
        assert (got["count"], got["status"], got["cap"]) == (count, 0, cap) and got["words"].tolist() == [c_new, 5, 0, 0]
        assert got["G"][:, :count].tobytes() == g[:, :count].tobytes()
        assert got["noise"].tobytes() == st["noise"].tobytes() and got["prior"].tobytes() == st["prior"].tobytes()
        u, X, _ = EN.analysis(x, st["hist"], c, wa, hop_s)
        if count:
            e = np.log2(n_fft) * EN.ETA * EN.EPS * np.sqrt(n_fft) * np.sqrt((u.astype(np.float64) ** 2).sum(axis=-1))[..., None]
            P = np.abs(X) ** 2
            tol_P = (2 * np.abs(X) * e + e * e) * (1 + 3 * EN.EPS) + 3 * EN.EPS * P + 1e-45
            RATIOS["P"] = max(RATIOS.get("P", 0.0), float((np.abs(got["P"][:, :count] - P) / tol_P).max()))
            assert (np.abs(got["P"][:, :count] - P) <= tol_P).all()
        assert got["hist"].tobytes() == EN.new_history(st["hist"], x).tobytes()
        xs.append(x)
        outs.append(got["out"])
        Gs.append(g[:, :count])
        st, c = _state_of(got), c_new
    want = EN.enhance(np.concatenate(xs, axis=1), first["hist"], first["ola"], c0, wa, ws, hop_s, G=np.concatenate(Gs, axis=1))
    assert want["c"] == c and want["count"] == sum(g.shape[1] for g in Gs)
    err = np.abs(np.concatenate([np.concatenate(outs, axis=1), st["ola"]], axis=1) - np.concatenate([want["out"], want["ola"]], axis=1))
    tol = np.concatenate([want["tol_out"], want["tol_ola"]], axis=1)
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    RATIOS["d_out, n_fft %d" % n_fft] = max(RATIOS.get("d_out, n_fft %d" % n_fft, 0.0), ratio)
    print("n_fft %d hop_s %d rows %d: worst error / bound %.4f" % (n_fft, hop_s, rows, ratio))
    assert (err <= tol).all(), ratio


@pytest.mark.parametrize("n_fft,div", [(32, 1), (32, 8), (64, 2), (512, 2), (1024, 4), (4096, 2)])
def test_unit_gains_return_the_input_delayed(nat, n_fft, div):
    hop_s = n_fft // div
    wa, ws, dev = _design(n_fft, hop_s)
    rng = np.random.default_rng([n_fft, div, 1])
    rows = 2
    F, n, hop, stride = (1, 2500, 0, 2500) if n_fft == 1024 else (1, 3 * n_fft + 40, 0, 3 * n_fft + 41)     # (4096: the largest frame, 48 KiB of LDS)
    w = _windows(rng, F, rows, n, stride)
    x = EN.stream(w[:, :, :n], n, hop)
    cap = EN.advance(0, n, hop_s)[2]
    ones = np.ones((rows, cap, n_fft // 2 + 1), np.float32)
    got = _run(nat, w, n, hop, _fresh(rows, n_fft), wa, ws, hop_s, gains=ones)
    want = EN.enhance(x, np.zeros((rows, n_fft - 1)), np.zeros((rows, n_fft)), 0, wa, ws, hop_s, G=ones)
    delayed = np.concatenate([np.zeros((rows, n_fft)), x.astype(np.float64)], axis=1)[:, :n]
    tol = want["tol_out"] + EN.cola_term(delayed, n_fft, dev) + div * EN.EPS * np.abs(delayed) * 1.01
    err = np.abs(got["out"] - delayed)
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    RATIOS["delayed input"] = max(RATIOS.get("delayed input", 0.0), ratio)
    assert (err <= tol).all(), ratio
    assert got["count"] == want["count"] and np.abs(got["out"][:, n_fft:]).max() > 0.1 * np.abs(x).max()


# ------------------------------------------------------------------ 2. the recursion on the bytes

def _hostile(rng, F, R, n, stride):
    """Rows of zeros, of 1e-20 (P is subnormal), of 1e19 (P overflows), noise with a NaN, noise with an Inf, plain noise, and subnormal
    samples (P underflows to zero)."""
    assert R == 7
    w = _windows(rng, F, R, n, stride, scale=1.0)
    w[:, 0, :n] = 0.0
    w[:, 1, :n] *= np.float32(1e-20)
    w[:, 6, :n] *= np.float32(1e-40)
    w[:, 2, :n] *= np.float32(1e19)
    w[F // 2, 3, n - 7] = np.nan
    w[F // 2, 4, n - 5] = np.inf
    return w


@pytest.mark.parametrize("n_fft,hop_s,shape,hostile", [(32, 16, (3, 96, 40, 100), False), (32, 16, (3, 96, 40, 100), True), (512, 64, (1, 600, 0, 601), False),
                                                       (64, 8, (3, 96, 40, 100), True), (1024, 512, (1, 2500, 0, 2500), False)])
def test_the_recursion_bit_for_bit(nat, n_fft, hop_s, shape, hostile):
    """Three consecutive calls: the device's d_power_out through enhance_np.gains gives d_gain_out, d_noise, d_prior and d_state bit for
    bit; n_init = 10 puts the end of the learning stretch inside the first, the second or the third call, by the shape."""
    wa, ws, _ = _design(n_fft, hop_s)
    F, n, hop, stride = shape
    rows = 7 if hostile else 3
    rng = np.random.default_rng([n_fft, hop_s, int(hostile)])
    par = dict(PAR, n_init=10, alpha=0.92, g_min=0.05)
    st = _fresh(rows, n_fft)
    seen, c, counts = 0, 0, []
    for call in range(3):
        w = _hostile(rng, F, rows, n, stride) if hostile else _windows(rng, F, rows, n, stride)
        got = _run(nat, w, n, hop, st, wa, ws, hop_s, par=par)
        count, c, cap = EN.advance(c, F * (hop or n), hop_s)
        assert (got["count"], got["status"]) == (count, 0)
        P = got["P"][:, :count]
        G, lam, prior, seen_new = EN.gains(P, st["noise"], st["prior"], seen, **par)
        assert not util.bits_differ(got["G"][:, :count], G, nan_is_nan=True), util.bits_differ(got["G"][:, :count], G, nan_is_nan=True)
        assert got["noise"].tobytes() == lam.tobytes() and got["prior"].tobytes() == prior.tobytes()
        assert got["words"].tolist() == [c, seen_new, 0, 0]
        assert np.isfinite(got["noise"]).all() and np.isfinite(got["prior"]).all() and (got["noise"] >= 0).all()
        if hostile:
            assert not got["out"][0].any() and (got["G"][0, :count] == np.float32(par["g_min"])).all()            # a row of zeros gives zeros
            assert not np.isfinite(P[2]).all() and np.isnan(got["G"][:, :count][~np.isfinite(P)]).all()
            assert np.isfinite(got["out"][[1, 5, 6]]).all()
            tiny = P[1][P[1] > 0]
            assert (tiny < EN.FLT_MIN).any() and ((got["noise"][1] > 0) & (got["noise"][1] < EN.FLT_MIN)).any()      # subnormal P and lam among them
        counts.append(count)
        st, seen = _state_of(got), seen_new
    assert seen == 10 and sum(counts) > 10


# ------------------------------------------------------------------ 3. promises on the bytes

SPLITS = [(64, 32, (5, 96, 40, 100), 2), (32, 4, (5, 95, 37, 100), 3), (1024, 128, (3, 700, 0, 703), 1), (512, 256, (4, 300, 300, 300), 1)]


@pytest.mark.parametrize("n_fft,hop_s,shape,F1", SPLITS)
def test_the_cut_of_the_stream_does_not_show(nat, n_fft, hop_s, shape, F1):
    """Two calls on F1 and F - F1 windows, the second with the first's state, against one call on F windows: d_out and all state, bit for
    bit; F1 leaves c != 0.  The same for a row alone against the row among three, and with every pointer 4 bytes further."""
    wa, ws, _ = _design(n_fft, hop_s)
    F, n, hop, stride = shape
    rng = np.random.default_rng([n_fft, hop_s, F1])
    w = _windows(rng, F, 3, n, stride)
    one = _run(nat, w, n, hop, _fresh(3, n_fft), wa, ws, hop_s)
    a = _run(nat, w[:F1], n, hop, _fresh(3, n_fft), wa, ws, hop_s)
    assert a["words"][0] != 0 and a["status"] == 0
    b = _run(nat, w[F1:], n, hop, _state_of(a), wa, ws, hop_s)
    assert a["count"] + b["count"] == one["count"] > 0
    assert np.concatenate([a["out"], b["out"]], axis=1).tobytes() == one["out"].tobytes()
    _same_state(b, one)
    assert np.concatenate([a["G"][:, :a["count"]], b["G"][:, :b["count"]]], axis=1).tobytes() == one["G"][:, :one["count"]].tobytes()
    for r, off in ((0, 0), (1, 1), (2, 3)):
        alone = _run(nat, w[:, r:r + 1], n, hop, _fresh(1, n_fft), wa, ws, hop_s, off=off)
        assert alone["out"][0].tobytes() == one["out"][r].tobytes() and alone["count"] == one["count"]
        for k in ("hist", "ola", "noise", "prior"):
            assert alone[k][0].tobytes() == one[k][r].tobytes(), k
    shifted = _run(nat, w, n, hop, _fresh(3, n_fft), wa, ws, hop_s, off=1)
    assert shifted["out"].tobytes() == one["out"].tobytes() and shifted["P"].tobytes() == one["P"].tobytes()
    _same_state(shifted, one)


@pytest.mark.parametrize("n_fft,hop_s", [(32, 8), (512, 256), (1024, 256)])
def test_a_nan_reaches_only_the_positions_its_frames_span(nat, n_fft, hop_s):
    wa, ws, _ = _design(n_fft, hop_s)
    wa = wa + np.float32(0.01)                                            # (no zero weight: a NaN under it would still be a NaN)
    rng = np.random.default_rng([n_fft, hop_s, 9])
    n = 6 * n_fft + 5
    w = _windows(rng, 1, 3, n, n + 1)
    clean = _run(nat, w, n, 0, _fresh(3, n_fft), wa, ws, hop_s)
    at = 2 * n_fft + hop_s // 2 + 1
    bad = w.copy()
    bad[0, 1, at] = np.nan
    got = _run(nat, bad, n, 0, _fresh(3, n_fft), wa, ws, hop_s)
    starts = [s for s in EN.frame_starts(0, n, n_fft, hop_s) if s <= at < s + n_fft]
    assert len(starts) == n_fft // hop_s
    hit = np.zeros(n, bool)
    hit[starts[0] + n_fft:min(starts[-1] + 2 * n_fft, n)] = True           # d_out[s] is position s - n_fft
    assert hit.any() and not hit[-n_fft:].any() and hit.sum() == 2 * n_fft - hop_s
    assert (~np.isfinite(got["out"][1]) == hit).all()
    assert np.isfinite(got["out"][1][at + 2 * n_fft:]).all()               # finite again 2 n_fft samples behind the NaN
    assert got["out"][[0, 2]].tobytes() == clean["out"][[0, 2]].tobytes()
    for k in ("noise", "prior", "ola", "hist"):
        assert np.isfinite(got[k]).all() and got[k][[0, 2]].tobytes() == clean[k][[0, 2]].tobytes(), k
    bad_frames = ~np.isfinite(got["P"][1]).all(axis=1)
    assert bad_frames.sum() == len(starts) and np.isnan(got["G"][1][bad_frames]).all() and np.isfinite(got["G"][1][~bad_frames]).all()


def test_a_corrupt_state_is_reported_and_nothing_moves(nat):
    n_fft, hop_s = 32, 16
    wa, ws, _ = _design(n_fft, hop_s)
    rng = np.random.default_rng(13)
    w = _windows(rng, 3, 3, 96, 100)
    st = _fresh(3, n_fft)
    for k in ("hist", "ola", "noise", "prior"):
        st[k] = np.abs(rng.standard_normal(st[k].shape)).astype(np.float32)
    for words in ([16, 0, 77, -5], [-1, 3, 0, 0], [5, -1, 0, 0], [1 << 30, 0, 0, 0], [-(1 << 31), -(1 << 31), 0, 0]):
        st["words"] = np.array(words, np.int32)
        got = _run(nat, w, 96, 40, st, wa, ws, hop_s)
        assert (got["count"], got["status"], got["cap"]) == (0, 1, 8) and got["words"].tolist() == words
        assert not got["out"].any() and not got["P"].any() and not got["G"].any()
        _same_state(got, st)
    st["words"] = np.array([15, 0, 77, -5], np.int32)
    got = _run(nat, w, 96, 40, st, wa, ws, hop_s)
    assert (got["count"], got["status"]) == (8, 0) and got["words"].tolist() == [7, 8, 0, 0]


# ------------------------------------------------------------------ 4. enhance.Enhancer under graph replay

def test_graph_replay_of_push(nat):
    """Enhancer.push captured after one warm-up push and replayed three times over fresh beams, against eager pushes on a second
    Enhancer: bytes, counts and the carried state."""
    torch = util.torch_gpu()
    import enhance
    N, hop, F, B = 64, 24, 3, 3
    util.configure_small(N)
    rng = np.random.default_rng(61)
    batches = [(rng.standard_normal((F, B, N)) * 0.3).astype(np.float32) for _ in range(4)]
    make = lambda: enhance.Enhancer(rows=B, hop=hop, n_fft=32, hop_s=16, n_init=5)
    eager_en = make()
    eager = []
    for c in range(4):
        clean, count = eager_en.push(torch.from_numpy(batches[c]).cuda())
        torch.cuda.synchronize()
        eager.append((clean.cpu().numpy(), count.cpu().numpy().copy()))
        assert eager[-1][1].tolist() == [eager_en.last_count, 0]
    assert [e[1][0] for e in eager] == [4, 5, 4, 5] and np.abs(eager[-1][0]).max() > 0
    en = make()
    x = torch.from_numpy(batches[0]).cuda()
    en.push(x)                                                           # the warm-up push: batch 0
    carried = tuple(t.data_ptr() for t in (en.hist, en.ola, en.noise, en.prior, en.state, en.count))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        clean, count = en.push(x)
    assert carried == tuple(t.data_ptr() for t in (en.hist, en.ola, en.noise, en.prior, en.state, en.count))
    for c in range(1, 4):
        x.copy_(torch.from_numpy(batches[c]).cuda())
        g.replay()
        torch.cuda.synchronize()
        assert count.cpu().numpy().tolist() == eager[c][1].tolist()
        assert clean.cpu().numpy().tobytes() == eager[c][0].tobytes()
    for name in ("hist", "ola", "noise", "prior", "state"):
        assert getattr(en, name).cpu().numpy().tobytes() == getattr(eager_en, name).cpu().numpy().tobytes(), name
    en.reset()
    assert all(not getattr(en, k).cpu().numpy().any() for k in ("hist", "ola", "noise", "prior", "state", "count")) and en.last_count == 0
    assert carried == tuple(t.data_ptr() for t in (en.hist, en.ola, en.noise, en.prior, en.state, en.count))


# ------------------------------------------------------------------ 5. the chain and the figure

def test_the_tone_scene_through_the_chain(nat):
    """The host test's scene (seed 0) through Enhancer.push -> AudioOut(hop=None).push_flat in blocks of 2048; the SNR behind the filter by
    the shadow method with the device's own gains (pushed again over the tones alone and the noise alone) beside the restatement's."""
    torch = util.torch_gpu()
    import audio_out
    import enhance
    util.configure_small(256)
    seed, block = 0, 2048
    s, d, active = EN.tone_scene(seed)
    total = s.size
    assert total % block == 0
    x = (s + d).astype(np.float32)
    en, en_s, en_d = (enhance.Enhancer(rows=1) for _ in range(3))
    ao = audio_out.AudioOut(48000, rows=1, hop=None)
    assert (en.n_fft, en.hop_s, en.delay, en.alpha, en.n_init) == (256, 128, 256, 0.98, 8)
    ys, yd, yx, audio_samples = [], [], [], 0
    for a in range(0, total, block):
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v[None, a:a + block])).cuda()
        clean, count, _, G = en.push(dev(x), observe=True)
        assert tuple(clean.shape) == (1, block)
        audio, pcm, n_audio = ao.push_flat(clean)
        ys.append(en_s.push(dev(s), gains=G)[0].cpu().numpy()[0])
        yd.append(en_d.push(dev(d), gains=G)[0].cpu().numpy()[0])
        yx.append(clean.cpu().numpy()[0])
        cnt = count.cpu().numpy()
        assert cnt.tolist() == [block // 128, 0] and en.last_count == block // 128
        audio_samples += int(n_audio.cpu().numpy()[0])
        assert np.isfinite(audio.cpu().numpy()).all() and pcm is not None
    assert abs(audio_samples - total * 48000 / 48828) < 2
    yx, y_s, y_d = np.concatenate(yx), np.concatenate(ys), np.concatenate(yd)
    assert np.abs(yx - (y_s + y_d)).max() < 1e-4                          # the filter is linear once its gains are fixed
    fig = EN.scene_figures(s, d, active, y_s, y_d, en.delay)
    host = [EN.host_scene(k) for k in range(4)]
    spread = max(h["snr_out"] for h in host) - min(h["snr_out"] for h in host)
    print("device: SNR over the active stretches %.2f dB in, %.2f dB out, distortion %.2f dB; restatement (float64, seed %d): %.2f dB out; spread over seeds 0-3: %.2f dB"
          % (fig["snr_in"], fig["snr_out"], fig["distortion"], seed, host[seed]["snr_out"], spread))
    assert fig["snr_out"] > fig["snr_in"]
    assert abs(fig["snr_out"] - host[seed]["snr_out"]) <= spread


def test_print_the_ratios():
    for name in sorted(RATIOS):
        print("largest error / bound, %s: %.4f" % (name, RATIOS[name]))
