"""GPU (-m gpu): bf_postfilter_device and postfilter.SpatialPostFilter against the NumPy restatement of the definition
(tests/postfilter_np.py): the raw numerator and denominator within the derived bound, the steering against the double formula, the
recursion bit for bit on the num and den the device reports, and the definition's promises on the bytes: the cut of the stream into
calls, m_total, the rows the microphones occupy, trailing slots, the pointer alignment, a NaN's reach, a corrupt state.  Every device
output sits between canaries, which must survive.

Measured on an MI355X (the last test prints them): see DESIGN.md section 2."""
import numpy as np
import pytest

import enhance_np as EN
import postfilter_np as PN
import util
from support import nat_restoring as nat

pytestmark = pytest.mark.gpu

CANARY = 64
CANARY_F = -1234.5
CANARY_I = 0x5A5A5A
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


def _window(n_fft, hop_s):
    import enhance
    return enhance.design_cola(n_fft, hop_s)[0]


def _fresh(n, slots, n_fft, lag):
    """The state at the start of a stream."""
    K = n_fft // 2 + 1
    return dict(hist=np.zeros((n, n_fft - 1 + lag), np.float32), N=np.zeros((slots, K), np.float32), D=np.zeros((slots, K), np.float32),
                words=np.zeros(2 + slots, np.int32))


class Setup:
    """What stays the same over the calls of a test."""

    def __init__(self, mics, tau, offset_per_dir, win, hop_s, lag=0, den_mode=0, beta=0.8, g_min=0.1):
        self.mics, self.tau, self.opd = np.asarray(mics, np.int32), np.ascontiguousarray(tau, np.float64), offset_per_dir
        self.win, self.hop_s, self.lag, self.den_mode, self.beta, self.g_min = win, hop_s, lag, den_mode, beta, g_min
        self.n, self.n_fft = self.mics.size, win.shape[0]


def _run(nat, su, frames, hop, offsets, st, off=0, observe=True):
    """bf_postfilter_device on device copies of frames [F, M_total, N] and the state st -> dict(G, num, den [slots, cap, K], steer, hist,
    N, D, words, status, count, call_status, cap).  The canaries round every output and the state are checked."""
    torch = util.torch_gpu()
    F, m_total, N = frames.shape
    n, n_fft, slots = su.n, su.n_fft, len(offsets)
    K, H = n_fft // 2 + 1, n_fft - 1 + su.lag
    S = F * (hop if hop > 0 else N)
    cap = (su.hop_s - 1 + S) // su.hop_s
    words = nat.lib.bf_postfilter_workspace(slots, S, n_fft, su.hop_s)
    assert words == PN.workspace(slots, S, n_fft, su.hop_s) > 0
    d_x, d_win = util.place_words(frames, off), util.place_words(su.win, off)
    d_tau = torch.from_numpy(su.tau).cuda()
    d_off = util.place_words(np.asarray(offsets, np.int32), off)
    f32 = lambda a: _canaried(np.asarray(a, np.float32), off, CANARY_F)
    i32 = lambda a: _canaried(np.asarray(a, np.int32), off, CANARY_I)
    cells = slots * cap * K
    b_g, b_work, b_steer = f32(np.full(cells, CANARY_F)), f32(np.full(words, CANARY_F)), f32(np.full(slots * n * K * 2, CANARY_F))
    b_num = f32(np.full(cells, CANARY_F)) if observe else None
    b_den = f32(np.full(cells, CANARY_F)) if observe else None
    b_hist, b_N, b_D = f32(st["hist"]), f32(st["N"]), f32(st["D"])
    b_state, b_status, b_count = i32(st["words"]), i32(np.full(slots, -9)), i32([-9, -9])
    ptr = lambda pair: None if pair is None else pair[0][pair[1]:].data_ptr()
    rc = nat.lib.bf_postfilter_device(d_x.data_ptr(), m_total, F, N, hop, nat.iptr(su.mics), n, d_tau.data_ptr(), su.tau.shape[0], d_off.data_ptr(), slots, su.opd,
                                      ptr(b_hist), ptr(b_N), ptr(b_D), ptr(b_state), d_win.data_ptr(), n_fft, su.hop_s, su.lag, su.den_mode, su.beta, su.g_min,
                                      ptr(b_work), ptr(b_steer), ptr(b_g), ptr(b_num), ptr(b_den), ptr(b_status), ptr(b_count), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, nat.lib.bf_last_error()
    _inner(b_work, words, CANARY_F)
    cnt = _inner(b_count, 2, CANARY_I)
    res = dict(G=_inner(b_g, cells, CANARY_F).reshape(slots, cap, K), steer=_inner(b_steer, slots * n * K * 2, CANARY_F).reshape(slots, n, K, 2),
               hist=_inner(b_hist, n * H, CANARY_F).reshape(n, H), N=_inner(b_N, slots * K, CANARY_F).reshape(slots, K), D=_inner(b_D, slots * K, CANARY_F).reshape(slots, K),
               words=_inner(b_state, 2 + slots, CANARY_I), status=_inner(b_status, slots, CANARY_I).tolist(), count=int(cnt[0]), call_status=int(cnt[1]), cap=cap)
    assert not res["G"][:, res["count"]:].any()
    if observe:
        res["num"] = _inner(b_num, cells, CANARY_F).reshape(slots, cap, K)
        res["den"] = _inner(b_den, cells, CANARY_F).reshape(slots, cap, K)
        assert not res["num"][:, res["count"]:].any() and not res["den"][:, res["count"]:].any()
    return res


def _state_of(res):
    return {k: res[k] for k in ("hist", "N", "D", "words")}


def _same_state(a, b):
    for k in ("hist", "N", "D"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["words"].tolist() == b["words"].tolist()


def _frames(rng, F, m_total, N, scale=None):
    """[F, M_total, N] noise, every row at its own scale.  Overlapping windows (hop < N) need not agree: only the last hop samples count."""
    s = np.exp2(rng.integers(-4, 5, size=(1, m_total, 1)).astype(np.float64)) if scale is None else scale
    return (rng.standard_normal((F, m_total, N)) * s).astype(np.float32)


def _check_recursion(su, got, st, offsets, c):
    """The device's own num and den through the restatement's recursion: gains, N, D and the state words, bit for bit -> the new c."""
    dirs = PN.slot_directions(offsets, su.opd, su.tau.shape[0])
    sources = [d >= 0 for d in dirs]
    count = got["count"]
    G, N, D, seen = PN.recursion(got["num"][:, :count], got["den"][:, :count], st["N"], st["D"], st["words"][2:].tolist(), sources, su.beta, su.g_min)
    diff = util.bits_differ(got["G"][:, :count], G, nan_is_nan=True)
    assert not diff, diff
    assert got["N"].tobytes() == N.tobytes() and got["D"].tobytes() == D.tobytes()
    assert got["status"] == [0 if s else 1 for s in sources]
    return seen


# ------------------------------------------------------------------ 1. the raw values, to the derived bound

def _shape(n_fft):
    """(F, N, hop): three windows of 96 at hop 40 (S = 120); one window of 2500 for n_fft = 1024."""
    return (1, 2500, 0) if n_fft == 1024 else (3, 96, 40)


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("div", [1, 2, 8])
@pytest.mark.parametrize("n_fft", [32, 64, 512, 1024])
def test_values_within_the_derived_bound(nat, n_fft, div, slots):
    """Two calls from a state in mid-stream (random history, c > 0, a carried N and D), so c wraps; n, lag and the denominator cycle with
    the case so that every value of each meets every n_fft.  num and den within raw_bound of the float64 restatement, the gains within
    gain_bound where it says anything, the steering against the double formula, history and state exactly, the recursion bit for bit."""
    case = [32, 64, 512, 1024].index(n_fft) * 3 + [1, 2, 8].index(div)
    n = (2, 3, 64)[(case + slots) % 3]
    lag = (0, 5)[(case // 3 + case + slots) % 2]
    den_mode = (case + slots // 2) % 2
    hop_s = n_fft // div
    F, N, hop = _shape(n_fft)
    rng = np.random.default_rng([n_fft, div, slots])
    m_total, dirs, opd = n + 2, 6, 5
    mics = rng.permutation(m_total)[:n]
    tau = rng.uniform(0.0, 9.0, (dirs, n))
    su = Setup(mics, tau, opd, _window(n_fft, hop_s), hop_s, lag=lag, den_mode=den_mode, beta=0.8, g_min=0.1)
    K = n_fft // 2 + 1
    scale = np.exp2(rng.integers(-4, 5, size=(1, m_total, 1)).astype(np.float64))
    st = _fresh(n, slots, n_fft, lag)
    st["hist"] = (rng.standard_normal(st["hist"].shape) * scale[0][mics]).astype(np.float32)
    c = (2 * hop_s) // 3
    st["words"][0], st["words"][1], st["words"][2] = c, 7, 1            # slot 0 has been seen; the reserved word is written 0
    st["N"][0] = np.abs(rng.standard_normal(K)).astype(np.float32)
    st["D"][0] = (st["N"][0] + np.abs(rng.standard_normal(K))).astype(np.float32)
    plans = ([[3 * opd], [3 * opd]] if slots == 1 else [[3 * opd, -1, 2 * opd + 1], [3 * opd, 5 * opd, -1]])        # an empty slot and one that is no multiple
    for offsets in plans:
        w = _frames(rng, F, m_total, N, scale)
        x = PN.stream(w, mics, hop)
        want = PN.postfilter(x, st["hist"], c, su.win, hop_s, lag, tau, offsets, opd, den_mode, su.beta, su.g_min, st["N"], st["D"], st["words"][2:].tolist())
        got = _run(nat, su, w, hop, offsets, st)
        count = want["count"]
        assert (got["count"], got["call_status"], got["cap"]) == (count, 0, want["cap"]) and got["status"] == want["status"]
        assert got["hist"].tobytes() == want["hist"].tobytes()
        # the steering: each component within half a float32 step of the double formula (2^-25 below 1), a tie of the two libraries aside
        assert np.abs(got["steer"].astype(np.float64) - want["steer"]).max() <= 2.0 ** -24
        RATIOS["steering values that differ from NumPy's"] = RATIOS.get("steering values that differ from NumPy's", 0) + int((got["steer"] != want["steer"]).sum())
        seen_before = st["words"][2:].tolist()
        for b, source in enumerate(want["sources"]):
            if not source:
                assert not got["G"][b].any() and not got["num"][b].any() and not got["den"][b].any() and got["words"][2 + b] == 0
                assert got["N"][b].tobytes() == st["N"][b].tobytes() and got["D"][b].tobytes() == st["D"][b].tobytes()
                continue
            for name, tol in (("num", want["dnum"]), ("den", want["dden"])):
                err = np.abs(got[name][b, :count] - want[name][b])
                ratio = float((err / tol[b]).max()) if count else 0.0
                RATIOS["%s, n_fft %d" % (name, n_fft)] = max(RATIOS.get("%s, n_fft %d" % (name, n_fft), 0.0), ratio)
                assert (err <= tol[b]).all(), (name, ratio)
            if count:
                Nb, Db, dN, dD = PN.smooth_bound(want["num"][b], want["den"][b], want["dnum"][b], want["dden"][b], st["N"][b], st["D"][b], seen_before[b], su.beta)
                tol_G = PN.gain_bound(Nb, Db, dN, dD, su.g_min)
                err = np.abs(got["G"][b, :count] - PN.gain_of(Nb, Db, su.g_min))
                said = tol_G < 1.0 - su.g_min
                assert said.any() and (err <= tol_G).all(), float((err / tol_G).max())
                RATIOS["G where D is away from 0"] = max(RATIOS.get("G where D is away from 0", 0.0), float((err[said] / tol_G[said]).max()))
        seen = _check_recursion(su, got, st, offsets, c)
        c = want["c"]
        assert got["words"].tolist() == [c, 0] + seen
        st = _state_of(got)
    print("n_fft %d hop_s %d n %d slots %d lag %d den %d: worst num error / bound %.4f" % (n_fft, hop_s, n, slots, lag, den_mode, RATIOS["num, n_fft %d" % n_fft]))


# ------------------------------------------------------------------ 2. the recursion on the bytes

def _hostile(rng, F, m_total, N):
    """Windows in turn: noise, noise with a NaN, noise, noise with an Inf, 1e-20 (num and den are subnormal), zeros and 1e-30 (the powers
    underflow to zero: together longer than a frame of 64), 1e25 (the powers overflow), and noise again."""
    assert F == 9
    w = _frames(rng, F, m_total, N, scale=1.0)
    w[1, :, N - 7] = np.nan
    w[3, :, N - 5] = np.inf
    w[4] *= np.float32(1e-20)
    w[5] = 0.0
    w[6] *= np.float32(1e-30)
    w[7] *= np.float32(1e25)
    return w


@pytest.mark.parametrize("n_fft,hop_s,n,beta,den_mode", [(32, 16, 3, 0.8, 0), (64, 8, 5, 0.0, 1), (512, 256, 4, 0.8, 1), (1024, 512, 2, 0.5, 0)])
def test_the_recursion_bit_for_bit(nat, n_fft, hop_s, n, beta, den_mode):
    """Three consecutive calls on hostile windows: the device's d_num_out / d_den_out through postfilter_np.recursion give d_gains, d_num,
    d_den and d_state bit for bit.  Slot 1 is a source, then empty, then a source again: it starts fresh."""
    big = n_fft >= 512
    F, N, hop = (9, 1100, 0) if big else (9, 96, 40)
    rng = np.random.default_rng([n_fft, hop_s, n])
    m_total, opd, dirs = n + 1, 3, 4
    su = Setup(rng.permutation(m_total)[:n], rng.uniform(0, 6, (dirs, n)), opd, _window(n_fft, hop_s), hop_s, lag=0, den_mode=den_mode, beta=beta, g_min=0.05)
    st = _fresh(n, 2, n_fft, 0)
    c, nan_frames, floor_frames = 0, 0, 0
    g_min = np.float32(0.05)
    for call, offsets in enumerate(([0, 2 * opd], [0, -1], [0, 3 * opd])):
        w = _hostile(rng, F, m_total, N)
        got = _run(nat, su, w, hop, offsets, st)
        count, c, cap = EN.advance(c, F * (hop or N), hop_s)
        assert (got["count"], got["call_status"]) == (count, 0)
        seen = _check_recursion(su, got, st, offsets, c)
        assert got["words"].tolist() == [c, 0] + seen and seen[0] == 1
        assert np.isfinite(got["N"]).all() and np.isfinite(got["D"]).all()
        G0 = got["G"][0, :count]
        bad = np.isnan(G0).any(axis=1)
        assert (np.isnan(G0).all(axis=1) == bad).all() and np.isfinite(G0[~bad]).all()                 # a frame is NaN in every bin or in none
        assert ((G0[~bad] >= np.float32(0.05)) & (G0[~bad] <= 1)).all()
        nan_frames += int(bad.sum())
        silent = (got["den"][0, :count] == 0).all(axis=1) & ~bad
        floor_frames += int(silent.sum())
        if beta == 0.0:                                                  # no smoothing: D = den = 0 gives the floor
            assert (G0[silent] == g_min).all()
        if call == 1:
            assert seen[1] == 0 and not got["G"][1].any() and got["N"][1].tobytes() == st["N"][1].tobytes()
        if call == 2:                                                                                 # fresh: the old N and D of slot 1 do not enter
            stale = dict(st, N=st["N"] + 100, D=st["D"] + 100)
            stale["N"][0], stale["D"][0] = st["N"][0], st["D"][0]
            again = _run(nat, su, w, hop, offsets, stale)
            assert again["G"].tobytes() == got["G"].tobytes() and again["N"].tobytes() == got["N"].tobytes()
        st = _state_of(got)
    assert nan_frames >= 6 and floor_frames >= 3            # the NaN, Inf and overflowing windows; the windows of zeros


# ------------------------------------------------------------------ 3. promises on the bytes

@pytest.mark.parametrize("F1", [1, 2, 3])
@pytest.mark.parametrize("n_fft,hop_s,shape", [(64, 32, (5, 96, 40)), (32, 4, (5, 95, 37)), (1024, 128, (4, 700, 0)), (512, 256, (4, 300, 300))])
def test_the_cut_of_the_stream_does_not_show(nat, n_fft, hop_s, shape, F1):
    """Two calls on F1 and F - F1 windows, the second with the first's state, against one call on F windows: outputs and state bit for bit."""
    F, N, hop = shape
    rng = np.random.default_rng([n_fft, hop_s, F1])
    n, m_total, opd = 5, 7, 2
    su = Setup(rng.permutation(m_total)[:n], rng.uniform(0, 6, (3, n)), opd, _window(n_fft, hop_s), hop_s, lag=3, den_mode=F1 % 2)
    offsets = [2 * opd, 0]
    w = _frames(rng, F, m_total, N)
    one = _run(nat, su, w, hop, offsets, _fresh(n, 2, n_fft, 3))
    a = _run(nat, su, w[:F1], hop, offsets, _fresh(n, 2, n_fft, 3))
    b = _run(nat, su, w[F1:], hop, offsets, _state_of(a))
    assert a["count"] + b["count"] == one["count"] > 0 and a["call_status"] == b["call_status"] == 0
    for k in ("G", "num", "den"):
        joined = np.concatenate([a[k][:, :a["count"]], b[k][:, :b["count"]]], axis=1)
        assert joined.tobytes() == one[k][:, :one["count"]].tobytes(), k
    _same_state(b, one)
    assert b["steer"].tobytes() == one["steer"].tobytes()


@pytest.mark.parametrize("n_fft,hop_s,shape,n", [(32, 16, (3, 96, 40), 3), (256, 128, (2, 256, 128), 64), (1024, 256, (1, 1500, 0), 6)])
def test_what_does_not_enter(nat, n_fft, hop_s, shape, n):
    """m_total and the rows the microphones occupy, slots behind the last, and every pointer 4 or 12 bytes further: the same bytes."""
    F, N, hop = shape
    rng = np.random.default_rng([n_fft, n])
    opd, lag = 4, 2
    tau = rng.uniform(0, 6, (5, n))
    win = _window(n_fft, hop_s)
    x = _frames(rng, F, n, N)                                             # the microphones' windows, in tau's order
    offsets = [opd, 3 * opd]
    base = _run(nat, Setup(np.arange(n), tau, opd, win, hop_s, lag=lag), x, hop, offsets, _fresh(n, 2, n_fft, lag))
    assert base["count"] > 0 and np.isfinite(base["G"]).all()
    perm = rng.permutation(n + 3)[:n]
    wide = _frames(rng, F, n + 3, N)
    wide[:, perm] = x
    moved = _run(nat, Setup(perm, tau, opd, win, hop_s, lag=lag), wide, hop, offsets, _fresh(n, 2, n_fft, lag), off=1)
    for k in ("G", "num", "den", "steer"):
        assert moved[k].tobytes() == base[k].tobytes(), k
    _same_state(moved, base)
    more = _run(nat, Setup(perm, tau, opd, win, hop_s, lag=lag), wide, hop, offsets + [0, -1, 2 * opd], _fresh(n, 5, n_fft, lag), off=3)
    for k in ("G", "num", "den", "steer", "N", "D"):
        assert more[k][:2].tobytes() == base[k].tobytes(), k
    assert more["hist"].tobytes() == base["hist"].tobytes() and more["words"][:4].tolist() == base["words"].tolist() and more["status"] == [0, 0, 0, 1, 0]


def test_a_frames_index_does_not_enter(nat):
    """The same windows twice in one call, beta = 0: the frames of the second half that do not reach into the first see the samples of
    the single call's frames that do not reach into the history, and give their bytes."""
    rng = np.random.default_rng(21)
    n, n_fft, hop_s, N = 3, 32, 16, 96
    su = Setup(np.arange(n), rng.uniform(0, 6, (2, n)), 1, _window(n_fft, hop_s), hop_s, beta=0.0)
    x = _frames(rng, 1, n, N)
    once = _run(nat, su, x, 0, [1, 0], _fresh(n, 2, n_fft, 0))
    twice = _run(nat, su, np.concatenate([x, x]), 0, [1, 0], _fresh(n, 2, n_fft, 0))
    assert (once["count"], twice["count"]) == (6, 12) and PN.frame_starts(0, N, n_fft, hop_s, 0)[1] == 0
    for k in ("G", "num", "den"):
        assert twice[k][:, 7:12].tobytes() == once[k][:, 1:6].tobytes(), k


@pytest.mark.parametrize("n_fft,hop_s", [(32, 8), (512, 256), (1024, 256)])
def test_a_nan_reaches_only_its_covering_frames(nat, n_fft, hop_s):
    rng = np.random.default_rng([n_fft, hop_s, 9])
    n, opd, lag = 4, 1, 3
    su = Setup(np.arange(n), rng.uniform(0, 6, (2, n)), opd, _window(n_fft, hop_s) + np.float32(0.01), hop_s, lag=lag)      # (no zero weight)
    N = 6 * n_fft + 5
    w = _frames(rng, 1, n, N)
    clean = _run(nat, su, w, 0, [0, 1], _fresh(n, 2, n_fft, lag))
    at = 2 * n_fft + hop_s // 2 + 1
    bad = w.copy()
    bad[0, 2, at] = np.nan
    got = _run(nat, su, bad, 0, [0, 1], _fresh(n, 2, n_fft, lag))
    starts = PN.frame_starts(0, N, n_fft, hop_s, lag)
    hit = np.array([s <= at < s + n_fft for s in starts])
    assert hit.sum() == n_fft // hop_s and got["count"] == len(starts)
    for b in range(2):
        assert np.isnan(got["G"][b, :len(starts)][hit]).all() and np.isfinite(got["G"][b, :len(starts)][~hit]).all()
    first = int(np.flatnonzero(hit)[0])
    assert got["G"][:, :first].tobytes() == clean["G"][:, :first].tobytes()
    assert np.isfinite(got["N"]).all() and np.isfinite(got["D"]).all() and got["words"].tolist() == clean["words"].tolist()
    # beta > 0: the frames behind the NaN continue from the state the NaN frames left alone -- the restatement says how
    _check_recursion(su, got, _fresh(n, 2, n_fft, lag), [0, 1], 0)


def test_zero_rows_give_the_floor(nat):
    su = Setup(np.arange(3), np.zeros((1, 3)), 1, _window(32, 16), 16, g_min=0.125)
    got = _run(nat, su, np.zeros((2, 3, 64), np.float32), 0, [0], _fresh(3, 1, 32, 0))
    assert got["count"] == 8 and (got["G"] == np.float32(0.125)).all() and not got["N"].any() and not got["D"].any() and got["words"].tolist() == [0, 0, 1]


def test_a_corrupt_state_is_reported_and_nothing_moves(nat):
    n_fft, hop_s, n = 32, 16, 3
    rng = np.random.default_rng(13)
    su = Setup(np.arange(n), rng.uniform(0, 4, (2, n)), 1, _window(n_fft, hop_s), hop_s, lag=1)
    w = _frames(rng, 3, n, 96)
    st = _fresh(n, 2, n_fft, 1)
    for k in ("hist", "N", "D"):
        st[k] = np.abs(rng.standard_normal(st[k].shape)).astype(np.float32)
    for words in ([16, 0, 0, 0], [-1, 0, 1, 1], [5, 0, 2, 0], [5, 0, 0, -1], [1 << 30, 0, 0, 0], [-(1 << 31), 0, 1, 1]):
        st["words"] = np.array(words, np.int32)
        got = _run(nat, su, w, 40, [0, 1], st)
        assert (got["count"], got["call_status"], got["cap"]) == (0, 1, 8) and got["words"].tolist() == words
        assert not got["G"].any() and not got["num"].any() and not got["den"].any()
        _same_state(got, st)
    st["words"] = np.array([15, 77, 1, 0], np.int32)                      # the reserved word is not part of the state
    got = _run(nat, su, w, 40, [0, 1], st)
    assert (got["count"], got["call_status"]) == (8, 0) and got["words"].tolist() == [7, 0, 1, 1]


# ------------------------------------------------------------------ 4. postfilter.SpatialPostFilter under graph replay

def test_graph_replay_of_gains(nat):
    """SpatialPostFilter.gains captured after one warm-up call and replayed twice over fresh frames (and a moved slot), against eager calls
    on a second instance: bytes, counts and the carried state."""
    torch = util.torch_gpu()
    import postfilter
    N, hop, F, M = 64, 24, 3, 6
    rng = np.random.default_rng(61)
    tau = rng.uniform(0, 5, (4, 4))
    batches = [(rng.standard_normal((F, M, N)) * 0.3).astype(np.float32) for _ in range(3)]
    rows = [np.array([2, 0], np.int32), np.array([2, 3], np.int32), np.array([-1, 3], np.int32)]
    make = lambda: postfilter.SpatialPostFilter(tau, [4, 1, 0, 3], 2, 1, hop, m_total=M, n_fft=32, hop_s=16, lag=2, den="beam")
    eager_pf, eager = make(), []
    for c in range(3):
        g, count, status = eager_pf.gains(torch.from_numpy(batches[c]).cuda(), torch.from_numpy(rows[c]).cuda())
        torch.cuda.synchronize()
        eager.append((g.cpu().numpy(), count.cpu().numpy().copy(), status.cpu().numpy().copy()))
        assert eager[-1][1].tolist() == [eager_pf.last_count, 0]
    assert [e[1][0] for e in eager] == [4, 5, 4] and eager[2][2].tolist() == [1, 0] and np.abs(eager[1][0]).max() > 0
    pf = make()
    x, offs = torch.from_numpy(batches[0]).cuda(), torch.from_numpy(rows[0]).cuda()
    pf.gains(x, offs)                                                    # the warm-up call: batch 0 (it also caches the adaptive array)
    carried = tuple(t.data_ptr() for t in (pf.hist, pf.num, pf.den_state, pf.state, pf.count, pf.status, pf.steer))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g, count, status = pf.gains(x, offs)
    assert carried == tuple(t.data_ptr() for t in (pf.hist, pf.num, pf.den_state, pf.state, pf.count, pf.status, pf.steer))
    for c in (1, 2):
        x.copy_(torch.from_numpy(batches[c]).cuda())
        offs.copy_(torch.from_numpy(rows[c]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert count.cpu().numpy().tolist() == eager[c][1].tolist() and status.cpu().numpy().tolist() == eager[c][2].tolist()
        assert g.cpu().numpy().tobytes() == eager[c][0].tobytes()
    for name in ("hist", "num", "den_state", "state", "steer"):
        assert getattr(pf, name).cpu().numpy().tobytes() == getattr(eager_pf, name).cpu().numpy().tobytes(), name
    pf.reset()
    assert all(not getattr(pf, k).cpu().numpy().any() for k in ("hist", "num", "den_state", "state", "count")) and pf.last_count == 0


# ------------------------------------------------------------------ 5. the chain and the figure

def test_the_scene_through_the_chain(nat):
    """The host test's scene (sensor noise 0.2, seed 0) as windows of 256 every 128 samples through StreamBeamformer("pad").listen ->
    SpatialPostFilter.push -> Enhancer, in batches of 64 windows; the SNR behind the filter by the shadow method (the gains of the
    mixture, from a second SpatialPostFilter, pushed over the tones' beam and the noise's beam) beside the restatement's, which filters the
    ideally aligned beam: whole-sample delays keep the beam's noise white and cost the 6.1 kHz tone under 0.3 dB, a tenth of the power."""
    torch = util.torch_gpu()
    import enhance
    import filtersum_np as fsn
    import postfilter
    import stream
    from interface import config
    from lib import directions
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=256, MAX_RES_X=fsn.GRID[0], MAX_RES_Y=fsn.GRID[1], N_TAPS=8)
    M, N, hop, batch = 64, 256, 128, 64
    tau = np.asarray(directions.calculate_delays(), np.float64).reshape(-1, M)
    assert np.allclose(tau, PN.scene_tau(), rtol=0, atol=1e-6)
    whole = tau.astype(int).astype(np.int32).ravel()
    nat.lib.load_coefficients_pad(nat.iptr(whole), whole.size); nat.check()
    s, parts, active = PN.scene(0)
    L = s.size
    look = fsn.flat(fsn.LOOK)
    offsets = torch.tensor([look * M], dtype=torch.int32, device="cuda")

    def windows(sig):                                                    # [F, M, N]: window f ends at stream sample (f + 1) * hop
        padded = np.concatenate([np.zeros((M, N - hop), np.float32), sig.astype(np.float32)], axis=1)
        return np.ascontiguousarray(np.stack([padded[:, f * hop:f * hop + N] for f in range(L // hop)]))

    comp = {k: windows(v) for k, v in parts.items()}
    comp["mix"] = windows(sum(parts.values()))
    sbs = {k: stream.StreamBeamformer("pad", hop=hop, mics=np.arange(M, dtype=np.int32)) for k in comp}
    pf = postfilter.SpatialPostFilter.for_listener(sbs["mix"], slots=1)
    pf2 = postfilter.SpatialPostFilter.for_listener(sbs["mix"], slots=1, tau=tau)
    assert (pf.n_fft, pf.hop_s, pf.hop, pf.lag, pf.beta, pf.g_min, pf.den, pf.offset_per_dir, pf.n) == (256, 128, hop, 0, 0.8, 0.1, "mics", M, M)
    ens = {k: enhance.Enhancer(rows=1, hop=hop) for k in comp}
    beams, outs = {k: [] for k in comp}, {k: [] for k in comp}
    for f0 in range(0, L // hop, batch):
        d = {k: torch.from_numpy(v[f0:f0 + batch]).cuda() for k, v in comp.items()}
        out = {k: sbs[k].listen(d[k], offsets, mic_gain=1.0)[0] for k in comp}
        clean, count, status = pf.push(ens["mix"], d["mix"], out["mix"], offsets)
        g, _, _ = pf2.gains(d["mix"], offsets)
        assert count.cpu().numpy().tolist() == [batch, 0] and status.cpu().numpy().tolist() == [0]
        outs["mix"].append(clean.cpu().numpy()[0])
        for k in parts:
            outs[k].append(ens[k].push(out[k], gains=g)[0].cpu().numpy()[0])
        for k in comp:
            beams[k].append(sbs[k].audio(out[k]).cpu().numpy()[0])
            sbs[k].advance(d[k])
    beams = {k: np.concatenate(v) for k, v in beams.items()}
    outs = {k: np.concatenate(v) for k, v in outs.items()}
    assert np.abs(outs["mix"] - sum(outs[k] for k in parts)).max() < 1e-4       # pf.push is pf2.gains + Enhancer.push, and that is linear
    fig = PN.figures({k: beams[k] for k in parts}, {k: outs[k] for k in parts}, s, active, 256)
    host = PN.host_scene(0)
    print("device chain: SNR over the active stretches %.2f dB in, %.2f dB out, noise %.2f dB; restatement (float64, the ideally aligned beam): %.2f dB in, %.2f dB out"
          % (fig["snr_in"], fig["snr_out"], fig["noise"], host["snr_in"], host["snr_out"]))
    RATIOS["chain SNR out, device - restatement (dB)"] = float(fig["snr_out"] - host["snr_out"])
    assert abs(fig["snr_out"] - host["snr_out"]) <= 0.5


def test_print_the_ratios():
    for name in sorted(RATIOS):
        print("largest error / bound, %s: %.4f" % (name, RATIOS[name]))
