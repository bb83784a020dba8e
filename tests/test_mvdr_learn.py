"""GPU (-m gpu): bf_mvdr_learn_device and FilterSumListener.learn / reaim / forget_all against the host statements in float64
(filtersum.mvdr_learn, design_mvdr_learned; tests/mvdr_learn_np.py restates them with the intermediates) and against
bf_mvdr_design_device, whose bytes the call must give at the settings where the two are the same operations.

As in tests/test_mvdr_design.py every output of every call, and the state, sits between canaries, and the stages are compared in order
by that file's _check_stages, bounds unchanged: a chain here has at most a few hundred roundings, as there."""
import numpy as np
import pytest

import filtersum_np as fsn
import lcmv_np
import mvdr_learn_np as mln
import mvdr_np
import test_mvdr_design as design_tests
import util
from support import nat_restoring as nat, scene_tau
from util import CANARY_VALUE

pytestmark = pytest.mark.gpu

_cplx, _worst = design_tests._cplx, design_tests._worst
NAMES = ["used", "snap", "cov", "chol", "gains", "taps", "status", "fallback"]


class State:
    """d_acc and d_mass between canaries, empty (zero) to begin with."""

    def __init__(self, K, m):
        torch = util.torch_gpu()
        self.K, self.m = K, m
        (self.acc_buf, self.acc), (self.mass_buf, self.mass) = util.canaried((K, m, m, 2), torch.float64), util.canaried((1,), torch.float64)
        self.acc.zero_()
        self.mass.zero_()

    def host(self):
        """-> (raw float64 [K, m, m, 2], mass float), the canaries checked."""
        assert util.intact(self.acc_buf, self.acc.numel()) and util.intact(self.mass_buf, 1)
        return self.acc.cpu().numpy().reshape(self.K, self.m, self.m, 2), float(self.mass.cpu().numpy()[0])

    def bytes(self):
        raw, _ = self.host()
        return raw.tobytes() + self.mass.cpu().numpy().tobytes()


def _learn(nat, st, frames, mics, tau, offsets, step, T, bins, loading, seg_first, seg_hop, segs, window=None, weights=None, forget=1.0, N=None, expect_rc=0,
           null_snap=False):
    """One call on device copies; frames None is the re-aim (N then says what N_SAMPLES is; d_snap points at canaries that must survive).
    -> test_mvdr_design._design's dict plus used int32 [2], acc complex128 [K, n, n], total (the mass), raw["acc"]."""
    torch = util.torch_gpu()
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    mics = np.ascontiguousarray(mics, dtype=np.int32)
    if frames is None:
        F, m_total = 0, int(mics.max()) + 1
        d_x = None
    else:
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        F, m_total, N = frames.shape
        d_x = torch.from_numpy(frames).cuda()
    util.configure_small(N)
    dirs, m = tau.shape
    S, K, P = offsets.size, len(bins), max(F, 1) * max(segs, 1)
    d_tau, d_off = torch.from_numpy(tau).cuda(), torch.from_numpy(offsets).cuda()
    d_win = None if window is None or F == 0 else torch.from_numpy(np.ascontiguousarray(window, dtype=np.float64)).cuda()
    d_w = None if weights is None or F == 0 else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).cuda()
    shapes = [((2,), torch.int32), ((P, K, m, 2), torch.float64), ((K, m, m, 2), torch.float64), ((K, m, m, 2), torch.float64), ((S, K, m, 2), torch.float64),
              ((S, m, T), torch.float32), ((S,), torch.int32), ((K,), torch.int32)]
    bufs = [util.canaried(shape, dtype) for shape, dtype in shapes]
    before = st.bytes()
    ptr = [view.data_ptr() for _, view in bufs]
    rc = nat.lib.bf_mvdr_learn_device(None if d_x is None else d_x.data_ptr(), m_total, F, nat.iptr(mics), m, seg_first, seg_hop, segs,
                                      None if d_win is None else d_win.data_ptr(), None if d_w is None else d_w.data_ptr(), forget, d_tau.data_ptr(), dirs,
                                      d_off.data_ptr(), S, step, T, int(bins[0]), int(bins[-1]), loading, st.acc.data_ptr(), st.mass.data_ptr(), ptr[0],
                                      None if null_snap else ptr[1], *ptr[2:], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (buf, view), (shape, _) in zip(bufs, shapes):
        assert util.intact(buf, view.numel()), shape
    untouched = lambda view: bool((view.cpu().numpy() == view.cpu().numpy().dtype.type(CANARY_VALUE)).all())
    if expect_rc != 0:
        assert rc == expect_rc and nat.lib.bf_last_error()
        nat.lib.bf_clear_error()
        assert all(untouched(view) for _, view in bufs) and st.bytes() == before          # nothing was enqueued
        return None
    assert rc == 0, nat.lib.bf_last_error()
    nat.check()
    raw = {name: view.cpu().numpy().reshape(shape) for name, (_, view), (shape, _) in zip(NAMES, bufs, shapes)}
    if F == 0:
        assert untouched(bufs[1][1]) and st.bytes() == before                             # the re-aim writes no snapshot and no state
    out = {name: (_cplx(raw[name]) if raw[name].dtype == np.float64 else raw[name]) for name in NAMES}
    raw["acc"], out["total"] = st.host()
    out["acc"], out["raw"] = _cplx(raw["acc"]), raw
    return out


def _hermitian_bits(raw, what):
    """[K, n, n, 2] as the device wrote it: the real part symmetric and the imaginary part antisymmetric bit for bit, the diagonal's zero."""
    re, im = np.ascontiguousarray(raw[..., 0]), np.ascontiguousarray(raw[..., 1])
    n = re.shape[1]
    off = np.broadcast_to(~np.eye(n, dtype=bool)[None], im.shape)
    assert np.array_equal(re.view(np.int64), np.ascontiguousarray(re.transpose(0, 2, 1)).view(np.int64)), (what, "the real part is not symmetric bit for bit")
    assert np.array_equal(im.view(np.int64)[off], np.ascontiguousarray(-im.transpose(0, 2, 1)).view(np.int64)[off]), (what, "the imaginary part is not antisymmetric bit for bit")
    assert not im[:, np.arange(n), np.arange(n)].any(), (what, "the diagonal's imaginary part is not zero")


def _check_state(got, r, what):
    """d_acc against the host's with the covariance bound at the state's scale, Hermitian bit for bit; d_mass to 4 ulp; d_used equal."""
    assert got["used"].tolist() == r["used"].tolist(), (what, "used", got["used"], r["used"])
    assert abs(got["total"] - r["total"]) <= 4.0 * np.spacing(r["total"]), (what, "mass", got["total"], r["total"])
    diag = np.sqrt(np.einsum("kaa,kbb->kab", r["acc"].real, r["acc"].real))
    at, ratio = _worst(np.abs(got["acc"] - r["acc"]), 1e-11 * diag)
    assert ratio <= 1.0, (what, "state: worst entry (bin, a, b) %s at %.3g of the bound" % (at, ratio))
    _hermitian_bits(got["raw"]["acc"], (what, "state"))
    return ratio


def _case_args(case):
    import filtersum
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading = case[:11]
    return dict(step=lcmv_np.offset_per_dir(n), T=T, bins=filtersum.band_bins(T, band, mln.FS), loading=loading, seg_first=seg_first, seg_hop=seg_hop, segs=segs)


def _case_state(case):
    n, T, band = case[0], case[3], case[9]
    import filtersum
    return State(filtersum.band_bins(T, band, mln.FS).size, n)


# ------------------------------------------------------------------ 1. the definition table, stage by stage

@pytest.fixture(scope="module")
def host_table():
    """The host chain of every case (two calls on one state), computed once, and the design behind either call for every row of
    offsets, with the input condition asserted BEFORE the device is consulted: cond(R') <= 1e4 at every bin."""
    table = {}
    for case in mln.TABLE:
        batches = mln.case_batches(case)
        rows = []
        for name, row in lcmv_np.offset_rows(case[0], case[2], case[3], 0):
            r1, r2 = mln.case_chain(case, row, batches)
            for r in (r1, r2):
                assert r["conds"].max() <= 1e4 and not r["fallback"].any(), (mln.case_id(case), float(r["conds"].max()))
            rows.append((name, row, r1, r2))
        table[mln.case_id(case)] = rows
    return table


@pytest.mark.parametrize("case", mln.TABLE, ids=mln.case_id)
def test_matches_the_host_chain_stage_by_stage(nat, host_table, case):
    """Every row of offsets of the case (tests/lcmv_np.offset_rows), each as two calls on one state that starts empty: the first batch
    with unit weights, then the table's batch with its weights; both with the case's forget.  After either call the stages are held to
    _check_stages' bounds and the state to _check_state's."""
    forget = case[13]
    first, frames, mics, tau, win, weights = mln.case_inputs(case)
    kw = _case_args(case)
    worst = np.zeros(6)
    for name, row, r1, r2 in host_table[mln.case_id(case)]:
        st = _case_state(case)
        for call, x, w, r in (("first batch", first, None, r1), ("the table's batch", frames, weights, r2)):
            what = (mln.case_id(case), name, call)
            got = _learn(nat, st, x, mics, tau, row, window=win, weights=w, forget=forget, **kw)
            res = design_tests._check_stages(got, r, kw["loading"], what)
            worst = np.maximum(worst, res[:5] + (_check_state(got, r, what),))
    print("%s: worst error as a fraction of its bound: snapshots %.3g, covariance %.3g, factor %.3g, gains %.3g, taps %.3g, state %.3g" % ((mln.case_id(case),) + tuple(worst)))


# ------------------------------------------------------------------ 2. the same bytes as bf_mvdr_design_device

@pytest.mark.parametrize("case", [mvdr_np.TABLE[4], mvdr_np.TABLE[3]], ids=mvdr_np.case_id)
def test_same_bytes_as_the_design_call_from_an_empty_state(nat, case):
    """Empty state, forget 1, weights NULL and again all 1.0: the chains are bf_mvdr_design_device's operations, so all seven of its
    outputs come out byte for byte; the mass is P exactly."""
    import filtersum
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window = case
    frames, mics, tau, win = mvdr_np.case_inputs(case)
    bins = filtersum.band_bins(T, band, mvdr_np.FS)
    name, row = lcmv_np.offset_rows(n, S, T, 0)[-1]
    want = design_tests._design(nat, frames, mics, tau, row, lcmv_np.offset_per_dir(n), T, bins, loading, seg_first, seg_hop, segs, window=win)
    for weights in (None, np.ones(F)):
        st = State(len(bins), n)
        got = _learn(nat, st, frames, mics, tau, row, lcmv_np.offset_per_dir(n), T, bins, loading, seg_first, seg_hop, segs, window=win, weights=weights, forget=1.0)
        assert got["total"] == float(F * segs) and got["used"].tolist() == [F, 0]
        for key in ("snap", "cov", "chol", "gains", "taps", "status", "fallback"):
            assert got["raw"][key].tobytes() == want["raw"][key].tobytes(), (name, key, "weights NULL" if weights is None else "weights 1.0")


# ------------------------------------------------------------------ 3. split invariance, and two runs

def test_a_batch_split_in_two_calls_gives_the_same_bits(nat):
    """n = 3, 7 frames of 5 segments: frames 0 .. 3 then 4 .. 6 (snapshot 20: inside the second staged chunk) on one state against one
    call on all 7, both from the state the first batch leaves; and the whole run twice.  d_acc, d_mass, d_cov, d_gains, d_taps by bytes."""
    case = mln.by_n(3)
    forget = case[13]
    first, frames, mics, tau, win, weights = mln.case_inputs(case)
    kw = _case_args(case)
    row = lcmv_np.offset_rows(case[0], case[2], case[3], 0)[0][1]

    def run(split):
        st = _case_state(case)
        _learn(nat, st, first, mics, tau, row, forget=forget, **kw)
        if split:
            _learn(nat, st, frames[:4], mics, tau, row, weights=weights[:4], forget=forget, **kw)
            got = _learn(nat, st, frames[4:], mics, tau, row, weights=weights[4:], forget=forget, **kw)
        else:
            got = _learn(nat, st, frames, mics, tau, row, weights=weights, forget=forget, **kw)
        return st.bytes(), got

    (whole_state, whole), (split_state, split), (again_state, again) = run(False), run(True), run(False)
    assert whole["used"].tolist() == [4, 0] and split["used"].tolist() == [1, 0]
    assert whole_state == split_state and whole_state == again_state
    for key in ("cov", "gains", "taps"):
        assert whole["raw"][key].tobytes() == split["raw"][key].tobytes(), key
    for key in NAMES:
        assert whole["raw"][key].tobytes() == again["raw"][key].tobytes(), key


# ------------------------------------------------------------------ 4. skips

def test_skipped_frames_leave_the_state_alone_and_an_empty_state_falls_back(nat):
    """Weights 0, -0.0, NaN, Inf, -1, 0 on a learned state: d_acc and d_mass keep their bytes, d_used = (0, 3), the snapshots are written
    all the same and the taps are the re-aim's on that state.  The same batch on the EMPTY state: still all-zero bytes, fallback at every
    bin, and the taps within 2^-23 of bf_lcmv_design_device's beam without nulls (as test_silence_and_a_nan... compares)."""
    torch = util.torch_gpu()
    case = mln.by_n(3)
    n, S, T, N, forget = case[0], case[2], case[3], case[4], case[13]
    first, frames, mics, tau, win, _ = mln.case_inputs(case)
    kw = _case_args(case)
    step, bins = kw["step"], kw["bins"]
    row = np.array([5 * step, -1, 2 * step], dtype=np.int32)
    weights = np.array([0.0, -0.0, np.nan, np.inf, -1.0, 0.0])
    st = _case_state(case)
    _learn(nat, st, first, mics, tau, row, forget=forget, **kw)
    before = st.bytes()
    got = _learn(nat, st, frames[:6], mics, tau, row, weights=weights, forget=forget, **kw)
    assert st.bytes() == before and got["used"].tolist() == [0, 3] and got["status"].tolist() == [0, 1, 0] and not got["fallback"].any()
    want_snap, _ = mln.snapshots(frames[:6], mics, T, bins, kw["seg_first"], kw["seg_hop"], kw["segs"], None)
    assert np.abs(got["snap"] - want_snap).max() <= 1e-12 * np.abs(frames[:6]).sum(axis=2).max()
    aim = _learn(nat, st, None, mics, tau, row, N=N, forget=forget, **kw)
    assert aim["used"].tolist() == [0, 0]
    for key in ("cov", "chol", "gains", "taps", "status", "fallback"):
        assert got["raw"][key].tobytes() == aim["raw"][key].tobytes(), key

    empty = _case_state(case)
    got = _learn(nat, empty, frames[:6], mics, tau, row, weights=weights, forget=forget, **kw)
    assert not any(empty.bytes()) and got["used"].tolist() == [0, 3] and got["fallback"].tolist() == [1] * len(bins) and got["status"].tolist() == [0, 1, 0]
    assert not got["cov"].any() and np.array_equal(got["chol"], np.broadcast_to(np.eye(n), got["chol"].shape)) and not got["taps"][1].any()
    d_tau = torch.from_numpy(np.ascontiguousarray(tau)).cuda()
    for i in (0, 2):
        d_off = torch.from_numpy(row[i:i + 1].copy()).cuda()
        g, t, k, s = (torch.zeros((1, len(bins), n, 2), dtype=torch.float64, device="cuda"), torch.zeros((1, n, T), dtype=torch.float32, device="cuda"),
                      torch.zeros((1, len(bins), 1), dtype=torch.int32, device="cuda"), torch.ones((1,), dtype=torch.int32, device="cuda"))
        assert nat.lib.bf_lcmv_design_device(d_tau.data_ptr(), tau.shape[0], n, d_off.data_ptr(), 1, step, T, int(bins[0]), int(bins[-1]), 0.95, g.data_ptr(),
                                             t.data_ptr(), k.data_ptr(), s.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        want = t.cpu().numpy()[0].astype(np.float64)
        assert s.item() == 0 and (np.abs(got["taps"][i].astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want).max()).all()


# ------------------------------------------------------------------ 5. the re-aim

def _check_design(got, r, what):
    """What a re-aim writes, against state_stages on the device's OWN state, with _check_stages' bounds: the covariance 1e-11 sqrt(R_aa
    R_bb) and Hermitian bit for bit, the gains 1e-9 of the largest of a (beam, bin), the taps 2^-23 of a beam's largest."""
    assert np.array_equal(got["status"], r["status"]) and np.array_equal(got["fallback"], r["fallback"]), (what, got["status"], got["fallback"])
    diag = np.sqrt(np.einsum("kaa,kbb->kab", r["cov"].real, r["cov"].real))
    at, ratio = _worst(np.abs(got["cov"] - r["cov"]), 1e-11 * diag)
    assert ratio <= 1.0, (what, "covariance: worst entry (bin, a, b) %s at %.3g of the bound" % (at, ratio))
    _hermitian_bits(got["raw"]["cov"], (what, "covariance"))
    for i in range(r["status"].size):
        if r["status"][i] == 1:
            assert not got["taps"][i].any() and not got["raw"]["gains"][i].any(), (what, "slot %d is no source but not silent" % i)
            continue
        scale = np.abs(r["gains"][i]).max(axis=1, keepdims=True)
        at, ratio = _worst(np.abs(got["gains"][i] - r["gains"][i]), 1e-9 * np.broadcast_to(scale, r["gains"][i].shape))
        assert ratio <= 1.0, (what, "gains: beam %d, worst entry (bin, mic) %s at %.3g of the bound" % (i, at, ratio))
        want = r["taps"][i].astype(np.float64)
        at, ratio = _worst(np.abs(got["taps"][i].astype(np.float64) - want), np.full(want.shape, 2.0 ** -23 * np.abs(want).max()))
        assert ratio <= 1.0, (what, "taps: beam %d, worst entry (mic, t) %s at %.3g of the bound" % (i, at, ratio))


def test_reaim_designs_from_the_state_as_it_stands(nat):
    """n = 70: learn, then frames = 0 with another row of offsets -- a -1 and a duplicate in it; d_signals, d_weights, d_window null.  The
    state keeps its bytes and d_snap's buffer its canaries (_learn asserts both), gains and taps are design_mvdr_learned's on the device's
    own d_acc / d_mass, and four slots designed alone are the first four of eight."""
    case = mln.by_n(70)
    n, T, N, band, loading, forget = case[0], case[3], case[4], case[9], case[10], case[13]
    first, frames, mics, tau, win, weights = mln.case_inputs(case)
    kw = _case_args(case)
    step = kw["step"]
    st = _case_state(case)
    learned = _learn(nat, st, frames, mics, tau, lcmv_np.offset_rows(n, case[2], T, 0)[0][1], weights=weights, forget=forget, **kw)
    four = np.array([5, -1, 9, 5], dtype=np.int32) * np.array([step, 1, step, step], dtype=np.int32)
    eight = np.concatenate([four, np.array([3 * step, -1, step + 1, 12 * step], dtype=np.int32)])
    a = _learn(nat, st, None, mics, tau, four, N=N, **kw)
    b = _learn(nat, st, None, mics, tau, eight, N=N, forget=0.25, **dict(kw, seg_first=0, seg_hop=1, segs=1))      # forget and the segments play no part
    assert a["used"].tolist() == [0, 0] and a["status"].tolist() == [0, 1, 0, 0] and b["status"].tolist() == [0, 1, 0, 0, 0, 1, 1, 1]
    assert a["raw"]["acc"].tobytes() == learned["raw"]["acc"].tobytes() and a["total"] == learned["total"]
    _check_design(a, mln.state_stages(a["acc"], a["total"], tau, four, step, T, band, loading), "four slots")
    _check_design(b, mln.state_stages(a["acc"], a["total"], tau, eight, step, T, band, loading), "eight slots")
    assert a["raw"]["cov"].tobytes() == learned["raw"]["cov"].tobytes()
    for key in ("cov", "chol", "fallback"):
        assert a["raw"][key].tobytes() == b["raw"][key].tobytes(), key
    assert a["raw"]["gains"].tobytes() == b["raw"]["gains"][:4].tobytes() and a["taps"].tobytes() == b["taps"][:4].tobytes()
    assert a["taps"][0].tobytes() == a["taps"][3].tobytes() and a["taps"][0].any()


# ------------------------------------------------------------------ 6. function, through FilterSumListener


def test_weights_cure_self_cancellation_and_forgetting_follows_a_moved_interferer(nat, scene_tau):
    """The two scenes of tests/mvdr_learn_np.py, ONE slot on LOOK.  Each design starts from forget_all(); the interferer alone then goes
    through listen(): its power is within 1 dB of what the host design's taps leak (filtersum_np.filter_sum), the response towards
    LOOK is f0 within M T 2^-24 max|g|.  Learned from the look-free windows the beam is at least 6 dB better than learned from all
    fourteen; with forget 0.7 at least 3 dB better on the moved interferer than with forget 1.  The README's rows are printed."""
    torch = util.torch_gpu()
    import filtersum
    design_tests._scene_sizes()
    M, N, hop, T = mln.M, mln.N, mln.HOP, mln.T
    tau = scene_tau
    look = fsn.flat(fsn.LOOK)
    d_off = torch.tensor([look * M], dtype=torch.int32, device="cuda")
    fl = filtersum.FilterSumListener.for_slots(tau, 1, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    w = 2.0 * np.pi * fl.bins / T

    def leak(sc, host_state, name):
        """-> the device design's leak of sc's interferer through listen(), checked against the host design's."""
        alone, alone_prev = mvdr_np.cut(sc["interferer"])
        fl.advance(torch.from_numpy(alone_prev[None]).cuda())
        leak_dev = fsn.db(util.audio_power(fl, fl.listen(torch.from_numpy(alone).cuda())))
        dev = fl.taps_host().copy()
        host = mln.host_taps(host_state, tau)
        leak_host = fsn.db(mvdr_np.power(fsn.filter_sum(alone, fl.mics, host, hop, alone_prev)[:, 0, N - hop:]))
        print("%s: interferer %.1f dB, white-noise gain %.1f dB, look %+.2f dB; through listen() %.2f dB, the host design %.2f dB; mass %.1f"
              % ((name,) + mvdr_np.row(sc, dev[0]) + (leak_dev, leak_host, fl.d_mass.item())))
        assert abs(leak_dev - leak_host) <= 1.0, name
        e = np.abs(filtersum.response(dev[0], tau[look], w) - np.exp(-1j * w * (T - 1) / 2.0))
        assert (e <= M * T * 2.0 ** -24 * float(np.abs(dev[0]).max())).all(), (name, float(e.max()))
        assert abs(fl.d_mass.item() - host_state[1]) <= 4.0 * np.spacing(host_state[1])
        return leak_dev

    sc, train = mln.gated_scene(tau)
    d_train = torch.from_numpy(mvdr_np.cut(train)[0]).cuda()
    leaks = {}
    for name, weights in (("all 14 windows, weights 1", None), ("windows 7..13 only", np.array(mln.LOOK_FREE))):
        fl.forget_all()
        status, fallback, used = fl.learn(d_train, d_off, weights=None if weights is None else torch.from_numpy(weights).cuda(), loading=mvdr_np.LOADING,
                                          seg_hop=mvdr_np.SEG_HOP)
        torch.cuda.synchronize()
        assert status.tolist() == [0] and not fallback.any().item() and used.tolist() == [14 if weights is None else 7, 0] and fl.taps is None
        leaks[name] = leak(sc, mln.host_learn(None, train, weights, 1.0), "covariance learned from " + name)
    assert leaks["all 14 windows, weights 1"] - leaks["windows 7..13 only"] >= 6.0

    old, new, train_old, train_new = mln.moved_scenes(tau)
    d_old, d_new = torch.from_numpy(mvdr_np.cut(train_old)[0]).cuda(), torch.from_numpy(mvdr_np.cut(train_new)[0]).cuda()
    for forget in (1.0, 0.7):
        fl.forget_all()
        fl.learn(d_old, d_off, forget=forget)
        fl.learn(d_new, d_off, forget=forget)
        leaks[forget] = leak(new, mln.host_learn(mln.host_learn(None, train_old, None, forget), train_new, None, forget), "forget %.1f, the interferer moved" % forget)
    assert leaks[1.0] - leaks[0.7] >= 3.0

    fl.forget_all()
    status, fallback = fl.reaim(d_off)
    assert fallback.all().item() and status.tolist() == [0] and not fl.d_acc.any().item() and fl.d_mass.item() == 0.0
    with pytest.raises(ValueError):
        filtersum.FilterSumListener(np.zeros((1, M, T), dtype=np.float32), hop=hop).learn(d_train, d_off)      # not built by for_slots
    with pytest.raises(ValueError):
        filtersum.FilterSumListener(np.zeros((1, M, T), dtype=np.float32), hop=hop).reaim(d_off)
    for bad in (dict(forget=0.0), dict(forget=1.5), dict(forget=float("nan")), dict(loading=0.0), dict(seg_hop=0), dict(window=np.ones(T + 1)),
                dict(weights=torch.ones(14, device="cuda")), dict(weights=torch.ones(13, dtype=torch.float64, device="cuda")),
                dict(weights=torch.ones(14, dtype=torch.float64))):
        with pytest.raises(ValueError):
            fl.learn(d_train, d_off, **bad)
    with pytest.raises(ValueError):
        fl.learn(d_train, d_off.to(torch.int64))
    with pytest.raises(ValueError):
        fl.reaim(d_off, loading=-1.0)


# ------------------------------------------------------------------ 7. learn -> listen in one captured graph

def test_graph_learn_then_listen(nat, scene_tau):
    """learn(d_frames, d_off, forget 0.7) and listen(d_frames) captured as one stream after an eager warm-up and forget_all() (in place:
    the warm-up learned too).  Replayed, d_frames overwritten ON THE DEVICE with the moved interferer's windows, replayed again: a replay
    advances the state, so state and taps are, byte for byte, those of two eager calls from an empty state on a second listener; no
    tensor moved; the beams are filtersum_np.filter_sum with the device's own taps bit for bit."""
    torch = util.torch_gpu()
    import filtersum
    design_tests._scene_sizes()
    M, N, hop, T = mln.M, mln.N, mln.HOP, mln.T
    tau = scene_tau
    old, new, train_old, train_new = mln.moved_scenes(tau)
    (frames_old, prev_old), (frames_new, prev_new) = mvdr_np.cut(train_old), mvdr_np.cut(train_new)
    d_off = torch.tensor([fsn.flat(fsn.LOOK) * M], dtype=torch.int32, device="cuda")
    fl = filtersum.FilterSumListener.for_slots(tau, 1, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    d_frames = torch.from_numpy(frames_old).cuda()
    fl.advance(torch.from_numpy(prev_old[None]).cuda())
    out = [None]

    def step(listener, frames):
        listener.learn(frames, d_off, forget=0.7)
        out[0] = listener.listen(frames)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(fl, d_frames)                              # eager warm-up: the adaptive array is uploaded, the state and the workspaces allocated
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    tensors = ("d_taps", "d_acc", "d_mass", "d_used", "d_snap", "d_cov", "d_chol", "d_gains", "d_fallback")
    at = [getattr(fl, name).data_ptr() for name in tensors]
    fl.forget_all()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(fl, d_frames)
    captured = out[0]
    graph.replay()
    torch.cuda.synchronize()
    mass_once = fl.d_mass.item()
    d_frames.copy_(torch.from_numpy(frames_new).cuda())                # the interferer moved: only device memory changes
    fl.advance(torch.from_numpy(prev_new[None]).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert [getattr(fl, name).data_ptr() for name in tensors] == at
    got, got_taps = captured.cpu().numpy().copy(), fl.taps_host().copy()
    assert fl.d_used.tolist() == [14, 0] and fl.d_mass.item() > mass_once > 0.0

    eager = filtersum.FilterSumListener.for_slots(tau, 1, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    eager.advance(torch.from_numpy(prev_new[None]).cuda())
    step(eager, torch.from_numpy(frames_old).cuda())
    step(eager, torch.from_numpy(frames_new).cuda())
    torch.cuda.synchronize()
    for name in ("d_acc", "d_mass", "d_taps", "d_cov"):
        assert getattr(fl, name).cpu().numpy().tobytes() == getattr(eager, name).cpu().numpy().tobytes(), name
    assert got.tobytes() == out[0].cpu().numpy().tobytes()
    assert np.array_equal(util.bits(got), util.bits(fsn.filter_sum(frames_new, fl.mics, got_taps, hop, prev_new)))


# ------------------------------------------------------------------ 8. refusals worth a device: nothing may be enqueued

def test_refused_calls_leave_the_outputs_and_the_state_untouched(nat):
    case = mln.by_n(16)
    n, T, N, forget = case[0], case[3], case[4], case[13]
    first, frames, mics, tau, win, weights = mln.case_inputs(case)
    kw = _case_args(case)
    row = np.arange(4, dtype=np.int32) * kw["step"]
    st = _case_state(case)
    _learn(nat, st, first, mics, tau, row, forget=forget, **kw)                                                      # a state worth keeping
    assert _learn(nat, st, frames, mics, tau, row, weights=weights, forget=0.0, expect_rc=-1, **kw) is None
    assert _learn(nat, st, frames[:1], mics, tau, row, weights=weights[:1], forget=forget, expect_rc=-1, null_snap=True, **kw) is None
    assert _learn(nat, st, frames, mics, tau, row, weights=weights, forget=forget, expect_rc=-1, **dict(kw, seg_first=N - T - 6, seg_hop=7, segs=2)) is None
    got = _learn(nat, st, frames, mics, tau, row, weights=weights, forget=forget, **kw)                              # and the same call accepted
    assert got["status"].tolist() == [0, 0, 0, 0] and not got["fallback"].any() and got["used"].tolist() == [2, 0]
