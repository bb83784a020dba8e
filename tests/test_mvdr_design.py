"""GPU (-m gpu): bf_mvdr_design_device and FilterSumListener.adapt against the host design in float64 (filtersum.design_mvdr_slots;
tests/mvdr_np.py restates it with the snapshots, the covariance, the loaded matrix and its factor, which it does not return).

Every output of every call sits in the middle of a buffer of canaries, which must survive.  The device's summation orders, sines and
cosines are not NumPy's, so each stage is compared to roundoff at its own scale (the bounds are worked out where they are used), and
the stages are checked in order: the first one that fails is reported with its worst entry."""
import numpy as np
import pytest

import filtersum_np as fsn
import lcmv_np
import mvdr_np
import util
from support import nat_restoring as nat, scene_tau
from util import CANARY_VALUE

pytestmark = pytest.mark.gpu


def _scene_sizes():
    from interface import config
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=mvdr_np.N, MAX_RES_X=fsn.GRID[0], MAX_RES_Y=fsn.GRID[1], N_TAPS=8)


def _cplx(a):
    return a[..., 0] + 1j * a[..., 1]


def _design(nat, frames, mics, tau, offsets, step, T, bins, loading, seg_first, seg_hop, segs, window=None, expect_rc=0, n=None):
    """One call on device copies (N_SAMPLES configured to the frames') -> dict(snap complex128 [P, K, n], cov, chol [K, n, n], gains
    [S, K, n], taps float32 [S, n, T], status int32 [S], fallback int32 [K], raw = the float64 (re, im) arrays as the device wrote them)."""
    torch = util.torch_gpu()
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    mics = np.ascontiguousarray(mics, dtype=np.int32)
    F, m_total, N = frames.shape
    util.configure_small(N)
    dirs, n = tau.shape[0], (tau.shape[1] if n is None else n)
    S, K, P = offsets.size, len(bins), F * max(segs, 1)
    d_x, d_tau, d_off = torch.from_numpy(frames).cuda(), torch.from_numpy(tau).cuda(), torch.from_numpy(offsets).cuda()
    d_win = None if window is None else torch.from_numpy(np.ascontiguousarray(window, dtype=np.float64)).cuda()
    m = tau.shape[1]
    names = ["snap", "cov", "chol", "gains", "taps", "status", "fallback"]
    shapes = [((P, K, m, 2), torch.float64), ((K, m, m, 2), torch.float64), ((K, m, m, 2), torch.float64), ((S, K, m, 2), torch.float64),
              ((S, m, T), torch.float32), ((S,), torch.int32), ((K,), torch.int32)]
    bufs = [util.canaried(shape, dtype) for shape, dtype in shapes]
    rc = nat.lib.bf_mvdr_design_device(d_x.data_ptr(), m_total, F, nat.iptr(mics), n, seg_first, seg_hop, segs, None if d_win is None else d_win.data_ptr(),
                                       d_tau.data_ptr(), dirs, d_off.data_ptr(), S, step, T, int(bins[0]), int(bins[-1]), loading,
                                       *[view.data_ptr() for _, view in bufs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (buf, view), (shape, _) in zip(bufs, shapes):
        assert util.intact(buf, view.numel()), shape
    if expect_rc != 0:
        assert rc == expect_rc and nat.lib.bf_last_error()
        nat.lib.bf_clear_error()
        for buf, view in bufs:                                        # nothing was enqueued
            assert (view.cpu().numpy() == view.cpu().numpy().dtype.type(CANARY_VALUE)).all()
        return None
    assert rc == 0, nat.lib.bf_last_error()
    nat.check()
    raw = {name: view.cpu().numpy().reshape(shape) for name, (_, view), (shape, _) in zip(names, bufs, shapes)}
    out = {name: (_cplx(raw[name]) if raw[name].dtype == np.float64 else raw[name]) for name in names}
    out["raw"] = raw
    return out


def _case_call(nat, case, row, **over):
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window = case
    import filtersum
    frames, mics, tau, win = mvdr_np.case_inputs(case)
    kw = dict(loading=loading, seg_first=seg_first, seg_hop=seg_hop, segs=segs, window=win)
    kw.update(over)
    return _design(nat, frames, mics, tau, row, lcmv_np.offset_per_dir(n), T, filtersum.band_bins(T, band, mvdr_np.FS), **kw)


# ------------------------------------------------------------------ 1. the definition table, stage by stage

@pytest.fixture(scope="module")
def host_table():
    """The host stages of every (case, row of offsets), computed once, with the input condition asserted BEFORE the device is
    consulted: cond(R') <= 1e4 at every bin (the loadings of the table keep n / loading + 1 below it)."""
    table = {}
    for case in mvdr_np.TABLE:
        n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window = case
        frames, mics, tau, win = mvdr_np.case_inputs(case)
        rows = []
        for name, row in lcmv_np.offset_rows(n, S, T, 0):
            r = mvdr_np.slot_stages(frames, mics, tau, row, lcmv_np.offset_per_dir(n), T, band, loading, seg_first, seg_hop, segs, win)
            assert r["conds"].max() <= 1e4, (mvdr_np.case_id(case), float(r["conds"].max()))
            rows.append((name, row, r))
        table[mvdr_np.case_id(case)] = rows
    return table


def _worst(err, bound):
    """-> (index of the entry with the largest err / bound, that ratio)."""
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return tuple(int(i) for i in at), float(ratio[at])


def _loaded_of(cov, loading, fallback):
    """R' from the DEVICE's covariance by the definition: the trace in ascending a, loading tr / n on the diagonal; I on a fallback bin."""
    K, n, _ = cov.shape
    out = np.empty_like(cov)
    for k in range(K):
        tr = 0.0
        for a in range(n):
            tr += cov[k, a, a].real
        out[k] = np.eye(n) if fallback[k] else cov[k] + (loading * tr / n) * np.eye(n)
    return out


def _check_stages(got, r, loading, what):
    """Stage by stage, in order; each assertion names the stage, the worst entry and its error as a multiple of the bound.
    snapshots : |dev - host| <= 1e-12 sum_t |win[t] x[t]|.  T <= 1024 roundings of 2^-53 come to 1.1e-13; the rest is slack for sincospi.
    covariance: |dev - host| <= 1e-11 sqrt(R_aa R_bb); Hermitian bit for bit; the diagonal's imaginary part exactly zero.
    factor    : strict upper exactly 0; |L L^H - R'| <= 1e-11 sqrt(R'_aa R'_bb), R' formed from the device's own covariance.
    gains     : |dev - host| <= 1e-9 max|G| per (beam, bin): 2^-53 x the cond cap 1e4 x about 1e3 of slack (tests/test_lcmv_design.py's bound).
    taps      : |dev - host| <= 2^-23 of the beam's largest tap."""
    assert np.array_equal(got["status"], r["status"]), (what, "status", got["status"], r["status"])
    assert np.array_equal(got["fallback"], r["fallback"]), (what, "fallback", got["fallback"], r["fallback"])
    at, ratio_s = _worst(np.abs(got["snap"] - r["snap"]), 1e-12 * np.broadcast_to(r["mass"][:, None, :], r["snap"].shape))
    assert ratio_s <= 1.0, (what, "snapshots: worst entry (p, bin, mic) %s at %.3g of the bound" % (at, ratio_s))
    diag = np.sqrt(np.einsum("kaa,kbb->kab", r["cov"].real, r["cov"].real))
    at, ratio_c = _worst(np.abs(got["cov"] - r["cov"]), 1e-11 * diag)
    assert ratio_c <= 1.0, (what, "covariance: worst entry (bin, a, b) %s at %.3g of the bound" % (at, ratio_c))
    re, im = got["raw"]["cov"][..., 0], got["raw"]["cov"][..., 1]
    n = re.shape[1]
    off = ~np.eye(n, dtype=bool)[None]
    assert np.array_equal(re.view(np.int64), np.ascontiguousarray(re.transpose(0, 2, 1)).view(np.int64)), \
        (what, "covariance: the real part is not symmetric bit for bit")
    neg_t = np.ascontiguousarray(-im.transpose(0, 2, 1))
    assert np.array_equal(im.view(np.int64)[np.broadcast_to(off, im.shape)], neg_t.view(np.int64)[np.broadcast_to(off, im.shape)]), \
        (what, "covariance: the imaginary part is not antisymmetric bit for bit")
    assert not im[:, np.arange(n), np.arange(n)].any(), (what, "covariance: the diagonal's imaginary part is not zero")
    L = got["chol"]
    assert not np.triu(got["raw"]["chol"][..., 0], 1).any() and not np.triu(got["raw"]["chol"][..., 1], 1).any(), (what, "factor: the strict upper triangle is not zero")
    loaded = _loaded_of(got["cov"], loading, got["fallback"])
    diag = np.sqrt(np.einsum("kaa,kbb->kab", loaded.real, loaded.real))
    at, ratio_l = _worst(np.abs(L @ L.conj().transpose(0, 2, 1) - loaded), 1e-11 * diag)
    assert ratio_l <= 1.0, (what, "factor: worst entry (bin, a, b) %s of L L^H - R' at %.3g of the bound" % (at, ratio_l))
    ratio_g = ratio_t = 0.0
    for i in range(r["status"].size):
        if r["status"][i] == 1:
            assert not got["taps"][i].any() and not got["raw"]["gains"][i].any(), (what, "slot %d is no source but not silent" % i)
            continue
        assert np.isfinite(got["gains"][i]).all(), (what, "gains of beam %d are not finite" % i)
        scale = np.abs(r["gains"][i]).max(axis=1, keepdims=True)
        at, ratio = _worst(np.abs(got["gains"][i] - r["gains"][i]), 1e-9 * np.broadcast_to(scale, r["gains"][i].shape))
        assert ratio <= 1.0, (what, "gains: beam %d, worst entry (bin, mic) %s at %.3g of the bound" % (i, at, ratio))
        ratio_g = max(ratio_g, ratio)
        want = r["taps"][i].astype(np.float64)
        at, ratio = _worst(np.abs(got["taps"][i].astype(np.float64) - want), np.full(want.shape, 2.0 ** -23 * np.abs(want).max()))
        assert ratio <= 1.0, (what, "taps: beam %d, worst entry (mic, t) %s at %.3g of the bound" % (i, at, ratio))
        ratio_t = max(ratio_t, ratio)
    return ratio_s, ratio_c, ratio_l, ratio_g, ratio_t, int((util.bits(got["taps"]) != util.bits(r["taps"])).sum()), got["taps"].size


@pytest.mark.parametrize("case", mvdr_np.TABLE, ids=mvdr_np.case_id)
def test_matches_the_host_design_stage_by_stage(nat, host_table, case):
    """Every row of offsets of the case (tests/lcmv_np.offset_rows: all valid, a -1, a non-multiple, a direction past the table, a
    duplicate), each call between canaries; the bounds are _check_stages'."""
    loading = case[10]
    worst = np.zeros(5)
    differ = total = 0
    for name, row, r in host_table[mvdr_np.case_id(case)]:
        got = _case_call(nat, case, row)
        res = _check_stages(got, r, loading, (mvdr_np.case_id(case), name))
        worst = np.maximum(worst, res[:5])
        differ, total = differ + res[5], total + res[6]
    print("%s: worst error as a fraction of its bound: snapshots %.3g, covariance %.3g, factor %.3g, gains %.3g, taps %.3g; %d of %d taps differ in bits"
          % ((mvdr_np.case_id(case),) + tuple(worst) + (differ, total)))


# ------------------------------------------------------------------ 2. the fallback

def test_silence_and_a_nan_fall_back_to_the_beam_without_nulls(nat):
    """All-zero frames: every bin falls back, L = I, and the taps are the device's own bf_lcmv_design_device with that slot alone (no
    nulls) to 2^-23 of the largest.  One NaN sample: the same fallback and the same taps; the factor, the gains and the taps stay finite."""
    torch = util.torch_gpu()
    import filtersum
    case = mvdr_np.TABLE[4]                                           # n = 70 of 72 rows, T = 33
    n, m_total, S, T, N, F = case[:6]
    frames, mics, tau, _ = mvdr_np.case_inputs(case)
    bins = filtersum.band_bins(T, case[9], mvdr_np.FS)
    step = lcmv_np.offset_per_dir(n)
    row = np.array([5 * step, -1, 2 * step], dtype=np.int32)
    kw = dict(loading=case[10], seg_first=case[6], seg_hop=case[7], segs=case[8])
    silent = _design(nat, np.zeros_like(frames), mics, tau, row, step, T, bins, **kw)
    assert silent["fallback"].tolist() == [1] * len(bins) and silent["status"].tolist() == [0, 1, 0]
    assert not silent["snap"].any() and not silent["cov"].any() and np.array_equal(silent["chol"], np.broadcast_to(np.eye(n), silent["chol"].shape))
    assert not silent["taps"][1].any()
    d_tau = torch.from_numpy(np.ascontiguousarray(tau)).cuda()
    for i in (0, 2):
        d_off = torch.from_numpy(row[i:i + 1].copy()).cuda()
        g, t, k, s = (torch.zeros((1, len(bins), n, 2), dtype=torch.float64, device="cuda"), torch.zeros((1, n, T), dtype=torch.float32, device="cuda"),
                      torch.zeros((1, len(bins), 1), dtype=torch.int32, device="cuda"), torch.ones((1,), dtype=torch.int32, device="cuda"))
        assert nat.lib.bf_lcmv_design_device(d_tau.data_ptr(), tau.shape[0], n, d_off.data_ptr(), 1, step, T, int(bins[0]), int(bins[-1]), 0.95, g.data_ptr(),
                                             t.data_ptr(), k.data_ptr(), s.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        want = t.cpu().numpy()[0].astype(np.float64)
        assert s.item() == 0 and (np.abs(silent["taps"][i].astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want).max()).all()
    bad = frames.copy()
    bad[1, int(mics[7]), 40] = np.nan
    nan = _design(nat, bad, mics, tau, row, step, T, bins, **kw)
    assert nan["fallback"].tolist() == [1] * len(bins) and nan["status"].tolist() == [0, 1, 0]
    assert np.isnan(nan["snap"].real).any() and np.isnan(nan["cov"].real).any()                 # the NaN went where the definition sends it ...
    for name in ("chol", "gains", "taps"):
        assert np.isfinite(nan[name]).all(), name                                                # ... and no further
    assert nan["taps"].tobytes() == silent["taps"].tobytes() and nan["raw"]["gains"].tobytes() == silent["raw"]["gains"].tobytes()


# ------------------------------------------------------------------ 3. two calls, and slots designed together

def test_same_bits_from_call_to_call_and_whatever_is_designed_together(nat):
    case = mvdr_np.TABLE[4]
    n = case[0]
    four = np.array([5, 2, 2, 9], dtype=np.int32) * lcmv_np.offset_per_dir(n)     # a duplicate among them
    eight = np.concatenate([four, np.full(4, -1, dtype=np.int32)])
    a, b, c = _case_call(nat, case, four), _case_call(nat, case, four), _case_call(nat, case, eight)
    assert a["status"].tolist() == [0, 0, 0, 0] and c["status"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and not a["fallback"].any()
    for name in ("snap", "cov", "chol", "gains", "taps", "status", "fallback"):
        assert a["raw"][name].tobytes() == b["raw"][name].tobytes(), name
    for name in ("snap", "cov", "chol", "fallback"):
        assert a["raw"][name].tobytes() == c["raw"][name].tobytes(), name
    assert a["raw"]["gains"].tobytes() == c["raw"]["gains"][:4].tobytes() and a["taps"].tobytes() == c["taps"][:4].tobytes()
    assert a["taps"][1].tobytes() == a["taps"][2].tobytes() and not c["raw"]["gains"][4:].any() and not c["taps"][4:].any()


# ------------------------------------------------------------------ 4. function: an interferer no slot names


def test_the_unnamed_interferer_is_suppressed(nat, scene_tau):
    """The scene of tests/mvdr_np.py; ONE slot, on the look direction, so the geometric designer (retarget) can only give delay-and-sum.
    adapt() on the interferer + noise windows, then the interferer alone through listen(): its power is within 1 dB of what the host
    design's taps leak (filtersum_np.filter_sum), at least 20 dB below the retarget beam's, and the device taps' response towards the
    look direction is f0 within n T 2^-24 max|g| (what the float32 rounding of the taps allows).  The README's three rows are printed."""
    torch = util.torch_gpu()
    import filtersum
    _scene_sizes()
    M, N, hop, T = mvdr_np.M, mvdr_np.N, mvdr_np.HOP, mvdr_np.T
    tau = scene_tau
    look = fsn.flat(fsn.LOOK)
    sc = mvdr_np.scene(tau)
    alone, alone_prev = mvdr_np.cut(sc["interferer"])
    d_off = torch.tensor([look * M], dtype=torch.int32, device="cuda")
    d_alone = torch.from_numpy(alone).cuda()
    fl = filtersum.FilterSumListener.for_slots(tau, 1, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    geo = filtersum.FilterSumListener.for_slots(tau, 1, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    for listener in (fl, geo):
        listener.advance(torch.from_numpy(alone_prev[None]).cuda())
    geo.retarget(d_off)
    leak_geo = fsn.db(util.audio_power(geo, geo.listen(d_alone)))
    bins = fl.bins
    w = 2.0 * np.pi * bins / T
    rows = []
    for name, train in mvdr_np.trainings(sc):
        frames, _ = mvdr_np.cut(train)
        status, fallback = fl.adapt(torch.from_numpy(frames).cuda(), d_off, loading=mvdr_np.LOADING, seg_hop=mvdr_np.SEG_HOP)
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [0] and not fallback.cpu().numpy().any() and fl.taps is None
        dev = fl.taps_host().copy()
        leak_dev = fsn.db(util.audio_power(fl, fl.listen(d_alone)))
        rows.append(mvdr_np.row(sc, dev[0]))
        print("device design, covariance from %s: interferer %.1f dB, white-noise gain %.1f dB, look %+.2f dB; through listen() %.1f dB (retarget: %.1f dB)"
              % ((name,) + rows[-1] + (leak_dev, leak_geo)))
        e = np.abs(filtersum.response(dev[0], tau[look], w) - np.exp(-1j * w * (T - 1) / 2.0))
        assert (e <= M * T * 2.0 ** -24 * float(np.abs(dev[0]).max())).all(), (name, float(e.max()))
        if len(rows) == 1:
            host, host_fallback, _ = filtersum.design_mvdr_slots(frames, fl.mics, tau, [look * M], M, n_taps=T, band=fsn.BAND, loading=mvdr_np.LOADING,
                                                                 seg_first=mvdr_np.SEG_FIRST, seg_hop=mvdr_np.SEG_HOP, segs=mvdr_np.SEGS, fs=fsn.FS)
            want = fsn.filter_sum(alone, fl.mics, host, hop, alone_prev)
            leak_host = fsn.db(mvdr_np.power(want[:, 0, N - hop:]))
            print("interferer alone: host design %.2f dB, device design %.2f dB, retarget (delay-and-sum) %.2f dB: %.1f dB better; %d of %d taps differ in bits"
                  % (leak_host, leak_dev, leak_geo, leak_geo - leak_dev, int((util.bits(dev) != util.bits(host)).sum()), dev.size))
            assert abs(leak_dev - leak_host) <= 1.0
            assert leak_geo - leak_dev >= 20.0
    with pytest.raises(ValueError):
        filtersum.FilterSumListener(np.zeros((1, M, T), dtype=np.float32), hop=hop).adapt(d_alone, d_off)      # not built by for_slots
    with pytest.raises(ValueError):
        fl.adapt(d_alone, d_off.to(torch.int64))
    with pytest.raises(ValueError):
        fl.adapt(d_alone, torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        fl.adapt(d_alone.double(), d_off)
    with pytest.raises(ValueError):
        fl.adapt(d_alone[:, :, :100], d_off)
    with pytest.raises(ValueError):
        fl.adapt(d_alone, d_off, loading=0.0)
    with pytest.raises(ValueError):
        fl.adapt(d_alone, d_off, seg_hop=0)
    with pytest.raises(ValueError):
        fl.adapt(d_alone, d_off, window=np.ones(T + 1))


# ------------------------------------------------------------------ 5. adapt -> listen in one captured graph

def test_graph_adapt_then_listen(nat, scene_tau):
    """adapt(d_frames, d_off) and listen(d_frames) captured as one linear stream after an eager warm-up.  Then d_frames is overwritten
    ON THE DEVICE with windows whose interferer sits at NEAR instead of INTERFERER and the graph replayed: the beam adapts without a
    host design.  The replay's bytes are an eager run's, the taps stay where they were, the beams are filtersum_np.filter_sum with the
    device's own taps bit for bit, and the new interferer alone comes out at least 20 dB below delay-and-sum's leak."""
    torch = util.torch_gpu()
    import filtersum
    _scene_sizes()
    M, N, hop, T = mvdr_np.M, mvdr_np.N, mvdr_np.HOP, mvdr_np.T
    tau = scene_tau
    look = fsn.flat(fsn.LOOK)
    first, near = mvdr_np.scene(tau), mvdr_np.scene(tau, interferer=fsn.NEAR, seed=1)
    train_first, prev_first = mvdr_np.cut(first["interferer"] + first["noise"])
    train_near, prev_near = mvdr_np.cut(near["interferer"] + near["noise"])
    alone, alone_prev = mvdr_np.cut(near["interferer"])

    fl = filtersum.FilterSumListener.for_slots(tau, 1, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    d_off = torch.tensor([look * M], dtype=torch.int32, device="cuda")
    d_frames = torch.from_numpy(train_first).cuda()
    fl.advance(torch.from_numpy(prev_first[None]).cuda())
    taps_at = fl.d_taps.data_ptr()
    out = [None]

    def step():
        fl.adapt(d_frames, d_off)
        out[0] = fl.listen(d_frames)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up: the adaptive array is uploaded and the workspaces allocated here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    work_at = (fl.d_snap.data_ptr(), fl.d_cov.data_ptr(), fl.d_chol.data_ptr())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = out[0]
    assert fl.d_taps.data_ptr() == taps_at and (fl.d_snap.data_ptr(), fl.d_cov.data_ptr(), fl.d_chol.data_ptr()) == work_at
    graph.replay()
    torch.cuda.synchronize()
    as_captured, taps_captured = captured.cpu().numpy().copy(), fl.taps_host().copy()

    d_frames.copy_(torch.from_numpy(train_near).cuda())                # the interferer moved: only device memory changes
    fl.advance(torch.from_numpy(prev_near[None]).cuda())               # in place as well: the graph reads the carried frame where it was
    graph.replay()
    torch.cuda.synchronize()
    got, got_taps = captured.cpu().numpy().copy(), fl.taps_host().copy()
    assert fl.d_taps.data_ptr() == taps_at and not np.array_equal(got_taps, taps_captured) and not np.array_equal(got, as_captured)
    step()                                              # eager, on the same windows
    torch.cuda.synchronize()
    assert got.tobytes() == out[0].cpu().numpy().tobytes() and got_taps.tobytes() == fl.taps_host().tobytes()
    assert np.array_equal(util.bits(got), util.bits(fsn.filter_sum(train_near, fl.mics, got_taps, hop, prev_near)))

    das_taps, _ = filtersum.design_lcmv(tau, [look], None, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    das = filtersum.FilterSumListener(das_taps, hop=hop)
    d_alone, d_alone_prev = torch.from_numpy(alone).cuda(), torch.from_numpy(alone_prev[None]).cuda()
    fl.advance(d_alone_prev)
    das.advance(d_alone_prev)
    leak_mvdr = fsn.db(util.audio_power(fl, fl.listen(d_alone)))          # listen() alone: the taps are the replay's
    leak_das = fsn.db(util.audio_power(das, das.listen(d_alone)))
    print("the interferer moved to NEAR, through the replayed design: delay-and-sum %.1f dB, adapted %.1f dB (%.1f dB better)" % (leak_das, leak_mvdr, leak_das - leak_mvdr))
    assert leak_das - leak_mvdr >= 20.0


# ------------------------------------------------------------------ 6. refusals worth a device: nothing may be enqueued

def test_refused_calls_leave_the_outputs_untouched(nat):
    case = mvdr_np.TABLE[2]                                           # n = 16, T = 9, N = 32
    n, T, N = case[0], case[3], case[4]
    row = np.arange(4, dtype=np.int32) * lcmv_np.offset_per_dir(n)
    assert _case_call(nat, case, row, seg_first=N - T - 6, seg_hop=7, segs=2, expect_rc=-1) is None                  # the last segment ends one sample late
    assert _case_call(nat, case, row, n=257, expect_rc=-1) is None
    assert _case_call(nat, case, row, loading=0.0, expect_rc=-1) is None
    got = _case_call(nat, case, row)                                                                                  # and the same call accepted
    assert got["status"].tolist() == [0, 0, 0, 0] and not got["fallback"].any()
