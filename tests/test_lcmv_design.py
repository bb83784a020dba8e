"""GPU (-m gpu): bf_lcmv_design_device and FilterSumListener.for_slots / retarget against the host design in float64
(filtersum.design_slots; tests/lcmv_np.py restates it with the gains, the coherences and the condition numbers it does not return).

Every output of every call sits in the middle of a buffer of canaries, which must survive.  The device's sines, cosines and
elimination order are not NumPy's, so gains are compared to roundoff times the condition number, taps to one float32 ulp of the
beam's largest tap, and decisions (kept, status) exactly -- on inputs whose every decision is at least 1e-9 away from rho, which is
asserted on the host design before the device is asked anything."""
import numpy as np
import pytest

import filtersum_np as fsn
import lcmv_np
import util
from support import nat_restoring as nat
from util import CANARY_VALUE

pytestmark = pytest.mark.gpu


def _design(nat, tau, offsets, step, T, bins, rho, expect_rc=0):
    """One call on device copies -> (gains complex128 [S, K, n], taps float32 [S, n, T], kept int32 [S, K, S], status int32 [S])."""
    torch = util.torch_gpu()
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    dirs, n = tau.shape
    S, K = offsets.size, len(bins)
    d_tau, d_off = torch.from_numpy(tau).cuda(), torch.from_numpy(offsets).cuda()
    shapes = [((S, K, n, 2), torch.float64), ((S, n, T), torch.float32), ((S, K, S), torch.int32), ((S,), torch.int32)]
    bufs = [util.canaried(shape, dtype) for shape, dtype in shapes]
    rc = nat.lib.bf_lcmv_design_device(d_tau.data_ptr(), dirs, n, d_off.data_ptr(), S, step, T, int(bins[0]), int(bins[-1]), rho,
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
    gains, taps, kept, status = [view.cpu().numpy().reshape(shape) for (_, view), (shape, _) in zip(bufs, shapes)]
    return gains[..., 0] + 1j * gains[..., 1], taps, kept, status


# ------------------------------------------------------------------ 1. the definition table

@pytest.fixture(scope="module")
def host_table():
    """The host design of every (case, row of offsets), computed once, with the input conditions asserted BEFORE the device is
    consulted: every comparison at least 1e-9 away from rho, every solved system with cond <= 1e4, and over the whole table at least
    a tenth of the (beam, bin, null) decisions kept and a tenth dropped."""
    import filtersum
    table, n_kept, n_dropped = {}, 0, 0
    for case in lcmv_np.TABLE:
        n, S, T, band, rho, seed = case
        tau = lcmv_np.table_tau(n, S, T, seed)
        step = lcmv_np.offset_per_dir(n)
        rows = []
        for name, row in lcmv_np.offset_rows(n, S, T, seed):
            r = lcmv_np.slot_gains(tau, row, step, T, band, rho)
            taps, kept, status = filtersum.design_slots(tau, row, step, n_taps=T, band=band, rho=rho, fs=lcmv_np.FS)
            assert np.array_equal(kept, r["kept"]) and np.array_equal(status, r["status"])
            assert all(abs(coh - rho) >= 1e-9 for _, _, _, coh, _ in r["decisions"]), (case[:3], name)
            assert all(c <= 1e4 for c in r["conds"]), (case[:3], name, max(r["conds"]))
            src = np.flatnonzero(status == 0)
            pairs = [(i, j) for i in src for j in src if i != j]
            n_kept += sum(int(kept[i, :, j].sum()) for i, j in pairs)
            n_dropped += sum(int((1 - kept[i, :, j]).sum()) for i, j in pairs)
            rows.append((name, row, r, taps))
        table[case[:3]] = (tau, step, rows)
    print("definition table: %d decisions kept, %d dropped" % (n_kept, n_dropped))
    assert n_kept >= 0.1 * (n_kept + n_dropped) and n_dropped >= 0.1 * (n_kept + n_dropped)
    return table


@pytest.mark.parametrize("n,S,T,band,rho,seed", lcmv_np.TABLE)
def test_matches_the_host_design(nat, host_table, n, S, T, band, rho, seed):
    """Every row of offsets of the case (tests/lcmv_np.offset_rows: S < 4 slots cannot hold a -1, a non-multiple and a duplicate at
    once, so a case designs several rows, each between canaries).
    kept, status: equal.  Taps: |dev - host| <= 2^-23 max|host taps of that beam|, one float32 ulp of the beam's largest tap (float64
    roundoff times cond <= 1e4 is below 1e-11 of that scale: a correct result differs only where the float32 rounding falls the
    other way).  Gains: |dev - host| <= 1e-9 max|G| of that (beam, bin) = 2^-53 x the cond cap 1e4 x about 1e3 of slack for the
    other sincos and elimination order.  Slots that are no source: taps, gains, kept all zero, status 1."""
    tau, step, rows = host_table[(n, S, T)]
    differ = total = 0
    worst_g = worst_t = 0.0
    for name, row, r, want_taps in rows:
        gains, taps, kept, status = _design(nat, tau, row, step, T, r["bins"], rho)
        assert np.array_equal(status, r["status"]), name
        assert np.array_equal(kept, r["kept"]), (name, np.argwhere(kept != r["kept"])[:8])
        for i in range(S):
            if r["status"][i] == 1:
                assert not taps[i].any() and not gains[i].any() and not kept[i].any() and not kept[:, :, i].any(), (name, i)
                continue
            scale_g = np.abs(r["gains"][i]).max(axis=1, keepdims=True)                     # per (beam, bin)
            err_g = np.abs(gains[i] - r["gains"][i]) / scale_g
            scale_t = float(np.abs(want_taps[i]).max())
            err_t = np.abs(taps[i].astype(np.float64) - want_taps[i].astype(np.float64)) / scale_t
            worst_g, worst_t = max(worst_g, float(err_g.max())), max(worst_t, float(err_t.max()))
            assert np.isfinite(gains[i]).all() and (err_g <= 1e-9).all(), (name, i, float(err_g.max()))
            assert (err_t <= 2.0 ** -23).all(), (name, i, float(err_t.max()))
        differ += int((util.bits(taps) != util.bits(want_taps)).sum())
        total += taps.size
    print("n %d S %d T %d: %d of %d taps differ in bits; worst gain error %.3g of the bin's largest, worst tap error %.3g of the beam's largest"
          % (n, S, T, differ, total, worst_g, worst_t))


# ------------------------------------------------------------------ 2. function, not only agreement

SCENE = [fsn.LOOK, fsn.INTERFERER, fsn.NEAR, (5, 3)]


@pytest.fixture(scope="module")
def scene_tau():
    import directions_np as D
    return D.calculate_delays(fsn.GRID[0], fsn.GRID[1], arrays=1).reshape(-1, 64)


def test_device_taps_meet_their_constraints(nat, scene_tau):
    """filtersum.response (float64) of the DEVICE taps at every in-band bin: |H(look) - e^{-jw(T-1)/2}| and |H(kept null)| are each
    within n T 2^-24 max|g|, what the float32 rounding of the taps alone allows (n T taps, each off by at most half an ulp of the
    largest, each weighted by a unit phasor).  The host taps are held to the same bound first."""
    import filtersum
    tau, M, T = scene_tau, 64, 65
    dirs = [fsn.flat(c) for c in SCENE]
    offsets = np.array(dirs, dtype=np.int32) * M
    bins = filtersum.band_bins(T, fsn.BAND, fsn.FS)
    w = 2.0 * np.pi * bins / T
    host, host_kept, _ = filtersum.design_slots(tau, offsets, M, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    _, dev, kept, status = _design(nat, tau, offsets, M, T, bins, 0.95)
    assert np.array_equal(kept, host_kept) and (status == 0).all() and kept.sum() == 76
    for what, taps in (("host", host), ("device", dev)):
        worst = 0.0
        for i in range(4):
            bound = M * T * 2.0 ** -24 * float(np.abs(taps[i]).max())
            e_look = np.abs(filtersum.response(taps[i], tau[dirs[i]], w) - np.exp(-1j * w * (T - 1) / 2.0))
            assert (e_look <= bound).all(), (what, i, float(e_look.max()), bound)
            worst = max(worst, float(e_look.max()) / bound)
            for j in range(4):
                if j != i:
                    h = np.abs(filtersum.response(taps[i], tau[dirs[j]], w))[kept[i, :, j] == 1]
                    assert (h <= bound).all(), (what, i, j, float(h.max()), bound)
                    worst = max(worst, float(h.max()) / bound if h.size else 0.0)
        print("%s taps: worst constraint error %.3g of the bound" % (what, worst))


def test_all_slots_valid_are_the_cross_null_beams(nat, scene_tau):
    """design_slots with every slot a source is cross_null's design bit for bit (slots = compacted beams), and the device agrees with it
    to an ulp of each beam's largest tap."""
    import filtersum
    from interface import config
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=256, MAX_RES_X=fsn.GRID[0], MAX_RES_Y=fsn.GRID[1], N_TAPS=8)
    M, T = 64, 33
    offsets = np.array([fsn.flat(c) for c in SCENE[:3]], dtype=np.int32) * M
    fl = filtersum.FilterSumListener.cross_null(scene_tau, offsets, M, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    host, _, _ = filtersum.design_slots(scene_tau, offsets, M, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    assert np.array_equal(util.bits(host), util.bits(fl.taps))
    _, dev, _, _ = _design(nat, scene_tau, offsets, M, T, filtersum.band_bins(T, fsn.BAND, fsn.FS), 0.95)
    assert (np.abs(dev.astype(np.float64) - host) <= 2.0 ** -23 * np.abs(host).max(axis=(1, 2), keepdims=True)).all()


# ------------------------------------------------------------------ 3. two calls, and slots designed together

def test_same_bits_from_call_to_call_and_whatever_is_designed_together(nat):
    import filtersum
    n, T, rho = 70, 33, 0.5
    tau = lcmv_np.table_tau(n, 8, T, 3)
    bins = filtersum.band_bins(T, lcmv_np.VOICE, lcmv_np.FS)
    four = np.array([5, 2, 2, 9], dtype=np.int32) * n                 # a duplicate among them
    eight = np.concatenate([four, np.full(4, -1, dtype=np.int32)])
    a = _design(nat, tau, four, n, T, bins, rho)
    b = _design(nat, tau, four, n, T, bins, rho)
    c = _design(nat, tau, eight, n, T, bins, rho)
    assert a[3].tolist() == [0, 0, 0, 0] and c[3].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and 0 < a[2].sum() < 12 * len(bins)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[0].tobytes() == c[0][:4].tobytes() and a[1].tobytes() == c[1][:4].tobytes()
    assert np.array_equal(a[2], c[2][:4, :, :4]) and not c[2][4:].any() and not c[2][:, :, 4:].any()
    assert not c[0][4:].any() and not c[1][4:].any()


# ------------------------------------------------------------------ 4. tracker offsets -> designer -> beams in one captured graph

def test_graph_retarget_then_listen(nat):
    """The two-talker scene of tests/test_filter_sum.py::test_listener_nulls_the_second_talker.  retarget(d_off) and listen(d_frames)
    are captured as one linear stream; then d_off is overwritten ON THE DEVICE with the two talkers swapped and the graph replayed:
    the beams follow without a host design.  The replayed beams are an eager run's bytes, and filtersum_np.filter_sum with
    design_slots' taps for the swapped offsets to within the taps' difference carried through the sum, sum|dg| max|x| per output;
    the interferer alone through beam 0 comes out at least 20 dB below the no-null design's (that test's own threshold)."""
    torch = util.torch_gpu()
    import filtersum
    from interface import config
    from lib import directions
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=256, MAX_RES_X=fsn.GRID[0], MAX_RES_Y=fsn.GRID[1], N_TAPS=8)
    M, N, hop, F, T = 64, 256, 128, 14, 65
    tau = directions.calculate_delays().reshape(-1, M)
    look, null = fsn.flat(fsn.LOOK), fsn.flat(fsn.INTERFERER)
    rng = np.random.default_rng(0)
    L = hop * (F + 1) + N
    x_look = fsn.at_microphones(fsn.band_noise(rng, L), tau[look], L)
    x_int = fsn.at_microphones(fsn.band_noise(rng, L), tau[null], L)
    cut = lambda s: (np.ascontiguousarray(np.stack([s[:, (f + 1) * hop:(f + 1) * hop + N] for f in range(F)]), dtype=np.float32),
                     np.ascontiguousarray(s[:, :N], dtype=np.float32))
    both, both_prev = cut(x_look + x_int)
    alone, alone_prev = cut(x_int)

    fl = filtersum.FilterSumListener.for_slots(tau, 2, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    assert fl.B == 2 and fl.taps is None and fl.delay == 32.0 and not fl.d_taps.any() and tuple(fl.d_gains.shape) == (2, len(fl.bins), M, 2)
    first = np.array([null * M, look * M], dtype=np.int32)            # as captured: beam 0 hears the interferer
    swapped = np.array([look * M, null * M], dtype=np.int32)          # as replayed: beam 0 hears the look source, the interferer is its null
    d_off = torch.from_numpy(first).cuda()
    d_frames = torch.from_numpy(both).cuda()
    fl.advance(torch.from_numpy(both_prev[None]).cuda())
    taps_at = fl.d_taps.data_ptr()
    out = [None]

    def step():
        fl.retarget(d_off)
        out[0] = fl.listen(d_frames)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up: the adaptive array is uploaded here, not in the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    captured = out[0]
    assert fl.d_taps.data_ptr() == taps_at              # designed in place: the address the captured beams read
    graph.replay()
    torch.cuda.synchronize()
    as_captured = captured.cpu().numpy().copy()

    d_off.copy_(torch.from_numpy(swapped).cuda())       # the tracker moved: only device memory changes
    graph.replay()
    torch.cuda.synchronize()
    got = captured.cpu().numpy().copy()
    got_taps = fl.taps_host().copy()
    assert fl.taps is not None and fl.d_status.cpu().numpy().tolist() == [0, 0] and fl.d_kept.cpu().numpy()[0, :, 1].all()
    step()                                              # eager, on the same offsets and windows
    torch.cuda.synchronize()
    assert got.tobytes() == out[0].cpu().numpy().tobytes() and got_taps.tobytes() == fl.taps_host().tobytes()
    assert not np.array_equal(got, as_captured) and np.array_equal(util.bits(got[:, 0]), util.bits(as_captured[:, 1]))      # the beams swapped with the talkers

    want_taps, _, _ = filtersum.design_slots(tau, swapped, M, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    dg = np.abs(got_taps.astype(np.float64) - want_taps.astype(np.float64)).sum(axis=(1, 2))                        # per beam
    print("taps that differ from the host design in bits: %d of %d; sum|dg| per beam %s" % (int((util.bits(got_taps) != util.bits(want_taps)).sum()), got_taps.size, dg))
    want = fsn.filter_sum(both, fl.mics, want_taps, hop, both_prev)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=(0, 2))
    bound = dg * float(np.abs(both).max())
    print("beams against filter_sum of the host design: worst difference per beam %s, bound %s" % (err, bound))
    assert (err <= bound).all()
    assert np.array_equal(util.bits(got), util.bits(fsn.filter_sum(both, fl.mics, got_taps, hop, both_prev)))               # and the device's own taps: bit for bit

    # the interferer alone, through the same graph: beam 0 against the same designer's beam without nulls
    das_taps, _ = filtersum.design_lcmv(tau, [look], None, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    das = filtersum.FilterSumListener(das_taps, hop=hop)
    d_alone_prev = torch.from_numpy(alone_prev[None]).cuda()
    d_frames.copy_(torch.from_numpy(alone).cuda())
    fl.advance(d_alone_prev)                            # in place as well: the graph reads the carried frame where it was
    das.advance(d_alone_prev)
    graph.replay()
    torch.cuda.synchronize()
    power = lambda y: float(np.mean(y.astype(np.float64) ** 2))
    leak_lcmv = fsn.db(power(fl.audio(captured).cpu().numpy()[0]))
    leak_das = fsn.db(power(das.audio(das.listen(d_frames)).cpu().numpy()[0]))
    print("interferer through the device-designed beam: delay-and-sum %.1f dB, null-steered %.1f dB (%.1f dB better)" % (leak_das, leak_lcmv, leak_das - leak_lcmv))
    assert leak_das - leak_lcmv >= 20.0

    with pytest.raises(ValueError):
        das.retarget(d_off)                                          # not built by for_slots
    with pytest.raises(ValueError):
        fl.retarget(d_off.to(torch.int64))
    with pytest.raises(ValueError):
        fl.retarget(torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        filtersum.FilterSumListener.for_slots(tau, 9, M)
    with pytest.raises(ValueError):
        filtersum.FilterSumListener.for_slots(tau, 2, M, rho=0.0)


# ------------------------------------------------------------------ 5. refusals worth a device: nothing may be enqueued

def test_refused_calls_leave_the_outputs_untouched(nat):
    import filtersum
    T = 9
    bins = filtersum.band_bins(T, lcmv_np.FULL, lcmv_np.FS)
    tau = lcmv_np.table_tau(16, 8, T, 0)
    assert _design(nat, tau, np.arange(9, dtype=np.int32) * 16, 16, T, bins, 0.95, expect_rc=-1) is None             # sources = 9
    assert _design(nat, tau[:, :3], np.arange(4, dtype=np.int32) * 3, 3, T, bins, 0.95, expect_rc=-1) is None        # sources = 4 > n = 3
    assert _design(nat, tau, np.arange(4, dtype=np.int32) * 16, 16, T, bins, 0.0, expect_rc=-1) is None              # rho = 0
    got = _design(nat, tau, np.arange(4, dtype=np.int32) * 16, 16, T, bins, 0.95)                                    # and the same call accepted
    assert got[3].tolist() == [0, 0, 0, 0]
