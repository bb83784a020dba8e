"""CPU: bf_mvdr_learn_device without a device -- filtersum.mvdr_learn / design_mvdr_learned (the host statements of the call, and the
oracle of tests/test_mvdr_learn.py) against the design they extend, the restatement with intermediates the GPU tests use
(tests/mvdr_learn_np.py) against them, the two scenes the carried covariance is for, every refusal that sits before device bring-up
(fake pointers, as tests/test_mvdr_design_host.py), and the binding."""
import ctypes as C

import numpy as np
import pytest

import filtersum_np as fsn
import lcmv_np
import mvdr_learn_np as mln
import mvdr_np
import util
from support import FAKE, scene_tau as tau, sized


def _close(taps, want):
    """Every beam within 2^-23 of its largest tap."""
    want = want.astype(np.float64)
    return all((np.abs(taps[i].astype(np.float64) - want[i]) <= 2.0 ** -23 * np.abs(want[i]).max()).all() for i in range(want.shape[0]))


# ------------------------------------------------------------------ 1, 2. the settings at which it is the existing design

@pytest.mark.parametrize("case", mvdr_np.TABLE, ids=mvdr_np.case_id)
def test_empty_state_unit_weights_and_no_forgetting_are_design_mvdr_slots(native, case):
    """From the empty state, weights None, forget 1: the state is P times design_mvdr_slots' covariance and the mass is P, so the taps
    are design_mvdr_slots' within 2^-23 of a beam's largest (the sums run in another order), fallback and status equal.  On the way:
    the state is exactly Hermitian, and tests/mvdr_learn_np.state_stages gives design_mvdr_learned's taps bit for bit."""
    import filtersum
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window = case
    frames, mics, tau_r, win = mvdr_np.case_inputs(case)
    step = lcmv_np.offset_per_dir(n)
    acc, mass, used = filtersum.mvdr_learn(None, 0.0, frames, mics, None, 1.0, n_taps=T, band=band, seg_first=seg_first, seg_hop=seg_hop, segs=segs, window=win,
                                           fs=mvdr_np.FS)
    assert mass == float(F * segs) and used.dtype == np.int32 and used.tolist() == [F, 0]
    assert np.array_equal(acc, acc.conj().transpose(0, 2, 1)) and not acc.imag[:, np.arange(n), np.arange(n)].any()
    for name, row in lcmv_np.offset_rows(n, S, T, 0):
        want, want_fallback, want_status = filtersum.design_mvdr_slots(frames, mics, tau_r, row, step, n_taps=T, band=band, loading=loading, seg_first=seg_first,
                                                                       seg_hop=seg_hop, segs=segs, window=win, fs=mvdr_np.FS)
        taps, fallback, status = filtersum.design_mvdr_learned(acc, mass, tau_r, row, step, n_taps=T, band=band, loading=loading, fs=mvdr_np.FS)
        assert np.array_equal(fallback, want_fallback) and np.array_equal(status, want_status), name
        assert taps.dtype == np.float32 and taps.shape == want.shape and _close(taps, want), name
        r = mln.state_stages(acc, mass, tau_r, row, step, T, band, loading)
        assert np.array_equal(util.bits(r["taps"]), util.bits(taps)) and np.array_equal(r["fallback"], fallback) and np.array_equal(r["status"], status), name
        assert r["conds"].max() <= n / loading + 1.0 + 1e-6 and r["conds"].max() <= 1e4


@pytest.mark.parametrize("case", mln.TABLE, ids=mln.case_id)
def test_zero_one_weights_are_a_design_on_the_learned_frames_alone(native, case):
    """Weights 1, 0, 1, .. : the design is design_mvdr_slots' on frames 0, 2, .. alone, to the same bound; forget 1."""
    import filtersum
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading = case[:11]
    _, frames, mics, tau_r, win, _ = mln.case_inputs(case)
    step = lcmv_np.offset_per_dir(n)
    weights = (np.arange(F) % 2 == 0).astype(np.float64)
    acc, mass, used = filtersum.mvdr_learn(None, 0.0, frames, mics, weights, 1.0, n_taps=T, band=band, seg_first=seg_first, seg_hop=seg_hop, segs=segs, window=win,
                                           fs=mln.FS)
    kept = np.ascontiguousarray(frames[weights > 0])
    assert used.tolist() == [kept.shape[0], 0] and mass == float(kept.shape[0] * segs) and kept.shape[0] < F
    name, row = lcmv_np.offset_rows(n, S, T, 0)[-1]
    want, want_fallback, want_status = filtersum.design_mvdr_slots(kept, mics, tau_r, row, step, n_taps=T, band=band, loading=loading, seg_first=seg_first,
                                                                   seg_hop=seg_hop, segs=segs, window=win, fs=mln.FS)
    taps, fallback, status = filtersum.design_mvdr_learned(acc, mass, tau_r, row, step, n_taps=T, band=band, loading=loading, fs=mln.FS)
    assert np.array_equal(fallback, want_fallback) and np.array_equal(status, want_status) and _close(taps, want), name


# ------------------------------------------------------------------ 3, 4. the state

@pytest.mark.parametrize("case", mln.TABLE, ids=mln.case_id)
def test_two_calls_are_one_call_on_the_concatenated_frames(native, case):
    """The first batch then the table's batch, against one call on both: acc to 1e-13 sqrt(acc_aa acc_bb), the mass equal, used added.
    The table's properties hold: cond(R') <= n / loading + 1 <= 1e4 after either call, and each case's weights do what its comment says."""
    import filtersum
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window, _, forget = case
    first, frames, mics, tau_r, win, weights = mln.case_inputs(case)
    assert frames.shape == (F, m_total, N) and len(set(mics.tolist())) == n and seg_first + (segs - 1) * seg_hop + T <= N
    kw = dict(n_taps=T, band=band, seg_first=seg_first, seg_hop=seg_hop, segs=segs, window=win, fs=mln.FS)
    a1, m1, u1 = filtersum.mvdr_learn(None, 0.0, first, mics, None, forget, **kw)
    a2, m2, u2 = filtersum.mvdr_learn(a1, m1, frames, mics, weights, forget, **kw)
    both = np.concatenate([np.ones(first.shape[0]), np.ones(F) if weights is None else weights])
    a, m, u = filtersum.mvdr_learn(None, 0.0, np.concatenate([first, frames]), mics, both, forget, **kw)
    diag = np.sqrt(np.einsum("kaa,kbb->kab", a.real, a.real))
    assert (np.abs(a2 - a) <= 1e-13 * diag).all() and m2 == m and (u1 + u2).tolist() == u.tolist()
    assert np.array_equal(a2, a2.conj().transpose(0, 2, 1))
    name, row = lcmv_np.offset_rows(n, S, T, 0)[0]
    r1, r2 = mln.case_chain(case, row)
    assert np.array_equal(r2["acc"], a2) and r2["total"] == m2 and r2["used"].tolist() == u2.tolist()
    for r in (r1, r2):
        assert not r["fallback"].any() and r["conds"].max() <= n / loading + 1.0 + 1e-6 and r["conds"].max() <= 1e4
    if n == 3:
        assert F * segs == 35 and mics.tolist() == [4, 0, 2] and weights[-3:-1].tolist() == [0.0, 0.0]
    if n == 16:
        assert segs == 16 and weights[1] == 0.0                       # snapshots 16 .. 31: one staged chunk, all of it skipped
    if n == 70:
        assert F * segs == 16 and weights[0] == 0.0


def test_invalid_and_zero_weights_are_skipped_and_an_empty_mass_falls_back(native):
    """NaN, Inf, a negative weight are skipped and counted, +-0 skipped silently: the state is the one the learned frames alone give,
    array_equal; a batch of nothing but such weights returns the state it was given; a mass of 0 is fallback at every bin, the taps
    design_lcmv's without nulls."""
    import filtersum
    case = mln.by_n(3)
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window, _, forget = case
    first, frames, mics, tau_r, win, _ = mln.case_inputs(case)
    kw = dict(n_taps=T, band=band, seg_first=seg_first, seg_hop=seg_hop, segs=segs, window=win, fs=mln.FS)
    a0, m0, _ = filtersum.mvdr_learn(None, 0.0, first, mics, None, forget, **kw)
    weights = np.array([0.5, np.nan, 2.0, np.inf, -1.0, -0.0, 0.25])
    a, m, used = filtersum.mvdr_learn(a0, m0, frames, mics, weights, forget, **kw)
    assert used.tolist() == [3, 3]
    b, mb, used_b = filtersum.mvdr_learn(a0, m0, np.ascontiguousarray(frames[[0, 2, 6]]), mics, weights[[0, 2, 6]], forget, **kw)
    assert np.array_equal(a, b) and m == mb and used_b.tolist() == [3, 0]
    keep = a0.copy()
    c, mc, used_c = filtersum.mvdr_learn(a0, m0, frames[:6], mics, np.array([0.0, -0.0, np.nan, np.inf, -1.0, 0.0]), forget, **kw)
    assert np.array_equal(c, keep) and np.array_equal(a0, keep) and mc == m0 and used_c.tolist() == [0, 3]
    d, md, used_d = filtersum.mvdr_learn(a0, m0, frames[:0], mics, None, forget, **kw)                       # no frames at all
    assert np.array_equal(d, keep) and md == m0 and used_d.tolist() == [0, 0]
    step = lcmv_np.offset_per_dir(n)
    row = lcmv_np.offset_rows(n, S, T, 0)[0][1]
    e, me, _ = filtersum.mvdr_learn(None, 0.0, frames, mics, np.zeros(F), forget, **kw)
    assert not e.any() and me == 0.0
    taps, fallback, status = filtersum.design_mvdr_learned(e, me, tau_r, row, step, n_taps=T, band=band, loading=loading, fs=mln.FS)
    want, _ = filtersum.design_lcmv(tau_r, [int(o) // step for o in row], None, n_taps=T, band=band, fs=mln.FS)
    assert fallback.tolist() == [1] * fallback.size and status.tolist() == [0] * S and _close(taps, want)
    taps_a, fallback_a, _ = filtersum.design_mvdr_learned(a, 0.0, tau_r, row, step, n_taps=T, band=band, loading=loading, fs=mln.FS)    # a state, but no mass
    assert fallback_a.all() and np.array_equal(util.bits(taps_a), util.bits(taps))
    for bad in (dict(forget=0.0), dict(forget=1.0000001), dict(forget=float("nan")), dict(forget=-0.5)):
        with pytest.raises(ValueError):
            filtersum.mvdr_learn(None, 0.0, frames, mics, None, **dict(kw, **bad))
    with pytest.raises(ValueError):
        filtersum.mvdr_learn(None, 0.0, frames, mics, np.ones(F + 1), 1.0, **kw)
    with pytest.raises(ValueError):
        filtersum.mvdr_learn(np.zeros((1, n, n)), 0.0, frames, mics, None, 1.0, **kw)
    with pytest.raises(ValueError):
        filtersum.design_mvdr_learned(a[:, :2, :2], m, tau_r, row, step, n_taps=T, band=band, loading=loading, fs=mln.FS)
    with pytest.raises(ValueError):
        filtersum.design_mvdr_learned(a, m, tau_r, row, step, n_taps=T, band=band, loading=0.0, fs=mln.FS)


# ------------------------------------------------------------------ 5. what it is for

def test_the_scenes_a_gated_talker_and_a_moved_interferer(native, tau):
    """The scene of tests/mvdr_np.py with FilterSumListener.learn's segments.  (a) The look talker, at the interferer's level, speaks in
    samples < 8 HOP: learned from the windows behind that alone (weights [0] * 7 + [1] * 7) the design is at least 6 dB better on the
    interferer than learned from all fourteen (9.7 dB measured in float64).  (b) Fourteen windows with the interferer at INTERFERER,
    then fourteen with it at NEAR: forget 0.7 is at least 3 dB better on the moved interferer than forget 1 (5.0 dB measured).  Both are
    conditions of the inputs; the rows are the README's."""
    import filtersum
    look = fsn.flat(fsn.LOOK)
    sc, train = mln.gated_scene(tau)
    das, _ = filtersum.design_lcmv(tau, [look], None, n_taps=mln.T, band=fsn.BAND, fs=fsn.FS)
    print("delay-and-sum: interferer %.1f dB, white-noise gain %.1f dB, look %+.2f dB" % mvdr_np.row(sc, das[0]))
    rows = {}
    for name, weights in (("all 14 windows, weights 1", None), ("windows 7..13 only", np.array(mln.LOOK_FREE))):
        state = mln.host_learn(None, train, weights, 1.0)
        assert state[2].tolist() == [14 if weights is None else 7, 0]
        rows[name] = mvdr_np.row(sc, mln.host_taps(state, tau)[0])
        print("covariance learned from %s: interferer %.1f dB, white-noise gain %.1f dB, look %+.2f dB" % ((name,) + rows[name]))
    assert rows["all 14 windows, weights 1"][0] - rows["windows 7..13 only"][0] >= 6.0
    old, new, train_old, train_new = mln.moved_scenes(tau)
    alone, _ = filtersum.design_mvdr(mvdr_np.cut(train_new)[0], np.arange(mln.M), tau, [look], n_taps=mln.T, band=fsn.BAND, loading=mvdr_np.LOADING,
                                     seg_first=mvdr_np.SEG_FIRST, seg_hop=mvdr_np.SEG_HOP, segs=mvdr_np.SEGS, fs=fsn.FS)
    print("the NEAR windows alone: new interferer %.1f dB" % mvdr_np.row(new, alone[0])[0])
    leak = {}
    for forget in (1.0, 0.9, 0.7, 0.5):
        state = mln.host_learn(mln.host_learn(None, train_old, None, forget), train_new, None, forget)
        g = mln.host_taps(state, tau)[0]
        leak[forget] = mvdr_np.row(new, g)[0]
        print("forget %.1f: new interferer %.1f dB, old interferer %.1f dB, final mass %.1f" % (forget, leak[forget], mvdr_np.row(old, g)[0], state[1]))
    assert leak[1.0] - leak[0.7] >= 3.0


# ------------------------------------------------------------------ 6. refusals before device bring-up

M_TOTAL, FRAMES, N_MICS, FIRST, SHOP, SEGS, DIRS, SRC, STEP, TAPS, LO, HI = 20, 3, 16, 4, 8, 5, 12, 4, 16, 9, 1, 3
K, P = HI - LO + 1, FRAMES * SEGS
(D_SIG, D_WIN, D_WEIGHTS, D_TAU, D_OFF, D_ACC, D_MASS, D_USED, D_SNAP, D_COV, D_CHOL, D_GAINS, D_TAPS, D_STATUS, D_FALL) = (FAKE + i * 0x1000000 for i in range(15))
SIG_BYTES, WIN_BYTES, WEIGHTS_BYTES, TAU_BYTES, OFF_BYTES = FRAMES * M_TOTAL * 256 * 4, TAPS * 8, FRAMES * 8, DIRS * N_MICS * 8, SRC * 4
SNAP_BYTES, COV_BYTES, GAINS_BYTES, TAPS_BYTES, STATUS_BYTES, FALL_BYTES = P * K * N_MICS * 16, K * N_MICS * N_MICS * 16, SRC * K * N_MICS * 16, SRC * N_MICS * TAPS * 4, SRC * 4, K * 4
ACC_BYTES, MASS_BYTES, USED_BYTES = COV_BYTES, 8, 8
MICS = np.arange(N_MICS, dtype=np.int32)
W = "bf_mvdr_learn_device: "


def _call(native, d_signals=D_SIG, m_total=M_TOTAL, frames=FRAMES, mics=MICS, n=N_MICS, seg_first=FIRST, seg_hop=SHOP, segs=SEGS, d_window=D_WIN, d_weights=D_WEIGHTS,
          forget=0.9, d_tau=D_TAU, dirs=DIRS, d_offsets=D_OFF, sources=SRC, offset_per_dir=STEP, n_taps=TAPS, bin_lo=LO, bin_hi=HI, loading=0.1, d_acc=D_ACC,
          d_mass=D_MASS, d_used=D_USED, d_snap=D_SNAP, d_cov=D_COV, d_chol=D_CHOL, d_gains=D_GAINS, d_taps=D_TAPS, d_status=D_STATUS, d_fallback=D_FALL):
    return native.lib.bf_mvdr_learn_device(d_signals, m_total, frames, None if mics is None else native.iptr(mics), n, seg_first, seg_hop, segs, d_window, d_weights,
                                           forget, d_tau, dirs, d_offsets, sources, offset_per_dir, n_taps, bin_lo, bin_hi, loading, d_acc, d_mass, d_used, d_snap,
                                           d_cov, d_chol, d_gains, d_taps, d_status, d_fallback, None)


BAD_ROW = MICS.copy()
BAD_ROW[5] = M_TOTAL


@pytest.mark.parametrize("kw,text", [
    (dict(d_acc=None), "d_acc is null"),
    (dict(d_mass=None), "d_mass is null"),
    (dict(d_used=None), "d_used is null"),
    (dict(mics=None), "adaptive_array is null"),
    (dict(d_tau=None), "d_tau is null"),
    (dict(d_offsets=None), "d_offsets is null"),
    (dict(d_cov=None), "d_cov is null"),
    (dict(d_chol=None), "d_chol is null"),
    (dict(d_gains=None), "d_gains is null"),
    (dict(d_taps=None), "d_taps is null"),
    (dict(d_status=None), "d_status is null"),
    (dict(d_fallback=None), "d_fallback is null"),
    (dict(frames=0, d_acc=None), "d_acc is null"),
    (dict(frames=0, mics=None), "adaptive_array is null"),
    (dict(frames=-1), "frames = -1 < 0"),
    (dict(frames=-1, d_signals=None, d_snap=None), "frames = -1 < 0"),
    (dict(frames=1, d_snap=None), "d_snap is null"),
    (dict(frames=1, d_signals=None), "d_signals is null"),
    (dict(d_signals=None, d_snap=None), "d_signals is null"),
    (dict(forget=0.0), "forget = 0 is not in (0, 1]"),
    (dict(forget=1.0000001), "forget = 1.0000001000000001 is not in (0, 1]"),
    (dict(forget=float("nan")), "forget = nan is not in (0, 1]"),
    (dict(forget=-0.5), "forget = -0.5 is not in (0, 1]"),
    (dict(frames=0, forget=0.0), "forget = 0 is not in (0, 1]"),
    # bf_mvdr_design_device's refusals, in its words
    (dict(n=0), "n = 0 < 1"),
    (dict(segs=0), "segs = 0 < 1"),
    (dict(seg_hop=0), "seg_hop = 0 < 1"),
    (dict(dirs=0), "dirs = 0 < 1"),
    (dict(sources=0), "sources = 0 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(n_taps=0), "n_taps = 0 < 1"),
    (dict(seg_first=-1), "seg_first = -1 < 0"),
    (dict(seg_first=216), "seg_first + (segs - 1) * seg_hop + n_taps = 257 > N_SAMPLES = 256 (a segment would leave its window)"),
    (dict(n=257), "n = 257 > 256"),
    (dict(sources=9), "sources = 9 > 8"),
    (dict(n_taps=1025), "n_taps = 1025 > 1024"),
    (dict(bin_hi=5), "bins [1, 5] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = 4"),
    (dict(loading=0.0), "loading = 0 is not finite and > 0"),
    (dict(loading=float("inf")), "loading = inf is not finite and > 0"),
    (dict(mics=BAD_ROW), "adaptive_array[5] = 20 is not a row of frames with m_total = 20 rows"),
    (dict(frames=0, mics=BAD_ROW), "adaptive_array[5] = 20 is not a row of frames with m_total = 20 rows"),
    # the state and d_used are outputs: each against another output and an input, the first or the last byte of a range
    (dict(d_mass=D_ACC + ACC_BYTES - 8), "d_acc overlaps d_mass"),
    (dict(d_used=D_ACC), "d_acc overlaps d_used"),
    (dict(d_snap=D_ACC - SNAP_BYTES + 8), "d_acc overlaps d_snap"),
    (dict(d_cov=D_ACC + ACC_BYTES - 8), "d_acc overlaps d_cov"),
    (dict(d_fallback=D_ACC), "d_acc overlaps d_fallback"),
    (dict(d_signals=D_ACC - SIG_BYTES + 4), "d_acc overlaps d_signals"),
    (dict(d_tau=D_ACC + ACC_BYTES - 8), "d_acc overlaps d_tau"),
    (dict(d_weights=D_ACC), "d_acc overlaps d_weights"),
    (dict(d_used=D_MASS + 4), "d_mass overlaps d_used"),
    (dict(d_mass=D_COV + COV_BYTES - 8), "d_mass overlaps d_cov"),
    (dict(d_mass=D_TAPS), "d_mass overlaps d_taps"),
    (dict(d_mass=D_OFF + OFF_BYTES - 4), "d_mass overlaps d_offsets"),
    (dict(d_weights=D_MASS - WEIGHTS_BYTES + 8), "d_mass overlaps d_weights"),
    (dict(d_used=D_SNAP + SNAP_BYTES - 4), "d_used overlaps d_snap"),
    (dict(d_status=D_USED + 4), "d_used overlaps d_status"),
    (dict(d_used=D_WIN + WIN_BYTES - 4), "d_used overlaps d_window"),
    (dict(d_used=D_SIG), "d_used overlaps d_signals"),
    (dict(d_weights=D_USED + 4), "d_used overlaps d_weights"),
    # d_weights is an input: against every other output
    (dict(d_weights=D_SNAP + SNAP_BYTES - 8), "d_snap overlaps d_weights"),
    (dict(d_weights=D_COV), "d_cov overlaps d_weights"),
    (dict(d_weights=D_CHOL - WEIGHTS_BYTES + 8), "d_chol overlaps d_weights"),
    (dict(d_weights=D_GAINS), "d_gains overlaps d_weights"),
    (dict(d_weights=D_TAPS + TAPS_BYTES - 4), "d_taps overlaps d_weights"),
    (dict(d_weights=D_STATUS), "d_status overlaps d_weights"),
    (dict(d_weights=D_FALL + FALL_BYTES - 4), "d_fallback overlaps d_weights"),
    # and the design's own pairs still hold
    (dict(d_cov=D_SNAP + SNAP_BYTES - 8), "d_snap overlaps d_cov"),
    (dict(d_window=D_TAPS + TAPS_BYTES - 8), "d_taps overlaps d_window"),
    (dict(frames=0, d_tau=D_ACC), "d_acc overlaps d_tau"),
])
def test_refusals(sized, kw, text):
    lib = sized.lib
    lib.bf_clear_error()
    assert _call(sized, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(sized):
    """Ranges that only touch, no weights, no window, either end of forget's range, and the re-aim (frames = 0) with d_signals, d_weights,
    d_window and d_snap null -- or pointing into an output: they are not touched -- all pass the argument checks, so without a GPU the
    one refusal left is the missing device (with one, fake pointers must not be launched: nothing is called)."""
    if sized.gpu_available():
        return
    lib = sized.lib
    for kw in (dict(), dict(d_weights=None), dict(d_window=None, d_weights=None), dict(forget=1.0), dict(forget=5e-324), dict(d_mass=D_ACC + ACC_BYTES),
               dict(d_used=D_MASS + MASS_BYTES), dict(d_snap=D_USED + USED_BYTES), dict(d_weights=D_ACC - WEIGHTS_BYTES), dict(d_weights=D_WIN), dict(frames=1),
               dict(frames=0, d_signals=None, d_weights=None, d_window=None, d_snap=None), dict(frames=0, d_signals=None, d_snap=None), dict(frames=0),
               dict(frames=0, d_snap=D_ACC, d_signals=D_COV, d_weights=D_MASS, d_window=D_USED), dict(seg_first=215), dict(sources=8), dict(n=1, mics=MICS[:1])):
        lib.bf_clear_error()
        assert _call(sized, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device"), kw
    lib.bf_clear_error()


# ------------------------------------------------------------------ 7. the binding

def test_the_symbol_is_exported_bound_and_declared(native):
    fn = native.lib.bf_mvdr_learn_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 31 and fn.argtypes[3] is native.IP
    assert [i for i, t in enumerate(fn.argtypes) if t is C.c_double] == [10, 19]
    assert [i for i, t in enumerate(fn.argtypes) if t is C.c_void_p] == [0, 8, 9, 11, 13] + list(range(20, 31))
    assert all(t is C.c_int for i, t in enumerate(fn.argtypes) if i in (1, 2, 4, 5, 6, 7, 12, 14, 15, 16, 17, 18))
    header = open(native.__file__.replace("zybo-rt-sampler-image-detection_amd/lib/_native.py", "include/beamformer_hip.h")).read()
    assert "int bf_mvdr_learn_device(" in header and "A REPLAY ADVANCES THE STATE" in header
    import filtersum
    assert callable(filtersum.mvdr_learn) and callable(filtersum.design_mvdr_learned)
    for name in ("learn", "reaim", "forget_all"):
        assert callable(getattr(filtersum.FilterSumListener, name))
