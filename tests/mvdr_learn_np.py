"""What the tests of bf_mvdr_learn_device share: filtersum.mvdr_learn's state and design_mvdr_learned restated with its INTERMEDIATES (the
snapshots, the covariance, the loaded matrix's condition, the factor, the gains) in the shape tests/mvdr_np.slot_stages gives them, the
cases of the definition table -- every one a first batch and then the table's batch on one state -- and the two scenes of the
README: a look talker that speaks in the first half of the capture, and an interferer that moves between two captures.

tests/test_mvdr_learn_host.py pins `state_stages` to design_mvdr_learned (the same fallback and status, the same taps bit for bit)."""
import numpy as np

import filtersum
import filtersum_np as fsn
import lcmv_np
import mvdr_np
from lcmv_np import FS, FULL, VOICE


def snapshots(frames, mics, T, bins, seg_first, seg_hop, segs, window):
    """slot_stages' snapshot loop -> (snap complex128 [P, K, M], rows float64 [P, M]: sum_t |win[t] x[t]|, the scale of a row's rounding)."""
    x = np.asarray(frames)
    mics = np.asarray(mics).astype(np.int64).ravel()
    win = np.ones(T) if window is None else np.asarray(window, dtype=np.float64)
    r = np.arange(T)
    table = np.cos(2.0 * np.pi * r / T) - 1j * np.sin(2.0 * np.pi * r / T)
    E = table[(np.arange(T)[:, None] * bins[None, :]) % T]
    snap = np.empty((x.shape[0] * segs, bins.size, mics.size), dtype=np.complex128)
    rows = np.empty((x.shape[0] * segs, mics.size))
    with np.errstate(all="ignore"):
        for f in range(x.shape[0]):
            for q in range(segs):
                s0 = seg_first + q * seg_hop
                seg = x[f][mics, s0:s0 + T].astype(np.float64) * win[None, :]
                snap[f * segs + q] = (seg @ E).T
                rows[f * segs + q] = np.abs(seg).sum(axis=1)
    return snap, rows


def state_stages(acc, mass, tau, offsets, offset_per_dir, n_taps, band, loading, fs=FS):
    """design_mvdr_learned with slot_stages' intermediates -> dict: cov / loaded / chol complex128 [K, M, M], conds float64 [K], gains
    complex128 [S, K, M], fallback int32 [K], status int32 [S], bins, taps float32 [S, M, T]."""
    tau = np.asarray(tau, dtype=np.float64)
    T, M = int(n_taps), tau.shape[1]
    dirs = filtersum.slot_directions(offsets, offset_per_dir, tau.shape[0])
    bins = filtersum.band_bins(T, band, fs)
    K = bins.size
    cov = np.zeros((K, M, M), dtype=np.complex128)
    with np.errstate(all="ignore"):
        if mass > 0.0:
            cov.real, cov.imag = acc.real / mass, acc.imag / mass
        loaded, chol = np.empty_like(cov), np.empty_like(cov)
        fallback = np.zeros(K, dtype=np.int32)
        conds = np.empty(K)
        G = np.zeros((len(dirs), K, M), dtype=np.complex128)
        for i, k in enumerate(bins):
            tr = float(np.sum(cov[i].diagonal().real))
            if np.isfinite(tr) and tr > 0.0:
                loaded[i] = cov[i] + (float(loading) * tr / M) * np.eye(M)
            else:
                loaded[i] = np.eye(M)
                fallback[i] = 1
            conds[i] = np.linalg.cond(loaded[i])
            L = np.linalg.cholesky(loaded[i])
            chol[i] = L
            w = 2.0 * np.pi * k / T
            for b, d in enumerate(dirs):
                if d < 0:
                    continue
                c = np.exp(1j * w * tau[d])
                y = np.linalg.solve(L, c)
                z = np.linalg.solve(L.conj().T, y)
                u = z * np.exp(1j * w * (T - 1) / 2.0) / np.sum(np.abs(y) ** 2)
                G[b, i] = u.conj()
    status = np.array([0 if d >= 0 else 1 for d in dirs], dtype=np.int32)
    return dict(cov=cov, loaded=loaded, chol=chol, conds=conds, gains=G, fallback=fallback, status=status, bins=bins, taps=lcmv_np.taps_of(G, bins, T))


def learn_batch(acc, mass, frames, mics, n_taps, band, seg_first, seg_hop, segs, window, weights, forget, fs=FS):
    """The part of one call that does not depend on the offsets -> dict: snap, mass (the rows' scale, slot_stages' name), and the state
    after the call by filtersum.mvdr_learn: acc, total (the scalar mass), used."""
    bins = filtersum.band_bins(int(n_taps), band, fs)
    snap, rows = snapshots(frames, mics, int(n_taps), bins, seg_first, seg_hop, segs, window)
    acc, total, used = filtersum.mvdr_learn(acc, mass, frames, mics, weights, forget, n_taps=n_taps, band=band, seg_first=seg_first, seg_hop=seg_hop, segs=segs,
                                            window=window, fs=fs)
    return dict(snap=snap, mass=rows, acc=acc, total=total, used=used)


def empty(case_or_K, M=None):
    """The empty state of a case of TABLE (or of K bins and M microphones) -> (acc, mass)."""
    if M is None:
        K, M = filtersum.band_bins(case_or_K[3], case_or_K[9], FS).size, case_or_K[0]
    else:
        K = case_or_K
    return np.zeros((K, M, M), dtype=np.complex128), 0.0


# ------------------------------------------------------------------ the definition table

#        n   m_total S  T   N   frames seg_first seg_hop segs  band  loading  window   weights                        forget
TABLE = [
    (1, 1, 1, 1, 8, 3, 0, 1, 8, FULL, 0.1, None, None, 1.0),                                       # the degenerate ends
    (3, 5, 3, 8, 32, 7, 1, 5, 5, FULL, 0.05, None, (0.5, 0.0, 2.0, 1.0, 0.0, 0.0, 0.25), 0.75),    # P = 35: frame boundaries inside staged chunks, trailing zeros, rows (4, 0, 2)
    (16, 16, 8, 9, 32, 3, 0, 1, 16, FULL, 0.01, None, (1.0, 0.0, 2.0), 0.5),                       # a staged chunk wholly skipped
    (70, 72, 8, 33, 64, 4, 0, 8, 4, VOICE, 0.05, None, (0.0, 1.0, 1.0, 0.5), 0.9),                 # leading skip, ragged last tile, P = 16 = one chunk
    (130, 130, 2, 17, 64, 2, 5, 6, 8, FULL, 0.1, None, (2.0, 1.0), 0.5),                           # 9 x 9 tiles
    (64, 64, 4, 65, 256, 3, 0, 16, 12, VOICE, 0.1, "hann", None, 0.9),                             # the shipped shape
    (256, 256, 1, 9, 32, 2, 0, 4, 6, VOICE, 0.1, None, (1.0, 1.0), 1.0),                           # the largest array
]
# cond(R') <= n / loading + 1 whatever the weights (R is a positive combination of X X^H): <= 1e4 by the loadings above
FIRST_FRAMES = 2                    # the batch every case learns BEFORE the table's: unit weights, the case's forget


def case_id(case):
    return "n%d_S%d_T%d" % (case[0], case[2], case[3])


def by_n(n):
    return [c for c in TABLE if c[0] == n][0]


def case_inputs(case):
    """-> (first float32 [FIRST_FRAMES, m_total, N], frames float32 [F, m_total, N], mics int32 [n], tau float64 [D, n], window or None,
    weights float64 [F] or None): seeded normals as mvdr_np.case_inputs', nothing configured."""
    n, m_total, S, T, N, F = case[:6]
    rng = np.random.default_rng([n, m_total, S, T, 11])
    first = rng.standard_normal((FIRST_FRAMES, m_total, N)).astype(np.float32)
    frames = rng.standard_normal((F, m_total, N)).astype(np.float32)
    mics = np.array([4, 0, 2], dtype=np.int32) if (n, m_total) == (3, 5) else rng.permutation(m_total)[:n].astype(np.int32)
    weights = None if case[12] is None else np.array(case[12], dtype=np.float64)
    return first, frames, mics, lcmv_np.table_tau(n, S, T, 0), (mvdr_np.hann(T) if case[11] == "hann" else None), weights


def case_batches(case):
    """The host chain of a case: the first batch from the empty state, then the table's batch -> (b1, b2), two learn_batch dicts."""
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window, _, forget = case
    first, frames, mics, tau, win, weights = case_inputs(case)
    acc, mass = empty(case)
    b1 = learn_batch(acc, mass, first, mics, T, band, seg_first, seg_hop, segs, win, None, forget)
    b2 = learn_batch(b1["acc"], b1["total"], frames, mics, T, band, seg_first, seg_hop, segs, win, weights, forget)
    return b1, b2


def case_chain(case, row, batches=None):
    """... and the design for one row of offsets behind each of the two calls -> (r1, r2): learn_batch's dict and state_stages' in one."""
    n, T, band, loading = case[0], case[3], case[9], case[10]
    tau = case_inputs(case)[3]
    return tuple(dict(b, **state_stages(b["acc"], b["total"], tau, row, lcmv_np.offset_per_dir(n), T, band, loading)) for b in (batches or case_batches(case)))


# ------------------------------------------------------------------ the scenes

M, N, HOP, F, T = mvdr_np.M, mvdr_np.N, mvdr_np.HOP, mvdr_np.F, mvdr_np.T
GATE = 8 * HOP                      # the look talker speaks in samples [0, GATE) of the period
LOOK_FREE = [0.0] * 7 + [1.0] * 7   # windows 7 .. 13: their segments start at (f + 1) HOP + SEG_FIRST >= GATE


def gated_scene(tau):
    """mvdr_np.scene with the look talker, at the interferer's level, gated on for samples < GATE -> (sc, training signal [M, L])."""
    sc = mvdr_np.scene(tau)
    gate = (np.arange(sc["look"].shape[1]) < GATE).astype(np.float64)
    return sc, gate[None, :] * sc["look"] + sc["interferer"] + sc["noise"]


def moved_scenes(tau):
    """Two captures: the interferer at INTERFERER (seed 0), then at NEAR (seed 1), sensor noise in both, the look talker silent
    -> (old scene, new scene, old training signal, new training signal)."""
    old, new = mvdr_np.scene(tau), mvdr_np.scene(tau, interferer=fsn.NEAR, seed=1)
    return old, new, old["interferer"] + old["noise"], new["interferer"] + new["noise"]


def host_learn(state, train, weights, forget):
    """filtersum.mvdr_learn on the windows of a training signal with FilterSumListener.learn's segments (state None: empty) -> (acc, mass, used)."""
    frames, _ = mvdr_np.cut(train)
    acc, mass = (None, 0.0) if state is None else state[:2]
    return filtersum.mvdr_learn(acc, mass, frames, np.arange(M), weights, forget, n_taps=T, band=fsn.BAND, seg_first=mvdr_np.SEG_FIRST, seg_hop=mvdr_np.SEG_HOP,
                                segs=mvdr_np.SEGS, fs=fsn.FS)


def host_taps(state, tau):
    """design_mvdr_learned for one slot on LOOK -> taps float32 [1, M, T]."""
    taps, fallback, status = filtersum.design_mvdr_learned(state[0], state[1], tau, [fsn.flat(fsn.LOOK) * M], M, n_taps=T, band=fsn.BAND, loading=mvdr_np.LOADING,
                                                           fs=fsn.FS)
    assert status.tolist() == [0] and not fallback.any()
    return taps
