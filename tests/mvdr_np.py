"""What the tests of bf_mvdr_design_device share: filtersum.design_mvdr_slots restated with its INTERMEDIATES (the snapshots, the
covariance, the loaded matrix, its condition, the Cholesky factor, the gains), which the design functions do not return, the cases
of the definition table, and the scene with an interferer no slot names.

`slot_stages` repeats design_mvdr_slots' expressions one for one; tests/test_mvdr_design_host.py pins it to design_mvdr_slots (irfft
of its gains rounded to float32 gives the same taps bit for bit), so what the device is held to is that design's arithmetic."""
import numpy as np

import filtersum
import filtersum_np as fsn
import lcmv_np
from lcmv_np import FS, FULL, VOICE


def slot_stages(frames, mics, tau, offsets, offset_per_dir, n_taps, band, loading, seg_first, seg_hop, segs, window, fs=FS):
    """-> dict: snap complex128 [P, K, M], mass float64 [P, M] (sum_t |win[t] x[t]| of every snapshot row: the scale of its rounding),
    cov / loaded / chol complex128 [K, M, M], conds float64 [K] (cond of the loaded matrix), gains complex128 [S, K, M] (zero for a
    slot that is no source), fallback int32 [K], status int32 [S], bins, taps float32 [S, M, T]."""
    x = np.asarray(frames)
    tau = np.asarray(tau, dtype=np.float64)
    mics = np.asarray(mics).astype(np.int64).ravel()
    F, m_total, N = x.shape
    M, T = int(mics.size), int(n_taps)
    dirs = filtersum.slot_directions(offsets, offset_per_dir, tau.shape[0])
    win = np.ones(T) if window is None else np.asarray(window, dtype=np.float64)
    bins = filtersum.band_bins(T, band, fs)
    K, P = bins.size, F * segs
    r = np.arange(T)
    table = np.cos(2.0 * np.pi * r / T) - 1j * np.sin(2.0 * np.pi * r / T)
    E = table[(np.arange(T)[:, None] * bins[None, :]) % T]
    snap = np.empty((P, K, M), dtype=np.complex128)
    mass = np.empty((P, M))
    with np.errstate(all="ignore"):
        for f in range(F):
            for q in range(segs):
                s0 = seg_first + q * seg_hop
                seg = x[f][mics, s0:s0 + T].astype(np.float64) * win[None, :]
                snap[f * segs + q] = (seg @ E).T
                mass[f * segs + q] = np.abs(seg).sum(axis=1)
        cov = np.einsum("pka,pkb->kab", snap, snap.conj()) / P
        loaded = np.empty_like(cov)
        chol = np.empty_like(cov)
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
    return dict(snap=snap, mass=mass, cov=cov, loaded=loaded, chol=chol, conds=conds, gains=G, fallback=fallback, status=status, bins=bins,
                taps=lcmv_np.taps_of(G, bins, T))


# ------------------------------------------------------------------ the definition table

def hann(T):
    return np.hanning(T + 2)[1:-1]


#        n   m_total S  T   N   frames seg_first seg_hop segs  band  loading  window
TABLE = [
    (1, 1, 1, 1, 8, 1, 0, 1, 8, FULL, 0.1, None),              # the degenerate ends: one microphone, one slot, one tap, bin 0 only
    (3, 5, 3, 8, 32, 2, 1, 5, 5, FULL, 0.05, None),            # even T: DC and Nyquist bins; rows (4, 0, 2) of 5: neither identity nor ordered
    (16, 16, 8, 9, 32, 1, 3, 7, 2, FULL, 0.01, None),          # P = 2 < n: rank deficient, only the loading makes it definite
    (64, 64, 4, 65, 256, 3, 0, 16, 12, VOICE, 0.1, "hann"),    # the shipped shape
    (70, 72, 8, 33, 64, 2, 0, 8, 4, VOICE, 0.05, None),        # n > 64: crosses one wave, and five 16-row tiles with a ragged last one
    (130, 130, 2, 17, 64, 2, 5, 6, 8, FULL, 0.1, None),        # more than two waves, 9 x 9 tiles, P = 16: exactly one staged chunk
    (256, 256, 1, 9, 32, 1, 0, 4, 6, VOICE, 0.1, None),        # the largest array, P small
]
# cond(R') <= (tr + load) / load = n / loading + 1 with load = loading tr / n: kept <= 1e4 by the loadings above (n = 256: 2561)


def case_id(case):
    return "n%d_S%d_T%d" % (case[0], case[2], case[3])


def case_inputs(case):
    """-> (frames float32 [F, m_total, N], mics int32 [n], tau float64 [D, n], window or None): seeded, nothing configured."""
    n, m_total, S, T, N, F, seg_first, seg_hop, segs, band, loading, window = case
    rng = np.random.default_rng([n, m_total, S, T, 7])
    frames = rng.standard_normal((F, m_total, N)).astype(np.float32)
    mics = np.array([4, 0, 2], dtype=np.int32) if (n, m_total) == (3, 5) else rng.permutation(m_total)[:n].astype(np.int32)
    return frames, mics, lcmv_np.table_tau(n, S, T, 0), (hann(T) if window == "hann" else None)


# ------------------------------------------------------------------ the scene: an interferer NO slot names

M, N, HOP, F, T = 64, 256, 128, 14, 65
NOISE = 0.05                        # sensor noise, RMS
LOADING, SEG_HOP = 0.1, 16          # the shipped defaults
SEG_FIRST = max(0, N - HOP - T + 1)                                   # FilterSumListener.adapt's choice with a hop
SEGS = (N - SEG_FIRST - T) // SEG_HOP + 1


def scene_tau():
    import directions_np as D
    return D.calculate_delays(fsn.GRID[0], fsn.GRID[1], arrays=1).reshape(-1, M)


def scene(tau, interferer=fsn.INTERFERER, seed=0):
    """-> dict of float64 [M, L] periodic signals: look, interferer, noise."""
    rng = np.random.default_rng(seed)
    L = HOP * (F + 1) + N
    x_look = fsn.at_microphones(fsn.band_noise(rng, L), tau[fsn.flat(fsn.LOOK)], L)
    x_int = fsn.at_microphones(fsn.band_noise(rng, L), tau[fsn.flat(interferer)], L)
    return dict(look=x_look, interferer=x_int, noise=NOISE * rng.standard_normal((M, L)))


def cut(s):
    """Periodic [M, L] -> (windows float32 [F, M, N] at hop HOP, the window before them float32 [M, N])."""
    return (np.ascontiguousarray(np.stack([s[:, (f + 1) * HOP:(f + 1) * HOP + N] for f in range(F)]), dtype=np.float32),
            np.ascontiguousarray(s[:, :N], dtype=np.float32))


def power(y):
    return float(np.mean(np.asarray(y, dtype=np.float64) ** 2))


def row(sc, g):
    """One beam's taps g [M, T] on the scene, circular float64 beams (filtersum_np.beam_f64) -> (interferer dB, white-noise gain dB, look dB)."""
    g = np.asarray(g, dtype=np.float32)
    return (fsn.db(power(fsn.beam_f64(sc["interferer"], g)) / power(sc["interferer"][0])), fsn.db(float(np.sum(g.astype(np.float64) ** 2))),
            fsn.db(power(fsn.beam_f64(sc["look"], g)) / power(sc["look"][0])))


def trainings(sc):
    """The three rows of the README's table: what the covariance is learned from."""
    return [("interferer + noise (look talker silent)", sc["interferer"] + sc["noise"]),
            ("the same, look talker 20 dB below the interferer", 0.1 * sc["look"] + sc["interferer"] + sc["noise"]),
            ("the same, look talker at the interferer's level", sc["look"] + sc["interferer"] + sc["noise"])]
