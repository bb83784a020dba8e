"""What the tests of bf_lcmv_design_device share: the float64 design of filtersum.design_lcmv restated with its INTERMEDIATES (the
gains G_k[m], the coherence of every drop decision, the condition of every solved system), which design_lcmv does not return, and
the cases of the definition table.

`slot_gains` repeats design_lcmv's loop expression for expression with design_slots' slot semantics; tests/test_lcmv_design_host.py
pins it to design_slots (the same kept entries, and irfft of its gains rounded to float32 gives the same taps bit for bit), so what
the device is held to is design_lcmv's arithmetic and nothing else."""
import numpy as np

import filtersum

FS = 48828.0
FULL = (0.0, FS / 2.0)              # every bin 0 .. T // 2
VOICE = (3000.0, 8000.0)
D = 12                              # directions of the random tables


def slot_gains(tau, offsets, offset_per_dir, n_taps, band, rho, fs=FS):
    """-> dict: gains complex128 [S, K, M] (zero for a slot that is no source), kept int32 [S, K, S], status int32 [S], bins,
    decisions = [(beam, bin index, null slot, coherence |c^H c'| / M, kept)] one entry per COMPARISON made (a null is compared with the
    look vector and with every null kept before it until one comparison fails -- as `all()` stops), conds = cond(C^H C) of every solve."""
    tau = np.asarray(tau, dtype=np.float64)
    M, T = tau.shape[1], int(n_taps)
    dirs = filtersum.slot_directions(offsets, offset_per_dir, tau.shape[0])
    S = len(dirs)
    bins = filtersum.band_bins(T, band, fs)
    G = np.zeros((S, bins.size, M), dtype=np.complex128)
    kept = np.zeros((S, bins.size, S), dtype=np.int32)
    decisions, conds = [], []
    for b in range(S):
        if dirs[b] < 0:
            continue
        for i, k in enumerate(bins):
            w = 2.0 * np.pi * k / T
            cols = [np.exp(1j * w * tau[dirs[b]])]
            for j in range(S):
                if j == b or dirs[j] < 0:
                    continue
                c = np.exp(1j * w * tau[dirs[j]])
                ok = True
                for other in cols:
                    coh = abs(np.vdot(c, other)) / M
                    ok = coh <= rho
                    decisions.append((b, i, j, float(coh), bool(ok)))
                    if not ok:
                        break
                if ok:
                    cols.append(c)
                    kept[b, i, j] = 1
            C = np.stack(cols, axis=1)
            f = np.zeros(C.shape[1], dtype=np.complex128)
            f[0] = np.exp(-1j * w * (T - 1) / 2.0)
            A = C.conj().T @ C
            conds.append(float(np.linalg.cond(A)))
            u = C @ np.linalg.solve(A, f.conj())
            G[b, i] = u.conj()
    status = np.array([0 if d >= 0 else 1 for d in dirs], dtype=np.int32)
    return dict(gains=G, kept=kept, status=status, bins=bins, decisions=decisions, conds=conds)


def taps_of(gains, bins, n_taps):
    """design_lcmv's last two lines: the gains on the whole grid, irfft, one rounding to float32.  gains [S, K, M] -> [S, M, T]."""
    S, K, M = gains.shape
    full = np.zeros((S, M, int(n_taps) // 2 + 1), dtype=np.complex128)
    full[:, :, bins] = gains.transpose(0, 2, 1)
    return np.ascontiguousarray(np.fft.irfft(full, n=int(n_taps), axis=2), dtype=np.float32)


# ------------------------------------------------------------------ the definition table

#        n   S   T    band   rho   seed
TABLE = [
    (1, 1, 1, FULL, 0.95, 0),        # the degenerate ends: one microphone, one slot, one tap, bin 0 only
    (3, 3, 8, FULL, 0.6, 0),         # even T: DC and Nyquist bins, s_k = 1
    (3, 3, 9, VOICE, 0.6, 0),
    (16, 8, 9, FULL, 0.3, 0),
    (64, 4, 65, VOICE, 0.95, 0),
    (70, 8, 33, VOICE, 0.15, 0),     # n > 64: more than one pass of a wave
    (70, 8, 64, FULL, 0.95, 0),
    (5, 4, 1024, VOICE, 0.5, 0),     # the longest filter
]


def table_tau(n, S, T, seed):
    """Random delays, uniform in +-8 samples: no geometry and no configuration is needed."""
    return np.random.default_rng([n, S, T, seed]).uniform(-8.0, 8.0, size=(D, n))


def offset_per_dir(n):
    return max(n, 3)                 # the tracker's n, but at least 3 so that a stray non-multiple exists


def offset_rows(n, S, T, seed):
    """The rows of offsets one case is designed for.  S slots cannot hold a -1, a stray non-multiple and a duplicated direction at
    once when S < 4 (a duplicate takes two slots), so every case designs several rows: all slots valid; one slot -1; one a
    non-multiple of offset_per_dir; one a direction past the table; (S >= 2) the last slot a duplicate of slot 0; (S >= 4) the
    -1, the non-multiple and the duplicate together."""
    rng = np.random.default_rng([n, S, T, seed, 1])
    step = offset_per_dir(n)
    base = (rng.permutation(D)[:S] * step).astype(np.int32)
    rows = [("all valid", base.copy())]
    r = base.copy(); r[1 % S] = -1; rows.append(("a -1 slot", r))
    r = base.copy(); r[S - 1] += 1; rows.append(("a non-multiple", r))
    r = base.copy(); r[S - 1] = D * step; rows.append(("a direction past the table", r))
    if S >= 2:
        r = base.copy(); r[S - 1] = base[0]; rows.append(("a duplicated direction", r))
    if S >= 4:
        r = base.copy(); r[1] = -1; r[2] += step - 1; r[S - 1] = base[0]; rows.append(("-1, non-multiple and duplicate", r))
    return rows
