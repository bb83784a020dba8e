"""CPU restatement of bf_das_select_device / bf_das_select_stream_device and of zoom.CoarseToFine (include/beamformer_hip.h).

The map at a listed offset is the committed C checker's map (oracle/das_oracle.py, Oracle.mimo_*) of a table that holds just the
listed rows: the checker then forms exactly the beam miso_* forms at that offset and applies the compiled reference's mean-power
rule to it, so the GPU values must be EQUAL.  The stream call's restatement is the extended-window one of tests/test_stream.py
(Case.want_power), used from there.  Lattice, windows and `locate` are index arithmetic on top of tests/peaks_np.py."""
import numpy as np

import peaks_np

NAN_BITS = 0x7FC00000


def verdicts(algo, offsets, n, T, entries):
    """bf_miso_device's codes for int offsets of any shape: 1 negative or offset + n * per > entries, 2 fir_vec offset off a multiple of T."""
    off = np.asarray(offsets, dtype=np.int64)
    per = T if algo == "fir_vec" else 1
    st = np.zeros(off.shape, dtype=np.int32)
    st[(off < 0) | (off + n * per > entries)] = 1
    if algo == "fir_vec":
        st[(st == 0) & (off % per != 0)] = 2
    return st


def powers(oracle_lib, tab, frames, mics, offsets, N):
    """tab: a test_miso_device.Tables (its flat table arrays, n, T, entries); frames float32 [F, M_total, N]; offsets int [F, B] ->
    (power float32 [F, B] with quiet NaNs at rejected entries, status int32 [F, B])."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    offsets = np.asarray(offsets, dtype=np.int64)
    F, B = offsets.shape
    n, T = tab.n, tab.T
    status = verdicts(tab.algo, offsets, n, T, tab.entries)
    power = np.full((F, B), np.nan, dtype=np.float32)
    power.view(np.uint32)[...] = NAN_BITS
    for f in range(F):
        ok = np.flatnonzero(status[f] == 0)
        if ok.size == 0:
            continue
        uniq, inverse = np.unique(offsets[f, ok], return_inverse=True)          # a repeated entry is computed once
        orc = oracle_lib.Oracle(N, uniq.size, 1, T)
        if tab.algo == "fir_vec":
            rows = np.stack([tab.h[o:o + n * T] for o in uniq])
            img = orc.mimo_convolve(frames[f], rows, mics, vectorized=True)
        else:
            src = tab.whole if tab.algo == "pad" else tab.d32
            rows = np.stack([src[o:o + n] for o in uniq])
            img = {"pad": orc.mimo_pad, "lerp": orc.mimo_lerp, "hybrid": orc.mimo_hybrid}[tab.algo](frames[f], rows, mics)
        power[f, ok] = img.ravel()[inverse]
    return power, status


# ------------------------------------------------------------------ lattice, windows, locate

def lattice(rows, cols, step):
    """-> (xs, ys, flat directions [Xc * Yc]) of every step-th cell from step // 2 on, in the grid's flat order d = x * cols + y."""
    xs, ys = np.arange(step // 2, rows, step), np.arange(step // 2, cols, step)
    return xs, ys, (xs[:, None] * cols + ys[None, :]).ravel()


def window(rows, cols, d, radius):
    """Flat directions of the (2 radius + 1)^2 window around direction d, x outer and y inner, -1 outside the grid (all -1 for d < 0)."""
    side = np.arange(-radius, radius + 1)
    if d < 0:
        return np.full(side.size * side.size, -1, dtype=np.int64)
    x, y = d // cols + side[:, None], d % cols + side[None, :]
    inside = (x >= 0) & (x < rows) & (y >= 0) & (y < cols)
    return np.where(inside, x * cols + y, -1).ravel()


def locate(full, rows, cols, step, radius, k, radius_c, floor_rel, floor_abs, opd):
    """full float32 [F, rows * cols]: the full maps -> (offsets int32 [F, k], values float32 [F, k], counts int32 [F, 3]) as
    zoom.CoarseToFine.locate defines them, every value read out of `full`."""
    full = np.asarray(full, dtype=np.float32)
    F = full.shape[0]
    xs, ys, lat = lattice(rows, cols, step)
    c_offs, _, counts = peaks_np.peaks(full[:, lat], xs.size, ys.size, radius_c, k, floor_rel, floor_abs, opd)
    offsets = np.full((F, k), -1, dtype=np.int32)
    values = np.zeros((F, k), dtype=np.float32)
    side = 2 * radius + 1
    for f in range(F):
        for s in range(k):
            if c_offs[f, s] < 0:
                continue
            win = window(rows, cols, int(lat[c_offs[f, s] // opd]), radius)
            vals = np.where(win >= 0, full[f, np.maximum(win, 0)], np.float32(np.nan)).astype(np.float32)
            w_offs, w_vals, _ = peaks_np.peaks(vals[None, :], side, side, 0, 1, 0.0, 0.0, 1)
            if w_offs[0, 0] >= 0:
                offsets[f, s], values[f, s] = win[w_offs[0, 0]] * opd, w_vals[0, 0]
    return offsets, values, counts


# ------------------------------------------------------------------ scenes of the coarse-to-fine tests

FS = 48828.0


def band_noise(rng, t, f_lo=3000.0, f_hi=8000.0, tones=96):
    """A 3-8 kHz noise source as a sum of random-phase tones, evaluated at the times t (seconds, any shape)."""
    f = rng.uniform(f_lo, f_hi, tones)
    ph = rng.uniform(0, 2 * np.pi, tones)
    a = rng.standard_normal(tones)
    s = np.zeros(np.shape(t))
    for fj, pj, aj in zip(f, ph, a):
        s += aj * np.cos(2 * np.pi * fj * t + pj)
    return s / np.sqrt(np.sum(a * a) / 2)


def scene(delays, sources, N, seed, noise=0.05, start=0):
    """delays float64 [X, Y, M]; sources [(x, y, amplitude)] -> float32 [M, N]: independent band-noise plane waves (microphone m LEADS
    by its delay, as synth.s3_plane_wave) plus white sensor noise of `noise` RMS; samples start .. start + N of the stream."""
    seed = [int(v) for v in np.atleast_1d(seed)]
    rng = np.random.default_rng(seed)
    M = delays.shape[2]
    k = (start + np.arange(N, dtype=np.float64))[None, :]
    sig = np.zeros((M, N))
    for x, y, amp in sources:
        src_rng = np.random.default_rng(seed + [x, y])
        sig += amp * band_noise(src_rng, (k + delays[x, y][:, None]) / FS)
    sig += noise * rng.standard_normal((M, N))
    return np.ascontiguousarray(sig.astype(np.float32))


# The scenes of tests/test_das_select.py's CoarseToFine cases; tests/test_das_select_host.py confirms for each, on the C checker's
# full map, that `locate` returns the full map's peaks (radius step * radius_c, the same floors).
ZOOM = {
    # grid, lattice step, window radius, k, coarse radius, floor_rel, frames as lists of (x, y, amplitude), seed
    "g41x23": dict(X=41, Y=23, N=64, step=4, radius=4, k=3, radius_c=2, floor_rel=0.25,
                   frames=[[(9, 17, 1.0), (30, 5, 0.7)], [(20, 11, 1.0)], []], seed=3),
    "g101": dict(X=101, Y=101, N=256, step=4, radius=4, k=4, radius_c=2, floor_rel=0.25,
                 frames=[[(37, 62, 1.0), (70, 21, 0.5)]], seed=13),
}


def zoom_frames(name, delays):
    """float32 [F, 64, N] of a ZOOM scene; a frame without sources is silence (all zeros: a constant map, one peak at index 0)."""
    z = ZOOM[name]
    M = delays.shape[2]
    return np.stack([scene(delays, src, z["N"], [z["seed"], f]) if src else np.zeros((M, z["N"]), np.float32) for f, src in enumerate(z["frames"])])
