"""NumPy restatement of bf_remove_sources_device (include/beamformer_hip.h) and of BeamListener.separate's loop.

The reference has no counterpart, so this module IS the definition the kernel is pinned to.  Every array operation below is one
float32 operation per element (NumPy fuses nothing), in the order the header states, so the GPU results must be equal, not close:
  remove        vectorised over (microphone, sample)                (what the GPU tests compare with)
  remove_naive  the definition read aloud, one sample at a time     (what test_remove_sources_host.py compares `remove` with)
  beam          the forward operators miso_pad / miso_lerp, for the adjoint identity
  separate      the CLEAN loop; maps and beams come from the committed C oracle, which is bit-identical to the library, the pick
                from tests/peaks_np.py
  scene         the two-source scene of the end-to-end tests
Tables are what the loaders keep: whole-sample delays clamped to N, and for lerp h = float32(1 - float32(frac))."""
import numpy as np

import peaks_np

PAD, LERP = 0, 1
F32 = np.float32


def pad_table(whole, N):
    """int32 delays as load_coefficients_pad keeps them -> (whole clamped to N, None)."""
    return np.minimum(np.asarray(whole, dtype=np.int32).ravel(), N).astype(np.int32), None


def lerp_table(delays_f32, N):
    """float32 delays as load_coefficients_lerp splits them (lerp_and_sum.c:139-153) -> (whole clamped to N, h)."""
    d = np.asarray(delays_f32, dtype=np.float32).ravel().astype(np.float64)
    frac, ip = np.modf(d)
    h = (1.0 - frac.astype(np.float32).astype(np.float64)).astype(np.float32)
    return np.minimum(ip.astype(np.int32), N).astype(np.int32), h


def status_of(offsets, n, entries):
    """bf_miso_device's verdicts: 1 for an offset that is negative or past the table."""
    o = np.asarray(offsets, dtype=np.int64)
    return ((o < 0) | (o + n > entries)).astype(np.int32)


def adjoint(algo, o, p, h, N):
    """o float32 [>= N] one beam, p int [n], h float32 [n] (lerp) -> a float32 [n, N]: the beam projected back onto n microphones."""
    j = np.arange(N)[None, :]
    t = j + p.astype(np.int64)[:, None]
    zero = F32(0)
    if algo == PAD:
        return np.where(t < N, o[np.minimum(t, N - 1)], zero).astype(np.float32)
    u = np.where(t + 1 < N, o[np.minimum(t + 1, N - 1)], zero).astype(np.float32)
    v = np.where((j >= 1) & (t < N), o[np.minimum(t, N - 1)], zero).astype(np.float32)
    hh = h.astype(np.float32)[:, None]
    w = F32(1) - hh                       # sub
    return w * u + hh * v                 # mul, mul, add


def remove(algo, x, mics, whole, h, offsets, beams, gain):
    """x float32 [F, M_total, N]; mics int [n]; (whole, h) from pad_table / lerp_table; offsets int [F, B]; beams float32 [F, B, >= N]
    -> (residual float32 [F, M_total, N], status int32 [F, B]).  Rows of `beams` at rejected offsets are not read."""
    x = np.asarray(x, dtype=np.float32)
    F, _, N = x.shape
    mics = np.asarray(mics, dtype=np.int64)
    n = mics.size
    offsets = np.asarray(offsets, dtype=np.int64)
    status = status_of(offsets, n, whole.size)
    c = F32(gain) / F32(n)
    res = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(F):
            acc = x[f, mics, :]
            for b in range(offsets.shape[1]):
                if status[f, b]:
                    continue
                off = int(offsets[f, b])
                a = adjoint(algo, np.asarray(beams[f, b], dtype=np.float32), whole[off:off + n], None if h is None else h[off:off + n], N)
                acc = acc - c * a         # mul, sub
            res[f, mics, :] = acc
    return res, status


def remove_naive(algo, x, mics, whole, h, offsets, beams, gain):
    x = np.asarray(x, dtype=np.float32)
    F, _, N = x.shape
    n = len(mics)
    status = status_of(offsets, n, whole.size)
    c = F32(gain) / F32(n)
    res = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(F):
            for m in range(n):
                for j in range(N):
                    acc = x[f, mics[m], j]
                    for b in range(np.asarray(offsets).shape[1]):
                        if status[f, b]:
                            continue
                        o = beams[f, b]
                        p = int(whole[int(offsets[f, b]) + m])
                        if algo == PAD:
                            a = o[j + p] if j + p < N else F32(0)
                        else:
                            hh = h[int(offsets[f, b]) + m]
                            u = o[j + p + 1] if j + p + 1 < N else F32(0)
                            v = o[j + p] if (j >= 1 and j + p < N) else F32(0)
                            a = F32(F32(F32(1) - hh) * u) + F32(hh * v)
                        acc = F32(acc - F32(c * a))
                    res[f, mics[m], j] = acc
    return res, status


def beam(algo, x, mics, p, h):
    """The forward operators, x float32 [M_total, N] -> out float32 [N], in the reference's microphone order:
    miso_pad out[p + i] += s[i] (i < N - p); miso_lerp out[p + i + 1] += s[i] + h * (s[i + 1] - s[i]) (i < N - p - 1)."""
    N = x.shape[1]
    out = np.zeros(N, dtype=np.float32)
    for m, r in enumerate(mics):
        s, pm = x[r], int(p[m])
        if algo == PAD:
            if pm < N:
                out[pm:] += s[:N - pm]
        elif N - pm - 1 > 0:
            L = N - pm - 1
            out[pm + 1:] += s[:L] + h[m] * (s[1:L + 1] - s[:L])
    return out


def separate(orc, algo, frames, mics, table, rows, cols, k, gain=1.0, floor_rel=0.0, floor_abs=0.0):
    """BeamListener.separate restated.  orc: das_oracle.Oracle(N, rows, cols, T); table: what the loader takes (int32 whole delays
    for pad, float32 delays for lerp) -> (offsets int32 [F, k], values float32 [F, k], beams float32 [F, k, N], residual)."""
    frames = np.asarray(frames, dtype=np.float32)
    F, _, N = frames.shape
    mics = np.ascontiguousarray(mics, dtype=np.int32)
    n = mics.size
    whole, h = pad_table(table, N) if algo == PAD else lerp_table(table, N)
    residual = frames.copy()
    offsets = np.empty((F, k), dtype=np.int32)
    values = np.empty((F, k), dtype=np.float32)
    beams = np.empty((F, k, N), dtype=np.float32)
    for i in range(k):
        if algo == PAD:
            power = np.stack([orc.mimo_pad(residual[f], table, mics).ravel() for f in range(F)])
        else:
            power = np.stack([orc.mimo_lerp(residual[f], table, mics).ravel() for f in range(F)])
        offs, vals, _ = peaks_np.peaks(power, rows, cols, max(rows, cols), 1, floor_rel, floor_abs, n)
        bm = np.full((F, 1, N), np.nan, dtype=np.float32)
        for f in range(F):
            if offs[f, 0] >= 0:
                bm[f, 0] = (orc.miso_pad if algo == PAD else orc.miso_lerp)(residual[f], table, mics, int(offs[f, 0]))
        residual, _ = remove(algo, residual, mics, whole, h, offs, bm, gain)
        offsets[:, i], values[:, i], beams[:, i] = offs[:, 0], vals[:, 0], bm[:, 0]
    return offsets, values, beams, residual


# ------------------------------------------------------------------ the two-source scene of the end-to-end tests

SCENE = dict(rows=41, cols=23, M=64, N=256, A=(13, 15), B=(30, 5), tones_a=(2000.0, 3100.0, 4700.0), tones_b=(2500.0, 3900.0, 5600.0),
             b_db=-10.0, noise=0.02, seed=1, fs=48828.0)


def scene(delays):
    """delays float64 [rows, cols, M] of the grid -> frames float32 [2, M, N]: source A plus source B 10 dB below it, every microphone's
    signal advanced by its delay of the source's direction, plus white noise; the second frame swaps the two directions."""
    s = SCENE
    k = np.arange(s["N"], dtype=np.float64)[None, :]
    rng = np.random.default_rng(s["seed"])

    def wave(direction, tones):
        t = (k + delays[direction[0], direction[1]][:, None]) / s["fs"]
        return sum(np.sin(2 * np.pi * f * t) for f in tones) / len(tones)

    amp_b = 10.0 ** (s["b_db"] / 20.0)
    frames = []
    for a_dir, b_dir in ((s["A"], s["B"]), (s["B"], s["A"])):
        x = wave(a_dir, s["tones_a"]) + amp_b * wave(b_dir, s["tones_b"]) + s["noise"] * rng.standard_normal((s["M"], s["N"]))
        frames.append(x.astype(np.float32))
    return np.ascontiguousarray(np.stack(frames))


_SCENE_CACHE = {}


def scene_reference(oracle_lib):
    """The scene, the restated loop on it (k = 2, gain 1, lerp) and its plain maps, computed once per process ->
    (frames [2, M, N], float32 delay table, (offsets, values, beams, residual), plain maps [2, rows * cols])."""
    if "ref" not in _SCENE_CACHE:
        import directions_np as D
        s = SCENE
        delays = D.calculate_delays(s["rows"], s["cols"], arrays=1)
        assert delays.shape == (s["rows"], s["cols"], s["M"])
        frames = scene(delays)
        orc = oracle_lib.Oracle(s["N"], s["rows"], s["cols"], 8)
        mics = np.arange(s["M"], dtype=np.int32)
        table = np.float32(delays)
        sep = separate(orc, LERP, frames, mics, table, s["rows"], s["cols"], 2, 1.0)
        plain = np.stack([orc.mimo_lerp(frames[f], table, mics).ravel() for f in range(2)])
        for a in (frames, table, plain) + sep:
            a.setflags(write=False)
        _SCENE_CACHE["ref"] = (frames, table, sep, plain)
    return _SCENE_CACHE["ref"]


def chebyshev(offset, n, cols, point):
    """Grid distance between the direction of table offset `offset` and `point` (None for an empty slot)."""
    if offset < 0:
        return None
    d = int(offset) // n
    return max(abs(d // cols - point[0]), abs(d % cols - point[1]))
