"""NumPy restatement of bf_postfilter_device (include/beamformer_hip.h): the framing in integers, u = window * x in float32 and the
steering rounded once to float32 exactly as defined, the transforms and the microphone sums in float64, the recursion in float32 NumPy
operations in the header's order (`recursion`; dtype=float64 gives the same recursion in double for the acoustic figures), and the
tolerance a float32 implementation of the definition has to keep on num and den, derived from the rounding model of a radix-2 FFT and of
recursive summation, not fitted to any implementation.

The tolerance (`raw_bound`).  u = 2^-24 is the unit roundoff, t = log2 n_fft, ETA as in stft_np.py, n the microphones.
  Analysis.   every X_{m,k} is within e_m = t ETA u sqrt(n_fft) ||u_m||_2 of the truth (enhance_np.py).
  Power.      q = fl(re re + im im), two products and an add:  dq_m = (2 |X_m| e_m + e_m^2) (1 + 3 u) + 3 u |X_m|^2.
  Steering.   a is GIVEN (the float32 pair is the definition's), |a| <= 1 + u; Z = fl(a X) is a complex product of four multiplies and
              two adds, within sqrt 8 u |a| |X| of the exact product (Higham, Lemma 3.5):
                  dz_m = (1 + u) (e_m + sqrt 8 u (|X_m| + e_m)).
  Sums.       n terms added in ANY order round by at most gamma = (n - 1) u (1 + n u) times the sum of the terms' magnitudes (Higham,
              section 4.2), per real component, sqrt 2 times that in modulus for the complex sum:
                  dY = sum dz_m + sqrt 2 gamma sum (|Z_m| + dz_m),        dQ = sum dq_m + gamma sum (q_m + dq_m).
  |Y|^2.      d|Y|^2 = (2 |Y| dY + dY^2) (1 + 3 u) + 3 u |Y|^2.
  num, den.   one subtraction and one division (the divisors n (n - 1), n, n^2 are exact):
                  dnum = ((d|Y|^2 + dQ) (1 + 2 u) + 2 u ||Y|^2 - Q|) / (n (n - 1))
                  dden = (dQ (1 + u) + u Q) / n          or          (d|Y|^2 (1 + u) + u |Y|^2) / n^2.
The bound is in units of u Q (and u |Y|^2), not of u |num|: for incoherent input |Y|^2 - Q cancels, num is small against Q, and a
relative bound on num -- hence on the gain N / D at face value -- would be meaningless.  What follows for the gain (`gain_bound`): N and
D are convex combinations of the frames' num and den, N_i = (1 - beta) num_i + beta N_{i-1}, so the errors combine the same way, plus the
two roundings of fmaf(beta, N - num, num):
                  dN_i = (1 - beta) dnum_i + beta dN_{i-1} + u (beta |N_{i-1} - num_i| + |N_i|) (1 + 2 u),
and where D is away from 0, D > 2 dD, the clamped ratio (clamping is 1-Lipschitz) is within
                  dG = (dN + r dD) / (D - dD) + u,        r = min(max(N, 0) / D, 1) ... taken at its upper estimate (N + dN) / (D - dD).
Elsewhere nothing can be said beyond g_min <= G <= 1.  The recursion itself has no tolerance: it is compared bit for bit, on the num and
den the device itself reports."""
import functools

import numpy as np

import stft_np
from enhance_np import db, fmaf
from stft_np import EPS, ETA, advance, analysis, frame_grid_ok, frame_starts, new_history   # (the tests reach the stream's and the grid's here)

MAX_SLOTS = 8
HEADER = 16


# ------------------------------------------------------------------ integers

def workspace(slots, samples, n_fft, hop_s):
    if slots < 1 or slots > MAX_SLOTS or not frame_grid_ok(samples, n_fft, hop_s):
        return -1
    return HEADER + slots * advance(0, samples, hop_s)[2] * (1 + 2 * (n_fft // 2 + 1))


def slot_directions(offsets, offset_per_dir, dirs):
    """The direction of every slot, -1 where the entry is no source (bf_lcmv_design_device's rule)."""
    return [int(o) // offset_per_dir if o >= 0 and o % offset_per_dir == 0 and o // offset_per_dir < dirs else -1 for o in np.asarray(offsets).tolist()]


def stream(frames, mics, hop):
    """frames float32 [F, M_total, N] -> x float32 [n, S]: the last len = hop or N samples of every window of the rows `mics`."""
    return stft_np.stream(frames, np.shape(frames)[2], hop, rows=mics)


# ------------------------------------------------------------------ as defined

def steering(tau, dirs, n_fft):
    """a float32 [slots, n, K, 2] = (cos, -sin)(pi * 2 k tau[d][m] / n_fft), the argument formed as the header writes it and reduced
    exactly (it is a double: fmod loses nothing), rounded once; zeros for a slot with direction -1."""
    tau = np.asarray(tau, dtype=np.float64)
    K = n_fft // 2 + 1
    a = np.zeros((len(dirs), tau.shape[1], K, 2), np.float32)
    k = np.arange(K, dtype=np.float64)
    for b, d in enumerate(dirs):
        if d < 0:
            continue
        arg = np.fmod(2.0 * k[None, :] * tau[d][:, None] / float(n_fft), 2.0)
        a[b, :, :, 0] = np.cos(np.pi * arg)
        a[b, :, :, 1] = -np.sin(np.pi * arg)
    return a


def raw(X, a, den_mode):
    """X complex [n, count, K], a float32 [slots, n, K, 2] -> dict(Z [slots, n, count, K], Y, Q [count, K], yy, num, den [slots, count, K])."""
    n = X.shape[0]
    ac = a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)
    Z = ac[:, :, None, :] * X[None]
    Y = Z.sum(axis=1)
    Q = (X.real ** 2 + X.imag ** 2).sum(axis=0)
    yy = Y.real ** 2 + Y.imag ** 2
    num = (yy - Q[None]) / (n * (n - 1))
    den = np.broadcast_to(Q[None] / n, yy.shape).copy() if den_mode == 0 else yy / (n * n)
    return dict(Z=Z, Y=Y, Q=Q, yy=yy, num=num, den=den)


def pair_mean(Z):
    """The explicit mean over the n (n - 1) / 2 pairs of Re(Z_i conj Z_j), Z [n, ...]."""
    n = Z.shape[0]
    total = 0.0
    for i in range(n):
        for j in range(i + 1, n):
            total = total + (Z[i] * np.conj(Z[j])).real
    return total / (n * (n - 1) / 2)


def raw_bound(u, X, r, den_mode):
    """(dnum, dden) [slots, count, K]: the tolerance of the raw numerator and denominator (module docstring); r = raw(X, a, den_mode)."""
    n, _, n_fft = u.shape
    t = np.log2(n_fft)
    e = t * ETA * EPS * np.sqrt(n_fft) * np.sqrt((u.astype(np.float64) ** 2).sum(axis=-1))[..., None]        # [n, count, 1]
    absX = np.abs(X)
    q = absX ** 2
    dq = (2 * absX * e + e * e) * (1 + 3 * EPS) + 3 * EPS * q
    dz = (1 + EPS) * (e + np.sqrt(8.0) * EPS * (absX + e))                                                      # [n, count, K], for every slot
    gamma = (n - 1) * EPS * (1 + n * EPS)
    absZ = np.abs(r["Z"])
    dY = dz.sum(axis=0)[None] + np.sqrt(2.0) * gamma * (absZ + dz[None]).sum(axis=1)
    dQ = dq.sum(axis=0) + gamma * (q + dq).sum(axis=0)
    absY = np.abs(r["Y"])
    dyy = (2 * absY * dY + dY * dY) * (1 + 3 * EPS) + 3 * EPS * r["yy"]
    dnum = ((dyy + dQ[None]) * (1 + 2 * EPS) + 2 * EPS * np.abs(r["yy"] - r["Q"][None])) / (n * (n - 1)) + 1e-45
    if den_mode == 0:
        dden = np.broadcast_to(((dQ * (1 + EPS) + EPS * r["Q"]) / n)[None], dnum.shape) + 1e-45
    else:
        dden = (dyy * (1 + EPS) + EPS * r["yy"]) / (n * n) + 1e-45
    return dnum, dden


def recursion(num, den, N, D, seen, sources, beta=0.8, g_min=0.1, dtype=np.float32):
    """The header's recursion over the frames of num, den [slots, count, K] in order -> (G [slots, count, K], N', D', seen').  N, D
    [slots, K], seen and sources [slots].  dtype float32: every operation one float32 NumPy operation in the header's order; float64:
    the same recursion in double."""
    f = dtype
    fma = fmaf if f is np.float32 else (lambda a, b, c: a * b + c)
    num, den = np.asarray(num, dtype=f), np.asarray(den, dtype=f)
    N, D = np.array(N, dtype=f), np.array(D, dtype=f)
    seen = [int(s) for s in seen]
    beta, g_min, zero, one = f(np.float32(beta)), f(np.float32(g_min)), f(0), f(1)
    G = np.zeros(num.shape, dtype=f)
    with np.errstate(all="ignore"):
        for b in range(num.shape[0]):
            if not sources[b]:
                seen[b] = 0
                continue
            n_b, d_b, s = N[b].copy(), D[b].copy(), seen[b]
            for i in range(num.shape[1]):
                if not (np.isfinite(num[b, i]).all() and np.isfinite(den[b, i]).all()):
                    G[b, i] = f(np.nan)
                    continue
                if s == 0:
                    n_b, d_b, s = num[b, i].copy(), den[b, i].copy(), 1
                else:
                    n_b = fma(beta, n_b - num[b, i], num[b, i]).astype(f)
                    d_b = fma(beta, d_b - den[b, i], den[b, i]).astype(f)
                ratio = (np.where(n_b < zero, zero, n_b) / d_b).astype(f)
                ratio = np.where(ratio < g_min, g_min, ratio)
                ratio = np.where(ratio > one, one, ratio)
                G[b, i] = np.where(d_b > zero, ratio, g_min)
            if s:
                N[b], D[b] = n_b, d_b
            seen[b] = s
    return G, N, D, seen


def smooth_bound(num, den, dnum, dden, N0, D0, seen, beta):
    """(N, D, dN, dD) [count, K] of ONE slot in float64 from exact-arithmetic num, den [count, K] with tolerances dnum, dden, the
    carried N0, D0 [K] (given, so exact) and seen: the docstring's propagation.  Every frame must be finite."""
    beta = float(np.float32(beta))
    N, D, dN, dD = (np.zeros(num.shape) for _ in range(4))
    n_p, d_p, dn_p, dd_p, s = np.asarray(N0, np.float64), np.asarray(D0, np.float64), 0.0, 0.0, seen
    for i in range(num.shape[0]):
        if s == 0:
            N[i], D[i], dN[i], dD[i], s = num[i], den[i], dnum[i], dden[i], 1
        else:
            N[i] = (1 - beta) * num[i] + beta * n_p
            D[i] = (1 - beta) * den[i] + beta * d_p
            lin_n, lin_d = (1 - beta) * dnum[i] + beta * dn_p, (1 - beta) * dden[i] + beta * dd_p
            # (the roundings act on the computed values: the exact ones and their errors)
            dN[i] = lin_n + EPS * (beta * (np.abs(n_p - num[i]) + dn_p + dnum[i]) + np.abs(N[i]) + lin_n) * (1 + 2 * EPS)
            dD[i] = lin_d + EPS * (beta * (np.abs(d_p - den[i]) + dd_p + dden[i]) + np.abs(D[i]) + lin_d) * (1 + 2 * EPS)
        n_p, d_p, dn_p, dd_p = N[i], D[i], dN[i], dD[i]
    return N, D, dN, dD


def gain_bound(N, D, dN, dD, g_min):
    """dG where D > 2 dD, 1 - g_min (nothing said) elsewhere."""
    safe = D > 2 * dD
    low = np.where(safe, D - dD, 1.0)
    r = np.minimum((np.maximum(N, 0.0) + dN) / low, 1.0)
    return np.where(safe, np.minimum((dN + r * dD) / low + EPS, 1.0 - g_min), 1.0 - g_min)


def gain_of(N, D, g_min):
    with np.errstate(all="ignore"):
        return np.where(D > 0, np.minimum(np.maximum(np.maximum(N, 0.0) / np.where(D > 0, D, 1.0), g_min), 1.0), g_min)


def postfilter(x, hist, c, window, hop_s, lag, tau, offsets, offset_per_dir, den_mode, beta, g_min, N, D, seen, dtype=np.float64):
    """One call on x float32 [n, S] (stream()) with the carried hist [n, n_fft - 1 + lag], c, N, D [slots, K] and seen [slots] -> dict(G,
    num, den [slots, count, K] (float64; G from the recursion in `dtype` on this restatement's own num and den), dnum, dden, N, D, seen,
    hist, c, count, cap, steer, status, u, X)."""
    x = np.asarray(x, dtype=np.float32)
    n_fft = window.shape[0]
    count, c_new, cap = advance(c, x.shape[1], hop_s)
    dirs = slot_directions(offsets, offset_per_dir, np.asarray(tau).shape[0])
    a = steering(tau, dirs, n_fft)
    u, X, _ = analysis(x, hist, c, window, hop_s, lag)
    r = raw(X, a, den_mode)
    dnum, dden = raw_bound(u, X, r, den_mode)
    sources = [d >= 0 for d in dirs]
    G, N2, D2, seen2 = recursion(r["num"], r["den"], N, D, seen, sources, beta, g_min, dtype=dtype)
    return dict(G=G, num=r["num"], den=r["den"], dnum=dnum, dden=dden, N=N2, D=D2, seen=seen2, hist=new_history(np.asarray(hist, np.float32), x), c=c_new,
                count=count, cap=cap, steer=a, status=[0 if s else 1 for s in sources], u=u, X=X, sources=sources)


# ------------------------------------------------------------------ the scenes (README)

SCENE = dict(fs=48828.0, tones=((1000.0, 0.5), (2500.0, 0.3), (6100.0, 0.2)), gate=4096, first=2048, total=65536, n_fft=256, hop_s=128, beta=0.8, g_min=0.1,
             interferer=0.3, interferer_noise=0.05)


@functools.lru_cache(maxsize=None)
def scene_tau():
    """float64 [41 * 23, 64]: the delays of filtersum_np.GRID on one 8 x 8 array."""
    import directions_np as Dn
    import filtersum_np as fsn
    return Dn.calculate_delays(fsn.GRID[0], fsn.GRID[1], arrays=1).reshape(-1, 64)


def scene(seed, noise=0.2, interferer=False):
    """-> (s [L], parts dict name -> float64 [64, L], active [L]): the gated three-tone signal of enhance_np.tone_scene, 65536 samples long,
    arriving from filtersum_np.LOOK, white sensor noise of `noise` RMS, and with interferer=True band noise (3-8 kHz) of 0.3 RMS from
    filtersum_np.INTERFERER.  The microphone signals are periodic over L (FFT phases): the signal is silent at both ends."""
    import filtersum_np as fsn
    rng = np.random.default_rng(seed)
    L = SCENE["total"]
    t = np.arange(L, dtype=np.float64)
    s = sum(a * np.sin(2 * np.pi * f * t / SCENE["fs"] + rng.uniform(0, 2 * np.pi)) for f, a in SCENE["tones"])
    active = (t >= SCENE["first"]) & (((t - SCENE["first"]) // SCENE["gate"]) % 2 == 0)
    s = np.where(active, s, 0.0)
    tau = scene_tau()
    parts = dict(tones=fsn.at_microphones(np.fft.rfft(s), tau[fsn.flat(fsn.LOOK)], L), noise=noise * rng.standard_normal((64, L)))
    if interferer:
        parts["interferer"] = fsn.at_microphones(SCENE["interferer"] * fsn.band_noise(rng, L), tau[fsn.flat(fsn.INTERFERER)], L)
    return s, parts, active


def aligned_beam(x, tau_row):
    """The ideally aligned beam of periodic microphone signals x [M, L]: every microphone delayed by its tau (an FFT phase), the mean."""
    L = x.shape[1]
    w = 2.0 * np.pi * np.arange(L // 2 + 1) / L
    return np.fft.irfft((np.fft.rfft(x, axis=1) * np.exp(-1j * w[None, :] * np.asarray(tau_row)[:, None])).mean(axis=0), n=L)


def apply_gains(y, G, win_a, win_s, hop_s):
    """A beam component y [L] through bf_enhance_device's restatement with the given gains [count, K] -> [L], n_fft late."""
    import enhance_np as EN
    n_fft = win_a.shape[0]
    z = lambda n: np.zeros((1, n), np.float32)
    return EN.enhance(np.asarray(y, np.float32)[None], z(n_fft - 1), z(n_fft), 0, win_a, win_s, hop_s, G=G[None])["out"][0]


def figures(parts_in, parts_out, s, active, delay):
    """SNR over the active stretches before and after (tones against everything else), the distortion of the tones and the change of
    every other part, in dB.  parts_in: the aligned beam's components [L]; parts_out: the same behind the gains, `delay` late."""
    on = active[:s.size - delay]
    cut = lambda v: np.asarray(v, np.float64)[:s.size - delay][on]
    late = lambda v: np.asarray(v, np.float64)[delay:][on]
    power = lambda v: float((v ** 2).sum())
    others = [k for k in parts_in if k != "tones"]
    fig = dict(snr_in=db(power(cut(parts_in["tones"])) / power(sum(cut(parts_in[k]) for k in others))),
               snr_out=db(power(late(parts_out["tones"])) / power(sum(late(parts_out[k]) for k in others))),
               distortion=db(power(late(parts_out["tones"]) - cut(s)) / power(cut(s))))
    for k in others:
        fig[k] = db(power(late(parts_out[k])) / power(cut(parts_in[k])))
    return fig


def scene_gains(mixture, den_mode, beta=None, dtype=np.float64):
    """The gains [count, K] of the look direction on the mixture [64, L], a stream from silence, by the restatement."""
    import enhance
    import filtersum_np as fsn
    n_fft, hop_s = SCENE["n_fft"], SCENE["hop_s"]
    win_a = enhance.design_cola(n_fft, hop_s)[0]
    K = n_fft // 2 + 1
    tau = scene_tau()
    x = mixture.astype(np.float32)
    G = []
    N, D, seen, hist, c = np.zeros((1, K)), np.zeros((1, K)), [0], np.zeros((64, n_fft - 1), np.float32), 0
    for lo in range(0, x.shape[1], 8192):                                  # (in pieces: the cut does not matter, the memory does)
        r = postfilter(x[:, lo:lo + 8192], hist, c, win_a, hop_s, 0, tau, [fsn.flat(fsn.LOOK)], 1, den_mode, SCENE["beta"] if beta is None else beta,
                       SCENE["g_min"], N, D, seen, dtype=dtype)
        N, D, seen, hist, c = r["N"], r["D"], r["seen"], r["hist"], r["c"]
        G.append(r["G"][0])
    return np.concatenate(G, axis=0)


@functools.lru_cache(maxsize=None)
def host_scene(seed, noise=0.2, interferer=False, den_mode=0, beta=None):
    """A scene through the restatement in float64: the gains found on the mixture, applied to the aligned beam's components separately."""
    import enhance
    import filtersum_np as fsn
    n_fft, hop_s = SCENE["n_fft"], SCENE["hop_s"]
    win_a, win_s, _ = enhance.design_cola(n_fft, hop_s)
    s, parts, active = scene(seed, noise, interferer)
    G = scene_gains(sum(parts.values()), den_mode, beta)
    row = scene_tau()[fsn.flat(fsn.LOOK)]
    beams = {k: aligned_beam(v, row) for k, v in parts.items()}
    out = {k: apply_gains(v, G, win_a, win_s, hop_s) for k, v in beams.items()}
    return figures(beams, out, s, active, n_fft)
