"""NumPy restatement of bf_enhance_device (include/beamformer_hip.h): the framing and the overlap-add bookkeeping in integers, u = win_a * x
in float32 exactly as defined, the transforms in float64, the gain recursion in float32 NumPy operations in the header's order (`gains`;
dtype=float64 gives the same recursion in double for the acoustic figures), and the tolerance a float32 implementation of the definition
has to keep on d_out, derived from the rounding model of a radix-2 FFT, not fitted to any implementation.

The tolerance (`synthesis_bound`).  u = 2^-24 is the unit roundoff, t = log2 n_fft, n = n_fft, ETA as in whiten_np.py (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., Theorem 24.2, with twiddles rounded once from double: eta = 5 sqrt 2 u, 1 % for the second-order
terms).  Per frame:
  Analysis.   every X_k is within e = t ETA u sqrt(n) ||u||_2 of the truth (complex modulus; Parseval turns the theorem's norm into it).
  Product.    Y^_k = fl(G X^_k), one rounding per component with the given G: |dY_k| <= G e + sqrt 2 u G (|X_k| + e).
  Inverse.    z[j] = sum over the n two-sided bins of Y_k exp(+2 pi i j k / n): the bins' errors add up to at most sum |dY_k| (two-sided);
              the transform's own rounding is at most t ETA u sqrt(n) (||Y||_2 + ||dY||_2) on every component.
  Window.     v = (win_s / n) z rounds twice (the product win_s * (1 / n) is exact unless it is subnormal):
                  dv[j] = |win_s[j]| / n (sum |dY| + t ETA u sqrt(n) (||Y||_2 + ||dY||_2)) + 2 u |v[j]|
A position of the stream is the ordered sum of its <= 8 covering frames' v behind the carried partial sum (given, so exact): its m adds
round by at most m u (1 + 8 u) times the sum of the terms' magnitudes, |v| + dv each.  So
    tol[pos] = sum over the covering frames of dv  +  m u (1 + 8 u) (|carried| + sum (|v| + dv))
On top of that, where the output is compared with the delayed INPUT (G = 1), the windows' own defect: the products of design_cola's
rounded pair overlap-add to 1 within `deviation`, so y differs from x by at most deviation * max |x| over the n samples around it
(`cola_term`).  The gain recursion has no tolerance: it is compared bit for bit, on the P the device itself reports."""
import functools

import numpy as np

from stft_np import EPS, ETA, advance, analysis, frame_grid_ok, frame_starts, new_history, stream, two_sided   # (the tests reach the stream's and the grid's here)

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def workspace(rows, samples, n_fft, hop_s):
    if rows < 1 or not frame_grid_ok(samples, n_fft, hop_s):
        return -1
    return 4 + rows * advance(0, samples, hop_s)[2] * (4 * (n_fft // 2 + 1) + n_fft)


# ------------------------------------------------------------------ float32, as defined (u = win_a * x: stft_np.windowed)

def fmaf(a, b, c):
    """fmaf on float32 arrays with ONE rounding: the product is exact in float64, the float64 sum is brought to round-to-odd with its
    exact error (TwoSum), and a round-to-odd double rounds to the nearest float32 as the exact value does (it keeps 29 bits more)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, toward), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def gains(P, lam, prior, seen, alpha=0.98, a_noise=0.9, g0=1.5, g1=5.0, g_min=0.1, n_init=8, dtype=np.float32):
    """The header's recursion over the frames of P [R, count, B] in order -> (G [R, count, B], lam', prior', seen').  dtype float32: every
    operation one float32 NumPy operation in the header's order; float64: the same recursion in double (the constants stay float32's)."""
    f = dtype
    fma = fmaf if f is np.float32 else (lambda a, b, c: a * b + c)
    P = np.asarray(P, dtype=f)
    lam, prior = np.array(lam, dtype=f), np.array(prior, dtype=f)
    alpha, a_noise, g0, g1, g_min = (f(np.float32(v)) for v in (alpha, a_noise, g0, g1, g_min))
    one, zero, fmin, fmax = f(1), f(0), f(FLT_MIN), f(FLT_MAX)
    one_minus_alpha, one_minus_a_noise, width = one - alpha, one - a_noise, g1 - g0
    G = np.zeros(P.shape, dtype=f)
    with np.errstate(all="ignore"):
        for i in range(P.shape[1]):
            finite = np.isfinite(P[:, i])
            p_i = np.where(finite, P[:, i], zero)
            s = min(seen + i, n_init)
            if s < n_init:
                new = p_i if s == 0 else lam + (p_i - lam) / f(s + 1)
            else:
                g = p_i / np.maximum(lam, fmin)
                p = np.minimum(np.maximum((g - g0) / width, zero), one)
                a = a_noise + one_minus_a_noise * p
                new = fma(one - a, p_i - lam, lam)
            lam = np.where(finite, new, lam).astype(f)
            den = np.maximum(lam, fmin)
            gam = p_i / den
            ratio = np.minimum(prior / den, fmax)
            xi = fma(alpha, ratio, one_minus_alpha * np.maximum(gam - one, zero))
            g_i = np.maximum(one - one / (one + xi), g_min)
            prior = np.where(finite, (g_i * g_i) * p_i, prior).astype(f)
            G[:, i] = np.where(finite, g_i, f(np.nan))
    return G, lam, prior, min(seen + P.shape[1], n_init)


# ------------------------------------------------------------------ the call in float64, with its tolerance

def synthesis_bound(u, X, G, win_s, v):
    """dv [R, count, n_fft]: the tolerance of every frame's v (module docstring)."""
    n = u.shape[-1]
    t = int(np.log2(n))
    two = two_sided(n)
    e = t * ETA * EPS * np.sqrt(n) * np.sqrt((u.astype(np.float64) ** 2).sum(axis=-1))[..., None]
    absG = np.abs(G)
    dY = absG * e + np.sqrt(2.0) * EPS * absG * (np.abs(X) + e)
    Y = G * X
    norm_Y = np.sqrt((two * np.abs(Y) ** 2).sum(axis=-1))[..., None]
    norm_dY = np.sqrt((two * dY ** 2).sum(axis=-1))[..., None]
    sum_dY = (two * dY).sum(axis=-1)[..., None]
    return np.abs(win_s.astype(np.float64)) / n * (sum_dY + t * ETA * EPS * np.sqrt(n) * (norm_Y + norm_dY)) + 2.0 * EPS * np.abs(v)


def enhance(x, hist, ola, c, win_a, win_s, hop_s, G=None, track=None, dtype=np.float64):
    """One call (or a whole stream: the cut into calls is not part of the mathematics) on x float32 [R, S] with the carried hist
    [R, n_fft - 1], ola [R, n_fft] and c.  G [R, count, B]: the given gains; else track = dict(lam, prior, seen, **parameters) and the
    recursion runs in `dtype` on this restatement's own P.  -> dict(out [R, S], ola, tol_out, tol_ola (float64), hist, c, count, cap,
    P, G, and lam / prior / seen where tracked)."""
    x = np.asarray(x, dtype=np.float32)
    R, S = x.shape
    n_fft = win_a.shape[0]
    count, c_new, cap = advance(c, S, hop_s)
    u, X, starts = analysis(x, hist, c, win_a, hop_s)
    P = X.real ** 2 + X.imag ** 2
    res = dict(hist=new_history(np.asarray(hist, np.float32), x), c=c_new, count=count, cap=cap, P=P)
    if G is None:
        par = dict(track)
        G, res["lam"], res["prior"], res["seen"] = gains(P, par.pop("lam"), par.pop("prior"), par.pop("seen"), dtype=dtype, **par)
    G = np.asarray(G, dtype=np.float64)[:, :count]
    Y = G * X
    Y[..., 0] = Y[..., 0].real
    Y[..., -1] = Y[..., -1].real
    ws = np.asarray(win_s, dtype=np.float32)
    v = ws.astype(np.float64) / n_fft * (np.fft.irfft(Y, n=n_fft, axis=-1) * n_fft) if count else np.zeros((R, 0, n_fft))
    dv = synthesis_bound(u, X, G, ws, v) if count else v
    acc = np.concatenate([np.asarray(ola, dtype=np.float64), np.zeros((R, S))], axis=1)      # index = position + n_fft
    mag = np.abs(acc)
    tol = np.zeros_like(acc)
    adds = np.zeros(acc.shape[1])
    for i, s in enumerate(starts):
        sl = slice(s + n_fft, s + 2 * n_fft)
        acc[:, sl] += v[:, i]
        mag[:, sl] += np.abs(v[:, i]) + dv[:, i]
        tol[:, sl] += dv[:, i]
        adds[sl] += 1
    tol = tol + adds * EPS * (1.0 + 8.0 * EPS) * mag
    res.update(out=acc[:, :S], ola=acc[:, S:], tol_out=tol[:, :S], tol_ola=tol[:, S:], G=G)
    return res


def cola_term(x_ext, n_fft, deviation):
    """deviation * max |x| over the n_fft samples on either side of every sample of x_ext [R, T]."""
    a = np.abs(np.asarray(x_ext, dtype=np.float64))
    pad = np.pad(a, ((0, 0), (n_fft, n_fft)))
    best = np.zeros_like(a)
    for k in range(0, 2 * n_fft + 1):
        best = np.maximum(best, pad[:, k:k + a.shape[1]])
    return deviation * best


# ------------------------------------------------------------------ the tone scene (README)

SCENE = dict(fs=48828.0, tones=((1000.0, 0.5), (2500.0, 0.3), (6100.0, 0.2)), gate=4096, first=2048, noise=0.2, total=2048 + 10 * 4096, n_fft=256, hop_s=128)


def tone_scene(seed):
    """-> (s, d, active): three tones gated on and off every 4096 samples from sample 2048, white noise of 0.2 RMS, and where the tones are on."""
    rng = np.random.default_rng(seed)
    t = np.arange(SCENE["total"], dtype=np.float64)
    s = sum(a * np.sin(2 * np.pi * f * t / SCENE["fs"] + rng.uniform(0, 2 * np.pi)) for f, a in SCENE["tones"])
    active = (t >= SCENE["first"]) & (((t - SCENE["first"]) // SCENE["gate"]) % 2 == 0)
    s = np.where(active, s, 0.0)
    d = SCENE["noise"] * rng.standard_normal(t.size)
    return s.astype(np.float32), d.astype(np.float32), active


def db(a):
    return 10.0 * np.log10(a)


def scene_figures(s, d, active, y_s, y_d, delay):
    """SNR over the active stretches before and after (the shadow-filter method: the gains found on s + d applied to s and to d alone),
    and the distortion of s, all in dB.  y_s, y_d: the delayed outputs."""
    on = active[:s.size - delay]
    s0, d0 = s[:s.size - delay].astype(np.float64)[on], d[:s.size - delay].astype(np.float64)[on]
    ys, yd = np.asarray(y_s, np.float64)[delay:][on], np.asarray(y_d, np.float64)[delay:][on]
    return dict(snr_in=db((s0 ** 2).sum() / (d0 ** 2).sum()), snr_out=db((ys ** 2).sum() / (yd ** 2).sum()), distortion=db(((ys - s0) ** 2).sum() / (s0 ** 2).sum()))


@functools.lru_cache(maxsize=None)
def host_scene(seed, g0=1.5, g1=5.0):
    """The scene through the restatement in float64 with the default parameters -> the figures, and noise_ratio = tracked / true noise
    power, averaged over the bins."""
    import enhance as E
    n_fft, hop_s = SCENE["n_fft"], SCENE["hop_s"]
    win_a, win_s, _ = E.design_cola(n_fft, hop_s)
    s, d, active = tone_scene(seed)
    zeros = lambda n: np.zeros((1, n), np.float32)
    x = (s + d).astype(np.float32)
    run = lambda sig, **kw: enhance(sig[None], zeros(n_fft - 1), zeros(n_fft), 0, win_a, win_s, hop_s, **kw)
    mixed = run(x, track=dict(lam=zeros(n_fft // 2 + 1), prior=zeros(n_fft // 2 + 1), seen=0, g0=g0, g1=g1))
    fig = scene_figures(s, d, active, run(s, G=mixed["G"])["out"][0], run(d, G=mixed["G"])["out"][0], n_fft)
    true_psd = SCENE["noise"] ** 2 * float((win_a.astype(np.float64) ** 2).sum())
    fig["noise_ratio"] = float(mixed["lam"].mean() / true_psd)
    return fig
