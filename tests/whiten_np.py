"""NumPy restatement of bf_whiten_device (include/beamformer_hip.h): u = window * x in float32 exactly as defined, everything behind it
in float64; and the tolerance a float32 implementation of the definition has to keep, derived from the rounding model of a radix-2
FFT, not fitted to any implementation.

The tolerance.  u = 2^-24 is the unit roundoff, t = log2 N.
  Transform.  Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Theorem 24.2: a radix-2 Cooley-Tukey FFT whose computed
    twiddles are within mu of the true ones returns y^ with ||y^ - y||_2 <= t eta / (1 - t eta) ||y||_2, eta = mu + gamma_4 (sqrt 2 + mu),
    gamma_4 = 4 u / (1 - 4 u): a butterfly is one complex multiply (two products and an add per component, sqrt 2 gamma_2 on the
    modulus) and one complex add (u).  The kernel's twiddles are rounded once from double, each component within u of the truth, so
    mu = sqrt 2 u and eta = (sqrt 2 + 4 sqrt 2) u = 5 sqrt 2 u to first order; ETA carries 1 % for the second-order terms (t eta < 1e-5).
    A component's error is at most the vector's: with Parseval, |dX_k| <= e = t ETA u sqrt(N) ||u||_2.
  Magnitude.  |X^_k| computed as sqrt(re^2 + im^2): two products and a sum (3 u on P) then a square root: 2.5 u relative; and
    ||X^_k| - |X_k|| <= e.
  Floor.  rms is a norm / sqrt(n) of the band's n bins, so the error of X moves it by at most e; its own arithmetic (n sums of
    non-negative terms in any order, a division, a square root, the product with floor_rel) by at most ((n + 3) / 2 + 3) u relative.
  Denominator.  d = max(|X|, floor): |d^ - d| <= dd = max(e + 2.5 u (|X| + e), floor_rel (e + ((n + 3) / 2 + 3) u rms)); d^ >= d_lo = d - dd.
  Weighted bin (complex modulus).
    beta == 0:  dW = e.
    beta == 1:  W^ = fl(X^ / d^): |dW| <= (e + |X| dd / d) / d_lo + sqrt 2 u (|X| + e) / d_lo        (|X| <= d)
    otherwise:  g^ = powf(d^, -beta), within 16 float32 steps (the OpenCL bound, 32 u relative): |g^ - g| <= d_lo^-beta (1 + 32 u) - d^-beta,
                |dW| <= g_hi e + |X| |g^ - g| + sqrt 2 u g_hi (|X| + e),    g_hi = d_lo^-beta (1 + 32 u)
    A bin whose d_lo is not positive has no bound (inf): the case does not count.
  Output.  y_j = sum over the N two-sided bins of Y_k exp(+2 pi i j k / N): the bins' errors add up to at most sum |dW_k| (two-sided);
    the inverse transform's own rounding is at most t ETA u sqrt(N) ||Y^||_2 per component; the final product with gain / N rounds once:
        tol_j = |gain| / N (sum |dW| + t ETA u sqrt(N) (||W||_2 + ||dW||_2)) + u |out_j|
The order-agnostic 2 (N + 2) u sum |u| bound of spectrogram_np.py is vacuous here from N = 256 up (summed over the bins and divided by
small d_k it reaches 86 times a row's RMS at N = 1024); the norm-wise bound is not."""
import numpy as np

from stft_np import EPS, ETA, two_sided, windowed


def clip_bins(bins, n):
    return [(min(max(int(lo), 0), n // 2 + 1), min(max(int(hi), 0), n // 2 + 1)) for lo, hi in np.asarray(bins).reshape(-1, 2)]


def whiten(x, window, bins, beta, gain, floor_rel=1e-3, floor_abs=0.0, with_tol=False):
    """x float32 [..., N] -> float64 [K, ..., N] (and, with_tol, the tolerance of the same shape)."""
    u = windowed(x, window)
    n = u.shape[-1]
    t = int(np.log2(n))
    assert 1 << t == n
    X = np.fft.rfft(u.astype(np.float64), axis=-1)
    mag = np.abs(X)
    k = np.arange(n // 2 + 1)
    two = two_sided(n)
    e = t * ETA * EPS * np.sqrt(n) * np.sqrt((u.astype(np.float64) ** 2).sum(axis=-1))[..., None]
    outs, tols = [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for (lo, hi), b, g in zip(clip_bins(bins, n), np.asarray(beta, dtype=np.float32), np.asarray(gain, dtype=np.float32)):
            b, g = float(b), float(g)
            inside = (k >= lo) & (k < hi)
            nb = hi - lo
            if b == 0.0:
                W = np.where(inside, X, 0.0)
                dW = np.where(inside, e, 0.0) * np.ones_like(mag)
            else:
                rms = np.sqrt((mag[..., lo:hi] ** 2).mean(axis=-1))[..., None]
                floor = np.maximum(float(np.float32(floor_abs)), float(np.float32(floor_rel)) * rms)
                d = np.maximum(mag, floor)
                dd = np.maximum(e + 2.5 * EPS * (mag + e), float(np.float32(floor_rel)) * (e + ((nb + 3) / 2.0 + 3.0) * EPS * rms))
                d_lo = d - dd
                if b == 1.0:
                    gk = np.where(d > 0, 1.0 / d, 0.0)
                    dWk = (e + mag * dd / d) / d_lo + np.sqrt(2.0) * EPS * (mag + e) / d_lo
                else:
                    gk = np.where(d > 0, d ** -b, 0.0)
                    g_hi = d_lo ** -b * (1.0 + 32.0 * EPS)
                    dWk = g_hi * e + mag * (g_hi - gk) + np.sqrt(2.0) * EPS * g_hi * (mag + e)
                dWk = np.where(d_lo > 0, dWk, np.inf)
                dWk = np.where((d == 0) & (e == 0), 0.0, dWk)            # a row of zeros: W = 0 exactly
                W = np.where(inside, gk * X, 0.0)
                dW = np.where(inside, dWk, 0.0)
            Y = W.copy()
            Y[..., 0] = Y[..., 0].real
            Y[..., -1] = Y[..., -1].real
            y = np.fft.irfft(Y, n=n, axis=-1) * n                          # the unnormalised sum over the two-sided bins
            out = g / n * y
            outs.append(out)
            if with_tol:
                norm_W = np.sqrt((two * np.abs(Y) ** 2).sum(axis=-1))[..., None]
                norm_dW = np.sqrt((two * dW ** 2).sum(axis=-1))[..., None]
                sum_dW = (two * dW).sum(axis=-1)[..., None]
                tols.append(abs(g) / n * (sum_dW + t * ETA * EPS * np.sqrt(n) * (norm_W + norm_dW)) + EPS * np.abs(out))
    out = np.stack(outs)
    return (out, np.stack(tols)) if with_tol else out


def row_rms(a):
    return np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean(axis=-1))


def noise_rows(rng, shape):
    """White-noise rows whose scales spread over 2^-6 .. 2^5, one scale per row."""
    scale = np.exp2(rng.integers(-6, 6, size=shape[:-1] + (1,)).astype(np.float64))
    return (rng.standard_normal(shape) * scale).astype(np.float32)


# ------------------------------------------------------------------ the hum scene (README)

HUM = dict(X=41, Y=23, src=(12, 8), hum=(30, 15), n=256, fs=48828.0, noise=0.05, bins=(5, 64))


def hum_frame(seed, delays, src, hum, n, fs, noise, **_):
    """One window on the 8 x 8 array: a plane wave from grid cell `src` -- 400 equal tones from 2 to 10 kHz, random phases, unit RMS --
    under a hum from cell `hum` -- 1200 / 2400 / 3600 Hz at amplitudes 1 / 0.5 / 0.25, unit RMS times 10 (20 dB above the source) --
    and sensor noise.  `delays` float64 [X, Y, mics] in samples.  Returns float32 [mics, n]."""
    rng = np.random.default_rng(seed)
    mics = delays.shape[2]
    t0 = np.arange(n, dtype=np.float64)[None, :]

    def wave(cell, freqs, amps, phases):
        t = (t0 + delays[cell[0], cell[1]][:, None]) / fs                    # microphone m leads by its delay
        s = np.zeros_like(t)
        for f, a, p in zip(freqs, amps, phases):
            s += a * np.sin(2 * np.pi * f * t + p)
        return s

    f_src = np.linspace(2000.0, 10000.0, 400)
    s = wave(src, f_src, np.ones(400), rng.uniform(0, 2 * np.pi, 400))
    s /= np.sqrt(np.mean(s ** 2))
    h = wave(hum, (1200.0, 2400.0, 3600.0), (1.0, 0.5, 0.25), rng.uniform(0, 2 * np.pi, 3))
    h *= 10.0 / np.sqrt(np.mean(h ** 2))
    return (s + h + noise * rng.standard_normal((mics, n))).astype(np.float32)


def pink_frame(seed, delays, src, n, fs, noise=0.02, dc=0.05):
    """The 1/f + DC scene of test_band_filter_host.py as one window: 400 tones from 100 Hz to 8 kHz with 1/f amplitudes, unit RMS, from
    cell `src`, microphone noise and a DC offset per microphone.  Returns float32 [mics, n]."""
    rng = np.random.default_rng(seed)
    mics = delays.shape[2]
    f = np.linspace(100.0, 8000.0, 400)
    ph = rng.uniform(0, 2 * np.pi, f.size)
    t = (np.arange(n, dtype=np.float64)[None, :] + delays[src[0], src[1]][:, None]) / fs
    s = np.zeros_like(t)
    for fi, pi in zip(f, ph):
        s += (1.0 / fi) * np.sin(2 * np.pi * fi * t + pi)
    s /= np.sqrt(np.mean(s ** 2))
    return (s + noise * rng.standard_normal((mics, n)) + dc * rng.standard_normal((mics, 1))).astype(np.float32)


def within_3db(img):
    return int(np.count_nonzero(img >= img.max() * 10 ** -0.3))


def argmax2(img):
    return tuple(int(v) for v in np.unravel_index(np.argmax(img), img.shape))
