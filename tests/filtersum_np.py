"""bf_filter_sum_device's definition (include/beamformer_hip.h) restated on top of tests/band_np.py:

    c_m  = band_np.band_filter of row r_m = adaptive_array[m] with the one tap row g[b][m]      (the fmaf chain t = 0 .. T-1, in order)
    out  = s_n,  s_0 = 0.0f,  s_{m+1} = s_m + c_m                                               (a float32 NumPy add over m, in order)

and `miso_pad`, the whole-sample delay-and-sum the delta-tap case must reproduce, written directly.

Also the two-source scene the null-steering tests share: band-limited noise sources on the 8 x 8 array, delayed per microphone by an
FFT phase, in float64."""
import numpy as np

import band_np


def filter_sum(x, mics, taps, hop=0, prev=None):
    """x float32 [F, m_total, N]; mics int [n] rows; taps float32 [B, n, T]; hop (0: independent windows); prev float32 [m_total, N]
    or None -> float32 [F, B, N]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    B, n, T = taps.shape
    F, m_total, N = x.shape
    assert len(mics) == n
    s = np.zeros((B, F, N), dtype=np.float32)
    for m in range(n):                                   # in this order: the sum of every output
        r = int(mics[m])
        p = None if prev is None else np.asarray(prev, dtype=np.float32)[r:r + 1]
        c = band_np.band_filter(x[:, r:r + 1, :], taps[:, m, :], hop, p)[:, :, 0, :]      # [B, F, N]: every beam's FIR on this row
        s = s + c
        assert s.dtype == np.float32
    return np.ascontiguousarray(s.transpose(1, 0, 2))


def delta_taps(delays, T):
    """delays int [B, n] -> float32 [B, n, T] with g[b][m][t] = (t == delays[b][m])."""
    delays = np.asarray(delays)
    assert delays.min() >= 0 and delays.max() < T
    g = np.zeros(delays.shape + (T,), dtype=np.float32)
    np.put_along_axis(g, delays[..., None], 1.0, axis=2)
    return g


def miso_pad(x, mics, delays):
    """The reference's whole-sample delay-and-sum on one window: x float32 [m_total, N], delays int [n] -> float32 [N]:
    out starts at 0.0f, and for m = 0 .. n-1 in order out[p_m + i] += x[r_m][i]."""
    x = np.asarray(x, dtype=np.float32)
    N = x.shape[1]
    out = np.zeros(N, dtype=np.float32)
    for m, r in enumerate(mics):
        p = int(delays[m])
        out[p:] += x[int(r), :N - p]
    return out


# ------------------------------------------------------------------ the two-source scene

GRID = (41, 23)                     # MAX_RES_X x MAX_RES_Y
LOOK, INTERFERER, NEAR = (20, 11), (28, 14), (23, 11)
BAND = (3000.0, 8000.0)
FS = 48828.0


def flat(cell):
    return cell[0] * GRID[1] + cell[1]


def band_noise(rng, L, band=BAND, fs=FS):
    """One period (L samples) of periodic gaussian noise limited to the band, as its rfft spectrum, unit RMS."""
    S = np.fft.rfft(rng.standard_normal(L))
    f = np.arange(S.size) * fs / L
    S[(f < band[0]) | (f > band[1])] = 0.0
    S /= np.sqrt(np.mean(np.fft.irfft(S, n=L) ** 2))
    return S


def at_microphones(S, tau_row, L):
    """The source with spectrum S as the microphones hear it, float64 [M, L]: microphone m LEADS by tau_row[m] samples (an FFT phase)."""
    w = 2.0 * np.pi * np.arange(S.size) / L
    return np.fft.irfft(S[None, :] * np.exp(1j * w[None, :] * np.asarray(tau_row)[:, None]), n=L, axis=1)


def beam_f64(x, g):
    """Filter-and-sum of periodic microphone signals x [M, L] with taps g [M, T] in float64 (circular: no edges), [L]."""
    L = x.shape[1]
    G = np.fft.rfft(np.asarray(g, dtype=np.float64), n=L, axis=1)
    return np.fft.irfft(np.sum(np.fft.rfft(x, axis=1) * G, axis=0), n=L)


def db(power_ratio):
    return 10.0 * np.log10(power_ratio)
