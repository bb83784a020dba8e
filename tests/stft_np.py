"""What the float64 restatements of the windowed-transform stages (whiten_np.py, enhance_np.py, spectrogram_np.py) share: the one float32
step of their definitions, the constants of the radix-2 rounding model (csrc/lds_fft.h states it on the device side) and the weights
of a two-sided sum over half-spectrum bins."""
import numpy as np

EPS = 2.0 ** -24            # the unit roundoff of float32
# Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Theorem 24.2, for twiddles rounded once from double: eta = 5 sqrt 2 u to
# first order, 1 % for the second-order terms (whiten_np.py derives it)
ETA = 5.0 * np.sqrt(2.0) * 1.01


def windowed(x, window):
    """u[t] = window[t] * x[t] along the last axis: one float32 multiply (u = x without a window)."""
    x = np.asarray(x, dtype=np.float32)
    return x if window is None else (x * np.asarray(window, dtype=np.float32)).astype(np.float32)


def two_sided(n):
    """Weights of the half-spectrum bins in a sum over all n bins: 1 for bins 0 and n / 2, 2 for the others."""
    w = np.full(n // 2 + 1, 2.0)
    w[0] = w[-1] = 1.0
    return w
