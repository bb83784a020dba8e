"""What the float64 restatements of the windowed-transform stages (whiten_np.py, enhance_np.py, spectrogram_np.py) share: the one float32
step of their definitions, the constants of the radix-2 rounding model (csrc/lds_fft.h states it on the device side), the weights
of a two-sided sum over half-spectrum bins, and the integers of the window stream and the frame grid that enhance_np.py and
postfilter_np.py walk (csrc/stream_grid.h states them on the device side)."""
import numpy as np

EPS = 2.0 ** -24            # the unit roundoff of float32
# Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Theorem 24.2, for twiddles rounded once from double: eta = 5 sqrt 2 u to
# first order, 1 % for the second-order terms (whiten_np.py derives it)
ETA = 5.0 * np.sqrt(2.0) * 1.01


def windowed(x, window):
    """u[t] = window[t] * x[t] along the last axis: one float32 multiply (u = x without a window)."""
    x = np.asarray(x, dtype=np.float32)
    return x if window is None else (x * np.asarray(window, dtype=np.float32)).astype(np.float32)


def stream(windows, n, hop, rows=None):
    """windows float32 [F, R, stride >= n] -> x float32 [R, S]: the last len = hop or n samples of every window (of the rows `rows`)."""
    length = hop if hop > 0 else n
    w = np.asarray(windows, dtype=np.float32)
    pick = slice(None) if rows is None else np.asarray(rows)
    return np.ascontiguousarray(np.concatenate([w[f][pick, n - length:n] for f in range(w.shape[0])], axis=1))


def new_history(hist, x):
    """The last H samples of hist [R, H] || x [R, S]."""
    H = hist.shape[1]
    return np.ascontiguousarray(np.concatenate([hist, x], axis=1)[:, x.shape[1]:x.shape[1] + H]) if H else hist.copy()


def advance(c, S, hop_s):
    """(count, c', cap) of a call on S samples with c samples since the last frame end."""
    return (c + S) // hop_s, (c + S) % hop_s, (hop_s - 1 + S) // hop_s


def frame_starts(c, S, n_fft, hop_s, lag=0):
    """Start (relative to x[0]) of every frame the call completes: frame i ends at (i + 1) hop_s - c - 1 - lag."""
    return [(i + 1) * hop_s - c - lag - n_fft for i in range((c + S) // hop_s)]


def analysis(x, hist, c, window, hop_s, lag=0):
    """-> (u float32 [R, count, n_fft], X complex128 [R, count, n_fft / 2 + 1], starts): the call's frames of hist || x, H = n_fft - 1 + lag."""
    n_fft = window.shape[0]
    H = n_fft - 1 + lag
    ext = np.concatenate([np.asarray(hist, np.float32), np.asarray(x, np.float32)], axis=1)
    starts = frame_starts(c, x.shape[1], n_fft, hop_s, lag)
    fr = np.stack([ext[:, H + s:H + s + n_fft] for s in starts], axis=1) if starts else np.zeros((x.shape[0], 0, n_fft), np.float32)
    u = windowed(fr, window)
    return u, np.fft.rfft(u.astype(np.float64), axis=-1), starts


def frame_grid_ok(samples, n_fft, hop_s):
    """Whether a call on `samples` stream samples has a workspace on the grid (n_fft, hop_s)."""
    return 1 <= samples <= (2 ** 31 - 1) // 2 and 32 <= n_fft <= 4096 and not n_fft & (n_fft - 1) and hop_s >= 1 and not n_fft % hop_s and n_fft // hop_s <= 8


def two_sided(n):
    """Weights of the half-spectrum bins in a sum over all n bins: 1 for bins 0 and n / 2, 2 for the others."""
    w = np.full(n // 2 + 1, 2.0)
    w[0] = w[-1] = 1.0
    return w
