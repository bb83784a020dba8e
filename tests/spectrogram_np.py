"""NumPy restatement of bf_spectrogram_device (include/beamformer_hip.h): u = window * x in float32 exactly as defined, everything behind
it in float64; Python ints for the state; and the bound a float32 implementation of the definition has to keep, whatever its transform
algorithm and summation orders are."""
import numpy as np

from stft_np import EPS, windowed


def capacity(length, hop):
    return -(-length // hop)


def advance(s0, L, n_win, hop):
    """(count, s0') of a call on L samples from a valid state."""
    count = (L - n_win - s0) // hop + 1 if s0 + n_win <= L else 0
    return count, s0 + count * hop - L


def next_history(hist, x, L):
    """The last n_win - 1 samples of hist || x[:, :L]."""
    H = hist.shape[1]
    joined = np.concatenate([hist, x[:, :L]], axis=1)
    return np.ascontiguousarray(joined[:, joined.shape[1] - H:])


def framed(x, hist, s0, L, n_win, hop, shift=0):
    """u's samples: float32 [rows, count, n_win] of hist || x[:, :L], frame j from s0 + j hop (+ shift: a deliberately wrong start)."""
    H = n_win - 1
    count, _ = advance(s0, L, n_win, hop)
    stream = np.concatenate([hist, x[:, :L]], axis=1)
    idx = (H + s0 + shift + hop * np.arange(count))[:, None] + np.arange(n_win)[None, :]
    idx = np.clip(idx, 0, max(stream.shape[1] - 1, 0))                   # (only a shifted start can leave the stream)
    return stream[:, idx] if count else np.zeros((x.shape[0], 0, n_win), np.float32)


def spectrum(u, n_fft):
    """X_k, k = 0 .. n_fft / 2, of u zero-padded to n_fft, in float64."""
    return np.fft.rfft(u.astype(np.float64), n=n_fft, axis=-1)


def _weights(bank, support, n_bins):
    """float64 [n_bands, n_bins]: the bank inside each band's support, zero outside it (weights outside are not read); widths hi - lo."""
    if bank is None:
        return np.eye(n_bins), np.ones(n_bins, dtype=np.int64)
    W = bank.astype(np.float64).copy()
    width = np.full(W.shape[0], n_bins, dtype=np.int64)
    if support is not None:
        k = np.arange(n_bins)[None, :]
        lo, hi = np.clip(support[:, :1], 0, n_bins), np.clip(support[:, 1:], 0, n_bins)
        W[~((k >= lo) & (k < hi))] = 0.0
        width = np.maximum(hi - lo, 0)[:, 0]
    return W, width


def spectrogram_bound(u, X, bank, support):
    """(E, dE), float64 [.., n_bands].  With A = sum_t |u[t]|, a component of X_k summed in float32 in any order is within
        g = 2 (n_win + 2) 2^-24 A
    of its exact value: the plain accumulation bound of n_win terms of magnitude <= |u[t]| (each a product with a twiddle that is itself
    rounded: the + 2), doubled for an unspecified order; an FFT's log2 n error sits inside it.  Then
        dP_k = 2 (|re| + |im|) g + 2 g^2 + 3 * 2^-24 P_k                        two squares and a sum
        dE_b = sum_k W dP_k + 2 (hi_b - lo_b + 1) 2^-24 sum_k W P_k             hi - lo products and sums, doubled"""
    n_win = u.shape[-1]
    A = np.abs(u.astype(np.float64)).sum(axis=-1)[..., None]
    g = 2.0 * (n_win + 2) * EPS * A
    P = X.real ** 2 + X.imag ** 2
    dP = 2.0 * (np.abs(X.real) + np.abs(X.imag)) * g + 2.0 * g * g + 3.0 * EPS * P
    W, width = _weights(bank, support, X.shape[-1])
    Wa = np.abs(W)
    E = P @ W.T
    dE = dP @ Wa.T + 2.0 * (width + 1)[None, None, :] * EPS * (P @ Wa.T)
    return E, dE


def to_output(E, scale, floor):
    """out = E for scale == 0, else scale * log10(E < floor ? floor : E) (a NaN stays)."""
    if scale == 0:
        return E
    with np.errstate(invalid="ignore"):
        return scale * np.log10(np.where(E < floor, floor, E))


def _ulps(v, n):
    return n * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def output_interval(E, dE, scale, floor):
    """[lo, hi] a float32 output must lie in: E +- dE for the linear output; for the log output the images of E - dE and E + dE, widened
    by 4 float32 ulps for log10f."""
    if scale == 0:
        return E - dE, E + dE
    a, b = to_output(E - dE, scale, floor), to_output(E + dE, scale, floor)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo - _ulps(lo, 4), hi + _ulps(hi, 4)


def spectrogram(x, hist, s0, window, n_fft, hop, bank=None, support=None, scale=0.0, floor=1e-10, L=None):
    """One call on x float32 [rows, len] (L of them there) behind hist float32 [rows, n_win - 1] from state s0 ->
    dict(count, status, s0, hist, cap, out float64 [rows, cap, n_bands], lo, hi: the interval of output_interval).  Slots behind count
    are 0 with lo = hi = 0."""
    rows, length = x.shape
    n_win = window.shape[0]
    L = length if L is None else min(max(int(L), 0), length)
    cap = capacity(length, hop)
    n_bands = n_fft // 2 + 1 if bank is None else bank.shape[0]
    out, lo, hi = (np.zeros((rows, cap, n_bands)) for _ in range(3))
    if s0 < -(n_win - 1):
        return dict(count=0, status=1, s0=s0, hist=hist.copy(), cap=cap, out=out, lo=lo, hi=hi)
    count, s1 = advance(s0, L, n_win, hop)
    if count:
        u = windowed(framed(x, hist, s0, L, n_win, hop), window)
        with np.errstate(invalid="ignore", over="ignore"):
            E, dE = spectrogram_bound(u, spectrum(u, n_fft), bank, support)
            out[:, :count] = to_output(E, scale, floor)
            lo[:, :count], hi[:, :count] = output_interval(E, dE, scale, floor)
    return dict(count=count, status=0, s0=s1, hist=next_history(hist, x, L), cap=cap, out=out, lo=lo, hi=hi)


def inside(got, want):
    """'' if every value of got (float32 [rows, cap, n_bands]) lies in want's interval (NaN where the restatement has NaN), else a
    description of the worst miss."""
    g = got.astype(np.float64)
    nan_w = np.isnan(want["lo"]) | np.isnan(want["hi"])
    bad = np.where(nan_w, ~np.isnan(g), ~((g >= want["lo"]) & (g <= want["hi"])))
    if not bad.any():
        return ""
    i = tuple(np.argwhere(bad)[0])
    return "%d of %d outside, first at %s: got %r, interval [%r, %r]" % (bad.sum(), bad.size, i, g[i], want["lo"][i], want["hi"][i])


def worst_ratio(got, want, where=None):
    """max |got - out| / (the interval's reach on that side of out) over the finite, non-degenerate slots (of `where`): how much of the
    bound is used."""
    g = got.astype(np.float64)
    err = g - want["out"]
    reach = np.where(err >= 0, want["hi"] - want["out"], want["out"] - want["lo"])
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(g) & np.isfinite(reach) & (reach > 0) & (True if where is None else where)
    return float(np.max(np.abs(err)[ok] / reach[ok])) if ok.any() else 0.0
