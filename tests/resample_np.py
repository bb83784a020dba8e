"""bf_resample_device's definition (include/beamformer_hip.h) restated in NumPy.

The taps run t = 0 .. T-1 in order over all outputs of a call, every step one single-rounding float32 fused multiply-add through
band_np._load()'s real fmaf (its step takes ONE coefficient and an array of outputs, so the outputs are taken phase by phase: those
that share p_k share h[p_k][t]).  The state arithmetic is in Python ints, the outputs are enumerated by the definition's loop
`while i_k < S` (closed_form is the header's formula, for the tests to compare), the PCM is formed with np.rint."""
import numpy as np

import band_np


def stream(x, hop, prev, T):
    """x float32 [F, R, n] (the columns past n of a strided buffer already cut), prev float32 [R, n] or None -> float32 [R, T - 1 + S]:
    the call's stream of every row behind its T - 1 samples of history, and S."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    F, R, n = x.shape
    ln = hop if hop > 0 else n
    assert 0 <= hop <= n and T - 1 <= ln
    S = F * ln
    ext = np.zeros((R, T - 1 + S), dtype=np.float32)
    ext[:, T - 1:] = x[:, :, n - ln:].transpose(1, 0, 2).reshape(R, S)
    if prev is not None and T > 1:
        prev = np.asarray(prev, dtype=np.float32)
        ext[:, :T - 1] = prev[:, prev.shape[1] - (T - 1):]              # the end of the window before
    return ext, S


def positions(o, phi, S, L, M):
    """The definition's loop: [(i_k, p_k)] for k = 0, 1, .. while i_k < S, in Python ints."""
    out, k = [], 0
    while True:
        a = phi + k * M
        i = o + a // L
        if i >= S:
            return out
        out.append((i, a % L))
        k += 1


def closed_form(o, phi, S, L, M):
    """The header's formulas -> (count, o', phi')."""
    count = -(-((S - o) * L - phi) // M) if o < S else 0
    A = phi + count * M
    return count, o + A // L - S, A % L


def capacity(S, L, M):
    return -(-(S * L) // M)


def to_pcm(v):
    """float32 [...] -> (int16 [...], clipped bool [...]): clamp(rint(v * 32768)), ties to even, a NaN gives 0 and is clipped."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(v * np.float32(32768.0))
    nan = np.isnan(r)
    clipped = nan | (r > 32767.0) | (r < -32768.0)
    q = np.clip(np.where(nan, np.float32(0.0), r), -32768.0, 32767.0).astype(np.int16)
    return q, clipped


def resample(x, taps, up, down, state=(0, 0), hop=0, prev=None, gain=1.0):
    """x float32 [F, R, n], taps float32 [up, T], state (o, phi) -> dict: y float32 [R, cap] (gain applied, zeros from count on), pcm int16
    [cap, R], clipped int [R], count, status, state (o', phi'), cap."""
    step = band_np._load()
    h = np.ascontiguousarray(taps, dtype=np.float32)
    L, M = int(up), int(down)
    assert h.shape[0] == L
    T = h.shape[1]
    ext, S = stream(x, hop, prev, T)
    R = ext.shape[0]
    cap = capacity(S, L, M)
    o, phi = int(state[0]), int(state[1])
    y = np.zeros((R, cap), dtype=np.float32)
    if o < 0 or not 0 <= phi < L:
        return dict(y=y, pcm=np.zeros((cap, R), np.int16), clipped=np.zeros(R, np.int64), count=0, status=1, state=(o, phi), cap=cap)
    pos = positions(o, phi, S, L, M)
    count = len(pos)
    if count:
        ik = np.array([i for i, _ in pos], dtype=np.int64) + (T - 1)        # index of x[i_k] in ext
        pk = np.array([p for _, p in pos], dtype=np.int64)
        for p in np.unique(pk):
            ks = np.nonzero(pk == p)[0]
            acc = np.zeros((R, ks.size), dtype=np.float32)
            for t in range(T):                  # in this order: the chain of every output
                step(h[p, t], ext[:, ik[ks] - t], acc)
            y[:, ks] = acc
        with np.errstate(over="ignore", invalid="ignore"):
            y[:, :count] = y[:, :count] * np.float32(gain)
    pcm, clipped = to_pcm(y)
    A = phi + count * M
    return dict(y=y, pcm=np.ascontiguousarray(pcm.T), clipped=clipped.sum(axis=1).astype(np.int64), count=count, status=0,
                state=(o + A // L - S, A % L), cap=cap)
