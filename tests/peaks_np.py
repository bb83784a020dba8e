"""NumPy restatement of bf_peaks_device (include/beamformer_hip.h): the K loudest separated sources of every map.

The reference has no counterpart, so this module IS the definition the kernels are pinned to, written twice:
  candidates        vectorised over the (2r+1)^2 shifts of the window (what the GPU tests compare with)
  candidates_naive  the definition read aloud, a double loop per entry (what test_peaks_host.py compares `candidates` with)
Everything is comparisons and one float32 multiplication, so the GPU results must be equal, not close."""
import numpy as np


def candidates(img, radius):
    """img float32 [rows, cols] -> bool [rows, cols]: finite entries that no other finite entry of their window comes before in the
    order (value descending, flat index ascending)."""
    img = np.asarray(img, dtype=np.float32)
    rows, cols = img.shape
    fin = np.isfinite(img)
    rx, ry = min(radius, rows - 1), min(radius, cols - 1)
    if rx == rows - 1 and ry == cols - 1:
        # every window is the whole grid: only the first entry of the order is left (721^2 shifts of a 361 x 361 map otherwise)
        cand = np.zeros_like(fin)
        if fin.any():
            v = np.where(fin, img, -np.inf).ravel()
            cand.ravel()[int(np.argmax(v))] = True          # np.argmax: the first of equal maxima
        return cand
    cand = fin.copy()
    for dx in range(-rx, rx + 1):
        for dy in range(-ry, ry + 1):
            if dx == 0 and dy == 0:
                continue
            # entries [xs, ys] and their neighbours at (+dx, +dy), both inside the grid
            xs, ys = slice(max(0, -dx), rows - max(0, dx)), slice(max(0, -dy), cols - max(0, dy))
            xn, yn = slice(max(0, -dx) + dx, rows - max(0, dx) + dx), slice(max(0, -dy) + dy, cols - max(0, dy) + dy)
            a, b = img[xs, ys], img[xn, yn]
            lower_index = dx < 0 or (dx == 0 and dy < 0)
            with np.errstate(invalid="ignore"):
                before = fin[xn, yn] & fin[xs, ys] & ((b > a) | ((b == a) & lower_index))
            cand[xs, ys] &= ~before
    return cand


def candidates_naive(img, radius):
    img = np.asarray(img, dtype=np.float32)
    rows, cols = img.shape
    cand = np.zeros((rows, cols), dtype=bool)
    for x in range(rows):
        for y in range(cols):
            if not np.isfinite(img[x, y]):
                continue
            ok = True
            for x2 in range(max(0, x - radius), min(rows, x + radius + 1)):
                for y2 in range(max(0, y - radius), min(cols, y + radius + 1)):
                    if (x2, y2) == (x, y) or not np.isfinite(img[x2, y2]):
                        continue
                    if img[x2, y2] > img[x, y] or (img[x2, y2] == img[x, y] and x2 * cols + y2 < x * cols + y):
                        ok = False
            cand[x, y] = ok
    return cand


def min_chebyshev(cand):
    """Smallest Chebyshev distance between two candidates (None with fewer than two)."""
    pts = np.argwhere(cand)
    if len(pts) < 2:
        return None
    d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)
    d[np.arange(len(pts)), np.arange(len(pts))] = np.iinfo(d.dtype).max
    return int(d.min())


def peaks(power, rows, cols, radius, k, floor_rel, floor_abs, offset_per_dir, cand_fn=candidates):
    """power float32 [F, stride >= rows*cols] -> (offsets int32 [F, k], values float32 [F, k], counts int32 [F, 3])."""
    power = np.asarray(power, dtype=np.float32)
    F, D = power.shape[0], rows * cols
    offsets = np.full((F, k), -1, dtype=np.int32)
    values = np.zeros((F, k), dtype=np.float32)
    counts = np.zeros((F, 3), dtype=np.int32)
    for f in range(F):
        img = power[f, :D].reshape(rows, cols)
        fin = np.isfinite(img)
        counts[f, 2] = D - int(fin.sum())
        if not fin.any():
            continue
        top = np.float32(img[fin].max())
        thr = np.maximum(np.float32(floor_abs), np.float32(np.float32(floor_rel) * top))
        with np.errstate(invalid="ignore"):
            kept = cand_fn(img, radius) & (img >= thr)
        idx = np.flatnonzero(kept.ravel())
        v = img.ravel()[idx]
        order = np.lexsort((idx, -v))               # value descending, then index ascending (0.0 and -0.0 compare equal)
        idx, v = idx[order], v[order]
        n = min(k, idx.size)
        counts[f, 0], counts[f, 1] = n, idx.size
        offsets[f, :n] = idx[:n] * offset_per_dir
        values[f, :n] = v[:n]
    return offsets, values, counts
