"""NumPy restatement of the reference's heat-map post-processing.  TEST INFRASTRUCTURE ONLY.

Follows PC/src/visual.py: calculate_heatmap :143-188, find_power_center :295-322, the blends of Viewer.loop :450-452.

Pinning status: the NumPy arithmetic of calculate_heatmap (clip, log10, normalise, threshold, power, LUT index, flip) is
restated line by line and the jet table is a committed fixture (tests/golden/jet_lut.npy, generated from matplotlib as
the reference does).  The three OpenCV calls (cv2.resize INTER_LINEAR, cv2.addWeighted, cv2.GaussianBlur) cannot be
executed here -- `opencv-python` is not installed and the reference does not pin its version (PC/requirements.txt:2) --
so they are restated from OpenCV's published algorithms: PARITY UNPINNED for those three."""
import os

import numpy as np

_LUT = None


def jet_lut():
    global _LUT
    if _LUT is None:
        _LUT = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "jet_lut.npy"))
    return _LUT


def small_heatmap(image, threshold=1e-7, amount=0.5, exponent=5):
    """visual.py:143-185 up to (not including) cv2.resize.  image float32 [X, Y] -> (uint8 [Y, X, 3], should_overlay)."""
    X, Y = image.shape
    small = np.zeros((Y, X, 3), dtype=np.uint8)
    colors = jet_lut()
    should = False
    safe = np.clip(image, 1e-12, None)
    if np.max(image) > threshold:
        img = np.log10(safe)
        img -= np.log10(np.min(safe))
        img /= np.max(img)
        should = True
        for x in range(X):
            for y in range(Y):
                level = img[x, y]
                if level >= amount:
                    level -= amount
                    level /= amount
                    small[Y - 1 - y, X - 1 - x] = colors[int(255 * level ** exponent)]
    return small, should


EPS32 = float(np.finfo(np.float32).eps)
CLIP = float(np.float32(1e-12))      # what np.clip(float32 image, 1e-12, None) clips to


def small_heatmap_f32(image, threshold=1e-7, amount=0.5, exponent=5):
    """small_heatmap with the two Python loops replaced by whole-array float32 operations (same values, same order)."""
    image = np.asarray(image, dtype=np.float32)
    X, Y = image.shape
    small = np.zeros((Y, X, 3), dtype=np.uint8)
    safe = np.clip(image, 1e-12, None)
    if not np.max(image) > threshold:
        return small, False
    with np.errstate(all="ignore"):
        img = np.log10(safe)
        img -= np.log10(np.min(safe))
        img /= np.max(img)
        on = img >= amount
        level = np.where(on, img, np.float32(amount))
        level = level - np.float32(amount)
        level = level / np.float32(amount)
        t = np.float32(255) * level ** exponent
    color = jet_lut()[np.minimum(t.astype(np.int64), 255)]     # (amount < 0.5 takes levels past 1: the reference's table lookup raises
    color[~on] = 0                                              # there, the kernel stays on the last entry)
    return np.ascontiguousarray(color[::-1, ::-1].transpose(1, 0, 2)), True


def heat_levels_f64(image, amount=0.5, exponent=5):
    """visual.py:159-181 in float64 on the float32 map: per pixel [X, Y] the level l and the index value
    t = 255 * ((l - amount) / amount) ** exponent (NaN where the reference's arithmetic gives NaN)."""
    s = np.clip(np.asarray(image, dtype=np.float64), CLIP, None)
    with np.errstate(all="ignore"):
        l = np.log10(s)
        l = l - np.log10(np.min(s))
        l = l / np.max(l)
        t = 255.0 * ((l - amount) / amount) ** exponent
    return l, t


def heat_units(image, amount=0.5, exponent=5):
    """What one float32 rounding is worth at each decision of the colouring (the error model of tests/test_postproc_f64.py).

    log10 of a float32 s carries eps32 * |log10 s|; the level l = (log10 s - log10 min) / (log10 max - log10 min) therefore
    level_unit = eps32 * max|log10| / (log10 max - log10 min): flat maps (a small range) amplify it.  The index value
    t = 255 u^e, u = (l - amount) / amount, moves by 255 e u^(e-1) / amount per unit of l and has its own rounding:
    index_unit = 255 eps32 (e u^(e-1) max|log10| / (range * amount) + u^e), per pixel.  -> (level_unit, index_unit [X, Y])."""
    s = np.clip(np.asarray(image, dtype=np.float64), CLIP, None)
    with np.errstate(all="ignore"):
        lo, hi = np.log10(np.min(s)), np.log10(np.max(s))
        amp = max(abs(lo), abs(hi)) / (hi - lo)
        l, _ = heat_levels_f64(image, amount, exponent)
        u = (l - amount) / amount
        iu = 255.0 * EPS32 * (exponent * u ** (exponent - 1.0) * amp / amount + u ** exponent)
    return EPS32 * amp, np.where(u > 0, iu, 0.0)


def check_small(got, image, threshold=1e-7, amount=0.5, exponent=5, mult=0.0):
    """A small colour image uint8 [Y, X, 3] against visual.py:143-185 executed in float64.

    A pixel is ambiguous when |l - amount| <= mult * level_unit (black, or the colour of the painted side), or when it is
    painted, not the peak (l = x / x = 1, t = 255 in any precision), t >= 1 - band and |t - rint(t)| <= band = mult * index_unit
    (the colour of either side of that step).  Every other pixel must equal lut[floor(t)], black below `amount`.
    -> (expected flag, wrong [X, Y] bool, ambiguous [X, Y] bool, dist [X, Y]: distance to the nearest decision, in units)."""
    image = np.asarray(image, dtype=np.float32)
    X, Y = image.shape
    lut = jet_lut()
    got_xy = np.asarray(got).transpose(1, 0, 2)[::-1, ::-1]
    with np.errstate(all="ignore"):
        flag = bool(np.max(image.astype(np.float64)) > float(np.float32(threshold)))
    if not flag:
        return False, got_xy.any(axis=-1), np.zeros((X, Y), dtype=bool), np.full((X, Y), np.inf)
    l, t = heat_levels_f64(image, amount, exponent)
    lu, iu = heat_units(image, amount, exponent)
    with np.errstate(all="ignore"):
        on = l >= amount
        tt = np.where(on, np.nan_to_num(t), 0.0)
        step = np.rint(tt)
        d_level = np.nan_to_num(np.abs(l - amount) / lu, nan=np.inf)
        d_index = np.where(on & (l != 1.0) & (iu > 0) & (step <= 255), np.abs(tt - step) / iu, np.inf)      # (past 255 every index is the last entry)
        amb_level = d_level <= mult
        amb_index = (d_index <= mult) & (tt >= 1.0 - mult * iu)
    idx = lambda v: np.clip(v, 0, 255).astype(np.int64)
    want = lut[idx(np.floor(tt))]
    want[~on] = 0
    eq = lambda c: (got_xy == c).all(axis=-1)
    ok = eq(want)
    ok |= amb_index & (eq(lut[idx(step - 1)]) | eq(lut[idx(step)]))
    ok |= amb_level & (eq(np.zeros(3, np.uint8)) | eq(lut[0]))
    dist = np.minimum(d_level, np.where(tt >= 0.5, d_index, np.inf))
    return True, ~ok, amb_level | amb_index, dist


def _reflect101(i, n):
    """cv2.BORDER_REFLECT_101 index map (gfedcb|abcdefgh|gfedcba), any overhang."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def find_power_center_f64(image):
    """find_power_center in float64 -> (center_x, center_y, gap, n_mask): gap = the smallest relative distance of a smoothed
    pixel from the 95 % line (a map with a small gap is a bad test input: the mask is a step function), n_mask = pixels in the mask."""
    img = np.clip(np.asarray(image, dtype=np.float64), CLIP, None)
    g = np.exp(-(np.arange(5) - 2.0) ** 2 / 2.0)
    g /= g.sum()
    rows, cols = img.shape
    ci, ri = _reflect101(np.arange(-2, cols + 2), cols), _reflect101(np.arange(-2, rows + 2), rows)
    tmp = sum(g[k] * img[:, ci[k:k + cols]] for k in range(5))
    sm = sum(g[k] * tmp[ri[k:k + rows], :] for k in range(5))
    thr = sm.max() * 0.95
    mask = sm >= thr
    yi, xi = np.indices(sm.shape)
    w = sm ** 3 * mask
    return float((xi * w).sum() / w.sum()), float((yi * w).sum() / w.sum()), float(np.abs(sm / thr - 1.0).min()), int(mask.sum())


def letterbox_u8(src, out_h, out_w, new_h, new_w, top, left, value):
    """The detector's letterbox: cv2.resize(INTER_LINEAR) to new_w x new_h (skipped for equal shapes) inside a canvas of `value`."""
    out = np.full((out_h, out_w, 3), value, dtype=np.uint8)
    out[top:top + new_h, left:left + new_w] = src if src.shape[:2] == (new_h, new_w) else resize_linear_u8(src, new_w, new_h)
    return out


def resize_linear_u8(src, out_w, out_h):
    """cv2.resize(src, (out_w, out_h), interpolation=cv2.INTER_LINEAR) for uint8 [h, w, c] (OpenCV's fixed-point path:
    half-pixel centres, weights rounded to 11 bits each, ((b0*(r0>>4))>>16 + (b1*(r1>>4))>>16 + 2) >> 2)."""
    sh, sw = src.shape[:2]

    def axis(dsz, ssz):
        o = np.arange(dsz)
        f = ((o + 0.5) * (float(ssz) / dsz) - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        f = f - i.astype(np.float32)
        lo = i < 0
        i[lo] = 0; f[lo] = 0
        hi = i >= ssz - 1
        i[hi] = ssz - 1; f[hi] = 0
        i1 = np.where(hi, i, i + 1)
        w0 = np.rint((np.float32(1.0) - f) * np.float32(2048)).astype(np.int64)
        w1 = np.rint(f * np.float32(2048)).astype(np.int64)
        return i, i1, w0, w1

    x0, x1, wx0, wx1 = axis(out_w, sw)
    y0, y1, wy0, wy1 = axis(out_h, sh)
    s = src.astype(np.int64)
    rows = s[:, x0] * wx0[None, :, None] + s[:, x1] * wx1[None, :, None]           # [sh, out_w, c]
    r0, r1 = rows[y0] >> 4, rows[y1] >> 4
    out = (((wy0[:, None, None] * r0) >> 16) + ((wy1[:, None, None] * r1) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def add_weighted_u8(a, alpha, b, beta):
    """cv2.addWeighted(a, alpha, b, beta, 0) for uint8: float32 arithmetic, round half to even, saturate."""
    v = np.float32(alpha) * a.astype(np.float32) + np.float32(beta) * b.astype(np.float32)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def calculate_heatmap(image, window=(1920, 1080), **kw):
    """visual.py:143-188 -> (heatmap uint8 [H, W, 3], should_overlay)."""
    small, should = small_heatmap(image, **kw)
    return resize_linear_u8(small, window[0], window[1]), should


def find_power_center(image):
    """visual.py:295-322 on clip(image, 1e-12): 5x5 Gaussian sigma 1 (BORDER_REFLECT_101), >= 95 % mask, cube weights."""
    img = np.clip(image, 1e-12, None).astype(np.float32)
    g = np.exp(-(np.arange(5) - 2.0) ** 2 / 2.0)
    g = (g / g.sum()).astype(np.float32)
    pad = np.pad(img, 2, mode="reflect")
    rows, cols = img.shape
    tmp = np.zeros((rows + 4, cols), dtype=np.float32)
    for k in range(5):
        tmp += g[k] * pad[:, k:k + cols]
    sm = np.zeros_like(img)
    for k in range(5):
        sm += g[k] * tmp[k:k + rows, :]
    mask = sm >= sm.max() * np.float32(0.95)
    yi, xi = np.indices(sm.shape)
    w = (sm ** 3) * mask
    tw = np.sum(w.astype(np.float64))
    return float(np.sum(xi * w.astype(np.float64)) / tw), float(np.sum(yi * w.astype(np.float64)) / tw)
