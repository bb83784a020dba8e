"""NumPy restatement of bf_fuse_boxes_device (include/beamformer_hip.h): a plain-loop float32 reading of the definition, one
operation per line where the rounding matters.  Every float is an np.float32 scalar, so each +, -, * rounds once to float32 as the
kernel's does (the build contracts nothing); everything after the conversion to int is Python integer arithmetic.

  fuse(power, rows, cols, per, boxes, box_counts, img_w, img_h, conf, src_offsets, fast)
      -> (peak_offsets [F, B], peak_power [F, B], center_offsets [F, B], rects [F, B, 4], src_box [F, n_src] or None, counts [F, 3])
  cell(u, cells, img)        the small-image index of display pixel u
  axis(a, b, img, cells)     the grid range of one axis of a box, or None
  pixel_set(x0, cells, img)  the display pixels the definition assigns to grid index x0

No input is modified; every returned array is new."""
import numpy as np

f32 = np.float32
MAX_SOURCES = 64
STAGE_MAX = 15360                     # BF_FUSE_STAGE_MAX: maps up to this many directions are staged into LDS
INT_SAFE = f32(2147483520.0)          # the largest float32 below 2^31


def cell(u, cells, img):
    return ((2 * u + 1) * cells) // (2 * img)


def _pixel(u, n):
    """(int)u for a float32 u in [0, float32(n - 1)], clamped to n - 1 (float32(n - 1) rounds up above 2^24)."""
    return min(int(min(u, INT_SAFE)), n - 1)


def axis(a, b, img, cells):
    a, b = f32(a), f32(b)
    if np.isnan(a) or np.isnan(b):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        ua = a - f32(0.5)
        ua = np.ceil(ua)
        ub = b - f32(0.5)
        ub = np.floor(ub)
    ua = ua if ua > 0 else f32(0)                     # fmaxf(ua, 0)  (ua is not NaN here)
    top = f32(img - 1)
    ub = ub if ub < top else top                      # fminf(ub, img - 1)
    if not ua <= ub:
        return None
    lo = cells - 1 - cell(_pixel(ub, img), cells, img)
    hi = cells - 1 - cell(_pixel(ua, img), cells, img)
    return lo, hi


def mid(a, b, img, cells):
    """The grid index under the midpoint of [a, b], or None."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = f32(a) + f32(b)
        s = s * f32(0.5)
        um = np.floor(s)
    if not (um >= 0 and um <= f32(img - 1)):
        return None
    return cells - 1 - cell(_pixel(um, img), cells, img)


def pixel_set(x0, cells, img):
    """Display pixels u in [0, img) with cells - 1 - cell(u) == x0."""
    return [u for u in range(img) if cells - 1 - cell(u, cells, img) == x0]


def _code(v):
    """bf_peaks_device's order as an integer: larger comes first; None for a non-finite value; -0.0 and 0.0 share a code."""
    b = int(np.asarray(v, dtype=np.float32).view(np.uint32))
    if (b & 0x7f800000) == 0x7f800000:
        return None
    if b == 0x80000000:
        b = 0
    return (~b & 0xffffffff) if b & 0x80000000 else (b | 0x80000000)


def is_source(o, per, D):
    return o >= 0 and o % per == 0 and o // per < D


def _first_plain(m, finite, cols, xa, xb, ya, yb):
    """The finite cell of the footprint that comes first in bf_peaks_device's order, or -1: the definition read aloud."""
    best, best_d = None, -1
    for x in range(xa, xb + 1):
        for y in range(ya, yb + 1):                    # ascending d: only a larger code replaces the best so far
            d = x * cols + y
            if not finite[d]:
                continue
            c = _code(m[d])
            if best is None or c > best:
                best, best_d = c, d
    return best_d


def _codes(m):
    """_code of every entry at once, -1 for a non-finite one."""
    bits = m.view(np.uint32).astype(np.int64)
    finite = (bits & 0x7f800000) != 0x7f800000
    bits = np.where(bits == 0x80000000, 0, bits)
    return np.where(finite, np.where(bits & 0x80000000, ~bits & 0xffffffff, bits | 0x80000000), -1)


def _first_fast(codes, cols, xa, xb, ya, yb):
    """_first_plain by whole-array operations: np.argmax takes the first maximum in row-major order, the lowest d."""
    win = codes.reshape(-1, cols)[xa:xb + 1, ya:yb + 1]
    i = int(np.argmax(win))
    if win.flat[i] < 0:
        return -1
    return (xa + i // win.shape[1]) * cols + ya + i % win.shape[1]


def fuse(power, rows, cols, per, boxes, box_counts, img_w, img_h, conf, src_offsets=None, fast=False):
    """fast: the cell loop of a footprint as whole-array operations (the large cases of the GPU tests; test_fuse_host.py compares
    the two forms)."""
    power = np.asarray(power, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32)
    F, B = boxes.shape[:2]
    D = rows * cols
    conf = f32(conf)
    n_src = 0 if src_offsets is None else np.asarray(src_offsets).shape[1]
    assert 0 <= n_src <= MAX_SOURCES and power.shape[0] == F and power.shape[1] >= D
    peak = np.full((F, B), -1, dtype=np.int32)
    value = np.zeros((F, B), dtype=np.float32)
    center = np.full((F, B), -1, dtype=np.int32)
    rects = np.full((F, B, 4), -1, dtype=np.int32)
    src_box = None if src_offsets is None else np.full((F, n_src), -1, dtype=np.int32)
    counts = np.zeros((F, 3), dtype=np.int32)
    for f in range(F):
        nb = B if box_counts is None else min(max(int(box_counts[f]), 0), B)
        m = np.ascontiguousarray(power[f, :D])
        finite = np.isfinite(m)
        codes = _codes(m) if fast else None
        for b in range(nb):
            x1, y1, x2, y2, score = boxes[f, b, :5]
            if not score >= conf:                      # (a NaN score is not a box)
                continue
            counts[f, 0] += 1
            cx, cy = mid(x1, x2, img_w, rows), mid(y1, y2, img_h, cols)
            if cx is not None and cy is not None:
                center[f, b] = (cx * cols + cy) * per
            ax, ay = axis(x1, x2, img_w, rows), axis(y1, y2, img_h, cols)
            if ax is None or ay is None:
                continue
            rects[f, b] = (ax[0], ax[1], ay[0], ay[1])
            d = _first_fast(codes, cols, ax[0], ax[1], ay[0], ay[1]) if fast else _first_plain(m, finite, cols, ax[0], ax[1], ay[0], ay[1])
            if d >= 0:
                peak[f, b] = d * per
                value[f, b] = m[d]
                counts[f, 1] += 1
        for s in range(n_src):
            o = int(src_offsets[f][s])
            if not is_source(o, per, D):
                continue
            d = o // per
            sx, sy = d // cols, d % cols
            for b in range(nb):
                xa, xb, ya, yb = rects[f, b]
                if xa >= 0 and xa <= sx <= xb and ya <= sy <= yb:
                    src_box[f, s] = b
                    counts[f, 2] += 1
                    break
    return peak, value, center, rects, src_box, counts
