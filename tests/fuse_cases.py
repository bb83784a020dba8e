"""Inputs the host and GPU tests of bf_fuse_boxes_device share (tests/test_fuse_host.py states what each must give, tests/test_fuse.py
runs them on the device)."""
import numpy as np

import fuse_np

NAN, INF = np.float32(np.nan), np.float32(np.inf)

# the display-path shapes (X, Y, W, H): grid X x Y overlaid on a W x H frame
SHAPES = [(5, 3, 7, 5), (11, 11, 64, 36), (11, 7, 640, 640), (41, 23, 640, 360), (57, 32, 640, 360), (101, 101, 640, 640)]


def hot_cells(X, Y):
    return [(0, 0), (0, Y - 1), (X - 1, 0), (X - 1, Y - 1), (X // 3, 2 * Y // 3), (X // 2, Y // 2)]


def box_of_cell(x0, y0, X, Y, W, H, grow=0):
    """The box [min u, max u + 1] x [min v, max v + 1] of the display pixels of the cells within `grow` of (x0, y0)."""
    us = [u for x in range(max(x0 - grow, 0), min(x0 + grow, X - 1) + 1) for u in fuse_np.pixel_set(x, X, W)]
    vs = [v for y in range(max(y0 - grow, 0), min(y0 + grow, Y - 1) + 1) for v in fuse_np.pixel_set(y, Y, H)]
    return [min(us), min(vs), max(us) + 1, max(vs) + 1]


def edge_batch():
    """rows 5, cols 3 on a 7 x 5 frame, 3 frames, 8 rows of boxes, 5 sources, image_stride 20 with NaN in the padding -> a dict.
    Display column u lies over grid x = 4 - (10u + 5) // 14 (u = 0..6 -> 4 3 3 2 1 1 0), display row v over grid
    y = 2 - (6v + 3) // 10 (v = 0..4 -> 2 2 1 0 0).
      frame 0, count 99 (clamped to 8): seven boxes without a footprint, then the full frame; the map is negative but for -0.0 at
               d = 3 and 0.0 at d = 7
      frame 1, count 5: a low score, a NaN score, box A = x[1,3] y[1,2], box B = x[0,2] y[0,2], a box over the two non-finite cells
               d = 9, 12; rows 5..7 are beyond the count; maxima 2.0 at d = 1, 5, 10 and +inf at d = 7
      frame 2, count -3 (clamped to 0): nothing is a box"""
    rows, cols, W, H, per, F, B, stride = 5, 3, 7, 5, 4, 3, 8, 20
    D = rows * cols
    rng = np.random.default_rng(11)
    power = np.full((F, stride), NAN, dtype=np.float32)
    power[:, :D] = -rng.uniform(0.5, 1.5, (F, D)).astype(np.float32)
    power[0, 3], power[0, 7] = -0.0, 0.0
    power[1, [1, 5, 10]] = 2.0
    power[1, 7], power[1, 9], power[1, 12] = INF, NAN, -INF
    full = [0, 0, W, H]
    boxes = np.zeros((F, B, 6), dtype=np.float32)
    boxes[:, :, :4] = full
    boxes[:, :, 4] = 0.9
    boxes[:, :, 5] = np.arange(B) % 3
    boxes[0, :7, :4] = [[NAN, 0, 7, 5], [5, 4, 1, 1], [-10, 0, -3, 5], [7.6, 0, 12, 5], [0, -9, 7, -2], [0, 5.6, 7, 9], [1.2, 1.2, 1.4, 1.4]]
    boxes[1, 0, 4], boxes[1, 1, 4] = 0.3, NAN
    boxes[1, 2, :4], boxes[1, 3, :4], boxes[1, 4, :4] = [1, 0, 5, 3], [3, 1, 7, 5], [0, 3, 2, 5]
    boxes[1, 5:, 4] = 0.99
    counts = np.array([99, 5, -3], dtype=np.int32)
    at = lambda x, y: (x * cols + y) * per
    sources = np.array([[-1, 6, D * per, at(0, 0), at(4, 2)],
                        [at(2, 2), at(0, 0), at(4, 2), at(4, 0), -1],
                        [at(0, 0), at(2, 1), at(4, 2), at(1, 1), at(3, 0)]], dtype=np.int32)
    return dict(rows=rows, cols=cols, W=W, H=H, per=per, conf=0.5, power=power, boxes=boxes, counts=counts, sources=sources)


def random_boxes(rng, F, B, W, H, conf=0.5):
    """Seeded boxes anywhere in (and a little beyond) the frame, scores in descending order per frame straddling conf."""
    c = rng.uniform([-0.1 * W, -0.1 * H], [1.1 * W, 1.1 * H], (F, B, 2))
    s = rng.uniform(0.0, 0.4, (F, B, 2)) ** 2 * [W, H]
    boxes = np.zeros((F, B, 6), dtype=np.float32)
    boxes[:, :, 0:2], boxes[:, :, 2:4] = c - s / 2, c + s / 2
    boxes[:, :, 4] = -np.sort(-rng.uniform(conf - 0.3, 1.0, (F, B)), axis=1)
    boxes[:, :, 5] = rng.integers(0, 80, (F, B))
    return boxes


def map_read_case(rows, cols, W=640, H=360, per=3, seed=0):
    """2 frames, 6 boxes: the full frame, one display pixel (one cell), the last row and column of the grid (display pixel (0, 0)),
    its first ones, and two seeded boxes; 3 sources; a few non-finite cells."""
    rng = np.random.default_rng(seed + rows * cols)
    F, B, D = 2, 6, rows * cols
    power = rng.standard_normal((F, D)).astype(np.float32)
    power[:, rng.integers(0, D, 40)] = NAN
    power[0, D - 1], power[1, 0] = 9.0, 9.0
    boxes = random_boxes(rng, F, B, W, H)
    boxes[:, :, 4] = [0.95, 0.9, 0.85, 0.8, 0.75, 0.7]
    boxes[:, 0, :4] = [0, 0, W, H]
    boxes[:, 1, :4] = [W // 3, H // 3, W // 3 + 1, H // 3 + 1]
    boxes[:, 2, :4] = [0, 0, 3, 2]
    boxes[:, 3, :4] = [W - 3, H - 2, W, H]
    sources = np.array([[(D - 1) * per, 0, (D // 2) * per], [0, -1, (D - 1) * per]], dtype=np.int32)
    return dict(rows=rows, cols=cols, W=W, H=H, per=per, conf=0.5, power=power, boxes=boxes, counts=np.array([6, 5], dtype=np.int32), sources=sources)


def many_boxes_case(F=64, B=300, n_src=64, rows=41, cols=23, W=640, H=360, per=5, seed=3):
    rng = np.random.default_rng(seed)
    D = rows * cols
    power = rng.standard_normal((F, D)).astype(np.float32)
    power[rng.uniform(0, 1, (F, D)) < 0.01] = NAN
    boxes = random_boxes(rng, F, B, W, H)
    counts = rng.integers(0, B + 1, F).astype(np.int32)
    counts[0], counts[-1] = B, B - 7
    sources = (rng.integers(0, D, (F, n_src)) * per).astype(np.int32)
    sources[rng.uniform(0, 1, (F, n_src)) < 0.1] = -1
    return dict(rows=rows, cols=cols, W=W, H=H, per=per, conf=0.5, power=power, boxes=boxes, counts=counts, sources=sources)


def scene_boxes(scene, W=640, H=360):
    """One hand-made box per source of separate_np.SCENE on a W x H frame: the pixel set of the source's true direction enlarged by
    two cells; row 0 (the better score) is source A's in both frames' naming of the scene -> float32 [2, 2, 6]."""
    rows, cols = scene["rows"], scene["cols"]
    boxes = np.zeros((2, 2, 6), dtype=np.float32)
    for f, dirs in enumerate(((scene["A"], scene["B"]), (scene["B"], scene["A"]))):      # the second frame swaps the two directions
        for b, (x0, y0) in enumerate(dirs):
            boxes[f, b, :4] = box_of_cell(x0, y0, rows, cols, W, H, grow=2)
            boxes[f, b, 4] = 0.9 - 0.1 * b
    return boxes
