"""CPU: the host-side contract of bf_fuse_boxes_device (every argument is checked before device bring-up, so the refusals run without
a GPU), the Python front end without a GPU, and the NumPy restatement the GPU tests compare with (tests/fuse_np.py): against the
display path it inverts (oracle/visual_np.calculate_heatmap: colourise's flip, then the half-pixel upscale), and against what the
definition promises."""
import math

import numpy as np
import pytest

import fuse_cases
import fuse_np
import separate_np as snp
import visual_np
from support import entry, FAKE, refused


_fuse = entry("bf_fuse_boxes_device", d_power=FAKE, frames=2, image_stride=1000, rows=41, cols=23, offset_per_dir=4, d_boxes=FAKE, d_box_counts=FAKE,
              max_boxes=300, img_w=640, img_h=360, conf=0.5, d_src_offsets=FAKE, n_src=4, d_peak_offsets=FAKE, d_peak_power=FAKE,
              d_center_offsets=FAKE, d_rects=FAKE, d_src_box=FAKE, d_counts=FAKE)


def test_symbol_is_exported(native):
    assert hasattr(native.lib, "bf_fuse_boxes_device")


@pytest.mark.parametrize("kw,match", [
    (dict(d_power=None), "bf_fuse_boxes_device: d_power is null"),
    (dict(d_boxes=None), "bf_fuse_boxes_device: d_boxes is null"),
    (dict(d_peak_offsets=None), "bf_fuse_boxes_device: d_peak_offsets is null"),
    (dict(frames=0), "bf_fuse_boxes_device: frames = 0 < 1"),
    (dict(frames=-2), "frames = -2 < 1"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(cols=-1), "cols = -1 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(max_boxes=0), "max_boxes = 0 < 1"),
    (dict(img_w=0), "img_w = 0 < 1"),
    (dict(img_h=-5), "img_h = -5 < 1"),
    (dict(rows=65536, cols=32768), r"rows \* cols = 2147483648 does not fit an int"),
    (dict(image_stride=942), r"image_stride = 942 < rows \* cols = 943"),
    (dict(rows=1, cols=3, offset_per_dir=2 ** 30), r"\(rows \* cols - 1\) \* offset_per_dir = 2147483648 does not fit"),
    (dict(conf=math.inf), "conf = inf is not finite"),
    (dict(conf=-math.inf), "conf = -inf is not finite"),
    (dict(conf=math.nan), "conf = -?nan is not finite"),
    (dict(n_src=-1), "n_src = -1 < 0"),
    (dict(n_src=65), "n_src = 65 > 64"),
    (dict(d_src_offsets=None), "d_src_offsets is null with n_src = 4"),
    (dict(d_src_box=None), "d_src_box is null with n_src = 4"),
])
def test_fuse_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _fuse(native, **kw), match)


def test_valid_arguments_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only: with one, valid arguments would enqueue")
    refused(native, _fuse(native), "no usable HIP device")
    refused(native, _fuse(native, n_src=0, d_src_offsets=None, d_src_box=None), "no usable HIP device")
    refused(native, _fuse(native, n_src=64), "no usable HIP device")
    refused(native, _fuse(native, max_boxes=1), "no usable HIP device")
    refused(native, _fuse(native, d_box_counts=None, d_peak_power=None, d_center_offsets=None, d_rects=None, d_counts=None), "no usable HIP device")
    refused(native, _fuse(native, rows=361, cols=361, offset_per_dir=2048, image_stride=361 * 361), "no usable HIP device")


def test_fusion_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only")
    import fuse
    import listen
    bl = listen.BeamListener("pad", mics=[0, 1, 2])
    with pytest.raises(native.BeamformerError, match="no usable HIP device"):
        fuse.SensorFusion(bl, image_size=(640, 640))


def test_pipeline_has_focus():
    import inspect
    import pipeline
    assert list(inspect.signature(pipeline.FusedPipeline.focus).parameters) == ["self", "power", "boxes", "counts", "fusion", "sources"]


# ------------------------------------------------------------------ the definition against the display path

def _one(rows, cols, W, H, per, box, power=None, score=0.9, conf=0.5):
    """The restatement on one frame with one box -> (peak, power, center, rect)."""
    power = np.zeros((1, rows * cols), dtype=np.float32) if power is None else power
    boxes = np.array([[list(box) + [score, 0]]], dtype=np.float32)
    peak, value, center, rects, _, _ = fuse_np.fuse(power, rows, cols, per, boxes, None, W, H, conf)
    return int(peak[0, 0]), value[0, 0], int(center[0, 0]), rects[0, 0].tolist()


@pytest.mark.parametrize("shape", fuse_cases.SHAPES, ids=lambda s: "%dx%d_on_%dx%d" % s)
def test_footprint_inverts_the_display_path(shape):
    """A single-hot map (1.0 in one cell, 1e-6 elsewhere) through calculate_heatmap: every display pixel that attains the maximum
    colour lies in the pixel set the definition assigns to the hot direction, and the bounding box of those pixels has that one
    direction as its footprint, its peak and its centre."""
    X, Y, W, H = shape
    per = 7
    for x0, y0 in fuse_cases.hot_cells(X, Y):
        img = np.full((X, Y), 1e-6, dtype=np.float32)
        img[x0, y0] = 1.0
        heat, should = visual_np.calculate_heatmap(img, window=(W, H))
        assert should and heat.shape == (H, W, 3)
        s = heat.astype(np.int64).sum(axis=-1)
        vs, us = np.nonzero(s == s.max())
        assert s.max() > 0 and vs.size > 0
        assert (fuse_np.cell(us, X, W) == X - 1 - x0).all(), (shape, x0, y0)
        assert (fuse_np.cell(vs, Y, H) == Y - 1 - y0).all(), (shape, x0, y0)
        box = [us.min(), vs.min(), us.max() + 1, vs.max() + 1]
        d0 = x0 * Y + y0
        peak, _, center, rect = _one(X, Y, W, H, per, box, power=img.reshape(1, -1))
        assert rect == [x0, x0, y0, y0] and peak == d0 * per and center == d0 * per, (shape, x0, y0, box, rect, peak, center)


@pytest.mark.parametrize("shape", [(5, 3, 7, 5), (11, 11, 64, 36), (41, 23, 640, 360)], ids=lambda s: "%dx%d_on_%dx%d" % s)
def test_round_trip_of_every_direction(shape):
    X, Y, W, H = shape
    for x0 in range(X):
        us = fuse_np.pixel_set(x0, X, W)
        assert us and fuse_np.axis(min(us), max(us) + 1, W, X) == (x0, x0)
    for y0 in range(Y):
        vs = fuse_np.pixel_set(y0, Y, H)
        assert vs and fuse_np.axis(min(vs), max(vs) + 1, H, Y) == (y0, y0)
    for x0, y0 in ((0, 0), (X - 1, Y - 1), (X // 2, Y // 3)):       # the two axes together, through the whole restatement
        assert _one(X, Y, W, H, 3, fuse_cases.box_of_cell(x0, y0, X, Y, W, H))[3] == [x0, x0, y0, y0]
    power = np.random.default_rng(X * Y).standard_normal((1, X * Y)).astype(np.float32)
    peak, value, _, rect = _one(X, Y, W, H, 3, (0, 0, W, H), power=power)
    assert rect == [0, X - 1, 0, Y - 1] and peak == int(np.argmax(power)) * 3 and value == power.max()


# ------------------------------------------------------------------ consequences of the definition

def test_boxes_without_a_footprint():
    rows, cols, W, H = 11, 11, 64, 36
    for box in ((np.nan, 1, 20, 20), (1, np.nan, 20, 20), (1, 1, np.nan, 20), (1, 1, 20, np.nan), (30, 20, 10, 5), (30, 5, 10, 20), (10, 20, 30, 5),
                (-20, 0, -1, 36), (64.6, 0, 90, 36), (0, -30, 64, -0.4), (0, 35.6, 64, 50), (10.2, 10.2, 10.4, 10.4)):
        peak, value, _, rect = _one(rows, cols, W, H, 2, box)
        assert peak == -1 and value == 0 and rect == [-1] * 4, box
    assert _one(rows, cols, W, H, 2, (10.2, 10.2, 10.6, 10.6))[0] >= 0          # the pixel centre (10.5, 10.5) is inside this one


def test_the_edge_batch():
    c = fuse_cases.edge_batch()
    per, cols = c["per"], c["cols"]
    before = [c[n].copy() for n in ("power", "boxes", "counts", "sources")]
    peak, value, center, rects, src_box, counts = fuse_np.fuse(c["power"], c["rows"], cols, per, c["boxes"], c["counts"], c["W"], c["H"], c["conf"], c["sources"])
    for n, b in zip(("power", "boxes", "counts", "sources"), before):
        assert c[n].tobytes() == b.tobytes()
    # frame 0: a count above max_boxes is clamped; seven boxes without a footprint; -0.0f ties with 0.0f and the lower d wins
    assert peak[0].tolist() == [-1] * 7 + [3 * per] and (rects[0, :7] == -1).all() and rects[0, 7].tolist() == [0, 4, 0, 2]
    assert np.signbit(value[0, 7]) and value[0, 7] == 0 and not value[0, :7].any()
    assert center[0, 0] == -1 and center[0, 1] >= 0                          # a NaN midpoint; reversed corners still have a midpoint
    assert src_box[0].tolist() == [-1, -1, -1, 7, 7] and counts[0].tolist() == [8, 1, 2]
    # frame 1: low and NaN scores and rows beyond the count are not boxes; equal maxima take the lower d; non-finite cells are skipped
    assert peak[1].tolist() == [-1, -1, 5 * per, 1 * per, -1, -1, -1, -1] and value[1].tolist() == [0, 0, 2, 2, 0, 0, 0, 0]
    assert rects[1, 2].tolist() == [1, 3, 1, 2] and rects[1, 3].tolist() == [0, 2, 0, 2] and rects[1, 4].tolist() == [3, 4, 0, 0]
    assert (rects[1, [0, 1, 5, 6, 7]] == -1).all() and (center[1, [0, 1, 5, 6, 7]] == -1).all()
    assert src_box[1].tolist() == [2, 3, -1, 4, -1] and counts[1].tolist() == [3, 2, 3]
    # frame 2: a negative count is no boxes at all
    assert (peak[2] == -1).all() and (center[2] == -1).all() and (rects[2] == -1).all() and (src_box[2] == -1).all() and not counts[2].any()
    # no count at all: every row is a candidate, so the rows beyond frame 1's count come back
    peak_all = fuse_np.fuse(c["power"], c["rows"], cols, per, c["boxes"], None, c["W"], c["H"], c["conf"], c["sources"])[0]
    assert (peak_all[1, 5:] == 1 * per).all() and (peak_all[2] >= 0).all()


def test_fast_form_of_the_restatement():
    for c in (fuse_cases.edge_batch(), fuse_cases.many_boxes_case(F=2, B=40, n_src=8)):
        args = (c["power"], c["rows"], c["cols"], c["per"], c["boxes"], c["counts"], c["W"], c["H"], c["conf"], c["sources"])
        for a, b in zip(fuse_np.fuse(*args), fuse_np.fuse(*args, fast=True)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_scene_boxes_on_the_plain_map(oracle_lib):
    """What tests/test_fuse.py's end-to-end case expects, on the CPU: the strong source's box has its peak within Chebyshev distance 1
    of that source (measured: 0 in both frames), and the loudest source of the plain map lies in that box.  The weak source's box
    does NOT: 10 dB down, it sits under the strong one's skirt on the plain map, and the loudest cell of its box is the corner
    towards the strong source -- measured distance 2 in both frames, the box's half-width.  That is the definition at work (the
    loudest cell under the box), so the GPU test expects the restatement's own answer there."""
    import peaks_np
    s = snp.SCENE
    rows, cols, M = s["rows"], s["cols"], s["M"]
    _, _, _, plain = snp.scene_reference(oracle_lib)
    boxes = fuse_cases.scene_boxes(s)
    src = peaks_np.peaks(plain, rows, cols, 3, 1, 0.0, 0.0, M)[0]
    peak, _, _, rects, src_box, counts = fuse_np.fuse(plain, rows, cols, M, boxes, None, 640, 360, 0.5, src)
    for f, dirs in enumerate(((s["A"], s["B"]), (s["B"], s["A"]))):
        dist = [snp.chebyshev(peak[f, b], M, cols, dirs[b]) for b in range(2)]
        print("frame %d: box peaks at distance %s of (A, B), rects %s" % (f, dist, rects[f].tolist()))
        assert dist[0] is not None and dist[0] <= 1
        assert dist[1] is not None and dist[1] <= 2                              # inside its box, which reaches two cells each way
    assert src_box.tolist() == [[0], [0]] and counts.tolist() == [[2, 2, 1], [2, 2, 1]]
