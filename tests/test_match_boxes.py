"""GPU (-m gpu): bf_match_boxes_device and bf_smooth_boxes_device EQUAL to their NumPy restatements (tests/match_np.py).

The matcher is integer arithmetic up to three correctly rounded float64 operations and the smoother a fixed sequence of float32
ones, so every output -- and the smoother's state words -- is compared as bytes.  One case per branch of the definitions
(tests/match_cases.py says what each one reaches; the host tests check that it does)."""
import numpy as np
import pytest

import match_cases as cases
import match_np as mn
import util
from support import nat

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F, TAIL = -77, -123.5, 16
MATCH_NAMES = ("moved", "score", "shift", "status")
SMOOTH_NAMES = ("out", "boosted", "counts", "state")


def _buf(torch, shape, flt):
    return torch.full((int(np.prod(shape)) + TAIL,), SENTINEL_F if flt else SENTINEL_I, dtype=torch.float32 if flt else torch.int32, device="cuda")


def _take(b, shape):
    """A sentinel-filled buffer back on the host: its tail untouched, its head in shape."""
    h = b.cpu().numpy()
    k = int(np.prod(shape))
    assert (h[k:] == h.dtype.type(SENTINEL_F if h.dtype == np.float32 else SENTINEL_I)).all()
    return h[:k].reshape(shape)


def _same(names, got, want, what):
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert g.tobytes() == w.tobytes()


def _match(nat, images, prev, boxes, n=None, t_pct=120, s_pct=150, stride=4, shift=True):
    """bf_match_boxes_device into sentinel-filled buffers with a tail -> (moved, score, shift or None, status) as host arrays; the
    tails are checked here, and that no input was written.  stride > 4 pads the rows with a score, a class and more."""
    torch = util.torch_gpu()
    F, B = boxes.shape[:2]
    H, W = images.shape[1:3]
    rows = np.full((F, B, stride), 0.625, dtype=np.float32)
    rows[:, :, :4] = boxes
    d_images, d_rows = torch.from_numpy(np.ascontiguousarray(images)).cuda(), torch.from_numpy(rows).cuda()
    d_prev = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev)).cuda()
    d_n = None if n is None else torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32)).cuda()
    shapes = ((F, B, 4), (F, B), (F, B, 2), (F, B))
    bufs = [_buf(torch, s, flt) if (shift or i != 2) else None for i, (s, flt) in enumerate(zip(shapes, (True, True, False, False)))]
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = nat.lib.bf_match_boxes_device(ptr(d_images), ptr(d_prev), F, H, W, ptr(d_rows), stride, ptr(d_n), B, t_pct, s_pct, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]),
                                       ptr(bufs[3]), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert d_images.cpu().numpy().tobytes() == images.tobytes() and d_rows.cpu().numpy().tobytes() == rows.tobytes()
    assert (d_prev is None or d_prev.cpu().numpy().tobytes() == prev.tobytes()) and (d_n is None or (d_n.cpu().numpy() == n).all())
    return [None if b is None else _take(b, s) for b, s in zip(bufs, shapes)]


# ------------------------------------------------------------------ parity with the restatement, one case per branch

@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_match_parity_with_restatement(nat, case):
    c, want, info = cases.reference(case)
    c["check"](want, info)
    got = _match(nat, c["images"], c["prev"], c["boxes"], None, c["t_pct"], c["s_pct"])
    _same(MATCH_NAMES, got, want, case)


@pytest.mark.parametrize("case", ["rolled", "borders", "hostile"])
def test_row_strides_counts_and_null_shift(nat, case):
    """A stride of 6 (detector rows) equals a stride of 4; d_n_boxes 0, in between, and above max_boxes; d_shift NULL."""
    c, want, _ = cases.reference(case)
    _same(MATCH_NAMES, _match(nat, c["images"], c["prev"], c["boxes"], None, c["t_pct"], c["s_pct"], stride=6), want, "stride 6")
    n = np.array([0, 4, cases.B + 5], dtype=np.int32)
    wn = mn.match_boxes_np(c["images"], c["prev"], c["boxes"], n, c["t_pct"], c["s_pct"])
    assert (wn[3][0] == 1).all() and (wn[3][1, 4:] == 1).all() and wn[3][2].tobytes() == want[3][2].tobytes()
    _same(MATCH_NAMES, _match(nat, c["images"], c["prev"], c["boxes"], n, c["t_pct"], c["s_pct"], stride=7), wn, "counts")
    bare = _match(nat, c["images"], c["prev"], c["boxes"], n, c["t_pct"], c["s_pct"], shift=False)
    assert bare[2] is None
    _same(MATCH_NAMES, bare, wn, "d_shift NULL")


def test_one_call_equals_one_call_per_frame(nat):
    for case in ("rolled", "borders"):
        c, want, _ = cases.reference(case)
        parts = [_match(nat, c["images"][f:f + 1], c["prev"] if f == 0 else c["images"][f - 1], c["boxes"][f:f + 1], None, c["t_pct"], c["s_pct"])
                 for f in range(cases.F)]
        _same(MATCH_NAMES, [np.concatenate([p[i] for p in parts]) for i in range(4)], want, case)


# ------------------------------------------------------------------ the smoother against its restatement

def _smooth(nat, c):
    torch = util.torch_gpu()
    B, S = c["boxes"].shape[0], c["slots"]
    words = mn.state_words(S)
    d_boxes = torch.from_numpy(c["boxes"]).cuda()
    d_n = None if c["n"] is None else torch.tensor([c["n"]], dtype=torch.int32, device="cuda")
    ins = [torch.from_numpy(c[k]).cuda() for k in ("moved", "score", "status")]
    d_state = torch.full((words + TAIL,), SENTINEL_I, dtype=torch.int32, device="cuda")
    d_state[:words] = torch.from_numpy(c["state"]).cuda()
    shapes = ((B, 6), (B,), (4,))
    bufs = [_buf(torch, s, flt) for s, flt in zip(shapes, (True, False, False))]
    kw = dict(conf_low=0.3, conf_high=0.7, iou=0.5, corr=0.8)
    kw.update(c["kw"])
    rc = nat.lib.bf_smooth_boxes_device(d_boxes.data_ptr(), None if d_n is None else d_n.data_ptr(), B, kw["conf_low"], kw["conf_high"], kw["iou"], kw["corr"], S,
                                        ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), d_state.data_ptr(), *[b.data_ptr() for b in bufs],
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert d_boxes.cpu().numpy().tobytes() == c["boxes"].tobytes() and all(t.cpu().numpy().tobytes() == c[k].tobytes() for t, k in zip(ins, ("moved", "score", "status")))
    h = d_state.cpu().numpy()
    assert (h[words:] == SENTINEL_I).all()
    return [_take(b, s) for b, s in zip(bufs, shapes)] + [h[:words]]


@pytest.mark.parametrize("case", sorted(cases.SMOOTH_CASES))
def test_smooth_parity_with_restatement(nat, case):
    c, want = cases.smooth_reference(case)
    _same(SMOOTH_NAMES, _smooth(nat, c), want, case)


# ------------------------------------------------------------------ the front end: a scene through SmoothDetections

def _scene_tensors(torch):
    images, boxes = cases.scene()
    return torch.from_numpy(images.copy()).cuda(), torch.from_numpy(boxes.copy()).cuda()


@pytest.mark.parametrize("corr", [2.0, 0.8])
def test_scene_through_the_front_end(nat, corr):
    """The object's row leaves every frame kept; with corr = 2.0 the stray candidate is dropped, with the reference's 0.8 it is boosted
    as well (the header says why).  One pass equals the same frames split over two update calls, state words included."""
    torch = util.torch_gpu()
    import pipeline
    import smooth
    want = cases.scene_reference(corr)
    assert (want[0][2:, 0, 4] == np.float32(0.7)).all() and (want[0][3:5, 1, 4] == np.float32(0.0 if corr > 1 else 0.7)).all()
    d_images, d_boxes = _scene_tensors(torch)
    sm = smooth.SmoothDetections(slots=4, corr=corr)
    assert sm.state.dtype == torch.int32 and sm.state.shape == (20,) and not sm.state.any()
    got = sm.update(d_images, d_boxes)
    torch.cuda.synchronize()
    names = ("out", "boosted", "counts", "moved", "score", "state", "prev_image")
    _same(names, [t.cpu().numpy() for t in got + (sm.state,)], want[:6], "one pass")
    assert sm.prev_image.cpu().numpy().tobytes() == want[6].tobytes()
    sm.reset()
    p = pipeline.FusedPipeline.__new__(pipeline.FusedPipeline)
    first = p.smooth(d_images[:3], d_boxes[:3], None, sm)
    mid = sm.state.cpu().numpy().copy()
    second = sm.update(d_images[3:], d_boxes[3:], None)
    torch.cuda.synchronize()
    assert mid[0] == 1 and mid.tobytes() == mn.smooth_stream_np(*[a[:3] for a in cases.scene()], None, 4, corr=corr)[5].tobytes()
    _same(names, [torch.cat([a, b]).cpu().numpy() for a, b in zip(first, second)] + [sm.state.cpu().numpy()], want[:6], "3 + 5 frames")
    # the plain call
    c, wm, _ = cases.reference("rolled")
    m = sm.match(torch.from_numpy(c["images"]).cuda(), torch.from_numpy(c["prev"]).cuda(), torch.from_numpy(c["boxes"]).cuda())
    torch.cuda.synchronize()
    _same(MATCH_NAMES, [t.cpu().numpy() for t in m], wm, "match")
    for bad in (lambda: sm.update(d_images.float(), d_boxes), lambda: sm.update(d_images, d_boxes[:, :, :5]), lambda: sm.update(d_images[:, :, :, :2], d_boxes),
                lambda: sm.update(d_images, d_boxes[:-1]), lambda: sm.match(d_images, d_images[0, :-1], d_boxes), lambda: smooth.SmoothDetections(slots=65)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(nat.BeamformerError, match="s_pct = 110 < t_pct = 120"):
        smooth.SmoothDetections(s_pct=110).update(d_images, d_boxes)


def test_graph_replays_on_images_overwritten_in_place(nat):
    """A captured update (one match and one smooth launch, and the copy of the image) replayed frame after frame on the same two
    tensors, overwritten in place, equals the stream's eager result."""
    torch = util.torch_gpu()
    import smooth
    want = cases.scene_reference(2.0)
    d_images, d_boxes = _scene_tensors(torch)
    sm = smooth.SmoothDetections(slots=4, corr=2.0)
    cam, rows = d_images[:1].clone(), d_boxes[:1].clone()
    sm.update(cam, rows)                                           # the warm-up call: it allocates prev_image and brings the device up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = sm.update(cam, rows)
    sm.reset()                                                     # the capture ran nothing; start the stream again from frame 0
    outs = []
    for f in range(cases.SCENE_FRAMES):
        cam.copy_(d_images[f:f + 1]); rows.copy_(d_boxes[f:f + 1])
        if f == 0:
            outs.append([t.clone() for t in sm.update(cam, rows)])
        else:
            g.replay()
            outs.append([t.clone() for t in held])
    torch.cuda.synchronize()
    got = [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(5)] + [sm.state.cpu().numpy()]
    _same(("out", "boosted", "counts", "moved", "score", "state"), got, want[:6], "graph replays")
