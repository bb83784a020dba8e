"""GPU (-m gpu): bf_track_boxes_device, SORT on the device, EQUAL to the NumPy restatement (tests/box_track_np.py).

The definition fixes every float32 operation, its order and the assignment's float64 steps, so every output and the state words are
compared as bytes.  One case per branch of the definition (tests/box_track_cases.py says what each one reaches)."""
import numpy as np
import pytest

import box_track_cases as cases
import box_track_np as bt
import util
from support import nat

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F, TAIL = -77, -123.5, 16
NAMES = ("tracks", "ids", "match", "live", "counts", "state")
FLOAT = (True, False, False, True, False)


def _shapes(F, slots):
    return ((F, slots, 6), (F, slots), (F, slots), (F, slots, 4), (F, 4))


def _call(nat, boxes, n, slots, conf=0.1, iou_threshold=0.3, max_age=1, min_hits=3, state=None, optional=True):
    """bf_track_boxes_device into sentinel-filled buffers with a tail -> (tracks, ids, match, live, counts, state) as host arrays
    (None for the optional outputs when optional is False); the tails, the state's included, are checked here, and that no input
    was written."""
    torch = util.torch_gpu()
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    F, B = boxes.shape[:2]
    words = bt.state_words(slots)
    d_boxes = torch.from_numpy(boxes).cuda()
    d_n = None if n is None else torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32)).cuda()
    d_state = torch.full((words + TAIL,), SENTINEL_I, dtype=torch.int32, device="cuda")
    d_state[:words] = 0 if state is None else torch.from_numpy(np.asarray(state, dtype=np.int32)).cuda()
    shapes = _shapes(F, slots)
    bufs = [torch.full((int(np.prod(s)) + TAIL,), SENTINEL_F if flt else SENTINEL_I, dtype=torch.float32 if flt else torch.int32, device="cuda")
            if (optional or i == 0) else None for i, (s, flt) in enumerate(zip(shapes, FLOAT))]
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = nat.lib.bf_track_boxes_device(ptr(d_boxes), ptr(d_n), F, B, conf, slots, iou_threshold, max_age, min_hits, ptr(d_state), ptr(bufs[0]), ptr(bufs[1]),
                                       ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert d_boxes.cpu().numpy().tobytes() == boxes.tobytes() and (d_n is None or (d_n.cpu().numpy() == n).all())
    out = []
    for b, s in zip(bufs, shapes):
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy()
        k = int(np.prod(s))
        assert (h[k:] == h.dtype.type(SENTINEL_F if h.dtype == np.float32 else SENTINEL_I)).all()
        out.append(h[:k].reshape(s))
    h = d_state.cpu().numpy()
    assert (h[words:] == SENTINEL_I).all()
    out.append(h[:words])
    return out


# ------------------------------------------------------------------ a - g, i: parity with the restatement, one case per branch

@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_parity_with_restatement(nat, case):
    c, want, br = cases.reference(case)
    cases.check_reaches(case, want, br)
    print(case, "born/ended/dropped/ignored", want[4].sum(axis=0).tolist(), "branches", {b: br.count(b) for b in sorted(set(br))})
    got = _call(nat, c["boxes"], c["n"], c["slots"], state=c["state"], **c["kw"])
    util.same_named(NAMES, got, want, case)


# ------------------------------------------------------------------ h. d_n_boxes = NULL and every optional output NULL

def test_null_count_and_null_outputs(nat):
    c, _, _ = cases.reference("hostile")
    kw = c["kw"]
    want = bt.track_boxes_np(c["boxes"], None, c["slots"], **kw)
    assert want[4][:, 3].min() >= 3 and want[4][:, 2].sum() > 0            # every row is a candidate: the rows beyond n_boxes too
    full = _call(nat, c["boxes"], None, c["slots"], **kw)
    util.same_named(NAMES, full, want, "n_boxes NULL")
    bare = _call(nat, c["boxes"], None, c["slots"], optional=False, **kw)
    assert all(b is None for b in bare[1:5])
    util.same_named(NAMES, bare, want, "optional outputs NULL")


# ------------------------------------------------------------------ j. one call of 33 frames against calls of 1 + 15 + 17 on one state

def test_state_carry(nat):
    c, want, _ = cases.reference("long_stream")
    boxes, n, slots, kw = c["boxes"], c["n"], c["slots"], c["kw"]
    assert boxes.shape[0] == 33
    state, parts = None, []
    for a, b in ((0, 1), (1, 16), (16, 33)):
        parts.append(_call(nat, boxes[a:b], n[a:b], slots, state=state, **kw))
        state = parts[-1][5]
        assert state[1] == b and state[4] != 0                             # frame_count carried, tracks alive at the cut
    joined = [np.concatenate([p[i] for p in parts]) for i in range(5)] + [state]
    util.same_named(NAMES, joined, want, "1 + 15 + 17")


# ------------------------------------------------------------------ k. a captured graph replayed three times against three eager calls

def test_graph_replays_advance_the_state(nat):
    torch = util.torch_gpu()
    c, _, _ = cases.reference("long_stream")
    slots, kw = c["slots"], c["kw"]
    boxes, n = c["boxes"][:11], c["n"][:11]
    F, B = boxes.shape[:2]
    eager, state = [], None
    for r in range(3):                                                      # the same 11 frames three times over on one state
        eager.append(_call(nat, boxes, n, slots, state=state, **kw))       # (also brings the library's device up outside the capture)
        state = eager[-1][5]
    want, wstate = [], None
    for r in range(3):
        want.append(bt.track_boxes_np(boxes, n, slots, state=wstate, **kw))
        wstate = want[-1][5]
        util.same_named(NAMES, eager[r], want[r], "eager call %d" % r)
    assert want[2][5][1] == 33 and want[1][0].tobytes() != want[0][0].tobytes()
    # a shape no call has had before: this launch is captured without a warm-up of its own
    slots2 = slots + 1
    d_boxes, d_n = torch.from_numpy(boxes).cuda(), torch.from_numpy(n).cuda()
    d_state = torch.zeros((bt.state_words(slots2),), dtype=torch.int32, device="cuda")
    bufs = [torch.full(s, SENTINEL_F if flt else SENTINEL_I, dtype=torch.float32 if flt else torch.int32, device="cuda") for s, flt in zip(_shapes(F, slots2), FLOAT)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert nat.lib.bf_track_boxes_device(d_boxes.data_ptr(), d_n.data_ptr(), F, B, 0.1, slots2, 0.3, kw["max_age"], kw["min_hits"], d_state.data_ptr(),
                                             *[b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream) == 0
    wstate = None
    for r in range(3):
        for b, flt in zip(bufs, FLOAT):
            b.fill_(SENTINEL_F if flt else SENTINEL_I)
        g.replay()
        torch.cuda.synchronize()
        w = bt.track_boxes_np(boxes, n, slots2, state=wstate, **kw)
        wstate = w[5]
        util.same_named(NAMES, [t.cpu().numpy() for t in bufs + [d_state]], w, "graph replay %d" % r)


# ------------------------------------------------------------------ l. the front end: BoxTracker.update -> SensorFusion.focus -> listen

def test_tracker_feeds_focus_and_listen(nat):
    torch = util.torch_gpu()
    import boxtrack
    import fuse
    import listen
    import pipeline
    c = util.configure("cfg1")
    table = util.table_for("lerp", "cfg1")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    bl = listen.BeamListener("lerp", mics=np.arange(c["M"], dtype=np.int32))
    rows, cols, per = c["X"], c["Y"], bl.offset_per_dir
    boxes, n, owner = bt.behaviour_scene()
    F, S = boxes.shape[0], 4
    rng = np.random.default_rng(31)
    d_frames = torch.from_numpy(rng.standard_normal((F, c["M"], c["N"])).astype(np.float32)).cuda()
    d_boxes, d_n = torch.from_numpy(boxes).cuda(), torch.from_numpy(n).cuda()
    tr = boxtrack.BoxTracker(slots=S)
    assert tr.state.dtype == torch.int32 and tr.state.shape == (84,) and tr.state.is_cuda and not tr.state.any()
    sf = fuse.SensorFusion(bl, image_size=(640, 640), conf=0.1)
    d_maps = bl.maps(d_frames)
    tracks, ids, match, live, counts = tr.update(d_boxes, d_n)
    peak, _, _, rects, _, _ = sf.focus(d_maps, tracks)
    out, status = bl.listen(d_frames, peak[:, :S])
    torch.cuda.synchronize()
    assert tracks.shape == (F, S, 6) and tracks.dtype == torch.float32 and live.shape == (F, S, 4) and counts.shape == (F, 4) and ids.dtype == torch.int32
    got = [t.cpu().numpy() for t in (tracks, ids, match, live, counts, tr.state)]
    want = bt.track_boxes_np(boxes, n, S)
    util.same_named(NAMES, got, want, "front end")
    peak, rects, status, out = (t.cpu().numpy() for t in (peak, rects, status, out))
    reported = want[0][:, :, 4] > 0
    assert reported[:, :2].sum() > 40 and not reported[:, 2:].any()
    assert ((peak >= 0) == reported).all() and ((status == 0) == reported).all() and (status[~reported] == 1).all()
    assert np.isnan(out[~reported]).all() and np.isfinite(out[reported]).all()
    d = peak[reported] // per                                               # a reported slot's peak lies under its tracked box
    xa, xb, ya, yb = rects[reported].T
    assert (peak[reported] % per == 0).all() and (xa <= d // cols).all() and (d // cols <= xb).all() and (ya <= d % cols).all() and (d % cols <= yb).all()
    # a second batch continues the tracks; FusedPipeline.track forwards; reset forgets
    p = pipeline.FusedPipeline.__new__(pipeline.FusedPipeline)
    _, ids2, _, _, counts2 = p.track(d_boxes[-3:], d_n[-3:], tr)
    torch.cuda.synchronize()
    assert (ids2.cpu().numpy()[:, :2] == [1, 2]).all() and not counts2.cpu().numpy()[:, 0].any() and tr.state[1].item() == F + 3
    tr.reset()
    _, ids3, _, _, counts3 = tr.update(d_boxes[-3:], None)
    torch.cuda.synchronize()
    assert (ids3.cpu().numpy()[:, :2] == [1, 2]).all() and counts3.cpu().numpy()[0, 0] == 2
    for bad in (lambda: tr.update(d_boxes.double(), d_n), lambda: tr.update(d_boxes[:, :, :5], d_n), lambda: tr.update(d_boxes.cpu(), d_n),
                lambda: tr.update(d_boxes, d_n.long()), lambda: tr.update(d_boxes, d_n[:-1]), lambda: tr.update(d_boxes[0], d_n),
                lambda: boxtrack.BoxTracker(slots=65), lambda: boxtrack.BoxTracker(slots=0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(nat.BeamformerError, match=r"iou_threshold = 1.5 is not in \[0, 1\]"):
        boxtrack.BoxTracker(iou=1.5).update(d_boxes, d_n)
