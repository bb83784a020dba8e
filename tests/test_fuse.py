"""GPU (-m gpu): bf_fuse_boxes_device, detector boxes against the acoustic map, EQUAL to the NumPy restatement (tests/fuse_np.py).

The definition is four float32 roundings per box and integers after that, so every output is compared as bytes."""
import numpy as np
import pytest

import fuse_cases
import fuse_np
import separate_np as snp
import util
from support import nat

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F, TAIL = -77, -123.5, 16
NAMES = ("peak", "power", "center", "rects", "src_box", "counts")
ALL = frozenset(NAMES)


def _call(nat, c, given=ALL, use_counts=True, use_sources=True):
    """bf_fuse_boxes_device on a case of fuse_cases into sentinel-filled buffers with a tail -> the six outputs as host arrays (None
    for the ones not in `given`); the tails are checked here, and that no input was written."""
    torch = util.torch_gpu()
    power, boxes = np.ascontiguousarray(c["power"], dtype=np.float32), np.ascontiguousarray(c["boxes"], dtype=np.float32)
    F, B = boxes.shape[:2]
    sources = c["sources"] if use_sources else None
    n_src = 0 if sources is None else sources.shape[1]
    inputs = [power, boxes, c["counts"] if use_counts else None, sources]
    d_in = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in inputs]
    shapes = dict(peak=(F, B), power=(F, B), center=(F, B), rects=(F, B, 4), src_box=(F, n_src), counts=(F, 3))
    bufs = {}
    for name in NAMES:
        want = name == "peak" or (name in given and (name != "src_box" or n_src > 0))
        flt = name == "power"
        bufs[name] = torch.full((int(np.prod(shapes[name])) + TAIL,), SENTINEL_F if flt else SENTINEL_I, dtype=torch.float32 if flt else torch.int32,
                                device="cuda") if want else None
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = nat.lib.bf_fuse_boxes_device(ptr(d_in[0]), F, power.shape[1], c["rows"], c["cols"], c["per"], ptr(d_in[1]), ptr(d_in[2]), B, c["W"], c["H"], c["conf"],
                                      ptr(d_in[3]), n_src, ptr(bufs["peak"]), ptr(bufs["power"]), ptr(bufs["center"]), ptr(bufs["rects"]),
                                      ptr(bufs["src_box"]), ptr(bufs["counts"]), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    for a, d in zip(inputs, d_in):
        assert a is None or d.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    out = []
    for name in NAMES:
        if bufs[name] is None:
            out.append(None)
            continue
        h = bufs[name].cpu().numpy()
        n = int(np.prod(shapes[name]))
        assert (h[n:] == h.dtype.type(SENTINEL_F if h.dtype == np.float32 else SENTINEL_I)).all(), name
        out.append(h[:n].reshape(shapes[name]))
    return out


def _want(c, use_counts=True, use_sources=True, fast=False):
    return fuse_np.fuse(c["power"], c["rows"], c["cols"], c["per"], c["boxes"], c["counts"] if use_counts else None, c["W"], c["H"], c["conf"],
                        c["sources"] if use_sources else None, fast=fast)


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        assert w is not None and g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ------------------------------------------------------------------ 1. edges

def test_edges(nat):
    c = fuse_cases.edge_batch()
    want = _want(c)
    got = _call(nat, c)
    _same(got, want, "edge batch")
    assert np.signbit(got[1][0, 7]) and got[0][1].tolist() == [-1, -1, 20, 4, -1, -1, -1, -1] and got[4][1].tolist() == [2, 3, -1, 4, -1]
    # every optional output once null; the others do not change
    for name in NAMES[1:]:
        if name == "src_box":
            part = _call(nat, c, use_sources=False)
            assert part[4] is None
            _same(part, _want(c, use_sources=False), "no sources")              # (counts[:, 2] is then 0)
            assert not part[5][:, 2].any() and part[0].tobytes() == got[0].tobytes()
            continue
        part = _call(nat, c, given=ALL - {name})
        assert part[NAMES.index(name)] is None
        _same(part, want, "without " + name)
    bare = _call(nat, c, given=frozenset(), use_sources=False)
    assert [x is None for x in bare] == [False, True, True, True, True, True] and bare[0].tobytes() == got[0].tobytes()
    # no count: every row is a candidate
    _same(_call(nat, c, use_counts=False), _want(c, use_counts=False), "no counts")


# ------------------------------------------------------------------ 2. both forms of the map read

@pytest.mark.parametrize("rows,cols", [(120, 128), (121, 127), (361, 361)])
def test_both_forms_of_the_map_read(nat, rows, cols):
    assert (rows * cols <= fuse_np.STAGE_MAX) == ((rows, cols) == (120, 128)) and 120 * 128 == fuse_np.STAGE_MAX
    c = fuse_cases.map_read_case(rows, cols)
    want = _want(c, fast=True)
    D, per = rows * cols, c["per"]
    assert want[3][0, 0].tolist() == [0, rows - 1, 0, cols - 1] and want[0][0, 0] == (D - 1) * per      # the full frame; its peak is the last cell
    assert (want[3][:, 1, 0] == want[3][:, 1, 1]).all() and (want[3][:, 1, 2] == want[3][:, 1, 3]).all()  # one cell
    assert want[3][0, 2, 1] == rows - 1 and want[3][0, 2, 3] == cols - 1 and want[0][0, 2] == (D - 1) * per
    assert want[3][1, 3, 0] == 0 and want[3][1, 3, 2] == 0 and want[0][1, 3] == 0
    assert want[4][0, 0] == 0 and want[5][1, 0] == 5
    _same(_call(nat, c), want, "%d x %d" % (rows, cols))


# ------------------------------------------------------------------ 3. many boxes: the per-wave loop and the split over workgroups

def test_many_boxes(nat):
    c = fuse_cases.many_boxes_case()
    want = _want(c, fast=True)
    assert 0 < want[5][:, 1].min() and (want[5][:, 0] < c["counts"]).any() and (want[0] == -1).any() and (want[4] >= 32).any() and (want[4] == -1).any()
    got = _call(nat, c)
    _same(got, want, "64 frames")
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    got1 = _call(nat, one)
    _same(got1, _want(one, fast=True), "1 frame")
    for name, a, b in zip(NAMES, got1, got):
        assert a.tobytes() == b[:1].tobytes(), name


# ------------------------------------------------------------------ 4. the front end

def _cfg1_listener(nat):
    import listen
    c = util.configure("cfg1")
    table = util.table_for("lerp", "cfg1")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    return c, listen.BeamListener("lerp", mics=np.arange(c["M"], dtype=np.int32))


def _cfg1_batch(c, F, seed, W=64, H=36, B=5):
    rng = np.random.default_rng(seed)
    frames = rng.standard_normal((F, c["M"], c["N"])).astype(np.float32)
    boxes = fuse_cases.random_boxes(rng, F, B, W, H)
    boxes[:, 0, :4] = [0, 0, W, H]
    boxes[:, 0, 4] = 0.99
    return frames, boxes, np.array([B - (f % 2) for f in range(F)], dtype=np.int32)


def test_front_end(nat):
    torch = util.torch_gpu()
    import fuse
    import pipeline
    c, bl = _cfg1_listener(nat)
    rows, cols, W, H, F = c["X"], c["Y"], 64, 36, 3
    frames, boxes, counts = _cfg1_batch(c, F, 21)
    d_frames, d_boxes, d_counts = (torch.from_numpy(a).cuda() for a in (frames, boxes, counts))
    sf = fuse.SensorFusion(bl, image_size=(W, H), conf=0.5)
    assert (sf.rows, sf.cols, sf.offset_per_dir) == (rows, cols, bl.offset_per_dir)
    d_maps = bl.maps(d_frames)
    src, _, _ = bl.sources(d_maps, k=3, radius=2, floor_rel=0.0)
    out = sf.focus(d_maps, d_boxes, d_counts, sources=src)
    beams, status = bl.listen(d_frames, out[0][:, :2])
    torch.cuda.synchronize()
    B = boxes.shape[1]
    for t, shape, dtype in zip(out, ((F, B), (F, B), (F, B), (F, B, 4), (F, 3), (F, 3)),
                               (torch.int32, torch.float32, torch.int32, torch.int32, torch.int32, torch.int32)):
        assert t.shape == shape and t.dtype == dtype and t.is_cuda
    maps = d_maps.cpu().numpy()
    want = fuse_np.fuse(maps, rows, cols, bl.offset_per_dir, boxes, counts, W, H, 0.5, src.cpu().numpy())
    _same([t.cpu().numpy() for t in out], want, "front end")
    assert (want[0][:, 0] == maps.argmax(axis=1) * bl.offset_per_dir).all()                 # the full-frame box hears the loudest direction
    host_beams, host_status = bl.listen(d_frames, torch.from_numpy(np.ascontiguousarray(want[0][:, :2])).cuda())
    torch.cuda.synchronize()
    assert beams.cpu().numpy().tobytes() == host_beams.cpu().numpy().tobytes() and (status.cpu().numpy() == host_status.cpu().numpy()).all()
    assert (status.cpu().numpy()[:, 0] == 0).all()
    # without sources and counts; FusedPipeline.focus forwards with its own frame size
    bare = sf.focus(d_maps, d_boxes)
    assert bare[4] is None
    _same([t if t is None else t.cpu().numpy() for t in bare], fuse_np.fuse(maps, rows, cols, bl.offset_per_dir, boxes, None, W, H, 0.5), "bare")
    p = pipeline.FusedPipeline.__new__(pipeline.FusedPipeline)
    p.size = 48
    via = p.focus(d_maps, d_boxes, d_counts, sf, sources=src)
    _same([t.cpu().numpy() for t in via], fuse_np.fuse(maps, rows, cols, bl.offset_per_dir, boxes, counts, 48, 48, 0.5, src.cpu().numpy()), "pipeline")
    for bad in (lambda: sf.focus(d_maps.double(), d_boxes), lambda: sf.focus(d_maps, d_boxes[:, :, :5]), lambda: sf.focus(d_maps, d_boxes, d_counts.long()),
                lambda: sf.focus(d_maps, d_boxes.cpu()), lambda: sf.focus(d_maps[:, :-1], d_boxes), lambda: sf.focus(d_maps, d_boxes, sources=src[:2])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(nat.BeamformerError, match="conf = nan is not finite|conf = -nan is not finite"):
        fuse.SensorFusion(bl, image_size=(W, H), conf=float("nan")).focus(d_maps, d_boxes)


# ------------------------------------------------------------------ 5. maps -> focus -> listen as one captured graph

def test_runs_in_a_captured_graph(nat):
    torch = util.torch_gpu()
    import fuse
    c, bl = _cfg1_listener(nat)
    W, H, F = 64, 36, 2
    sf = fuse.SensorFusion(bl, image_size=(W, H))
    batches = [_cfg1_batch(c, F, seed) for seed in (31, 32, 33)]
    d_frames, d_boxes, d_counts = (torch.from_numpy(a).cuda() for a in batches[0])

    def chain():
        maps = bl.maps(d_frames)
        peak, power, center, rects, _, counts = sf.focus(maps, d_boxes, d_counts)
        beams, status = bl.listen(d_frames, peak[:, :2])
        return peak, power, center, rects, counts, beams, status

    def eager(batch):
        for d, a in zip((d_frames, d_boxes, d_counts), batch):
            d.copy_(torch.from_numpy(a))
        out = chain()
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in out]

    eager(batches[0])                                      # the one warm-up
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = chain()
    replays = []
    for batch in batches[1:]:
        want = eager(batch)
        for t in held:
            t.fill_(-77)
        g.replay()
        torch.cuda.synchronize()
        got = [t.cpu().numpy().copy() for t in held]
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        assert (got[6] == (got[0][:, :2] < 0)).all()       # a beam for every box that has a peak, status 1 for the -1 of one that has none
        assert (got[6][:, 0] == 0).all() and np.isfinite(got[5][:, 0]).all()                # the full-frame row always has one
        replays.append(got)
    assert replays[0][0].tobytes() != replays[1][0].tobytes() and replays[0][5].tobytes() != replays[1][5].tobytes()


# ------------------------------------------------------------------ 6. end to end: a box around each of two sources

def test_boxes_hear_their_sources(nat, oracle_lib):
    """separate_np.SCENE (41 x 23, source A and source B 10 dB below it; the second frame swaps them), one hand-made box on a
    640 x 360 frame around each source's true direction (its pixel set enlarged by two cells), row 0 around the strong one.
    The strong source's box peaks within Chebyshev distance 1 of that source (the bound test_separate_finds_the_weak_source allows
    the strong source), and the loudest source of the plain map (`sources`, k = 1) lies in that box.  The weak source's box cannot
    meet that bound on a plain map: measured on the CPU (tests/test_fuse_host.py::test_scene_boxes_on_the_plain_map), the loudest
    cell under it is the box's corner towards the strong source, at distance 2 in both frames -- the strong one's skirt.  For that
    box the restatement's own answer is the expected value."""
    torch = util.torch_gpu()
    import fuse
    import listen
    from interface import config
    s = snp.SCENE
    rows, cols, M, N = s["rows"], s["cols"], s["M"], s["N"]
    frames, table, _, plain = snp.scene_reference(oracle_lib)
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=rows, MAX_RES_Y=cols, N_TAPS=8)
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    bl = listen.BeamListener("lerp", mics=np.arange(M, dtype=np.int32))
    boxes = fuse_cases.scene_boxes(s)
    d_frames = torch.from_numpy(frames.copy()).cuda()
    d_maps = bl.maps(d_frames)
    src, _, _ = bl.sources(d_maps, k=1, radius=3, floor_rel=0.0)
    sf = fuse.SensorFusion(bl, image_size=(640, 360))
    out = sf.focus(d_maps, torch.from_numpy(boxes).cuda(), None, sources=src)
    beams, status = bl.listen(d_frames, out[0])
    torch.cuda.synchronize()
    assert d_maps.cpu().numpy().tobytes() == plain.tobytes()
    got = [t.cpu().numpy() for t in out]
    want = fuse_np.fuse(plain, rows, cols, M, boxes, None, 640, 360, 0.5, src.cpu().numpy())
    _same(got, want, "scene")
    peak, src_box = got[0], got[4]
    for f, (strong, weak) in enumerate(((s["A"], s["B"]), (s["B"], s["A"]))):
        d_strong, d_weak = snp.chebyshev(peak[f, 0], M, cols, strong), snp.chebyshev(peak[f, 1], M, cols, weak)
        print("frame %d: the strong source's box peaks %s from it, the weak source's %s from it" % (f, d_strong, d_weak))
        assert d_strong is not None and d_strong <= 1
        assert peak[f, 1] == want[0][f, 1] and peak[f, 1] >= 0
    assert src_box.tolist() == [[0], [0]]
    assert (status.cpu().numpy() == 0).all() and np.isfinite(beams.cpu().numpy()).all()
