"""GPU (-m gpu): bf_track_sources_device, identity over time for bf_peaks_device's sources, EQUAL to the NumPy restatement
(tests/track_np.py).

The definition fixes every float32 operation and its order, so every output and the state words are compared as bytes."""
import numpy as np
import pytest

import track_np
import util
from support import nat

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F, TAIL = -77, -123.5, 16
NAMES = ("offsets", "ids", "pos", "match", "counts", "state")


def _call(nat, offs, rows, cols, per, slots, gate=3.0, max_miss=5, min_hits=3, q=0.1, r=0.1, state=None, optional=True):
    """bf_track_sources_device into sentinel-filled buffers with a tail -> (offsets, ids, pos, match, counts, state) as host arrays
    (None for the optional outputs when optional is False); the tails, the state's included, are checked here."""
    torch = util.torch_gpu()
    F, k = offs.shape
    words = track_np.state_words(slots)
    d_in = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int32)).cuda()
    d_state = torch.full((words + TAIL,), SENTINEL_I, dtype=torch.int32, device="cuda")
    d_state[:words] = 0 if state is None else torch.from_numpy(np.asarray(state, dtype=np.int32)).cuda()
    sizes = (F * slots, F * slots, F * slots * 4, F * slots, F * 4)
    bufs = [torch.full((n + TAIL,), SENTINEL_F if i == 2 else SENTINEL_I, dtype=torch.float32 if i == 2 else torch.int32, device="cuda")
            if (optional or i == 0) else None for i, n in enumerate(sizes)]
    ptr = [b.data_ptr() if b is not None else None for b in bufs]
    rc = nat.lib.bf_track_sources_device(d_in.data_ptr(), F, k, rows, cols, per, slots, gate, max_miss, min_hits, q, r, d_state.data_ptr(),
                                         ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    out = []
    shapes = ((F, slots), (F, slots), (F, slots, 4), (F, slots), (F, 4))
    for b, n, shape in zip(bufs, sizes, shapes):
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy()
        assert (h[n:] == h.dtype.type(SENTINEL_F if h.dtype == np.float32 else SENTINEL_I)).all()
        out.append(h[:n].reshape(shape))
    h = d_state.cpu().numpy()
    assert (h[words:] == SENTINEL_I).all()
    out.append(h[:words])
    return out


# ------------------------------------------------------------------ 1. parity with the restatement, one case per branch

def _random_scene(seed, F, k, rows, cols, per, fill=0.5):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, rows * cols, (F, k))
    return np.where(rng.uniform(0, 1, (F, k)) < fill, d * per, -1).astype(np.int32)


def _crowded_row(F=33, k=7, cols=50, per=2):
    """Five sources drifting along a one-row grid (more than the three slots), the columns rotated every frame, now and then a hole."""
    rng = np.random.default_rng(77)
    offs = np.full((F, k), -1, dtype=np.int32)
    for f in range(F):
        ys = [3 + f // 8, 14, 25 - f // 6, 36, 47]
        ys = [y for y in ys if rng.uniform() > 0.15]
        for j, y in enumerate(ys):
            offs[f, (j + f) % k] = y * per
    return offs


def _large_offsets(F=20, k=5, rows=361, cols=361, per=256):
    """Three walkers far out on a 361 x 361 grid at offset_per_dir 256, with -1, non-multiples and d >= rows*cols mixed in."""
    rng = np.random.default_rng(5)
    pos = np.array([[350, 355], [10, 300], [180, 7]])
    offs = np.full((F, k), -1, dtype=np.int32)
    for f in range(F):
        pos = np.clip(pos + rng.integers(-2, 3, pos.shape), 0, rows - 1)
        cols_used = rng.permutation(k)
        for j, (x, y) in zip(cols_used, pos):
            offs[f, j] = (x * cols + y) * per
        spare = cols_used[3:]
        offs[f, spare[0]] = [-1, (pos[0, 0] * cols + pos[0, 1]) * per + 7, (rows * cols + f) * per][f % 3]
        offs[f, spare[1]] = [(rows * cols) * per, -1, 129][f % 3]
    assert offs.max() > rows * cols * per
    return offs


CASES = {
    # name: (offsets, rows, cols, offset_per_dir, slots, keyword arguments)
    "scripted": lambda: (track_np.scripted_scene(40, 4, 41, 23, 3), 41, 23, 3, 4, {}),
    "dense_ties": lambda: (_random_scene(1, 64, 64, 16, 16, 5), 16, 16, 5, 64, dict(gate=2.0, max_miss=2, min_hits=2)),
    "crowded_row": lambda: (_crowded_row(), 1, 50, 2, 3, dict(gate=2.5, max_miss=1, min_hits=2)),
    "large_offsets": lambda: (_large_offsets(), 361, 361, 256, 5, dict(gate=4.0)),
    "gate_0": lambda: (_random_scene(2, 24, 8, 6, 6, 1, 0.7), 6, 6, 1, 8, dict(gate=0.0, max_miss=2, min_hits=2)),
    "max_miss_0": lambda: (_random_scene(3, 24, 8, 6, 6, 1, 0.7), 6, 6, 1, 8, dict(gate=1.5, max_miss=0, min_hits=2)),
    "min_hits_1": lambda: (_random_scene(4, 24, 8, 6, 6, 1, 0.7), 6, 6, 1, 8, dict(gate=1.5, max_miss=1, min_hits=1)),
    "q_0": lambda: (track_np.scripted_scene(40, 4, 41, 23, 3), 41, 23, 3, 2, dict(q=0.0, r=0.5, gate=5.0)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_restatement(nat, case):
    offs, rows, cols, per, slots, kw = CASES[case]()
    got = _call(nat, offs, rows, cols, per, slots, **kw)
    want = track_np.track(offs, rows, cols, per, slots, **kw)
    counts = want[4].sum(axis=0)
    print(case, "born/ended/dropped/ignored", counts.tolist(), "matches", int((want[3] >= 0).sum()), "next_id", int(want[5][0]))
    util.same_named(NAMES, got, want, case)
    # each case reaches what it is there for
    if case == "dense_ties":
        assert counts[1] > 0 and counts[2] > 0 and (want[3] >= 0).sum(axis=1).max() > 32
    if case == "crowded_row":
        assert counts[2] > 0
    if case == "large_offsets":
        assert (want[4][:, 3] == 2).all() and want[0].max() > 2 ** 24 and counts[0] >= 3
    if case == "gate_0":
        assert (want[3] >= 0).sum() > counts[0]                                  # exact hits did continue tracks


# ------------------------------------------------------------------ 2. the state carries from call to call

def test_state_carry(nat):
    offs = track_np.scripted_scene(40, 4, 41, 23, 3)
    whole = _call(nat, offs, 41, 23, 3, 4)
    first = _call(nat, offs[:20], 41, 23, 3, 4)
    assert first[5][0] > 0 and first[5][4] != 0                                   # tracks are alive at the cut
    second = _call(nat, offs[20:], 41, 23, 3, 4, state=first[5])
    for name, w, a, b in zip(NAMES, whole[:5], first[:5], second[:5]):
        assert w.tobytes() == np.concatenate([a, b]).tobytes(), name
    assert whole[5].tobytes() == second[5].tobytes()


# ------------------------------------------------------------------ 3. optional outputs

def test_null_outputs_and_repeatability(nat):
    offs = _random_scene(9, 30, 12, 12, 12, 4)
    kw = dict(gate=2.0, max_miss=2, min_hits=2)
    warm = _call(nat, offs[:10], 12, 12, 4, 6, **kw)
    full = _call(nat, offs[10:], 12, 12, 4, 6, state=warm[5], **kw)
    again = _call(nat, offs[10:], 12, 12, 4, 6, state=warm[5], **kw)
    bare = _call(nat, offs[10:], 12, 12, 4, 6, state=warm[5], optional=False, **kw)
    for x, y in zip(full, again):
        assert x.tobytes() == y.tobytes()
    assert bare[1] is None and bare[4] is None
    assert bare[0].tobytes() == full[0].tobytes() and bare[5].tobytes() == full[5].tobytes()


# ------------------------------------------------------------------ 4. graph capture from the first call

def test_runs_in_a_captured_graph(nat):
    torch = util.torch_gpu()
    rows, cols, per, slots = 41, 23, 3, 4
    offs = track_np.scripted_scene(40, 4, rows, cols, per)
    F, k = offs.shape
    want = track_np.track(offs, rows, cols, per, slots)
    eager = _call(nat, offs, rows, cols, per, slots)        # (its own buffers; also brings the library's device up outside the capture)
    util.same_named(NAMES, eager, want, "eager")
    # a shape no call has had before: this launch is captured without a warm-up of its own
    slots2 = 5
    want2 = track_np.track(offs, rows, cols, per, slots2)
    d_in = torch.from_numpy(offs).cuda()
    d_state = torch.zeros((track_np.state_words(slots2),), dtype=torch.int32, device="cuda")
    d_o, d_i, d_m = (torch.full((F, slots2), SENTINEL_I, dtype=torch.int32, device="cuda") for _ in range(3))
    d_p = torch.full((F, slots2, 4), SENTINEL_F, dtype=torch.float32, device="cuda")
    d_c = torch.full((F, 4), SENTINEL_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert nat.lib.bf_track_sources_device(d_in.data_ptr(), F, k, rows, cols, per, slots2, 3.0, 5, 3, 0.1, 0.1, d_state.data_ptr(), d_o.data_ptr(),
                                               d_i.data_ptr(), d_p.data_ptr(), d_m.data_ptr(), d_c.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    for _ in range(2):
        d_state.zero_()
        for t in (d_o, d_i, d_m, d_c):
            t.fill_(SENTINEL_I)
        d_p.fill_(SENTINEL_F)
        g.replay()
        torch.cuda.synchronize()
        util.same_named(NAMES, [t.cpu().numpy() for t in (d_o, d_i, d_p, d_m, d_c, d_state)], want2, "graph replay")


# ------------------------------------------------------------------ 5. the front end: sources -> SourceTracker

def test_tracker_front_end(nat):
    torch = util.torch_gpu()
    import listen
    import track
    util.configure("cfg1")
    rows, cols, F = 41, 23, 24
    bl = listen.BeamListener("pad", mics=np.arange(5))
    x, y = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    bump = lambda cx, cy: np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / 8.0).ravel()
    a, b = bump(10, 6), bump(30, 15)
    level = np.linspace(0.5, 1.5, F)                                              # B passes A (level 1) between frames 11 and 12
    maps = np.stack([a + l * b for l in level]).astype(np.float32)
    d_maps = torch.from_numpy(maps).cuda()
    src, _, cnt = bl.sources(d_maps, k=4, radius=4, floor_rel=0.25, shape=(rows, cols))
    tr = track.SourceTracker(bl, slots=4, min_hits=2, shape=(rows, cols))
    assert tr.state.dtype == torch.int32 and tr.state.shape == (52,) and tr.state.is_cuda and not tr.state.any()
    offsets, ids, pos, match, counts = tr.update(src)
    torch.cuda.synchronize()
    assert offsets.shape == (F, 4) and offsets.dtype == torch.int32 and pos.shape == (F, 4, 4) and pos.dtype == torch.float32 and counts.shape == (F, 4)
    src_h = src.cpu().numpy()
    got = [t.cpu().numpy() for t in (offsets, ids, pos, match, counts, tr.state)]
    per = bl.offset_per_dir
    da, db = (10 * cols + 6) * per, (30 * cols + 15) * per
    assert (cnt.cpu().numpy()[:, 0] == 2).all()
    assert (src_h[:12, 0] == da).all() and (src_h[12:, 0] == db).all()            # sources' slot 0 changes direction at the crossing
    assert (got[0][1:, 0] == da).all() and (got[0][1:, 1] == db).all()            # the tracker's does not (confirmed from frame 1 on)
    assert (got[0][0] == -1).all() and (got[0][:, 2:] == -1).all()
    assert (got[1][:, 0] == 1).all() and (got[1][:, 1] == 2).all() and (got[1][:, 2:] == 0).all()
    assert (got[3][:12, 0] == 0).all() and (got[3][12:, 0] == 1).all()
    want = track_np.track(src_h, rows, cols, per, 4, min_hits=2)
    util.same_named(NAMES, got, want, "front end")
    # a second batch continues the tracks; reset forgets them
    offsets2, ids2, _, _, counts2 = tr.update(src[-3:])
    torch.cuda.synchronize()
    assert (ids2.cpu().numpy()[:, :2] == [1, 2]).all() and not counts2.cpu().numpy()[:, :3].any()
    tr.reset()
    _, ids3, _, _, counts3 = tr.update(src[-3:])
    torch.cuda.synchronize()
    assert (ids3.cpu().numpy()[:, :2] == [1, 2]).all() and counts3.cpu().numpy()[0].tolist() == [2, 0, 0, 2]
    with pytest.raises(ValueError):
        tr.update(src.to(torch.int64))
    with pytest.raises(ValueError):
        track.SourceTracker(bl, slots=65)
    with pytest.raises(nat.BeamformerError, match="min_hits = 0 < 1"):
        track.SourceTracker(bl, min_hits=0).update(src)


# ------------------------------------------------------------------ 6. end to end: maps -> sources -> tracker -> listen

def test_tracked_beams_follow_one_source(nat):
    """Two plane waves at the as-shipped size, the second one scaled per frame so that the louder of the two alternates: `sources`
    swaps them from frame to frame, the tracker's slots do not, and each slot's beam is bf_miso_device's at that source's offset."""
    torch = util.torch_gpu()
    import listen
    import synth
    import track
    from test_peaks import two_source_frame
    c = util.configure("shipped")
    M, N, X, Y = c["M"], c["N"], c["X"], c["Y"]
    mics = np.arange(M, dtype=np.int32)
    table = util.table_for("lerp", "shipped")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    base = two_source_frame()                                                      # (19, 21) + 0.7 x (42, 8)
    louder = np.ascontiguousarray(base + np.float32(0.7) * synth.s3_plane_wave(util.oracle_delays("shipped")[42, 8], N, seed=2), dtype=np.float32)
    F = 8
    frames = np.stack([louder if f % 2 else base for f in range(F)])
    d_frames = torch.from_numpy(frames).cuda()
    bl = listen.BeamListener("lerp", mics=mics)
    tr = track.SourceTracker(bl, slots=4, min_hits=1)
    src, _, _ = bl.sources(bl.maps(d_frames), k=4, radius=4, floor_rel=0.25)
    offsets, ids, pos, match, counts = tr.update(src)
    out, status = bl.listen(d_frames, offsets)
    raw, _ = bl.listen(d_frames, src)
    d1, d2 = (19 * Y + 21) * M, (42 * Y + 8) * M
    fixed, fixed_status = bl.listen(d_frames, torch.tensor([d1, d2], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    src, offsets, ids, match, status, out, raw, fixed = (t.cpu().numpy() for t in (src, offsets, ids, match, status, out, raw, fixed))
    print("sources", (src[:, :2] // M).tolist(), "tracked", (offsets[:, :2] // M).tolist(), "match", match[:, :2].tolist())
    assert (fixed_status.cpu().numpy() == 0).all()
    for f in range(F):
        assert src[f].tolist() == ([d2, d1, -1, -1] if f % 2 else [d1, d2, -1, -1])
    assert (offsets == np.array([d1, d2, -1, -1])).all() and (ids == np.array([1, 2, 0, 0])).all()
    assert (status == np.array([0, 0, 1, 1])).all()
    assert out[:, :2].tobytes() == fixed.tobytes()                                # slot b is ONE source in every frame
    assert np.isnan(out[:, 2:]).all()
    assert raw[::2, :2].tobytes() == fixed[::2].tobytes()
    for f in range(1, F, 2):                                                       # the raw slots are swapped in every second frame
        assert raw[f, 0].tobytes() == fixed[f, 1].tobytes() and raw[f, 0].tobytes() != fixed[f, 0].tobytes()
    assert raw[:, :2].tobytes() != fixed.tobytes()
