"""Cases for bf_track_boxes_device shared by the host tests (restatement against float64) and the GPU tests (device against the
restatement): CASES[name]() -> dict(boxes float32 [F, max_boxes, 6], n int32 [F] or None, slots, kw, state or None).  The shapes
are the smallest that reach each branch of the definition; `reference(name)` computes the restatement once per case and keeps it."""
import numpy as np

import box_track_np as bt

_row = lambda x1, y1, x2, y2, score=0.9, cls=0.0: (x1, y1, x2, y2, score, cls)


def _frames(rows_per_frame, max_boxes):
    F = len(rows_per_frame)
    boxes = np.zeros((F, max_boxes, 6), dtype=np.float32)
    n = np.zeros(F, dtype=np.int32)
    for f, rows in enumerate(rows_per_frame):
        for j, r in enumerate(rows):
            boxes[f, j] = r
        n[f] = len(rows)
    return boxes, n


def shortcut():
    """a. F = 40, three well separated walkers, their score order rotating: every frame pairs off without the assignment."""
    objs = [lambda f: (100.0 + 4 * f, 120.0 + f, 60.0, 90.0), lambda f: (420.0 - 3 * f, 300.0, 110.0, 70.0), lambda f: (300.0, 520.0 - 2 * f, 50.0, 50.0 + f)]
    boxes, n, _ = bt.scene_rows(40, 5, objs, seed=1, jitter=1.5, score=lambda f, k: 0.4 + 0.15 * ((k + f // 5) % 3))
    return dict(boxes=boxes, n=n, slots=4, kw={}, state=None)


def crossing():
    """b. Two objects side by side (IoU 0.45 with each other) and a third far away: each of the two tracks has two detections over
    the threshold and each of those detections two tracks, so every frame after the first runs the assignment."""
    objs = [lambda f: (140.0 + 2 * f, 140.0, 80.0, 80.0), lambda f: (170.0 + 2 * f, 141.0 + f, 80.0, 80.0), lambda f: (500.0, 400.0 - 3 * f, 60.0, 100.0)]
    boxes, n, _ = bt.scene_rows(12, 4, objs, seed=2, jitter=1.0, score=lambda f, k: 0.5 + 0.1 * ((k + f) % 3))
    return dict(boxes=boxes, n=n, slots=5, kw={}, state=None)


def tie_shortcut():
    """c. A track at exactly (0, 0, 64, 64) and a detection (0, 0, 128, 128): 4096 / ((16384 + 4096) - 4096) == 0.25f == the
    threshold.  Nothing is over the threshold, the frame takes the shortcut, and the pair is NOT matched."""
    boxes, n = _frames([[_row(0, 0, 64, 64), _row(300, 300, 364, 364, 0.8)],
                        [_row(0, 0, 128, 128), _row(300, 300, 364, 364, 0.8)]], 4)
    return dict(boxes=boxes, n=n, slots=4, kw=dict(iou_threshold=0.25, max_age=2, min_hits=0), state=None)


def tie_assignment():
    """c. The same pair while the other track has two detections over the threshold: the assignment runs and KEEPS the pair."""
    boxes, n = _frames([[_row(0, 0, 64, 64), _row(300, 300, 364, 364, 0.8)],
                        [_row(0, 0, 128, 128), _row(300, 300, 364, 364, 0.8), _row(304, 300, 368, 364, 0.7)]], 4)
    return dict(boxes=boxes, n=n, slots=4, kw=dict(iou_threshold=0.25, max_age=2, min_hits=0), state=None)


def crowded():
    """d. Five objects for three slots: two detections are dropped in every frame; object 1 leaves after frame 5, its track dies
    max_age frames later, and the frame after that the first dropped object takes the freed slot (the lowest free one)."""
    objs = [lambda f, k=k: None if (k == 1 and f > 5) else (80.0 + 120 * k, 100.0 + 40 * k + 2 * f, 70.0, 70.0) for k in range(5)]
    boxes, n, _ = bt.scene_rows(14, 6, objs, seed=3, jitter=1.0)
    return dict(boxes=boxes, n=n, slots=3, kw={}, state=None)


def hostile():
    """e. Two honest walkers among rows that are not detections: NaN and infinite coordinates, x2 <= x1, y2 <= y1, a NaN score, an
    infinite score, a score equal to conf and one below it, rows at and beyond n_boxes, and n_boxes of 0, negative and > max_boxes."""
    F, B = 12, 8
    nan, inf = np.nan, np.inf
    bad = [_row(nan, 10, 50, 60), _row(10, -inf, 50, 60), _row(10, 10, inf, 60), _row(10, 10, 50, nan), _row(50, 10, 50, 60), _row(60, 10, 50, 60),
           _row(10, 60, 50, 60), _row(10, 10, 50, 60, nan), _row(10, 10, 50, 60, inf), _row(10, 10, 50, 60, np.float32(0.1)), _row(10, 10, 50, 60, 0.05),
           _row(10, 10, 50, 60, -inf)]
    boxes = np.zeros((F, B, 6), dtype=np.float32)
    n = np.zeros(F, dtype=np.int32)
    for f in range(F):
        a = _row(100 + 3 * f, 100, 180 + 3 * f, 220, 0.7, 1.0)
        b = _row(400, 300 - 2 * f, 500, 360 - 2 * f, 0.6, 2.0)
        rows = [bad[(2 * f) % len(bad)], a, bad[(2 * f + 1) % len(bad)], b, bad[(f + 5) % len(bad)]]
        beyond = _row(250, 250, 330, 330, 0.95)               # a perfectly good box where the count says there is none
        rows += [beyond] * (B - len(rows))
        boxes[f] = rows
        n[f] = 5
    n[3], n[4], n[5], n[6], n[7] = 0, -3, B + 7, B, 2         # none; none; every row, `beyond` included; the same; the first walker only
    n[8] = 2 ** 31 - 1
    n[9] = -2 ** 31
    return dict(boxes=boxes, n=n, slots=4, kw=dict(max_age=2, min_hits=1), state=None)


def shrinking():
    """f. A box whose area collapses (ds far below zero) and which then goes undetected: coasting, ds + s <= 0 and ds is set to 0.
    Slot 1 of the carried state holds a track whose area is negative: its box is NaN and the slot is freed in the first frame."""
    side = lambda f: 200.0 * 0.55 ** f
    objs = [lambda f: (300.0, 300.0, side(f), side(f)) if f < 5 else None, lambda f: (520.0, 100.0 + f, 60.0, 40.0)]
    boxes, n, _ = bt.scene_rows(10, 3, objs)
    state = np.zeros(bt.state_words(3), dtype=np.int32)
    fw = state.view(np.float32)
    state[0], state[1] = 7, 20
    b = 4 + 20 * 1
    state[b:b + 4] = (7, 0, 5, 5)
    fw[b + 4:b + 11] = (50.0, 50.0, -400.0, 1.0, 0.0, 0.0, 0.0)
    fw[b + 11:b + 18] = (2.0, 0.5, 1.0, 2.0, 0.5, 1.0, 3.0)
    return dict(boxes=boxes, n=n, slots=3, kw=dict(max_age=6, min_hits=1), state=state)


def _reporting(max_age, min_hits):
    def make():
        objs = [lambda f: (150.0 + 3 * f, 200.0, 80.0, 120.0) if f not in (6, 7) else None, lambda f: (450.0, 320.0 - 2 * f, 100.0, 60.0) if f >= 4 else None]
        boxes, n, _ = bt.scene_rows(14, 3, objs, seed=5, jitter=0.5)
        return dict(boxes=boxes, n=n, slots=3, kw=dict(max_age=max_age, min_hits=min_hits), state=None)
    make.__doc__ = "g. One track from frame 0 with a two-frame dropout, one born in frame 4: max_age %d, min_hits %d." % (max_age, min_hits)
    return make


def largest():
    """i. max_boxes = 300, all valid, slots = 64, F = 3, and the assignment at its longest.  Frame 0 fills the 64 slots with nested
    squares of side 40 + i around one centre, the smallest first.  The 300 detections of frames 1 and 2 are nested squares too, all
    larger than every track: the gain of (track i, detection j) is close to side_i^2 / side_j^2, so every row wants the smallest
    detection most and each new row, larger than all before it, takes it and pushes every earlier row one detection on: the
    augmenting path of row i visits i + 1 columns (64 rows over 300 + 64 columns, about 2000 steps per frame)."""
    rng = np.random.default_rng(9)
    F, B, S = 3, 300, 64
    boxes = np.zeros((F, B, 6), dtype=np.float32)
    for f in range(F):
        side = np.concatenate([40.0 + np.arange(S), 110.0 + 0.5 * np.arange(B - S)]) if f == 0 else rng.permutation(108.0 + 2 * f + 0.5 * np.arange(B))
        c = (300.0, 300.0) + rng.uniform(-1, 1, (B, 2))
        boxes[f, :, 0:2] = c - side[:, None] / 2
        boxes[f, :, 2:4] = c + side[:, None] / 2
        boxes[f, :, 4] = np.sort(rng.uniform(0.2, 0.95, B))[::-1]
        boxes[f, :, 5] = rng.integers(0, 3, B)
    return dict(boxes=boxes, n=np.full(F, B, dtype=np.int32), slots=64, kw={}, state=None)


def long_stream():
    """j, k. 33 frames of four walkers with dropouts; two of them converge, so the last frames need the assignment."""
    objs = [lambda f: (120.0 + 5 * f, 150.0, 70.0, 90.0), lambda f: (330.0 - 2 * f, 150.0 + f, 70.0, 90.0) if f % 9 != 4 else None,
            lambda f: (480.0 - 6 * f, 160.0 + f, 76.0, 84.0), lambda f: (520.0, 480.0 - 4 * f, 40.0, 60.0) if 6 <= f < 27 else None]
    boxes, n, _ = bt.scene_rows(33, 6, objs, seed=11, jitter=1.0, score=lambda f, k: 0.3 + 0.2 * ((k + f // 3) % 4))
    return dict(boxes=boxes, n=n, slots=5, kw=dict(max_age=2, min_hits=2), state=None)


CASES = dict(shortcut=shortcut, crossing=crossing, tie_shortcut=tie_shortcut, tie_assignment=tie_assignment, crowded=crowded, hostile=hostile,
             shrinking=shrinking, largest=largest, long_stream=long_stream)
for _a in (1, 3):
    for _h in (0, 1, 3):
        CASES["reporting_age%d_hits%d" % (_a, _h)] = _reporting(_a, _h)

_cache = {}


def reference(name):
    """-> (case, the restatement's six outputs, the list of branches it went through); computed once, never modified by a test."""
    if name not in _cache:
        c = CASES[name]()
        br = []
        want = bt.track_boxes_np(c["boxes"], c["n"], c["slots"], state=c["state"], branches=br, **c["kw"])
        for a in want:
            a.setflags(write=False)
        _cache[name] = (c, want, br)
    return _cache[name]


def check_reaches(name, want, br):
    """Each case reaches what it is there for (asserted on the restatement, which both test files trust)."""
    tracks, ids, match, live, counts, state = want
    tot = counts.sum(axis=0)
    if name == "shortcut":
        assert set(br) == {"none", "shortcut"} and tot[0] == 3 and tot[1] == 0 and (ids[-1] == [1, 2, 3, 0]).all() and (tracks[5:, :3, 4] > 0).all()
    if name == "crossing":
        assert br.count("assignment") == len(br) - 1 and tot[0] == 3 and tot[1] == 0 and (match[1:, :3] >= 0).all()
    if name == "tie_shortcut":
        assert br == ["none", "shortcut"] and match[1].tolist() == [-1, 1, 0, -1] and ids[1].tolist() == [1, 2, 3, 0] and counts[1, 0] == 1
    if name == "tie_assignment":
        assert br == ["none", "assignment"] and match[1].tolist() == [0, 1, 2, -1] and ids[1].tolist() == [1, 2, 3, 0]
    if name == "crowded":
        assert (counts[:6, 2] == 2).all() and tot[1] == 1
        f = int(np.flatnonzero(counts[:, 1])[0])
        assert counts[f + 1, 0] == 1 and ids[f + 1, 1] == 4 and ids[f, 1] == 2 and (counts[f + 1:, 2] == 1).all()
    if name == "hostile":
        assert counts[:, 3].tolist() == [3, 3, 3, 0, 0, 3, 3, 1, 3, 0] + [3, 3] and counts[:, 2].tolist() == [0] * 5 + [1, 1, 0, 1, 0, 0, 0] and ids[5].tolist() == [1, 2, 3, 4]
    if name == "shrinking":
        assert "clamp" in br and br.count("freed") == 1 and counts[0, 1] == 1 and ids[0].tolist() == [8, 9, 0] and state[0] == 9 and state[1] == 30
    if name == "largest":
        assert br == ["none", "assignment", "assignment"] and counts[0].tolist() == [64, 0, 236, 0] and (match[1] >= 0).sum() >= 30 and counts[2, 1] > 0
    if name == "long_stream":
        assert "assignment" in br and "shortcut" in br and tot[0] >= 4 and tot[1] >= 1
    if name.startswith("reporting"):
        min_hits, max_age = c_kw(name)
        early = tracks[:, :, 4] > 0
        assert early[0, 0] and ids[4, 1] == 2                                                   # frame_count 1 <= min_hits, or min_hits 0
        assert early[4 + min_hits, 1] and not early[4:4 + min_hits, 1].any()                    # the later birth waits for its streak
        assert (ids[8, 0] == 1) == (max_age >= 3) and not early[6:8, 0].any()


def c_kw(name):
    kw = CASES[name]()["kw"]
    return kw["min_hits"], kw["max_age"]
