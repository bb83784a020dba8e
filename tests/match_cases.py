"""The case table of bf_match_boxes_device and bf_smooth_boxes_device, shared by the host tests (which run the NumPy restatement and
check that every case reaches the branch it is named for) and the GPU tests (which compare the device's bytes with it).

A match case is dict(images uint8 [F, H, W, 3], prev uint8 [H, W, 3] or None, boxes float32 [F, B, 4], t_pct, s_pct, check);
check(want, info) asserts on the restatement's outputs (moved, score, shift, status) and on its notes, one per box that reached the
sums.  Images are 96 x 128 with F = 3 and 6 rows unless the case needs otherwise."""
import functools

import numpy as np

import match_np as mn

H, W, F, B = 96, 128, 3, 6
ONE = np.float32(1.0).view(np.int32)


def texture(seed, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def roll(img, dx, dy):
    return np.roll(img, (dy, dx), axis=(0, 1))


def rolled_stream(seed, dx, dy, frames=F, h=H, w=W):
    """prev, and `frames` images each the one before it rolled by (dx, dy)."""
    prev = texture(seed, h, w)
    images, cur = [], prev
    for _ in range(frames):
        cur = roll(cur, dx, dy)
        images.append(cur)
    return prev, np.stack(images)


def same_rows(rows, frames=F):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(rows, dtype=np.float32), (frames, len(rows), 4)))


INTERIOR = [(40, 30, 80, 70), (20.7, 10.2, 50.9, 44.5), (60, 20, 100, 50), (30.5, 40.5, 61.25, 75.75), (70, 35, 95, 68), (44, 22, 66, 60)]


def case_rolled():
    prev, images = rolled_stream(1, 3, -2)

    def check(want, info):
        moved, score, shift, status = want
        assert not status.any() and (shift == (3, -2)).all() and (score.view(np.int32) == ONE).all()
        assert all(n["q"] == 1 and n["nu"] > 1 and n["nv"] > 1 for n in info)
    return dict(images=images, prev=prev, boxes=same_rows(INTERIOR), t_pct=120, s_pct=150, check=check)


def case_borders():
    """Boxes clipped at each of the four borders (and at a corner), and boxes wholly outside."""
    prev, images = rolled_stream(2, 1, 1)
    rows = [(-10, 30, 22, 60), (30, -12, 70, 20), (100, 30, 140, 66), (40, 70, 80, 110), (200, 10, 240, 50), (-60, -60, -20, -20)]

    def check(want, info):
        moved, score, shift, status = want
        assert (status == [0, 0, 0, 0, 2, 2]).all()
        assert not moved[:, 4:].any() and not score[:, 4:].any() and not shift[:, 4:].any()
        notes = info[:4]
        assert notes[0]["dx0"] == 0 and notes[1]["dy0"] == 0                        # clipped left / top: no room before the template
        assert notes[2]["sw"] - notes[2]["tw"] == notes[2]["dx0"] and notes[3]["sh"] - notes[3]["th"] == notes[3]["dy0"]   # right / bottom: none after
    return dict(images=images, prev=prev, boxes=same_rows(rows), t_pct=120, s_pct=150, check=check)


def case_hostile():
    """Rows that are no box: NaN, Inf, 2^20, inverted, zero width after truncation; one good row between them."""
    prev, images = rolled_stream(3, -2, 1)
    rows = [(np.nan, 30, 80, 70), (40, 30, np.inf, 70), (40, 30, 2.0 ** 20, 70), (80, 30, 40, 70), (40.2, 30, 40.9, 70), (40, 30, 80, 70)]

    def check(want, info):
        moved, score, shift, status = want
        assert (status == [1, 1, 1, 1, 1, 0]).all() and not moved[:, :5].any() and (shift[:, 5] == (-2, 1)).all()
    return dict(images=images, prev=prev, boxes=same_rows(rows), t_pct=120, s_pct=150, check=check)


def case_flat_template():
    """A 1 x 1 template (a box at the corner, clipped to one pixel) and a template inside a flat block: A == 0."""
    prev, images = rolled_stream(4, 1, 0)
    prev = prev.copy()
    prev[20:80, 30:100] = 77
    images = images.copy()
    images[:] = roll(prev, 1, 0)
    rows = [(-1, -1, 1, 1), (45, 35, 75, 60), (5, 5, 40, 40), (-1, 40, 1, 80), (45.5, 35.5, 75, 60), (90, 10, 120, 40)]

    def check(want, info):
        moved, score, shift, status = want
        assert (status == [3, 3, 0, 0, 3, 0]).all()
        assert info[0]["P"] == 1 and info[0]["status"] == 3
        rows32 = np.asarray(rows, dtype=np.float32)
        for j in (0, 1, 4):
            assert (moved[:, j] == rows32[j]).all() and not score[:, j].any() and not shift[:, j].any()
    return dict(images=images, prev=prev, boxes=same_rows(rows), t_pct=120, s_pct=150, check=check)


def case_flat_windows():
    """Flat windows inside a textured search area: their B is 0, they score 0.0 and lose to the true position."""
    prev = texture(5)
    cur = roll(prev, 2, 0).copy()
    cur[:, :40] = 200                                   # the left part of every search area is flat
    images = np.stack([cur, cur, cur])
    rows = [(44, 30, 64, 50), (46, 50, 66, 70), (44, 10, 64, 30), (45, 60, 65, 80), (44.5, 20.5, 64, 40), (47, 41, 67, 61)]

    def check(want, info):
        moved, score, shift, status = want
        assert not status.any() and (shift[0] == (2, 0)).all() and (score.view(np.int32) == ONE).all()
        assert sum(n["flat_windows"] > 0 for n in info[:B]) >= 2, [n["flat_windows"] for n in info[:B]]
    return dict(images=images, prev=prev, boxes=same_rows(rows), t_pct=120, s_pct=400, check=check)


def case_period4():
    """A texture of period 4 in x: the shifts -4, 0 and +4 tie exactly, and the first in row-major order wins."""
    base = texture(6)
    prev = np.ascontiguousarray(base[:, np.arange(W) % 4])
    images = np.stack([prev] * F)
    rows = [(40, 30, 80, 70), (20.7, 10.2, 50.9, 44.5), (60, 20, 100, 50), (30.5, 40.5, 61.25, 75.75), (70, 35, 102, 68), (44, 22, 80, 60)]   # every dx0 >= 4

    def check(want, info):
        moved, score, shift, status = want
        assert not status.any() and (score.view(np.int32) == ONE).all()
        assert (shift[:, :, 1] == 0).all() and (shift[:, :, 0] % 4 == 0).all() and (shift[:, :, 0] < 0).all()
        for n in info:
            assert (n["r"] == n["r"].max()).sum() >= 2                      # an exact tie, not a near one
    return dict(images=images, prev=prev, boxes=same_rows(rows), t_pct=120, s_pct=150, check=check)


def case_inverted():
    """A smooth blob and its negative: every position scores below zero, and the greatest is still chosen."""
    y, x = np.mgrid[0:H, 0:W]
    blob = 20 + 200 * np.exp(-((x - 62.0) ** 2 + (y - 48.0) ** 2) / (2 * 26.0 ** 2))
    prev = np.stack([blob, 0.8 * blob + 9, 0.6 * blob + 30], axis=2).astype(np.uint8)
    images = np.stack([255 - prev, roll(255 - prev, 1, 1), roll(255 - prev, 2, 2)])

    def check(want, info):
        moved, score, shift, status = want
        assert not status[0].any() and (score[0] < 0).all()
        assert all(n["r"].max() < 0 for n in info[:B])
    rows = [(42, 28, 82, 68), (44.5, 30.5, 80, 66), (50, 36, 74, 60), (40, 30, 70, 60), (55, 40, 85, 70), (48, 26, 78, 50)]
    return dict(images=images, prev=prev, boxes=same_rows(rows), t_pct=120, s_pct=150, check=check)


def case_one_position():
    prev, images = rolled_stream(8, 1, -1)

    def check(want, info):
        moved, score, shift, status = want
        assert not status.any() and not shift.any() and all(n["nu"] == 1 and n["nv"] == 1 for n in info)
        assert (np.abs(score) < 0.5).all()
    return dict(images=images, prev=prev, boxes=same_rows(INTERIOR), t_pct=130, s_pct=130, check=check)


def case_wide_search():
    """t_pct = 100, s_pct = 400 on 260 x 300: a 240 x 240 search area (169 KiB), beyond any LDS staging."""
    prev, images = rolled_stream(9, -37, 52, frames=1, h=260, w=300)

    def check(want, info):
        moved, score, shift, status = want
        n = info[0]
        assert n["sw"] * n["sh"] * 3 > 160 * 1024 and n["nu"] == 181 and n["nv"] == 181 and n["q"] == 1
        assert status[0, 0] == 0 and tuple(shift[0, 0]) == (-37, 52) and score.view(np.int32)[0, 0] == ONE
    return dict(images=images, prev=prev, boxes=same_rows([(120, 100, 180, 160)], 1), t_pct=100, s_pct=400, check=check)


def case_decimated_q2():
    """A 200 x 200 box on 260 x 300: q = 2, P = 14400; a roll by (-6, 4) lies on the lattice and is found exactly."""
    prev, images = rolled_stream(10, -6, 4, frames=1, h=260, w=300)

    def check(want, info):
        n = info[0]
        assert n["q"] == 2 and n["P"] == 14400 and want[3][0, 0] == 0
        assert tuple(want[2][0, 0]) == (-6, 4) and want[1].view(np.int32)[0, 0] == ONE
    return dict(images=images, prev=prev, boxes=same_rows([(50, 30, 250, 230)], 1), t_pct=120, s_pct=150, check=check)


def case_decimated_q3():
    """An elongated box: q = 3, pw != ph, tw not a multiple of q, and a zero displacement that is not a multiple of q either."""
    prev, images = rolled_stream(11, 3, -3, frames=1, h=260, w=300)

    def check(want, info):
        n = info[0]
        assert n["q"] == 3 and n["pw"] != n["ph"] and n["tw"] % 3 and n["dx0"] % 3 and n["dy0"] % 3
        assert want[3][0, 0] == 0 and tuple(want[2][0, 0]) == (3, -3) and want[1].view(np.int32)[0, 0] == ONE
    return dict(images=images, prev=prev, boxes=same_rows([(5, 15, 295, 245)], 1), t_pct=100, s_pct=110, check=check)


def case_x_bound():
    """An all-255 image with a single 0 pixel inside a template of exactly 16384 pixels: X next to its 32-bit bound."""
    prev = np.full((260, 300, 3), 255, dtype=np.uint8)
    prev[52, 62] = 0
    images = prev[None].copy()

    def check(want, info):
        n = info[0]
        assert n["q"] == 1 and n["P"] == 16384 and n["X_max"] == (16384 - 1) * 3 * 255 ** 2 and n["X_max"] > 2 ** 31 and n["flat_windows"] > 0
        assert want[3][0, 0] == 0 and not want[2].any() and want[1].view(np.int32)[0, 0] == ONE
    return dict(images=images, prev=prev, boxes=same_rows([(60, 50, 188, 178)], 1), t_pct=100, s_pct=120, check=check)


def case_no_previous_image():
    c = case_rolled()

    def check(want, info):
        moved, score, shift, status = want
        assert (status[0] == 4).all() and not moved[0].any() and not score[0].any() and not status[1:].any() and (shift[1:] == (3, -2)).all()
    return dict(c, prev=None, check=check)


CASES = dict(rolled=case_rolled, borders=case_borders, hostile=case_hostile, flat_template=case_flat_template, flat_windows=case_flat_windows,
             period4=case_period4, inverted=case_inverted, one_position=case_one_position, wide_search=case_wide_search,
             decimated_q2=case_decimated_q2, decimated_q3=case_decimated_q3, x_bound=case_x_bound, no_previous_image=case_no_previous_image)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, the restatement's outputs, its notes): computed once and shared; nobody writes to them."""
    c = CASES[name]()
    info = []
    want = mn.match_boxes_np(c["images"], c["prev"], c["boxes"], None, c["t_pct"], c["s_pct"], info)
    return c, want, info


# ------------------------------------------------------------------ the hysteresis

def _state(rows, slots):
    s = np.zeros(4 + 4 * slots, dtype=np.int32)
    s[0] = len(rows)
    s[4:4 + 4 * len(rows)] = np.asarray(rows, dtype=np.float32).ravel().view(np.int32)
    return s


def _smooth_case(boxes, prev_rows, moved, score, status, slots=4, n=None, want_kind=None, **kw):
    S = slots
    mv, sc, st = np.zeros((S, 4), np.float32), np.zeros(S, np.float32), np.ones(S, np.int32)
    k = len(moved)
    if k:
        mv[:k], sc[:k], st[:k] = np.asarray(moved, np.float32), np.asarray(score, np.float32), np.asarray(status, np.int32)
    return dict(boxes=np.asarray(boxes, dtype=np.float32), n=n, state=_state(prev_rows, S), moved=mv, score=sc, status=st, slots=S, kw=kw, want_kind=want_kind)


P0 = (0, 0, 10, 10)
SMOOTH_CASES = {
    # scores above conf_high exist: they are kept, everything else goes to zero, the previous boxes play no part
    "valid_branch": lambda: _smooth_case([(0, 0, 10, 10, 0.9, 1), (20, 20, 30, 30, 0.5, 2), (0, 0, 10, 10, 0.71, 3), (5, 5, 8, 8, 0.2, 0)], [P0], [P0], [0.99], [0],
                                         want_kind=dict(out=[0.9, 0, 0.71, 0], boosted=[0, 0, 0, 0], counts=[2, 1, 0, 0], m=2)),
    # overlap only: the moved box covers the first candidate and not the second; the correlation is below corr
    "boost_by_overlap": lambda: _smooth_case([(1, 1, 11, 11, 0.5, 1), (40, 40, 50, 50, 0.5, 2), (1, 1, 11, 11, 0.3, 3)], [P0], [(1, 0, 11, 10)], [0.5], [0],
                                             want_kind=dict(out=[0.7, 0, 0], boosted=[1, 0, 0], counts=[0, 2, 1, 0], m=1)),
    # correlation only: nothing overlaps, one previous box correlates above corr, and EVERY candidate is boosted
    "boost_by_correlation": lambda: _smooth_case([(60, 60, 70, 70, 0.5, 1), (40, 40, 50, 50, 0.31, 2), (1, 1, 11, 11, 0.3, 3)], [P0, P0], [P0, P0], [0.5, 0.81], [0, 0],
                                                 want_kind=dict(out=[0.7, 0.7, 0], boosted=[1, 1, 0], counts=[0, 2, 2, 0], m=2)),
    "not_boosted": lambda: _smooth_case([(60, 60, 70, 70, 0.5, 1), (40, 40, 50, 50, 0.31, 2)], [P0], [P0], [0.8], [0],
                                        want_kind=dict(out=[0, 0], boosted=[0, 0], counts=[0, 2, 0, 0], m=0)),
    # score == conf_high is a candidate, not valid (float32(0.7) against the float32 threshold)
    "score_equals_conf_high": lambda: _smooth_case([(0, 0, 10, 10, 0.7, 1)], [P0], [P0], [0.1], [0],
                                                   want_kind=dict(out=[0.7], boosted=[1], counts=[0, 1, 1, 0], m=1)),
    # IoU == iou_threshold exactly (50 / 100) does not boost; 60 / 100 does
    "iou_equals_threshold": lambda: _smooth_case([(0, 0, 10, 5, 0.5, 1), (0, 0, 10, 6, 0.5, 2)], [P0], [P0], [0.1], [0],
                                                 want_kind=dict(out=[0, 0.7], boosted=[0, 1], counts=[0, 2, 1, 0], m=1)),
    # previous rows whose match failed (status != 0) or that lie beyond m are ignored, whatever their score and box
    "failed_matches_ignored": lambda: _smooth_case([(0, 0, 10, 10, 0.5, 1)], [P0, P0], [P0, P0, P0], [0.99, 0.99, 0.99], [3, 2, 0],
                                                   want_kind=dict(out=[0], boosted=[0], counts=[0, 1, 0, 0], m=0)),
    "empty_state": lambda: _smooth_case([(0, 0, 10, 10, 0.5, 1)], [], [], [], [],
                                        want_kind=dict(out=[0], boosted=[0], counts=[0, 1, 0, 0], m=0)),
    # six valid rows on four slots: the first four are kept, two are counted
    "more_kept_than_slots": lambda: _smooth_case([(i, i, i + 10, i + 10, 0.8 + 0.01 * i, i) for i in range(6)] + [(0, 0, 5, 5, 0.5, 9)], [], [], [], [],
                                                 want_kind=dict(out=[np.float32(0.8 + 0.01 * i) for i in range(6)] + [0], boosted=[0] * 7, counts=[6, 1, 0, 2], m=4)),
    # rows with a NaN, an infinity, an inverted box or a NaN score are nothing; rows from n on are nothing
    "nan_rows": lambda: _smooth_case([(np.nan, 0, 10, 10, 0.9, 1), (0, 0, np.inf, 10, 0.9, 1), (10, 0, 0, 10, 0.9, 1), (0, 0, 10, 10, np.nan, 1), (0, 0, 10, 10, 0.5, 1),
                                      (0, 0, 10, 10, 0.9, 1)], [P0], [P0], [0.1], [0], n=5,
                                     want_kind=dict(out=[0, 0, 0, 0, 0.7, 0], boosted=[0, 0, 0, 0, 1, 0], counts=[0, 1, 1, 0], m=1)),
}


def smooth_reference(name):
    c = SMOOTH_CASES[name]()
    want = mn.smooth_np(c["boxes"], c["n"], c["state"], c["moved"], c["score"], c["status"], c["slots"], **c["kw"])
    return c, want


# ------------------------------------------------------------------ a scene through the whole smoother

SCENE_FRAMES = 8


@functools.lru_cache(maxsize=None)
def scene():
    """Background noise of amplitude 64, a 40 x 40 full-amplitude textured object moving (3, -2) a frame.  Detector rows: the object
    at its true position, score 0.9 in frames 0-1 and 0.5 afterwards; a stray 0.5 candidate far away in frames 3-4.
    -> (images uint8 [8, 96, 128, 3], boxes float32 [8, 4, 6])"""
    rng = np.random.default_rng(12)
    back = rng.integers(0, 64, (H, W, 3), dtype=np.uint8)
    obj = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    images = np.empty((SCENE_FRAMES, H, W, 3), dtype=np.uint8)
    boxes = np.zeros((SCENE_FRAMES, 4, 6), dtype=np.float32)
    for f in range(SCENE_FRAMES):
        x, y = 50 + 3 * f, 40 - 2 * f
        images[f] = back
        images[f, y:y + 40, x:x + 40] = obj
        boxes[f, 0] = (x, y, x + 40, y + 40, 0.9 if f < 2 else 0.5, 1)
        if f in (3, 4):
            boxes[f, 1] = (5, 50, 25, 80, 0.5, 2)
    images.setflags(write=False); boxes.setflags(write=False)
    return images, boxes


@functools.lru_cache(maxsize=None)
def scene_reference(corr, slots=4):
    images, boxes = scene()
    return mn.smooth_stream_np(images, boxes, None, slots, corr=corr)
