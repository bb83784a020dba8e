"""CPU: the host-side contract of bf_track_boxes_device (every argument is checked before device bring-up, so the refusals run
without a GPU), the Python front end without a GPU, and the NumPy restatement the GPU tests compare with (tests/box_track_np.py):
against the published algorithm in float64 matrix form, against scipy's assignment, and against what the definition promises about
identity."""
import math
import os
import re

import numpy as np
import pytest

import box_track_cases as cases
import box_track_np as bt
import util
from support import entry, FAKE, refused


_track = entry("bf_track_boxes_device", d_boxes=FAKE, d_n_boxes=FAKE, frames=2, max_boxes=300, conf=0.1, slots=16, iou_threshold=0.3, max_age=1,
               min_hits=3, d_state=FAKE, d_tracks=FAKE, d_ids=FAKE, d_match=FAKE, d_live=FAKE, d_counts=FAKE)


def test_symbols_are_exported_bound_and_declared(native):
    text = open(os.path.join(util.ROOT, "include", "beamformer_hip.h")).read()
    for name, n_args in (("bf_track_boxes_device", 16), ("bf_box_track_state_words", 1)):
        assert hasattr(native.lib, name)
        assert len(getattr(native.lib, name).argtypes) == n_args
        assert re.search(r"^int %s\(" % name, text, flags=re.M)
    assert "#define BF_BOX_TRACK_MAX_SLOTS 64" in text and "#define BF_BOX_TRACK_MAX_BOXES 1024" in text


def test_state_words(native):
    native.lib.bf_clear_error()
    w = native.lib.bf_box_track_state_words
    assert w(1) == 24 and w(16) == 324 and w(64) == 1284
    assert w(0) == -1 and w(65) == -1 and w(-3) == -1
    native.check()                                                             # the refusals of this one record no error
    assert [bt.state_words(s) for s in (1, 64, 0, 65)] == [24, 1284, -1, -1]


@pytest.mark.parametrize("kw,match", [
    (dict(d_boxes=None), "bf_track_boxes_device: d_boxes is null"),
    (dict(d_state=None), "bf_track_boxes_device: d_state is null"),
    (dict(d_tracks=None), "bf_track_boxes_device: d_tracks is null"),
    (dict(frames=0), "bf_track_boxes_device: frames = 0 < 1"),
    (dict(frames=-2), "frames = -2 < 1"),
    (dict(max_boxes=0), "max_boxes = 0 < 1"),
    (dict(max_boxes=1025), "max_boxes = 1025 > 1024"),
    (dict(slots=0), "slots = 0 < 1"),
    (dict(slots=65), "slots = 65 > 64"),
    (dict(conf=math.nan), r"conf = -?nan is not finite"),
    (dict(conf=math.inf), r"conf = inf is not finite"),
    (dict(iou_threshold=math.nan), r"iou_threshold = -?nan is not in \[0, 1\]"),
    (dict(iou_threshold=math.inf), r"iou_threshold = inf is not in \[0, 1\]"),
    (dict(iou_threshold=-0.25), r"iou_threshold = -0.25 is not in \[0, 1\]"),
    (dict(iou_threshold=1.5), r"iou_threshold = 1.5 is not in \[0, 1\]"),
    (dict(max_age=-1), "max_age = -1 < 0"),
    (dict(min_hits=-1), "min_hits = -1 < 0"),
])
def test_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _track(native, **kw), match)


def test_valid_arguments_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only: with one, valid arguments would enqueue")
    refused(native, _track(native), "no usable HIP device")
    # the edges of every range pass the checks; the count and the optional outputs may be null
    refused(native, _track(native, slots=64, max_boxes=1024, iou_threshold=1.0, max_age=0, min_hits=0, conf=-1e30), "no usable HIP device")
    refused(native, _track(native, slots=1, max_boxes=1, frames=1, iou_threshold=0.0, conf=1e30, max_age=2 ** 31 - 1, min_hits=2 ** 31 - 1), "no usable HIP device")
    refused(native, _track(native, d_n_boxes=None, d_ids=None, d_match=None, d_live=None, d_counts=None), "no usable HIP device")


def test_tracker_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only")
    import boxtrack
    with pytest.raises(native.BeamformerError, match="no usable HIP device"):
        boxtrack.BoxTracker(slots=4)


# ------------------------------------------------------------------ the restatement against the published algorithm in float64

def _pairs_scene():
    """Ten objects in five overlapping pairs (IoU 0.45 within a pair), drifting: ten rows for the assignment, so the float64 side
    solves it with scipy."""
    objs = []
    for p in range(5):
        objs.append(lambda f, p=p: (80.0 + 110 * p + 1.5 * f, 100.0 + 90 * p, 70.0, 70.0))
        objs.append(lambda f, p=p: (106.0 + 110 * p + 1.5 * f, 101.0 + 90 * p, 70.0, 70.0))
    return bt.scene_rows(10, 12, objs, seed=4, jitter=0.75, score=lambda f, k: 0.2 + 0.07 * ((k + f) % 10))


F64_SCENES = ["shortcut", "crossing", "crowded", "behaviour"] + sorted(k for k in cases.CASES if k.startswith("reporting"))
TOL_PX = 4 * 8.6e-5


def _f64_scene(name):
    if name == "behaviour":
        boxes, n, _ = bt.behaviour_scene()
        return boxes, n, 4, {}
    if name == "pairs":
        boxes, n, _ = _pairs_scene()
        return boxes, n, 12, {}
    c = cases.CASES[name]()
    return c["boxes"], c["n"], c["slots"], c["kw"]


def _against_f64(name):
    boxes, n, slots, kw = _f64_scene(name)
    br = []
    got = bt.track_boxes_np(boxes, n, slots, branches=br, **kw)
    want = bt.sort_f64(boxes, n, slots, **kw)                                # (asserts the two margins on the scene)
    for what, g, w in zip(("ids", "match", "counts"), (got[1], got[2], got[4]), (want[1], want[2], want[4])):
        assert (g == w).all(), (name, what)
    assert ((got[0][:, :, 4] > 0) == (want[0][:, :, 4] > 0)).all() and (got[0][:, :, 4:] == want[0][:, :, 4:]).all(), (name, "reported set")
    worst = max(np.abs(got[0][:, :, :4] - want[0][:, :, :4]).max(), np.abs(got[3] - want[3]).max())
    print("%-22s branches %s  worst |float32 - float64| = %.3g px" % (name, sorted(set(br)), worst))
    assert worst <= TOL_PX, (name, worst)
    return br


@pytest.mark.parametrize("name", F64_SCENES)
def test_restatement_against_float64_sort(name):
    """Scenes on 640-pixel frames whose every pair gain is at least 0.02 away from iou_threshold and whose optimal assignment beats
    the runner-up by at least 1e-3 (sort_f64 asserts both): the decisions -- ids, matches, the reported set, born / ended / dropped
    -- are EQUAL, and the boxes (d_tracks and d_live) agree within 3.44e-4 px = 4 x 8.6e-5 px.  8.6e-5 px is the largest
    float32-against-float64 difference measured over these scenes and the ten-object one below, which sets it (shortcut 5.22e-5,
    crossing 5.12e-5, crowded 4.26e-5, the others below 4e-5; each run prints its own).  That is about 1.4 units in the last place
    of a 600-pixel coordinate: the gain of every update damps what the steps before it rounded."""
    br = _against_f64(name)
    if name == "crossing":
        assert "assignment" in br


def test_restatement_against_float64_sort_with_scipy():
    """Ten rows: more than the brute force takes, so the float64 side's assignment is scipy.optimize.linear_sum_assignment."""
    pytest.importorskip("scipy")
    br = _against_f64("pairs")
    assert br.count("assignment") >= 8


def test_assignment_totals_equal_scipy():
    """The definition's assignment maximises the total gain: on random rectangular gain matrices of up to 64 x 300 -- dense, sparse
    and quantised so that ties abound -- its total equals scipy's to 1e-9, and no column is used twice."""
    sp = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(0)
    shapes = [(64, 300), (64, 40), (1, 1), (1, 300), (64, 1), (7, 7)] + [(int(rng.integers(1, 65)), int(rng.integers(1, 301))) for _ in range(34)]
    for it, (R, D) in enumerate(shapes):
        G = rng.uniform(0, 1, (R, D)).astype(np.float32)
        if it % 3 == 0:
            G = (np.round(G * 4) / 4).astype(np.float32)
        if it % 5 == 0:
            G[rng.uniform(size=G.shape) < 0.8] = 0
        col = bt.assign(G)
        assert len(set(col.tolist())) == R and col.min() >= 0 and col.max() < D + R
        total = sum(float(G[i, c]) for i, c in enumerate(col) if c < D)
        pad = np.hstack([G.astype(np.float64), np.zeros((R, R))])
        r, c = sp.linear_sum_assignment(pad, maximize=True)
        assert abs(total - pad[r, c].sum()) < 1e-9, (R, D, total, pad[r, c].sum())


def test_assignment_ties_take_the_lowest_column():
    G = np.full((2, 3), 0.5, dtype=np.float32)
    assert bt.assign(G).tolist() == [0, 1]
    assert bt.assign(np.zeros((2, 2), dtype=np.float32)).tolist() == [0, 1]        # zero gains: -0.0 == 0.0, the detections come first
    took, branch = bt.associate(G, np.float32(0.3))
    assert branch == "assignment" and took.tolist() == [0, 1]
    took, branch = bt.associate(np.zeros((2, 2), dtype=np.float32), np.float32(0.0))
    assert branch == "shortcut" and took.tolist() == [-1, -1]                   # nothing is over the threshold: nothing is matched


# ------------------------------------------------------------------ consequences of the definition

def test_every_case_reaches_its_branch():
    for name in sorted(cases.CASES):
        c, want, br = cases.reference(name)
        cases.check_reaches(name, want, br)
        assert want[5].size == bt.state_words(c["slots"])


def test_a_gain_equal_to_the_threshold():
    """The float32 gain of (0, 0, 64, 64) and (0, 0, 128, 128) is exactly 0.25; with iou_threshold 0.25 the shortcut does not match
    the pair (it is not over the threshold) and the assignment keeps it (it is not under it)."""
    g = bt.gains([(0, 0, 64, 64)], [(0, 0, 128, 128)])
    assert g.dtype == np.float32 and g[0, 0] == np.float32(0.25)
    _, s, _ = cases.reference("tie_shortcut")
    _, a, _ = cases.reference("tie_assignment")
    assert s[2][1, 0] == -1 and s[1][1].tolist() == [1, 2, 3, 0] and s[4][1].tolist() == [1, 0, 0, 0]
    assert a[2][1, 0] == 0 and a[1][1].tolist() == [1, 2, 3, 0] and a[4][1].tolist() == [1, 0, 0, 0]
    assert a[3][1, 0].tolist() != [0.0, 0.0, 64.0, 64.0] and s[3][1, 0].tolist() == [0.0, 0.0, 64.0, 64.0]     # updated / coasting


def test_behaviour_scene_shows_the_point():
    """Two objects whose score order swaps every four frames, one missed detection, one single-frame false alarm after frame
    min_hits: the raw rows swap, the tracked slots do not, the false alarm is never reported, the miss shows in live but not in
    tracks."""
    boxes, n, owner = bt.behaviour_scene()
    F = boxes.shape[0]
    tracks, ids, match, live, counts, state = bt.track_boxes_np(boxes, n, 4)
    assert (owner[:4, 0] == 0).all() and (owner[4:8, 0] == 1).all() and (owner[8, 0] == 0)                  # row 0 changes its object
    assert (ids[:, 0] == 1).all() and (ids[:, 1] == 2).all()                                                # slot s does not
    for f in range(F):
        for s in (0, 1):
            if match[f, s] >= 0:
                assert owner[f, match[f, s]] == s
    reported = tracks[:, :, 4] > 0
    assert reported[:, 0].all()
    # the false alarm of frame 9 takes slot 2, lives max_age frames more and is never reported
    assert ids[:, 2].tolist() == [0] * 9 + [3] * 3 + [0] * (F - 12) and not reported[:, 2].any() and owner[9, match[9, 2]] == 2
    assert counts[9].tolist() == [1, 0, 0, 0] and counts[11].tolist() == [0, 1, 0, 0] and counts[:, 0].sum() == 3 and counts[:, 1].sum() == 1
    # the miss of frame 14: slot 1 coasts (live goes on, 2 px a frame to the left), nothing is reported until the streak is back
    assert match[14, 1] == -1 and not reported[14:17, 1].any() and reported[:14, 1].all() and reported[17:, 1].all()
    assert (live[14, 1] != 0).all() and abs((live[14, 1, 0] + live[14, 1, 2]) / 2 - (450.0 - 2 * 14)) < 1.0
    assert not tracks[14, 1].any() and not tracks[:, 3].any() and not live[:, 3].any()
    # a reported row is the tracked box with the detection's score and class
    assert (tracks[5, 0, 4:] == boxes[5, match[5, 0], 4:]).all() and np.abs(tracks[5, 0, :4] - boxes[5, match[5, 0], :4]).max() < 2.0


def test_state_carries_between_calls_of_the_restatement():
    c, whole, _ = cases.reference("long_stream")
    boxes, n, slots, kw = c["boxes"], c["n"], c["slots"], c["kw"]
    first = bt.track_boxes_np(boxes[:16], n[:16], slots, **kw)
    second = bt.track_boxes_np(boxes[16:], n[16:], slots, state=first[5], **kw)
    for w, a, b in zip(whole[:5], first[:5], second[:5]):
        assert w.tobytes() == np.concatenate([a, b]).tobytes()
    assert whole[5].tobytes() == second[5].tobytes() and whole[5][1] == 33
