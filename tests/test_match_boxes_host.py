"""CPU: the host-side contract of bf_match_boxes_device and bf_smooth_boxes_device (every argument is checked before device bring-up,
so the refusals run without a GPU), and the NumPy restatements the GPU tests compare with (tests/match_np.py): the integer patch rule
against the reference's float expression, the integer score against the published mean-subtracted formula in float64, the bounds the
header states, and that every case of tests/match_cases.py reaches the branch it is named for."""
import math
import os
import re

import numpy as np
import pytest

import match_cases as cases
import match_np as mn
import util
from support import entry, FAKE, refused


_match = entry("bf_match_boxes_device", d_images=FAKE, d_prev=FAKE, frames=2, height=96, width=128, d_boxes=FAKE, box_stride=6, d_n_boxes=FAKE,
               max_boxes=300, t_pct=120, s_pct=150, d_moved=FAKE, d_score=FAKE, d_shift=FAKE, d_status=FAKE)


_smooth = entry("bf_smooth_boxes_device", d_boxes=FAKE, d_n_boxes=FAKE, max_boxes=300, conf_low=0.3, conf_high=0.7, iou_threshold=0.5,
                corr_threshold=0.8, slots=16, d_moved=FAKE, d_score=FAKE, d_status=FAKE, d_state=FAKE, d_out=FAKE, d_boosted=FAKE, d_counts=FAKE)


def test_symbols_are_exported_bound_and_declared(native):
    text = open(os.path.join(util.ROOT, "include", "beamformer_hip.h")).read()
    for name, n_args in (("bf_match_boxes_device", 16), ("bf_smooth_state_words", 1), ("bf_smooth_boxes_device", 16)):
        assert hasattr(native.lib, name)
        assert len(getattr(native.lib, name).argtypes) == n_args
        assert re.search(r"^int %s\(" % name, text, flags=re.M)
    assert "#define BF_MATCH_MAX_PIXELS 16384" in text and "#define BF_SMOOTH_MAX_SLOTS 64" in text
    for letter in "abcd":                                                          # the four deliberate differences
        assert "(%s)" % letter in text[text.index("Four deliberate differences"):text.index("#define BF_MATCH_MAX_PIXELS")]


def test_state_words(native):
    native.lib.bf_clear_error()
    w = native.lib.bf_smooth_state_words
    assert w(1) == 8 and w(16) == 68 and w(64) == 260
    assert w(0) == -1 and w(65) == -1 and w(-3) == -1
    native.check()                                                             # the refusals of this one record no error
    assert [mn.state_words(s) for s in (1, 64, 0, 65)] == [8, 260, -1, -1]


@pytest.mark.parametrize("kw,match", [
    (dict(d_images=None), "bf_match_boxes_device: d_images is null"),
    (dict(d_boxes=None), "bf_match_boxes_device: d_boxes is null"),
    (dict(d_moved=None), "bf_match_boxes_device: d_moved is null"),
    (dict(d_score=None), "bf_match_boxes_device: d_score is null"),
    (dict(d_status=None), "bf_match_boxes_device: d_status is null"),
    (dict(frames=0), "bf_match_boxes_device: frames = 0 < 1"),
    (dict(height=0), "height = 0 < 1"),
    (dict(height=8193), "height = 8193 > 8192"),
    (dict(width=-1), "width = -1 < 1"),
    (dict(width=8193), "width = 8193 > 8192"),
    (dict(max_boxes=0), "max_boxes = 0 < 1"),
    (dict(max_boxes=1025), "max_boxes = 1025 > 1024"),
    (dict(box_stride=3), "box_stride = 3 < 4"),
    (dict(t_pct=99), "t_pct = 99 < 100"),
    (dict(t_pct=160), "s_pct = 150 < t_pct = 160"),
    (dict(s_pct=401), "s_pct = 401 > 400"),
    (dict(frames=2 ** 22, max_boxes=1024), r"frames \* max_boxes = 4294967296 does not fit an int"),
])
def test_match_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _match(native, **kw), match)


@pytest.mark.parametrize("kw,match", [
    (dict(d_boxes=None), "bf_smooth_boxes_device: d_boxes is null"),
    (dict(d_moved=None), "bf_smooth_boxes_device: d_moved is null"),
    (dict(d_score=None), "bf_smooth_boxes_device: d_score is null"),
    (dict(d_status=None), "bf_smooth_boxes_device: d_status is null"),
    (dict(d_state=None), "bf_smooth_boxes_device: d_state is null"),
    (dict(d_out=None), "bf_smooth_boxes_device: d_out is null"),
    (dict(max_boxes=0), "max_boxes = 0 < 1"),
    (dict(max_boxes=1025), "max_boxes = 1025 > 1024"),
    (dict(slots=0), "slots = 0 < 1"),
    (dict(slots=65), "slots = 65 > 64"),
    (dict(conf_low=math.nan), r"conf_low = -?nan is not finite"),
    (dict(conf_high=math.inf), r"conf_high = inf is not finite"),
    (dict(iou_threshold=math.nan), r"iou_threshold = -?nan is not finite"),
    (dict(corr_threshold=-math.inf), r"corr_threshold = -inf is not finite"),
])
def test_smooth_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _smooth(native, **kw), match)


def test_valid_arguments_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only: with one, valid arguments would enqueue")
    refused(native, _match(native), "no usable HIP device")
    # the edges of every range pass the checks; the previous image, the count and the shift may be null
    refused(native, _match(native, height=8192, width=8192, max_boxes=1024, box_stride=4, t_pct=100, s_pct=400, frames=1), "no usable HIP device")
    refused(native, _match(native, height=1, width=1, max_boxes=1, t_pct=400, s_pct=400), "no usable HIP device")
    refused(native, _match(native, d_prev=None, d_n_boxes=None, d_shift=None), "no usable HIP device")
    refused(native, _smooth(native), "no usable HIP device")
    refused(native, _smooth(native, slots=64, max_boxes=1024, corr_threshold=2.0, conf_low=-1e30, d_n_boxes=None, d_boosted=None, d_counts=None), "no usable HIP device")
    import smooth
    with pytest.raises(native.BeamformerError, match="no usable HIP device"):
        smooth.SmoothDetections(slots=4)


# ------------------------------------------------------------------ the integer rules against the reference's expressions

def test_patch_scales_equal_the_reference_float_expression():
    """extract_patch computes int(w * scale) in float64; the definition computes w * pct / 100 in integers."""
    for w in range(1, 8193):
        assert int(w * 1.2) == w * 120 // 100, w
        assert int(w * 1.5) == w * 150 // 100, w


def test_search_area_contains_the_template_on_random_boxes():
    rng = np.random.default_rng(0)
    seen = 0
    for _ in range(2000):
        H, W = int(rng.integers(1, 700)), int(rng.integers(1, 700))
        x1, y1 = rng.uniform(-50, W + 20), rng.uniform(-50, H + 20)
        box = np.array([x1, y1, x1 + rng.uniform(1, 400), y1 + rng.uniform(1, 400)], dtype=np.float32)
        b = mn.box_ints(box)
        if b is None:
            continue
        t_pct = int(rng.integers(100, 401))
        ta, tb, tc, td = mn.patch(*b, t_pct, W, H)
        sa, sb, sc, sd = mn.patch(*b, int(rng.integers(t_pct, 401)), W, H)
        if tb > ta and td > tc:
            seen += 1
            assert 0 <= sa <= ta and tb <= sb <= W and 0 <= sc <= tc and td <= sd <= H
    assert seen > 1000


def test_integer_score_equals_the_mean_subtracted_formula():
    """TM_CCOEFF_NORMED as OpenCV publishes it: per-channel means subtracted, sum of products over the root of the product of the sums of
    squares, in float64 -- against N / sqrt(A B) from exact integers."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in range(200):
        ph, pw = int(rng.integers(2, 24)), int(rng.integers(2, 24))
        hi = int(rng.choice([2, 16, 256]))
        t = rng.integers(0, hi, (ph, pw, 3))
        w = rng.integers(0, hi, (ph, pw, 3)) if k % 4 else np.clip(t + rng.integers(-3, 4, t.shape), 0, 255)
        N, A, B, X = mn.sums(t, w)
        if A == 0 or B == 0:
            continue
        td, wd = t - t.mean(axis=(0, 1)), w - w.mean(axis=(0, 1))
        direct = (td * wd).sum() / math.sqrt((td * td).sum() * (wd * wd).sum())
        worst = max(worst, abs(float(mn.score_of(N, A, B)) - direct))
    print("largest difference from the float64 formula: %.3g" % worst)
    assert worst <= 1e-12


def test_bounds_at_the_saturated_extreme():
    P = mn.MAX_PIXELS
    full = np.full((128, 128, 3), 255, dtype=np.int64)
    N, A, B, X = mn.sums(full, full)
    assert X == P * 3 * 255 ** 2 == 3196108800 < 2 ** 32 and A == 0 and B == 0 and N == 0
    half = full.copy()
    half[:64] = 0                                       # the largest variance a byte image has
    N, A, B, X = mn.sums(half, half)
    assert N == A == B and 0 < A < 2 ** 46 and A < 2 ** 53 and float(A) == A
    N, _, _, _ = mn.sums(half, 255 - half)
    assert N == -A
    assert float(mn.score_of(A, A, A)) == 1.0 and float(mn.score_of(-A, A, A)) == -1.0
    # the decimation rule: the smallest q, at the cap and one pixel over it
    assert mn.decimation(128, 128) == 1 and mn.decimation(129, 128) == 2 and mn.decimation(8192, 8192) == 64 and mn.decimation(8192, 2) == 1
    assert mn.decimation(290, 230) == 3


# ------------------------------------------------------------------ the case tables reach what they are named for

@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_match_case_reaches_its_branch(case):
    c, want, info = cases.reference(case)
    c["check"](want, info)
    assert want[0].dtype == np.float32 and want[1].dtype == np.float32 and want[2].dtype == np.int32 and want[3].dtype == np.int32


@pytest.mark.parametrize("case", sorted(cases.SMOOTH_CASES))
def test_smooth_case_reaches_its_branch(case):
    c, (out, boosted, counts, state) = cases.smooth_reference(case)
    k = c["want_kind"]
    assert np.array_equal(out[:, 4], np.asarray(k["out"], dtype=np.float32)) and boosted.tolist() == k["boosted"]
    assert counts.tolist() == k["counts"] and state[0] == k["m"] and not state[1:4].any()
    assert out[:, :4].tobytes() == c["boxes"][:, :4].tobytes() and out[:, 5].tobytes() == c["boxes"][:, 5].tobytes()      # NaNs pass through as they are


def test_scene_keeps_the_object_and_the_correlation_arm_is_indiscriminate():
    images, boxes = cases.scene()
    for corr, stray in ((2.0, 0.0), (0.8, 0.7)):
        out, boosted, counts, moved, score, state, last = cases.scene_reference(corr)
        assert (out[:2, 0, 4] == np.float32(0.9)).all() and (out[2:, 0, 4] == np.float32(0.7)).all()            # the object's row is kept in every frame
        assert (out[3:5, 1, 4] == np.float32(stray)).all() and not out[:, 2:, 4].any() and not out[[0, 1, 2, 5, 6, 7], 1, 4].any()
        assert (moved[1:, 0] == boxes[1:, 0, :4]).all() and (score[1:, 0] > 0.8).all() and not score[0].any()     # re-found exactly where it went
        assert state[0] == 1 and (state[4:8].view(np.float32) == boxes[-1, 0, :4]).all() and np.array_equal(last, images[-1])
