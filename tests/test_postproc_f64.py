"""The display and detector post-processing kernels (colorize, power centre, letterbox, decode, NMS) against float64.

Every checker is a vectorised float64 restatement under oracle/ (visual_np.py, detect_np.py) of the float32 restatement it sits
beside; the CPU tests hold the two to each other and assert, for every array a GPU test hands to a kernel (tests/postproc_cases.py),
the conditions that make an exact comparison fair.  No tolerance below is chosen: each is a figure measured on the CPU, float32
restatement against float64, times 4 (the device's log10f / powf / expf are allowed a few ulp where glibc's are within one, and the
device contracts and orders sums differently).

Colouriser.  A pixel may differ from lut[floor(t)] only where float32 rounding can move it across a decision, and then only to the
other side of that decision.  Distances to a decision are counted in units of one float32 rounding (visual_np.heat_units):
    level_unit = eps32 * max|log10 s| / (log10 max - log10 min)                    (the level against `amount`)
    index_unit = 255 * eps32 * (e u^(e-1) max|log10 s| / (range * amount) + u^e)   (t = 255 u^e against an integer step)
so the band follows each map's flatness (1 / range) and the exponent instead of being one constant.  Measured, float32 NumPy against
float64 over all 285 maps of color_cases(): 44 disagreeing pixels, the farthest 0.461 units from its decision (101 x 101 batch;
57 x 32 golden maps 0.341 -- `shipped` s2, 4.3e-4 index units --, exponent 0.5: 0.060) -> COLOR_MEASURED = 0.47, the GPU band is
COLOR_BAND = 4 * 0.47 = 1.88 units (the MI355X's farthest pixel: 0.591).  Cap: at that band at most 1 % of a map's pixels (or 3) are ambiguous, asserted for every map.
`amount` < 0.5 takes (l - amount) / amount past 1 and the reference's table lookup raises IndexError; the kernel stays on the last
entry, and that is what is asserted there.

Power centre.  Inputs keep every smoothed pixel 1e-5 (relative) clear of the 95 % line, so the mask is the same set in float32 and
float64 (cfg2 s3 lies 8.8e-6 from it and stays under the old 1e-3 check only).  Measured |float32 restatement - float64| over the 80
maps of center_cases(): 2.85e-7 -> CENTER_MEASURED = 2.9e-7; tolerance 4 * (2.9e-7 + 2^-24 * grid extent), the second term being the
float32 rounding of the returned coordinate.

Decode.  Logits on a 1/64 lattice (exact in float16): two class logits are equal or 1/64 apart.  Measured over DECODE_CASES, float32
restatement against float64: boxes 1.44e-7 of the largest coordinate, scores 1.53e-7 -> BOX_MEASURED = 1.5e-7 (relative to the
largest |coordinate|), SCORE_MEASURED = 1.6e-7; tolerances 4 * (measured + 2^-24).  A box whose objectness or score lies within the
score tolerance of conf_thres may be filtered or not; at most 0.1 % of the boxes may be such (here: none).

NMS.  Nothing to tolerate: with no pair's IoU within 1e-5 of the threshold (postproc_cases.nms_keeps_clear) the kept rows are copies.
"""
import ctypes as C

import numpy as np
import pytest

import postproc_cases as P
import util

COLOR_MEASURED = 0.47
COLOR_BAND = 4 * COLOR_MEASURED
CENTER_MEASURED = 2.9e-7
BOX_MEASURED = 1.5e-7
SCORE_MEASURED = 1.6e-7
N_COLOR_CASES, N_CENTER_CASES = 13, 7


def center_tol(extent):
    return 4 * (CENTER_MEASURED + 2.0 ** -24 * extent)


def ambiguous_cap(n_pixels):
    return max(3, n_pixels // 100)


def _kw(case):
    return dict(threshold=case["threshold"], amount=case["amount"], exponent=case["exponent"])


# ---------------------------------------------------------------- CPU: the restatements against each other, the inputs' conditions

def test_vectorised_colour_restatement_equals_the_loop():
    import visual_np as V
    for m, kw in ((P.golden_map("cfg1", "s3"), {}), (P.golden_map("shipped", "s2"), dict(amount=0.75, exponent=2)),
                  (P.beam_map(9, 13, 1), dict(threshold=0.0, exponent=0.5)), (P.golden_map("shipped", "s1") * np.float32(1e-9), {})):
        a, fa = V.small_heatmap(m, **kw)
        b, fb = V.small_heatmap_f32(m, **kw)
        assert fa == fb and np.array_equal(a, b)


def test_colour_restatements_agree_inside_the_measured_band_and_inputs_stay_under_the_cap(oracle_lib):
    import visual_np as V
    cases = P.color_cases(oracle_lib)
    assert len(cases) == N_COLOR_CASES
    assert sorted({c["maps"].shape[0] for c in cases} & {1, 2, 7, 64, 190}) == [1, 2, 7, 64, 190]
    worst = 0.0
    goldens = [dict(maps=np.stack([P.golden_map(n, s)]), threshold=1e-7, amount=0.5, exponent=5, name=n + s) for n in ("cfg1", "cfg2", "shipped") for s in ("s1", "s2", "s3")]
    for c in cases + goldens:
        for f, m in enumerate(c["maps"]):
            got, flag = V.small_heatmap_f32(m, **_kw(c))
            want_flag, wrong, _, dist = V.check_small(got, m, mult=0.0, **_kw(c))
            assert flag == want_flag, (c["name"], f)
            if wrong.any():
                worst = max(worst, float(dist[wrong].max()))
            _, wrong, _, _ = V.check_small(got, m, mult=COLOR_MEASURED, **_kw(c))      # and a disagreeing pixel shows the other side's colour
            assert not wrong.any(), (c["name"], f, int(wrong.sum()))
            _, _, amb, _ = V.check_small(got, m, mult=COLOR_BAND, **_kw(c))
            assert amb.sum() <= ambiguous_cap(m.size), (c["name"], f, int(amb.sum()))
    print("farthest float32 / float64 disagreement: %.3f units" % worst)
    assert 0.25 * COLOR_MEASURED < worst <= COLOR_MEASURED                          # the constant is the measurement, not a guess above it
    quiet = [bool(m.max() > 1e-7) for m in cases[0]["maps"]]
    assert not all(quiet) and any(quiet)                                              # the 190-frame batch mixes frames under and over the threshold


def test_colour_degenerate_maps_follow_the_reference_in_float64(oracle_lib):
    """visual.py:143-185 on the degenerate frames: what the float64 checker expects of each."""
    import visual_np as V
    c = P.color_cases(oracle_lib)[-1]
    zeros, const, mixed, inf, nan, neg, plain = c["maps"]
    blank = np.zeros((11, 11, 3), np.uint8)
    for m, flag, black in ((zeros, False, True), (const, True, True), (mixed, True, False), (inf, True, True), (nan, False, True), (neg, False, True), (plain, True, False)):
        got, f32_flag = V.small_heatmap_f32(m)
        want_flag, wrong, _, _ = V.check_small(got, m, mult=COLOR_MEASURED)
        assert want_flag == flag == f32_flag and not wrong.any()
        assert black == (not got.any())
        assert V.check_small(blank, m)[1].any() == (not black)
    l, _ = V.heat_levels_f64(mixed)
    assert l.min() == 0.0 and np.isclose(np.log10(V.CLIP), -12.0, atol=1e-8)           # zeros and negatives sit on the clip: lmin = -12


def test_center_inputs_keep_clear_of_the_mask_line_and_float32_stays_inside_the_measured_error():
    import visual_np as V
    cases = P.center_cases()
    assert len(cases) == N_CENTER_CASES and sorted({m.shape[0] for _, m in cases}) == [1, 3, 64]
    worst = 0.0
    for name, maps in cases:
        for f, m in enumerate(maps):
            cx, cy, gap, n_mask = V.find_power_center_f64(m)
            assert gap >= 1e-5 and n_mask >= 1, (name, f, gap)
            fx, fy = V.find_power_center(m)
            worst = max(worst, abs(fx - cx), abs(fy - cy))
    assert 0.25 * CENTER_MEASURED < worst <= CENTER_MEASURED, worst
    assert V.find_power_center_f64(P.golden_map("cfg2", "s3"))[2] < 1e-5               # why that map is not among the cases
    big = cases[0][1]
    for f, want in ((0, (50, 50)), (5, None), (10, (40, 50)), (11, (50, 50)), (12, (50, 50)), (15, (88, 17))):
        cx, cy, _, n_mask = V.find_power_center_f64(big[f])
        if want is not None:                                                          # middle blob, two equal blobs, constant, zeros, hot pixel
            assert abs(cx - want[0]) < 1e-9 and abs(cy - want[1]) < 1e-9, (f, cx, cy)
        else:                                                                         # a corner blob: the reflected border keeps the centre near the corner
            assert 0 <= cx < 1.5 and 0 <= cy < 1.5
    assert V.find_power_center_f64(big[11])[3] == 101 * 101 and V.find_power_center_f64(big[15])[3] == 1


LETTERBOX_REJECTED = [  # (h, w, out_h, out_w, new_h, new_w, top, left, value)
    (0, 640, 384, 640, 360, 640, 12, 0, 114), (360, -1, 384, 640, 360, 640, 12, 0, 114), (360, 640, 0, 640, 360, 640, 0, 0, 114),
    (360, 640, 384, 640, 0, 640, 12, 0, 114), (360, 640, 384, 640, 360, -3, 12, 0, 114), (360, 640, 384, 640, 360, 640, 25, 0, 114),
    (360, 640, 384, 640, 360, 640, 12, 1, 114), (360, 640, 384, 640, 360, 640, -1, 0, 114), (360, 640, 384, 640, 360, 640, 12, 0, 256),
    (360, 640, 384, 640, 360, 640, 12, 0, -1)]


def test_letterbox_rejects_bad_geometry_before_touching_the_device(native):
    buf = np.zeros(16, dtype=np.uint8)                   # never read: every case is refused by the argument check
    for args in LETTERBOX_REJECTED:
        native.lib.bf_clear_error()
        h, w, oh, ow, nh, nw, top, left, value = args
        assert native.lib.bf_letterbox_bgr8_device(buf.ctypes.data, h, w, buf.ctypes.data, oh, ow, nh, nw, top, left, value, None) == -1, args
        with pytest.raises(native.BeamformerError, match="bf_letterbox_bgr8_device"):
            native.check()
    for h, w, oh, ow, nh, nw, top, left, value in P.letterbox_cases():             # and the geometries the GPU test uses are none of those
        assert min(h, w, nh, nw) >= 1 and top >= 0 and left >= 0 and top + nh <= oh and left + nw <= ow and 0 <= value <= 255
    geo = {(c[0], c[1]): c for c in P.letterbox_cases()}
    assert geo[(640, 360)][7] > 0 and geo[(480, 640)][2:6] == (480, 640, 480, 640) and geo[(320, 320)][4:6] == (640, 640)


def test_decode_restatements_agree_and_inputs_stay_under_the_cap():
    import detect_np as D
    from image_detection.model import yolov5s
    assert {c[0] for c in P.DECODE_CASES} == {1, 3, 80} and {c[1] for c in P.DECODE_CASES} == {0, 1, 2} and {c[2] for c in P.DECODE_CASES} == {1, 3}
    conf = float(np.float32(P.DECODE_CONF))
    worst_box = worst_score = 0.0
    for nc, lv, B in P.DECODE_CASES:
        raw = P.decode_raw(nc, lv, B)
        assert all(np.array_equal(r, r.astype(np.float16).astype(np.float32)) for r in raw)
        b32, s32, c32 = D.decode(list(raw), yolov5s.ANCHORS, yolov5s.STRIDES, nc, P.DECODE_CONF)
        b64, o64, s64, c64 = D.decode_f64(raw, yolov5s.ANCHORS, yolov5s.STRIDES, nc)
        assert np.array_equal(c32, c64)
        if nc > 1:
            logits = [r.reshape(B, 3, 5 + nc, -1)[:, :, 5:] for r in raw]
            tied = np.concatenate([(np.sort(l, axis=2)[:, :, -1] == np.sort(l, axis=2)[:, :, -2]).reshape(B, -1) for l in logits], axis=1)
            assert tied.mean() > 0.01                                                 # class ties are really there
        passed = (o64 > conf) & (s64 > conf)
        near = (np.abs(o64 - conf) <= 4 * (SCORE_MEASURED + 2.0 ** -24)) | (np.abs(s64 - conf) <= 4 * (SCORE_MEASURED + 2.0 ** -24))
        assert near.mean() <= 1e-3 and 0.2 < passed.mean() < 0.9
        assert np.array_equal(passed | near, (s32 > 0) | near)
        worst_box = max(worst_box, float(np.abs(b32 - b64).max() / np.abs(b64).max()))
        worst_score = max(worst_score, float(np.abs(s32 - s64)[passed & (s32 > 0)].max()))
    assert 0.25 * BOX_MEASURED < worst_box <= BOX_MEASURED and 0.25 * SCORE_MEASURED < worst_score <= SCORE_MEASURED, (worst_box, worst_score)


def test_nms_inputs_keep_clear_of_the_threshold_and_the_matrix_walk_equals_the_loop(native):
    import detect_np as D
    assert {c[0] for c in P.NMS_CASES} == {1, 63, 64, 65, 1000, 1024, 4000, 4096} and {c[3] for c in P.NMS_CASES} == {0.0, 0.45, 1.0}
    assert max(len(c[1]) for c in P.NMS_CASES) == 8
    cut = chains = far = 0
    for i, (K, counts, max_det, thr) in enumerate(P.NMS_CASES):
        boxes, scores, cls, cnt = P.nms_inputs(i)
        assert max_det in (1, 300, K)
        for b, n in enumerate(counts):
            assert (scores[b, :n] > 0).all() and (np.diff(scores[b, :n]) < 0).all() and (scores[b, n:] == -1).all()
            if n == 0:
                continue
            assert np.array_equal(boxes[b, :n] * 4, np.rint(boxes[b, :n] * 4)) and P.nms_keeps_clear(boxes[b, :n], thr), (K, b)
            iou = D.iou_matrix_f64(boxes[b, :n])
            every = D.nms_f64(boxes[b], n, thr, n, iou)
            if n <= 130:
                assert every == D.nms(boxes[b, :n].astype(np.float64), scores[b, :n], thr, n)
            kept = np.zeros(n, dtype=bool)
            kept[every] = True
            over = np.triu(iou > thr, 1)
            cut += len(every) > max_det
            chains += int(over[~kept][:, kept].any())            # a suppressed box overlaps a later box that is kept all the same
            far += int(n > 1024 and over[kept][:, 1024:].any())  # a kept box suppresses one past mask word 16
    assert cut >= 1 and chains >= 3 and far >= 2
    z = np.zeros(8, dtype=np.int64)                                # K = 4097 is refused before any pointer is used
    p = z.ctypes.data
    assert native.lib.bf_nms_device(p, p, p, p, 1, 4097, 0.45, 300, p, p, p, None) == -1
    native.lib.bf_clear_error()


# ---------------------------------------------------------------- GPU

def _guarded(n, dtype, fill):
    """A device buffer of n elements followed by 64 canary elements."""
    import torch
    t = torch.full((n + 64,), fill, dtype=dtype, device="cuda")
    return t, lambda: bool((t[n:] == fill).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(N_COLOR_CASES))
def test_gpu_colorize_equals_float64_outside_the_ambiguous_band(native, oracle_lib, case):
    """bf_heatmap_colorize_device on a whole batch: every frame's flag, every pixel equal to the float64 colour except the ambiguous
    ones (either side of their decision), quiet / NaN frames blank with flag 0, nothing written past either output."""
    import torch
    import visual_np as V
    c = P.color_cases(oracle_lib)[case]
    maps = c["maps"]
    F, X, Y = maps.shape
    try:
        util.configure("cfg1", MAX_RES_X=X, MAX_RES_Y=Y)
        d = torch.from_numpy(maps.reshape(F, -1)).cuda()
        small, small_ok = _guarded(F * Y * X * 3, torch.uint8, 0xA5)
        flags, flags_ok = _guarded(F, torch.int32, -7)
        assert native.lib.bf_heatmap_colorize_device(d.data_ptr(), F, c["threshold"], c["amount"], float(c["exponent"]), small.data_ptr(), flags.data_ptr(), None) == 0, native.check()
        torch.cuda.synchronize()
    finally:
        util.configure("cfg1")
    assert small_ok() and flags_ok()
    got = small[: F * Y * X * 3].cpu().numpy().reshape(F, Y, X, 3)
    got_flags = flags[:F].cpu().numpy()
    worst = n_amb = 0
    for f in range(F):
        want_flag, wrong, amb, dist = V.check_small(got[f], maps[f], mult=COLOR_BAND, **_kw(c))
        assert got_flags[f] == int(want_flag), (c["name"], f, got_flags[f])
        assert amb.sum() <= ambiguous_cap(X * Y), (c["name"], f)
        assert not wrong.any(), (c["name"], f, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
        if want_flag:
            strict = V.check_small(got[f], maps[f], mult=0.0, **_kw(c))[1]
            worst = max(worst, float(dist[strict].max()) if strict.any() else 0.0)
            n_amb += int(strict.sum())
    print("%s: %d pixels on the other side of a decision, the farthest %.3f units from it (band %.2f)" % (c["name"], n_amb, worst, COLOR_BAND))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(N_CENTER_CASES))
def test_gpu_power_center_equals_float64(native, case):
    """bf_power_center_device, `frames` distinct maps per launch with the workspace [frames][X * Y]."""
    import torch
    import visual_np as V
    name, maps = P.center_cases()[case]
    F, X, Y = maps.shape
    try:
        util.configure("cfg1", MAX_RES_X=X, MAX_RES_Y=Y)
        d = torch.from_numpy(maps.reshape(F, -1)).cuda()
        centers, centers_ok = _guarded(F * 2, torch.float32, -7.0)
        ws, ws_ok = _guarded(F * X * Y, torch.float32, -7.0)
        assert native.lib.bf_power_center_device(d.data_ptr(), F, centers.data_ptr(), ws.data_ptr(), None) == 0, native.check()
        torch.cuda.synchronize()
    finally:
        util.configure("cfg1")
    assert centers_ok() and ws_ok()
    got = centers[: F * 2].cpu().numpy().reshape(F, 2)
    tol = center_tol(max(X, Y))
    for f in range(F):
        cx, cy, _, _ = V.find_power_center_f64(maps[f])
        assert abs(got[f, 0] - cx) <= tol and abs(got[f, 1] - cy) <= tol, (name, f, got[f].tolist(), cx, cy, tol)


@pytest.mark.gpu
def test_gpu_find_power_center_clips_the_map_itself(native):
    """visual.find_power_center on a map with zeros in it, not clipped by the caller."""
    import visual
    import visual_np as V
    m = P.blob(57, 32, 20, 9, 3.0, floor=0.0)
    m[m < 1e-3] = 0.0
    try:
        util.configure("shipped")
        cx, cy = visual.find_power_center(m)
    finally:
        util.configure("cfg1")
    wx, wy, gap, _ = V.find_power_center_f64(m)
    assert gap >= 1e-5 and (m == 0).any()
    assert abs(cx - wx) <= center_tol(57) and abs(cy - wy) <= center_tol(57), (cx, cy, wx, wy)


@pytest.mark.gpu
def test_gpu_letterbox_equals_the_oracle_byte_for_byte(native):
    import torch
    import visual_np as V
    for i, (h, w, oh, ow, nh, nw, top, left, value) in enumerate(P.letterbox_cases()):
        src = np.random.default_rng(900 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        d_src = torch.from_numpy(src).cuda()
        out, out_ok = _guarded(oh * ow * 3, torch.uint8, 0x5A)
        assert native.lib.bf_letterbox_bgr8_device(d_src.data_ptr(), h, w, out.data_ptr(), oh, ow, nh, nw, top, left, value, None) == 0, native.check()
        torch.cuda.synchronize()
        want = V.letterbox_u8(src, oh, ow, nh, nw, top, left, value)
        assert out_ok() and np.array_equal(out[: oh * ow * 3].cpu().numpy().reshape(oh, ow, 3), want), (h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("nc,lv,B", P.DECODE_CASES)
def test_gpu_decode_equals_float64(native, nc, lv, B, fmt):
    """bf_yolo_decode_device directly: all B * T boxes, scores and class ids (format bit 0: float16 maps, bit 1: NHWC)."""
    import torch
    import detect_np as D
    from image_detection.model import yolov5s
    raw = P.decode_raw(nc, lv, B)
    dev = [torch.from_numpy(r).cuda().to(torch.float16 if fmt & 1 else torch.float32) for r in raw]
    if fmt & 2:
        dev = [r.permute(0, 2, 3, 1).contiguous() for r in dev]
    T = 3 * sum(r.shape[2] * r.shape[3] for r in raw)
    boxes, boxes_ok = _guarded(B * T * 4, torch.float32, -7.0)
    scores, scores_ok = _guarded(B * T, torch.float32, -7.0)
    cls, cls_ok = _guarded(B * T, torch.int32, -7)
    anchors = np.ascontiguousarray(np.asarray(yolov5s.ANCHORS, dtype=np.float32).reshape(3, 3, 2))
    hs = (C.c_int * 3)(*[r.shape[2] for r in raw]); ws = (C.c_int * 3)(*[r.shape[3] for r in raw]); st = (C.c_int * 3)(*yolov5s.STRIDES)
    ptrs = (C.c_void_p * 3)(*[r.data_ptr() for r in dev])
    assert native.lib.bf_yolo_decode_device(ptrs, hs, ws, st, native.fptr(anchors), B, nc, fmt, P.DECODE_CONF, boxes.data_ptr(), scores.data_ptr(), cls.data_ptr(), None) == 0, native.check()
    torch.cuda.synchronize()
    assert boxes_ok() and scores_ok() and cls_ok()
    got_b = boxes[: B * T * 4].cpu().numpy().reshape(B, T, 4).astype(np.float64)
    got_s = scores[: B * T].cpu().numpy().reshape(B, T).astype(np.float64)
    got_c = cls[: B * T].cpu().numpy().reshape(B, T)
    b64, o64, s64, c64 = D.decode_f64(raw, yolov5s.ANCHORS, yolov5s.STRIDES, nc)
    assert np.array_equal(got_c, c64)
    box_tol = 4 * (BOX_MEASURED + 2.0 ** -24) * np.abs(b64).max()
    assert np.abs(got_b - b64).max() <= box_tol, (np.abs(got_b - b64).max(), box_tol)
    conf, tol = float(np.float32(P.DECODE_CONF)), 4 * (SCORE_MEASURED + 2.0 ** -24)
    passed = (o64 > conf) & (s64 > conf)
    near = (np.abs(o64 - conf) <= tol) | (np.abs(s64 - conf) <= tol)
    filtered = got_s == -1.0
    assert np.array_equal(filtered | near, ~passed | near)
    assert np.abs(got_s - s64)[~filtered].max() <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(P.NMS_CASES)))
def test_gpu_nms_equals_the_float64_walk(native, case):
    """bf_nms_device directly on sorted synthetic candidates: kept rows are copies (boxes, score and class), rows past n are zero, n is
    right, nothing is written past d_out or d_mask."""
    import torch
    import detect_np as D
    K, counts, max_det, thr = P.NMS_CASES[case]
    boxes, scores, cls, cnt = P.nms_inputs(case)
    B, words = len(counts), (K + 63) // 64
    dev = lambda a: torch.from_numpy(a).cuda()
    d_b, d_s, d_c, d_n = dev(boxes), dev(scores), dev(cls), dev(cnt)
    mask, mask_ok = _guarded(B * K * words, torch.int64, 0x5A5A5A5A)
    out, out_ok = _guarded(B * max_det * 6, torch.float32, -7.0)
    n_out, n_ok = _guarded(B, torch.int32, -7)
    assert native.lib.bf_nms_device(d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_n.data_ptr(), B, K, thr, max_det, mask.data_ptr(), out.data_ptr(), n_out.data_ptr(), None) == 0, native.check()
    torch.cuda.synchronize()
    assert mask_ok() and out_ok() and n_ok()
    got = out[: B * max_det * 6].cpu().numpy().reshape(B, max_det, 6)
    got_n = n_out[:B].cpu().numpy()
    for b, n in enumerate(counts):
        keep = D.nms_f64(boxes[b], n, thr, max_det)
        want = np.zeros((max_det, 6), dtype=np.float32)
        want[: len(keep), :4], want[: len(keep), 4], want[: len(keep), 5] = boxes[b][keep], scores[b][keep], cls[b][keep]
        assert got_n[b] == len(keep), (K, b, got_n[b], len(keep))
        assert np.array_equal(got[b], want), (K, b)


@pytest.mark.gpu
def test_gpu_nms_refuses_more_than_4096_candidates(native):
    import torch
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = z.data_ptr()
    native.lib.bf_clear_error()
    assert native.lib.bf_nms_device(p, p, p, p, 1, 4097, 0.45, 300, p, p, p, None) == -1
    with pytest.raises(native.BeamformerError, match="4096"):
        native.check()


@pytest.mark.gpu
def test_gpu_overlay_takes_the_one_pixel_kernel_for_an_unaligned_camera(native):
    """out_w % 4 == 0 but the camera frames start one pixel (3 bytes) into their allocation: launch_overlay must fall back to
    overlay_kernel, and the bytes equal the oracle's resize + blend chain."""
    import torch
    import visual_np as V
    c = util.configure("cfg2")
    w, h, F = 64, 40, 3
    rng = np.random.default_rng(12)
    small = rng.integers(0, 256, (F, c["Y"], c["X"], 3), dtype=np.uint8)
    cam = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    prev0 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    d_small, d_prev = torch.from_numpy(small).cuda(), torch.from_numpy(prev0).cuda()
    d_cam = torch.zeros(cam.size + 16, dtype=torch.uint8, device="cuda")
    d_cam[3:3 + cam.size] = torch.from_numpy(cam.ravel()).cuda()
    out = torch.zeros((F, h, w, 3), dtype=torch.uint8, device="cuda")
    assert (d_cam.data_ptr() + 3) % 4 != 0 and d_prev.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 0
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        assert native.lib.bf_heatmap_overlay_device(d_small.data_ptr(), F, w, h, d_prev.data_ptr(), d_cam.data_ptr() + 3, out.data_ptr(), 0.4, 0.7, 0.9, 0.8, None) == 0, native.check()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if "overlay" in e.key]
    assert names and all("overlay_tile_kernel" not in n for n in names), names
    got, prev = out.cpu().numpy(), prev0
    for f in range(F):
        prev = V.add_weighted_u8(prev, 0.4, V.resize_linear_u8(small[f], w, h), 0.7)
        assert np.array_equal(got[f], V.add_weighted_u8(cam[f], 0.9, prev, 0.8))
    assert np.array_equal(d_prev.cpu().numpy(), prev)
