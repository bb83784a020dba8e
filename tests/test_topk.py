"""bf_topk_candidates_device against tests/topk_np.py on every row of tests/topk_cases.py: all four kernels, the key bytes and scan arms
of the radix select, the shapes of tie admission, NaN / inf / subnormal / signed-zero scores on both sides of the K-th place.  Scores and
boxes are compared bit for bit, classes and counts exactly; nothing is excluded and there is no tolerance.  What the table covers is
asserted on the CPU (tests/test_topk_host.py).  Every pointer is 16-byte aligned (the kernels move boxes as float4)."""
import ctypes as C

import numpy as np
import pytest

import topk_cases as TC
import topk_np
import util


def _run(native, scores, boxes, cls, K):
    """The entry point on device copies of the inputs, outputs between canaries -> (top scores, top boxes, top classes, counts) as NumPy."""
    import torch
    B, T = scores.shape
    d_s, d_b, d_c = (torch.from_numpy(np.array(a)).cuda() for a in (scores, boxes, cls))          # (copies: the table's arrays are read-only)
    outs = [util.canaried(shape, dt) for shape, dt in (((B, K), torch.float32), ((B, K, 4), torch.float32), ((B, K), torch.int32), ((B,), torch.int32))]
    assert all(t.data_ptr() % 16 == 0 for t in (d_s, d_b, d_c)) and all(view.data_ptr() % 16 == 0 for _, view in outs)
    (top_buf, top), (tb_buf, tb), (tc_buf, tc), (n_buf, n) = outs
    assert native.lib.bf_topk_candidates_device(d_s.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), B, T, K, top.data_ptr(), tb.data_ptr(), tc.data_ptr(),
                                                n.data_ptr(), None) == 0, native.check()
    torch.cuda.synchronize()
    for what, (buf, view) in zip(("top scores", "top boxes", "top classes", "counts"), outs):
        assert util.intact(buf, view.numel()), what
    return top.cpu().numpy().reshape(B, K), tb.cpu().numpy().reshape(B, K, 4), tc.cpu().numpy().reshape(B, K), n.cpu().numpy()


def _rule(scores_row, got_row, want_row, keff):
    """Which rule of the order a differing score row breaks, for the message."""
    bad = np.flatnonzero(util.bits(got_row) != util.bits(want_row))
    if not bad.size:
        return ""
    i = int(bad[0])
    g, w = got_row[i], want_row[i]
    if i >= keff:
        return "slot %d past min(k, total) does not hold -1" % i
    if g == 0 and w == 0:
        return "slot %d: +0.0 and -0.0 tie and the lower index comes first" % i
    if np.isnan(g) or np.isnan(w):
        return "slot %d: a NaN ranks below every number, lower index first among NaNs" % i
    return "slot %d: descending score, lower index first among equals" % i


@pytest.mark.gpu
@pytest.mark.parametrize("name", TC.NAMES)
def test_gpu_topk_equals_the_restatement(native, name):
    _, B, T, K, pops = TC.ROWS[TC.NAMES.index(name)]
    scores, boxes, cls = TC.inputs(name)
    want = topk_np.topk(scores, boxes, cls, K)
    got = _run(native, scores, boxes, cls, K)
    keff = min(K, T)
    for b in range(B):
        rule = _rule(scores[b], got[0][b], want[0][b], keff)
        assert not rule, (name, TC.kernel_of(T), b, pops[b], rule, util.bits_differ(got[0][b], want[0][b]))
    util.same_bits(got[0], want[0])
    util.same_bits(got[1], want[1])
    assert np.array_equal(got[2], want[2]), name
    assert np.array_equal(got[3], want[3]), (name, got[3].tolist(), want[3].tolist())


@pytest.mark.gpu
def test_gpu_decode_topk_nms_chain_equals_the_restatements(native):
    """Decode on the device, then the device's own scores and boxes through bf_topk_candidates_device and bf_nms_device: the kept rows equal
    topk_np followed by the float64 greedy walk, row for row.  Fair because no pair of the selected candidates has an IoU within 1e-5 of the
    threshold (asserted here on the device's boxes, and on the CPU for the decode's restatement)."""
    import torch
    import detect_np as D
    import postproc_cases as P
    from image_detection.model import yolov5s
    nc, lv, B = TC.CHAIN_CASE
    K, thr, max_det = TC.CHAIN_K, TC.CHAIN_IOU, TC.CHAIN_MAX_DET
    raw = P.decode_raw(nc, lv, B)
    dev = [torch.from_numpy(r).cuda() for r in raw]
    T = 3 * sum(r.shape[2] * r.shape[3] for r in raw)
    d_boxes = torch.empty((B, T, 4), dtype=torch.float32, device="cuda")
    d_scores = torch.empty((B, T), dtype=torch.float32, device="cuda")
    d_cls = torch.empty((B, T), dtype=torch.int32, device="cuda")
    anchors = np.ascontiguousarray(np.asarray(yolov5s.ANCHORS, dtype=np.float32).reshape(3, 3, 2))
    hs = (C.c_int * 3)(*[r.shape[2] for r in raw]); ws = (C.c_int * 3)(*[r.shape[3] for r in raw]); st = (C.c_int * 3)(*yolov5s.STRIDES)
    ptrs = (C.c_void_p * 3)(*[r.data_ptr() for r in dev])
    lib = native.lib
    assert lib.bf_yolo_decode_device(ptrs, hs, ws, st, native.fptr(anchors), B, nc, 0, P.DECODE_CONF, d_boxes.data_ptr(), d_scores.data_ptr(), d_cls.data_ptr(), None) == 0, native.check()
    top = torch.empty((B, K), dtype=torch.float32, device="cuda")
    tb = torch.empty((B, K, 4), dtype=torch.float32, device="cuda")
    tc = torch.empty((B, K), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    mask = torch.empty((B, K, (K + 63) // 64), dtype=torch.int64, device="cuda")
    out_buf, out = util.canaried((B, max_det, 6), torch.float32)
    n_buf, n_out = util.canaried((B,), torch.int32)
    assert lib.bf_topk_candidates_device(d_scores.data_ptr(), d_boxes.data_ptr(), d_cls.data_ptr(), B, T, K, top.data_ptr(), tb.data_ptr(), tc.data_ptr(), cnt.data_ptr(), None) == 0, native.check()
    assert lib.bf_nms_device(tb.data_ptr(), top.data_ptr(), tc.data_ptr(), cnt.data_ptr(), B, K, thr, max_det, mask.data_ptr(), out.data_ptr(), n_out.data_ptr(), None) == 0, native.check()
    torch.cuda.synchronize()
    assert util.intact(out_buf, out.numel()) and util.intact(n_buf, B)
    scores, boxes, cls = d_scores.cpu().numpy(), d_boxes.cpu().numpy(), d_cls.cpu().numpy()
    w_top, w_tb, w_tc, w_cnt = topk_np.topk(scores, boxes, cls, K)
    util.same_bits(top.cpu().numpy(), w_top)
    util.same_bits(tb.cpu().numpy(), w_tb)
    assert np.array_equal(tc.cpu().numpy(), w_tc) and np.array_equal(cnt.cpu().numpy(), w_cnt)
    got, got_n = out.cpu().numpy().reshape(B, max_det, 6), n_out.cpu().numpy()
    for b in range(B):
        n = int(w_cnt[b])
        assert n >= 20 and P.nms_keeps_clear(w_tb[b, :n], thr), b
        keep = D.nms_f64(w_tb[b], n, thr, max_det)
        want = np.zeros((max_det, 6), dtype=np.float32)
        want[: len(keep), :4], want[: len(keep), 4], want[: len(keep), 5] = w_tb[b][keep], w_top[b][keep], w_tc[b][keep]
        assert got_n[b] == len(keep) and len(keep) < n, (b, got_n[b], len(keep), n)
        util.same_bits(got[b], want)
