"""CPU: the restatement tests/topk_np.py against a sort with an explicit comparator and against NumPy's stable argsort, and what the
table of tests/topk_cases.py covers -- every kernel, key byte, scan arm, tie shape and special that tests/test_topk.py is there for.
A class that no row reaches fails here with its name."""
import numpy as np
import pytest

import topk_cases as TC
import topk_np


def _small_rows():
    rng = np.random.default_rng(11)
    every = TC.from_bits(np.asarray((TC.PINF, TC.NINF, TC.FLT_MAX, TC.FLT_MAX | 0x80000000, TC.PZERO, TC.NZERO) + TC.NANS_POS + TC.NANS_NEG
                                    + TC.SUBS_POS + TC.SUBS_NEG, dtype=np.uint32))
    rows = [every, every[::-1].copy(), np.concatenate([every, every])[rng.permutation(2 * every.size)]]
    for n in (1, 2, 37, 90):
        r = (rng.standard_normal(n) * np.exp2(rng.integers(-3, 4, n))).astype(np.float32)
        mix = np.where(rng.random(n) < 0.5, rng.choice(every, n), r).astype(np.float32)
        rows += [r, mix, np.round(r)]                         # np.round: many exact ties, -0.0 among them
    return rows


def test_restatement_equals_a_sort_with_the_explicit_comparator():
    seen = set()
    for s in _small_rows():
        got, want = topk_np.order(s), topk_np.order_by_comparator(s)
        assert got.tolist() == want.tolist(), TC.bits(s).tolist()
        seen |= {k for k, m in TC.special_kind(TC.bits(s)).items() if m.any()}
    assert seen == set(TC.SPECIAL_KINDS)
    # the rules one by one
    f = lambda *u: TC.from_bits(np.asarray(u, dtype=np.uint32))
    assert topk_np.order(f(TC.NZERO, TC.PZERO, TC.NZERO)).tolist() == [0, 1, 2]                    # the zeros tie: index decides
    assert topk_np.order(f(TC.PZERO, TC.NZERO, 0x00000001, 0x80000001)).tolist() == [2, 0, 1, 3]
    assert topk_np.order(f(0xFFC00000, TC.NINF, 0x7FC00000, TC.PINF, 0x7F800001)).tolist() == [3, 1, 0, 2, 4]   # NaNs under -inf, by index
    assert topk_np.order(np.asarray([-3.0, -1.0, -2.0, -1.0], dtype=np.float32)).tolist() == [1, 3, 2, 0]


def test_restatement_equals_the_stable_argsort_without_nan():
    for name in TC.NAMES:
        scores, _, _ = TC.inputs(name)
        for s in scores:
            if not np.isnan(s).any():
                assert np.array_equal(topk_np.order(s), np.argsort(-s, kind="stable")), name


def test_restatement_outputs():
    s = np.asarray([[0.5, np.nan, -0.0, 0.0, -1.0, 2.0]], dtype=np.float32)
    boxes = np.arange(24, dtype=np.float32).reshape(1, 6, 4)
    cls = np.arange(6, dtype=np.int32)[None] + 10
    top, tb, tc, n = topk_np.topk(s, boxes, cls, 8)
    assert TC.bits(top[0]).tolist() == TC.bits(np.asarray([2.0, 0.5, -0.0, 0.0, -1.0, np.nan, -1.0, -1.0], dtype=np.float32)).tolist()
    assert tb[0, :, 0].tolist() == [20, 0, 8, 12, 16, 4, 0, 0] and tc[0].tolist() == [15, 10, 12, 13, 14, 11, 0, 0] and n.tolist() == [2]
    top, tb, tc, n = topk_np.topk(s, boxes, cls, 1)
    assert top.tolist() == [[2.0]] and tb[0, 0].tolist() == [20, 21, 22, 23] and n.tolist() == [1]


def test_key_map_is_monotone_and_inverts():
    """The construction aid: float order equals key order on numbers, the zeros share a key, NaN takes 0, float_of inverts key_of."""
    rng = np.random.default_rng(3)
    f = TC.float_of(rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32))
    f = np.concatenate([f[~np.isnan(f)], TC.from_bits(np.asarray([TC.PINF, TC.NINF, TC.PZERO, TC.NZERO, 1, 0x80000001], dtype=np.uint32))])
    k = TC.key_of(f)
    a, b = f[:, None].astype(np.float64), f[None, :].astype(np.float64)
    assert np.array_equal(a > b, k[:, None] > k[None, :]) and np.array_equal(a == b, k[:, None] == k[None, :])
    assert np.array_equal(TC.key_of(TC.float_of(k)), k)
    assert TC.key_of(TC.from_bits(np.asarray(TC.NANS_POS + TC.NANS_NEG, dtype=np.uint32))).tolist() == [0] * 8
    assert TC.key_of(np.asarray([np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)).tolist() == [0xFF800000, 0x007FFFFF, 0x80000000, 0x80000000]


def test_key_order_equals_the_restatement_on_every_row():
    """(key descending, index ascending) is the order the kernels sort by: on the table's data it is the restatement's order, and the
    key map with the zeros apart -- +0.0 above -0.0 -- is not."""
    apart = 0
    for name in TC.NAMES:
        scores, _, _ = TC.inputs(name)
        for s in scores:
            key = TC.key_of(s).astype(np.int64)
            idx = np.arange(s.size)
            want = topk_np.order(s)
            assert np.array_equal(np.lexsort((idx, -key)), want), name
            old = np.where(TC.bits(s) == TC.NZERO, 0x7FFFFFFF, key)
            apart += not np.array_equal(np.lexsort((idx, -old)), want)
    assert apart >= 8


def test_dispatch_rule_and_row_sizes():
    assert [TC.kernel_of(t) for t in (1, 8192, 8193, 16384, 16385, 32768, 32769, 40001)] == ["reg8", "reg8", "reg16", "reg16", "reg32", "reg32", "generic", "generic"]
    assert len(set(TC.NAMES)) == len(TC.NAMES)
    for name, B, T, K, pops in TC.ROWS:
        assert B == len(pops) and 1 <= K <= 1024 and B * T <= TC.MAX_SCORES, name
        assert all(p in TC.POPULATIONS for p in pops), name
        scores, boxes, cls = TC.inputs(name)
        assert scores.shape == (B, T) and boxes.shape == (B, T, 4) and cls.shape == (B, T), name
        assert np.array_equal(boxes[..., 0], np.broadcast_to(np.arange(T, dtype=np.float32), (B, T)))
    assert {p for r in TC.ROWS for p in r[4]} == set(TC.POPULATIONS)              # no population is left unused


def test_table_covers_every_class():
    seen = set()
    for name in TC.NAMES:
        seen |= TC.covers(name)
    missing = [c for c in TC.REQUIRED if c not in seen]
    assert not missing, "no row covers: " + "; ".join(missing)


def test_signed_zero_rows_would_see_the_old_key_map():
    """Under the key map before this table (+0.0 above -0.0) a selected +0.0 overtakes a -0.0 at a lower index: such rows exist for
    the register kernels and for the generic one, so a regression of score_key fails test_topk on them."""
    rows = [n for n in TC.NAMES if any(c.endswith("selected -0.0 before +0.0") for c in TC.covers(n))]
    assert {TC.kernel_of(TC.ROWS[TC.NAMES.index(n)][2]) for n in rows} == {"reg8", "reg16", "reg32", "generic"}, rows


def test_chained_case_keeps_clear_of_the_iou_threshold():
    """The chained GPU test's fairness condition on the float32 restatement of the decode: among the candidates topk_np selects,
    no pair's IoU lies within 1e-5 of the threshold (here not within 1e-4: the device's decode differs from the restatement by a few
    units in the last place, far less than the spare factor of ten)."""
    import detect_np as D
    import postproc_cases as P
    from image_detection.model import yolov5s
    nc, lv, B = TC.CHAIN_CASE
    assert TC.CHAIN_CASE in P.DECODE_CASES
    raw = P.decode_raw(nc, lv, B)
    boxes, scores, cls = D.decode(list(raw), yolov5s.ANCHORS, yolov5s.STRIDES, nc, P.DECODE_CONF)
    top, tb, tc, counts = topk_np.topk(scores, boxes, cls.astype(np.int32), TC.CHAIN_K)
    suppressed = 0
    for b in range(B):
        n = int(counts[b])
        assert n >= 20, (b, n)
        iou = D.iou_matrix_f64(tb[b, :n])
        gap = np.abs(iou - TC.CHAIN_IOU)[np.triu_indices(n, 1)].min()
        assert gap >= 1e-4, (b, gap)
        assert P.nms_keeps_clear(tb[b, :n], TC.CHAIN_IOU)
        suppressed += n - len(D.nms_f64(tb[b], n, TC.CHAIN_IOU, TC.CHAIN_MAX_DET))
    assert suppressed >= 10                     # NMS has work to do on these candidates
