"""bf_topk_candidates_device restated as float comparisons (no integer key anywhere in this file).

The order of one image's boxes: numbers before NaNs; numbers by value, descending, where -0.0 == +0.0 as floats compare; equal
values -- and all NaNs, whatever their sign and payload -- by index, ascending.  The first min(k, T) boxes of that order are gathered
bit for bit, the slots past them hold score -1, a zero box and class 0, and counts[b] is the number of gathered scores > 0."""
import functools

import numpy as np


def order(scores):
    """Indices of a float32 [T] row in selection order."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    nan = np.isnan(s)
    value = np.where(nan, np.float32(0.0), s).astype(np.float64)
    return np.lexsort((np.arange(s.size), -value, nan))       # last key first: NaN-ness, then -value (a float compare: the zeros tie), then index


def _before(s, i, j):
    """The definition read aloud: does box i come before box j?"""
    a, b = float(s[i]), float(s[j])
    if (a != a) != (b != b):
        return b != b
    if a == a and a != b:               # (-0.0 != +0.0 is False: the zeros fall through to the index)
        return a > b
    return i < j


def order_by_comparator(scores):
    """The same order from a Python sort with the explicit comparator (small rows only)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    cmp = lambda i, j: -1 if _before(s, i, j) else (1 if _before(s, j, i) else 0)
    return np.asarray(sorted(range(s.size), key=functools.cmp_to_key(cmp)), dtype=np.int64)


def topk(scores, boxes, cls, k):
    """scores float32 [B, T], boxes float32 [B, T, 4], cls int32 [B, T] -> top scores [B, k], top boxes [B, k, 4], top classes [B, k], counts [B]."""
    scores, boxes = np.ascontiguousarray(scores, dtype=np.float32), np.ascontiguousarray(boxes, dtype=np.float32)
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    B, T = scores.shape
    keff = min(k, T)
    top = np.full((B, k), -1.0, dtype=np.float32)
    tb = np.zeros((B, k, 4), dtype=np.float32)
    tc = np.zeros((B, k), dtype=np.int32)
    counts = np.zeros(B, dtype=np.int32)
    for b in range(B):
        o = order(scores[b])[:keff]
        top[b, :keff].view(np.uint32)[:] = scores[b].view(np.uint32)[o]          # copies of the bits: a NaN's payload and a zero's sign survive
        tb[b, :keff].view(np.uint32)[:] = boxes[b].view(np.uint32)[o]
        tc[b, :keff] = cls[b][o]
        counts[b] = int((scores[b][o] > 0).sum())
    return top, tb, tc, counts
