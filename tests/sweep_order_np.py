"""NumPy restatement of the sweep-order rule (csrc/sweep_order.h), shared by test_sweep_order_host.py and test_sweep_order.py.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

DPW = 8   # directions a wave of the pad / lerp pair kernels carries


def run_changes(p, order, dpw=DPW):
    """Changes of the whole-sample delay inside runs of dpw positions counted from position 0: what the sweep re-reads."""
    q = p[np.asarray(order)]
    diff = (q[1:] != q[:-1]).sum(axis=1)
    inside = (np.arange(1, len(q)) % dpw) != 0
    return int(diff[inside].sum())


def sweep_order(whole, dir_begin, dir_end, dpw=DPW):
    """whole int32 [D, M] -> (order int32 [dir_end - dir_begin] of flat directions, info dict).  The rule, step by step."""
    p = np.asarray(whole)[dir_begin:dir_end]
    n, M = p.shape
    c = (p[1:] != p[:-1]).sum(axis=1)                                  # 1. mics that change from s to s + 1
    cuts = [0] + [s + 1 for s in range(n - 1) if 2 * int(c[s]) > M] + [n]   # 2. segments
    placed, reversed_ = [], 0
    for k in range(len(cuts) - 1):
        a, b = cuts[k], cuts[k + 1]
        seg = list(range(a, b))
        if k > 0:                                                      # 3. the first runs forward
            last = p[placed[-1]]
            if int((last != p[b - 1]).sum()) < int((last != p[a]).sum()):   # 4. strictly closer to the segment's end: reversed
                seg.reverse()
                reversed_ += 1
        placed += seg
    ident = list(range(n))
    ch_id, ch_new = run_changes(p, ident, dpw), run_changes(p, placed, dpw)
    keep = ch_new < ch_id                                              # 5. strictly fewer changes, or the identity
    order = np.asarray(placed if keep else ident, dtype=np.int32) + dir_begin
    return order, dict(segments=len(cuts) - 1, reversed=reversed_, changes_identity=ch_id, changes_candidate=ch_new,
                       changes=ch_new if keep else ch_id, identity=not keep)


@functools.lru_cache(maxsize=None)
def grid_delays(X, Y, every=1):
    """float64 [X * Y, 64 / every]: the 64-microphone array's delays over an X x Y grid, every `every`-th microphone."""
    import directions_np as D
    return np.ascontiguousarray(D.calculate_delays(X, Y, arrays=1).reshape(X * Y, 64)[:, ::every])


def whole_of(delays):
    """The whole-sample table both pad (truncation of the float64 delay) and lerp (floor of the float32 delay) load: delays are >= 0."""
    return np.ascontiguousarray(np.floor(np.float32(delays)).astype(np.int32))
