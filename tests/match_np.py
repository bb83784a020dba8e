"""NumPy restatements of bf_match_boxes_device and bf_smooth_boxes_device (include/beamformer_hip.h holds the definitions).

The matcher is integer arithmetic up to the last three float64 operations: the sums are taken in int64 (the sum of products through
float64 matrix products of integers below 2^53, which are exact whatever the order), the score with NumPy's float64 product, square
root and division, each correctly rounded.  The smoother is float32, one operation at a time."""
import numpy as np

MAX_PIXELS = 16384
F32 = np.float32


def state_words(slots):
    return 4 + 4 * slots if 1 <= slots <= 64 else -1


def patch(ix1, iy1, w, h, pct, width, height):
    """PATCH(pct): (a, b, c, d) = columns [a, b), rows [c, d); every operand of // is >= 0."""
    nw, nh = w * pct // 100, h * pct // 100
    cx, cy = ix1 + w // 2, iy1 + h // 2
    return max(0, cx - nw // 2), min(width, cx + nw // 2), max(0, cy - nh // 2), min(height, cy + nh // 2)


def decimation(tw, th):
    q = 1
    while -(-tw // q) * -(-th // q) > MAX_PIXELS:
        q += 1
    return q


def box_ints(row):
    """(ix1, iy1, w, h) of a row that is a box, else None (step 1 without the j < n clause)."""
    c = np.asarray(row[:4], dtype=np.float32)
    if not (np.isfinite(c).all() and (np.abs(c) < 2.0 ** 20).all()):
        return None
    ix1, iy1, ix2, iy2 = (int(v) for v in c)            # truncation toward zero
    w, h = ix2 - ix1, iy2 - iy1
    return (ix1, iy1, w, h) if w >= 1 and h >= 1 else None


def sums(tmpl, win):
    """(N, A, B, X) of one template / window pair, int64 arrays [ph, pw, 3] -> Python ints."""
    t, w = tmpl.astype(np.int64), win.astype(np.int64)
    P = t.shape[0] * t.shape[1]
    st, si = t.sum(axis=(0, 1)), w.sum(axis=(0, 1))
    X = int((t * w).sum())
    return (P * X - int((st * si).sum()), P * int((t * t).sum()) - int((st * st).sum()), P * int((w * w).sum()) - int((si * si).sum()), X)


def score_of(N, A, B):
    """Step 6 on arrays (or scalars) of exact integers."""
    N, A, B = np.asarray(N, dtype=np.float64), np.float64(A), np.asarray(B, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = N / np.sqrt(A * B)
    return np.where(B == 0, 0.0, r)


def match_one(prev, cur, row, t_pct, s_pct, info=None):
    """One box -> (status, shift_x, shift_y, r)."""
    b = box_ints(row)
    if b is None:
        return 1, 0, 0, 0.0
    H, W = cur.shape[:2]
    ta, tb, tc, td = patch(*b, t_pct, W, H)
    sa, sb, sc, sd = patch(*b, s_pct, W, H)
    tw, th, sw, sh = tb - ta, td - tc, sb - sa, sd - sc
    if tw < 1 or th < 1:
        return 2, 0, 0, 0.0
    if prev is None:
        return 4, 0, 0, 0.0
    assert sa <= ta and tb <= sb and sc <= tc and td <= sd
    q = decimation(tw, th)
    pw, ph = -(-tw // q), -(-th // q)
    P = pw * ph
    dx0, dy0 = ta - sa, tc - sc
    dxb, dyb = dx0 % q, dy0 % q
    nu, nv = (sw - tw - dxb) // q + 1, (sh - th - dyb) // q + 1
    T = prev[tc:td:q, ta:tb:q].astype(np.int64)
    assert T.shape == (ph, pw, 3)
    S = cur[sc + dyb:sd:q, sa + dxb:sb:q].astype(np.int64)[:ph + nv - 1, :pw + nu - 1]
    assert S.shape == (ph + nv - 1, pw + nu - 1, 3), (S.shape, ph, nv, pw, nu)
    note = dict(q=q, pw=pw, ph=ph, P=P, nu=nu, nv=nv, tw=tw, th=th, sw=sw, sh=sh, dx0=dx0, dy0=dy0, status=0)
    if info is not None:
        info.append(note)
    ST = T.sum(axis=(0, 1))
    A = P * int((T * T).sum()) - int((ST * ST).sum())
    if A == 0:
        note["status"] = 3
        return 3, 0, 0, 0.0
    # window sums by summed-area tables, per channel; squares over all channels
    def box_sums(a):
        c = np.zeros((a.shape[0] + 1, a.shape[1] + 1) + a.shape[2:], dtype=np.int64)
        c[1:, 1:] = a.cumsum(axis=0).cumsum(axis=1)
        return c[ph:ph + nv, pw:pw + nu] - c[:nv, pw:pw + nu] - c[ph:ph + nv, :nu] + c[:nv, :nu]
    SI = box_sums(S)                                   # [nv, nu, 3]
    QI = box_sums((S * S).sum(axis=2))                 # [nv, nu]
    # the products: for every column u, G[r, j] = <search row r from u on, template row j>; X[v, u] = sum_j G[v + j, j]
    Tf = T.reshape(ph, pw * 3).astype(np.float64)
    Sf = S.reshape(S.shape[0], -1).astype(np.float64)
    X = np.empty((nv, nu), dtype=np.int64)
    for u in range(nu):
        G = np.ascontiguousarray(Sf[:, 3 * u:3 * (u + pw)] @ Tf.T)
        diag = np.lib.stride_tricks.as_strided(G, shape=(nv, ph), strides=(G.strides[0], G.strides[0] + G.strides[1]))
        X[:, u] = diag.sum(axis=1).astype(np.int64)
    assert X.max() < 2 ** 32
    N = P * X - (SI * ST).sum(axis=2)
    B = P * QI - (SI * SI).sum(axis=2)
    r = score_of(N, A, B)
    note.update(r=r, flat_windows=int((B == 0).sum()), X_max=int(X.max()))
    k = int(np.argmax(r))                              # the first maximum in (dy, dx) row-major order
    v, u = divmod(k, nu)
    return 0, dxb + q * u - dx0, dyb + q * v - dy0, float(r[v, u])


def match_boxes_np(images, prev, boxes, n_boxes=None, t_pct=120, s_pct=150, info=None):
    """images uint8 [F, H, W, 3], prev uint8 [H, W, 3] or None, boxes float32 [F, B, stride >= 4], n_boxes int32 [F] or None ->
    (moved float32 [F, B, 4], score float32 [F, B], shift int32 [F, B, 2], status int32 [F, B])."""
    boxes = np.asarray(boxes, dtype=np.float32)
    F, B = boxes.shape[:2]
    moved, score = np.zeros((F, B, 4), np.float32), np.zeros((F, B), np.float32)
    shift, status = np.zeros((F, B, 2), np.int32), np.zeros((F, B), np.int32)
    for f in range(F):
        n = B if n_boxes is None else min(max(int(n_boxes[f]), 0), B)
        old = prev if f == 0 else images[f - 1]
        for j in range(B):
            if j >= n:
                status[f, j] = 1
                continue
            st, sx, sy, r = match_one(old, images[f], boxes[f, j], t_pct, s_pct, info)
            status[f, j] = st
            if st == 0:
                shift[f, j] = (sx, sy)
                d = np.array([sx, sy, sx, sy], dtype=np.float32)
                moved[f, j] = boxes[f, j, :4] + d
                score[f, j] = np.float32(r)
            elif st == 3:
                moved[f, j] = boxes[f, j, :4]
    return moved, score, shift, status


# ------------------------------------------------------------------ the hysteresis

def iou_f32(p, g):
    """compute_iou(moved box p, candidate g) of the reference, in float32."""
    p, g = [F32(v) for v in p], [F32(v) for v in g]
    mx = lambda a, b: a if a > b else b
    mn = lambda a, b: a if a < b else b
    dw, dh = F32(mn(p[2], g[2]) - mx(p[0], g[0])), F32(mn(p[3], g[3]) - mx(p[1], g[1]))
    iw, ih = (dw if dw > 0 else F32(0)), (dh if dh > 0 else F32(0))
    inter = F32(iw * ih)
    a1, a2 = F32(F32(p[2] - p[0]) * F32(p[3] - p[1])), F32(F32(g[2] - g[0]) * F32(g[3] - g[1]))
    uni = F32(F32(a1 + a2) - inter)
    return F32(inter / uni) if uni > 0 else F32(0)


def smooth_np(boxes, n, state, moved, score, status, slots, conf_low=0.3, conf_high=0.7, iou=0.5, corr=0.8):
    """boxes float32 [B, 6], n int or None, state int32 [4 + 4 * slots], the match results of the state's rows ->
    (out float32 [B, 6], boosted int32 [B], counts int32 [4], new state int32 [4 + 4 * slots])."""
    boxes = np.asarray(boxes, dtype=np.float32)
    B = boxes.shape[0]
    n = B if n is None else min(max(int(n), 0), B)
    lo, hi, iou, corr = F32(conf_low), F32(conf_high), F32(iou), F32(corr)
    m = min(max(int(state[0]), 0), slots)
    part = [p for p in range(m) if status[p] == 0]
    kind = np.zeros(B, dtype=np.int32)                  # 1 valid, 2 candidate, 3 boosted
    with np.errstate(invalid="ignore"):
        for j in range(n):
            b = boxes[j]
            if np.isfinite(b[:5]).all() and b[2] > b[0] and b[3] > b[1]:
                kind[j] = 1 if b[4] > hi else 2 if b[4] > lo else 0
    out = boxes.copy()
    out[:, 4] = 0
    valid_branch = bool((kind == 1).any())
    if valid_branch:
        out[kind == 1, 4] = boxes[kind == 1, 4]
    else:
        any_corr = any(F32(score[p]) > corr for p in part)
        for j in np.flatnonzero(kind == 2):
            if any_corr or any(iou_f32(moved[p], boxes[j, :4]) > iou for p in part):
                kind[j] = 3
                out[j, 4] = hi
    keep = np.flatnonzero(kind == (1 if valid_branch else 3))
    new = np.zeros(4 + 4 * slots, dtype=np.int32)
    new[0] = min(len(keep), slots)
    new[4:4 + 4 * new[0]] = boxes[keep[:slots], :4].ravel().view(np.int32)
    counts = np.array([(kind == 1).sum(), (kind >= 2).sum(), (kind == 3).sum(), max(0, len(keep) - slots)], dtype=np.int32)
    return out, (kind == 3).astype(np.int32), counts, new


def smooth_stream_np(images, boxes, n_boxes, slots, prev=None, state=None, t_pct=120, s_pct=150, **kw):
    """SmoothDetections.update restated: per frame the match of the state's rows (previous image -> image f), then the hysteresis.
    -> (out [F, B, 6], boosted [F, B], counts [F, 4], moved [F, slots, 4], score [F, slots], state, the last image)."""
    boxes = np.asarray(boxes, dtype=np.float32)
    F, B = boxes.shape[:2]
    state = np.zeros(4 + 4 * slots, dtype=np.int32) if state is None else np.asarray(state, dtype=np.int32).copy()
    outs, boosts, cnts, moveds, scores = [], [], [], [], []
    for f in range(F):
        rows = state[4:].view(np.float32).reshape(1, slots, 4)
        mv, sc, _, st = match_boxes_np(images[f:f + 1], prev, rows, state[:1], t_pct, s_pct)
        o, b, c, state = smooth_np(boxes[f], None if n_boxes is None else n_boxes[f], state, mv[0], sc[0], st[0], slots, **kw)
        outs.append(o); boosts.append(b); cnts.append(c); moveds.append(mv[0]); scores.append(sc[0])
        prev = images[f]
    return np.stack(outs), np.stack(boosts), np.stack(cnts), np.stack(moveds), np.stack(scores), state, prev
