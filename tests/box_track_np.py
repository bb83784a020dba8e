"""Two restatements of bf_track_boxes_device (include/beamformer_hip.h).

  track_boxes_np(boxes, n_boxes, slots, ...) -> (tracks [F, slots, 6], ids [F, slots], match [F, slots], live [F, slots, 4],
                                                 counts [F, 4], state)
      the header's definition operation by operation: every float is an np.float32 (scalar or array element), so each +, -, *, /
      and sqrt rounds once to float32 as the kernel's does (the build contracts nothing); the potentials of the assignment are
      float64.  This is the byte oracle of the GPU tests.
  assign(G)                                  -> the column each row of the gain matrix takes (the definition's assignment)
  sort_f64(boxes, n_boxes, slots, ...)       -> the published algorithm (Bewley et al., "Simple online and realtime tracking", 2016)
      in plain float64: the full 7x7 constant-velocity filter with np.linalg.inv, the optimal assignment by brute force over every
      partial matching (<= 7 rows) or scipy.optimize.linear_sum_assignment (larger).  It also asserts the two margins that make a
      float32 / float64 comparison of DECISIONS meaningful; they are conditions on the scene, not on the code under test.

`state` is an int32 array in the d_state word layout (floats stored by their bits); None or all zeros is a fresh stream.  Inputs are
not modified.  `branches`, when a list, collects what the call went through: each frame's association ('none', 'shortcut',
'assignment'), 'clamp' for a ds set to 0 in step 1, 'freed' for a slot freed over a box that is not finite."""
import itertools

import numpy as np

f32 = np.float32
MAX_SLOTS, MAX_BOXES, SLOT_WORDS = 64, 1024, 20
HALF, ZERO, ONE, TWO, TEN = f32(0.5), f32(0), f32(1), f32(2), f32(10)
Q_POS, Q_AREA, Q_ASPECT = (f32(1), f32(0.01)), (f32(1), f32(1e-4)), f32(1)
R_POS, R_AREA, R_ASPECT = f32(1), f32(10), f32(10)
P0_X, P0_V = f32(10), f32(1e4)


def state_words(slots):
    return 4 + SLOT_WORDS * slots if 1 <= slots <= MAX_SLOTS else -1


# ------------------------------------------------------------------ the definition's pieces

def state_box(u, v, s, r):
    """w = sqrtf(s * r); h = s / w; (u - w/2, v - h/2, u + w/2, v + h/2) in float32."""
    with np.errstate(all="ignore"):
        w = np.sqrt(s * r)
        h = s / w
        hw = HALF * w
        hh = HALF * h
        return (u - hw, v - hh, u + hw, v + hh)


def measurement(box):
    """z = (x1 + w/2, y1 + h/2, w*h, w/h) with w = x2 - x1, h = y2 - y1 in float32."""
    x1, y1, x2, y2 = (f32(c) for c in box)
    with np.errstate(all="ignore"):
        w = x2 - x1
        h = y2 - y1
        return (x1 + HALF * w, y1 + HALF * h, w * h, w / h)


def _predict_block(p, q):
    p00, p01, p11 = p
    a = p00 + p01
    b = p01 + p11
    return ((a + b) + q[0], b, p11 + q[1])


def _update_block(p, r):
    """-> (k0, k1, the Joseph-form covariance) of one 2x2 block measured in its first state with noise r."""
    p00, p01, p11 = p
    S = p00 + r
    k0 = p00 / S
    k1 = p01 / S
    m = ONE - k0
    n00 = (m * m) * p00 + (k0 * k0) * r
    t = p01 - k1 * p00
    n01 = m * t + (k0 * k1) * r
    kk = k1 * k1
    n11 = ((p11 - (TWO * k1) * p01) + kk * p00) + kk * r
    return k0, k1, (n00, n01, n11)


def gains(tbox, dbox):
    """float32 [R, D]: g of every (track box, detection box) pair, in the definition's operation order."""
    t = np.asarray(tbox, dtype=np.float32).reshape(-1, 4)[:, None, :]
    d = np.asarray(dbox, dtype=np.float32).reshape(-1, 4)[None, :, :]
    big = lambda a, b: np.where(a > b, a, b)
    small = lambda a, b: np.where(a < b, a, b)
    with np.errstate(all="ignore"):
        xx1 = big(d[..., 0], t[..., 0])
        yy1 = big(d[..., 1], t[..., 1])
        xx2 = small(d[..., 2], t[..., 2])
        yy2 = small(d[..., 3], t[..., 3])
        w = big(ZERO, xx2 - xx1)
        h = big(ZERO, yy2 - yy1)
        wh = w * h
        area_d = (d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1])
        area_t = (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1])
        o = wh / ((area_d + area_t) - wh)
        g = np.where(o > 0, o, ZERO)
    assert g.dtype == np.float32
    return g


def assign(G):
    """The definition's assignment: rows in order, columns = the D detections then one zero-gain dummy per row, cost -(double)g,
    shortest augmenting paths with float64 potentials, the next column the minimum by (reduced cost, column index).
    -> int array [R]: the column of every row (a column >= D is a dummy: the row is unmatched)."""
    G = np.asarray(G, dtype=np.float32)
    R, D = G.shape
    C = D + R
    c = np.zeros((R, C), dtype=np.float64)
    c[:, :D] = -G.astype(np.float64)
    u = np.zeros(R, dtype=np.float64)
    v = np.zeros(C, dtype=np.float64)
    col_row = np.full(C, -1, dtype=np.int64)
    for i in range(R):
        minv = np.full(C, np.inf)
        used = np.zeros(C, dtype=bool)
        way = np.full(C, -1, dtype=np.int64)
        i0, j0 = i, -1
        while True:
            free = ~used
            cur = (c[i0] - u[i0]) - v
            better = free & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            j1 = int(np.argmin(np.where(free, minv, np.inf)))       # the first minimum: the lowest column among equals
            delta = minv[j1]
            u[i] = u[i] + delta
            rows = col_row[used]
            u[rows] = u[rows] + delta                               # (the rows of distinct used columns are distinct)
            v[used] = v[used] - delta
            minv[free] = minv[free] - delta
            used[j1] = True
            j0 = j1
            if col_row[j0] < 0:
                break
            i0 = int(col_row[j0])
        while True:
            jp = int(way[j0])
            col_row[j0] = i if jp < 0 else col_row[jp]
            j0 = jp
            if j0 < 0:
                break
    out = np.full(R, -1, dtype=np.int64)
    for j in range(C):
        if col_row[j] >= 0:
            out[col_row[j]] = j
    assert (out >= 0).all()
    return out


def associate(G, thr):
    """-> (took [R]: the detection index each row takes or -1, branch: 'none' | 'shortcut' | 'assignment')."""
    R, D = G.shape
    took = np.full(R, -1, dtype=np.int64)
    if R == 0 or D == 0:
        return took, "none"
    over = G > thr
    if over.sum(axis=1).max() <= 1 and over.sum(axis=0).max() <= 1:
        for i, j in zip(*np.nonzero(over)):
            took[i] = j
        return took, "shortcut"
    col = assign(G)
    for i in range(R):
        if col[i] < D and not G[i, col[i]] < thr:
            took[i] = col[i]
    return took, "assignment"


def detections(rows, n, conf):
    """The frame's detections in row order -> list of row indices; rows float32 [max_boxes, 6], n already clamped."""
    out = []
    for j in range(n):
        x1, y1, x2, y2, sc = rows[j, :5]
        if np.isfinite(rows[j, :5]).all() and x2 > x1 and y2 > y1 and sc > conf:
            out.append(j)
    return out


# ------------------------------------------------------------------ the byte oracle

def track_boxes_np(boxes, n_boxes, slots, conf=0.1, iou_threshold=0.3, max_age=1, min_hits=3, state=None, branches=None):
    boxes = np.asarray(boxes, dtype=np.float32)
    F, B, six = boxes.shape
    assert six == 6 and 1 <= B <= MAX_BOXES and 1 <= slots <= MAX_SLOTS
    conf, thr = f32(conf), f32(iou_threshold)
    words = np.zeros(state_words(slots), dtype=np.int32) if state is None else np.array(state, dtype=np.int32).ravel()
    assert words.size == state_words(slots)
    fw = words.view(np.float32)
    next_id, frame_count = int(words[0]), int(words[1])
    base = lambda s: 4 + SLOT_WORDS * s
    tid = [int(words[base(s)]) for s in range(slots)]
    tsu = [int(words[base(s) + 1]) for s in range(slots)]
    hits = [int(words[base(s) + 2]) for s in range(slots)]
    streak = [int(words[base(s) + 3]) for s in range(slots)]
    X = [[f32(fw[base(s) + 4 + i]) for i in range(7)] for s in range(slots)]               # u, v, s, r, du, dv, ds
    PA = [tuple(f32(fw[base(s) + 11 + i]) for i in range(3)) for s in range(slots)]        # the block of (u, du) and (v, dv)
    PS = [tuple(f32(fw[base(s) + 14 + i]) for i in range(3)) for s in range(slots)]        # the block of (s, ds)
    PR = [f32(fw[base(s) + 17]) for s in range(slots)]                                     # the scalar of r

    tracks = np.zeros((F, slots, 6), dtype=np.float32)
    ids = np.zeros((F, slots), dtype=np.int32)
    match = np.full((F, slots), -1, dtype=np.int32)
    live = np.zeros((F, slots, 4), dtype=np.float32)
    counts = np.zeros((F, 4), dtype=np.int32)

    def free_slot(s):
        tid[s] = tsu[s] = hits[s] = streak[s] = 0
        X[s] = [ZERO] * 7
        PA[s] = PS[s] = (ZERO, ZERO, ZERO)
        PR[s] = ZERO

    with np.errstate(all="ignore"):
        for f in range(F):
            n = B if n_boxes is None else min(max(int(n_boxes[f]), 0), B)
            det = detections(boxes[f], n, conf)
            born = ended = dropped = 0
            ignored = n - len(det)
            # 1. predict
            frame_count += 1
            tbox = {}
            for s in range(slots):
                if tid[s] == 0:
                    continue
                x = X[s]
                if x[6] + x[2] <= 0:
                    if branches is not None and x[6] != 0:
                        branches.append("clamp")
                    x[6] = ZERO
                x[0] = x[0] + x[4]
                x[1] = x[1] + x[5]
                x[2] = x[2] + x[6]
                PA[s] = _predict_block(PA[s], Q_POS)
                PS[s] = _predict_block(PS[s], Q_AREA)
                PR[s] = PR[s] + Q_ASPECT
                if tsu[s] > 0:
                    streak[s] = 0
                tsu[s] += 1
                bx = state_box(x[0], x[1], x[2], x[3])
                if not np.isfinite(np.array(bx)).all():
                    if branches is not None:
                        branches.append("freed")
                    free_slot(s)
                    ended += 1
                else:
                    tbox[s] = bx
            # 2. gains, 3. association
            rows = sorted(tbox)
            G = gains([tbox[s] for s in rows], boxes[f, det, :4]) if rows and det else np.zeros((len(rows), len(det)), dtype=np.float32)
            took, branch = associate(G, thr)
            if branches is not None:
                branches.append(branch)
            taken = set()
            for i, s in enumerate(rows):
                if took[i] < 0:
                    continue
                # 4. update
                j = det[took[i]]
                taken.add(j)
                match[f, s] = j
                tsu[s] = 0
                hits[s] += 1
                streak[s] += 1
                z = measurement(boxes[f, j, :4])
                x = X[s]
                k0, k1, PA[s] = _update_block(PA[s], R_POS)
                e = z[0] - x[0]
                x[0] = x[0] + k0 * e
                x[4] = x[4] + k1 * e
                e = z[1] - x[1]
                x[1] = x[1] + k0 * e
                x[5] = x[5] + k1 * e
                k0, k1, PS[s] = _update_block(PS[s], R_AREA)
                e = z[2] - x[2]
                x[2] = x[2] + k0 * e
                x[6] = x[6] + k1 * e
                S = PR[s] + R_ASPECT
                k = PR[s] / S
                e = z[3] - x[3]
                x[3] = x[3] + k * e
                m = ONE - k
                PR[s] = (m * m) * PR[s] + (k * k) * R_ASPECT
            # 5. birth
            for j in det:
                if j in taken:
                    continue
                free = [s for s in range(slots) if tid[s] == 0]
                if not free:
                    dropped += 1
                    continue
                s = free[0]
                next_id = (next_id + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31
                tid[s], tsu[s], hits[s], streak[s] = next_id, 0, 0, 0
                z = measurement(boxes[f, j, :4])
                X[s] = [z[0], z[1], z[2], z[3], ZERO, ZERO, ZERO]
                PA[s] = PS[s] = (P0_X, ZERO, P0_V)
                PR[s] = P0_X
                match[f, s] = j
                born += 1
            # 6. report, then retire
            for s in range(slots):
                if tid[s] == 0:
                    continue
                ids[f, s] = tid[s]
                x = X[s]
                bx = state_box(x[0], x[1], x[2], x[3])
                live[f, s] = bx
                if tsu[s] < 1 and (streak[s] >= min_hits or frame_count <= min_hits):
                    tracks[f, s, :4] = bx
                    tracks[f, s, 4:] = boxes[f, match[f, s], 4:]
                if tsu[s] > max_age:
                    free_slot(s)
                    ended += 1
            counts[f] = (born, ended, dropped, ignored)

    out = np.zeros_like(words)
    fo = out.view(np.float32)
    out[0], out[1] = next_id, frame_count
    for s in range(slots):
        if tid[s] == 0:
            continue
        b = base(s)
        out[b:b + 4] = (tid[s], tsu[s], hits[s], streak[s])
        fo[b + 4:b + 11] = X[s]
        fo[b + 11:b + 14] = PA[s]
        fo[b + 14:b + 17] = PS[s]
        fo[b + 17] = PR[s]
    return tracks, ids, match, live, counts, out


# ------------------------------------------------------------------ the published algorithm in float64

F7 = np.eye(7)
F7[0, 4] = F7[1, 5] = F7[2, 6] = 1.0
H7 = np.eye(4, 7)
R7 = np.diag([1.0, 1.0, 10.0, 10.0])
Q7 = np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001])
P7 = np.diag([10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4])


def _box64(x):
    with np.errstate(all="ignore"):
        w = np.sqrt(x[2] * x[3])
        h = x[2] / w
        return np.array([x[0] - w / 2, x[1] - h / 2, x[0] + w / 2, x[1] + h / 2])


def _z64(b):
    w, h = b[2] - b[0], b[3] - b[1]
    return np.array([b[0] + w / 2, b[1] + h / 2, w * h, w / h])


def _iou64(t, d):
    with np.errstate(all="ignore"):
        w = max(0.0, min(t[2], d[2]) - max(t[0], d[0]))
        h = max(0.0, min(t[3], d[3]) - max(t[1], d[1]))
        o = w * h / ((t[2] - t[0]) * (t[3] - t[1]) + (d[2] - d[0]) * (d[3] - d[1]) - w * h)
    return o if o > 0 else 0.0


def _partial_matchings(R, D):
    """Every injective partial map rows -> detections as a tuple of length R (-1 = unmatched)."""
    for k in range(min(R, D) + 1):
        for rows in itertools.combinations(range(R), k):
            for cols in itertools.permutations(range(D), k):
                m = [-1] * R
                for i, j in zip(rows, cols):
                    m[i] = j
                yield tuple(m)


def best_assignment_f64(G, thr, margin=1e-3):
    """The matching of maximal total gain and what survives the threshold -> took [R].  Asserts that every matching which keeps a
    DIFFERENT set of pairs after the threshold has a total at least `margin` lower (margin None: not checked)."""
    R, D = G.shape
    keep = lambda m: tuple(j if j >= 0 and not G[i, j] < thr else -1 for i, j in enumerate(m))
    total = lambda m: sum(G[i, j] for i, j in enumerate(m) if j >= 0)
    if R <= 7 and D <= 7:
        scored = sorted(((total(m), m) for m in _partial_matchings(R, D)), reverse=True)
        best = keep(scored[0][1])
        if margin is not None:
            for t, m in scored[1:]:
                if keep(m) != best:
                    assert scored[0][0] - t >= margin, ("runner-up too close", scored[0], (t, m))
                    break
        return np.array(best)
    from scipy.optimize import linear_sum_assignment
    pad = np.hstack([G, np.zeros((R, R))])                           # a dummy per row: any row may stay unmatched
    solve = lambda M: (lambda r, c: (M[r, c].sum(), c))(*linear_sum_assignment(M, maximize=True))
    top, cols = solve(pad)
    best = keep(tuple(int(c) if c < D else -1 for c in cols))
    if margin is not None:                                           # the runner-up differs in a kept pair: forbid each in turn
        for i, j in enumerate(best):
            if j < 0:
                continue
            M = pad.copy()
            M[i, j] = -1e9
            t, c2 = solve(M)
            if keep(tuple(int(c) if c < D else -1 for c in c2)) != best:
                assert top - t >= margin, ("runner-up too close", top, t, i, j)
    return np.array(best)


def sort_f64(boxes, n_boxes, slots, conf=0.1, iou_threshold=0.3, max_age=1, min_hits=3, thr_margin=0.02, assign_margin=1e-3):
    """-> (tracks float64 [F, slots, 6], ids, match, live float64 [F, slots, 4], counts); a fresh stream.  Tracks sit in the lowest
    free slot like the definition's, so that the outputs compare entry by entry; conf and iou_threshold are taken as the float32
    values the device gets, so that a score or threshold test means the same on both sides."""
    boxes = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    F, B, _ = boxes.shape
    conf, thr = float(f32(conf)), float(f32(iou_threshold))
    trk = [None] * slots                                             # dict(id, tsu, hits, streak, x, P)
    next_id = frame_count = 0
    tracks = np.zeros((F, slots, 6))
    ids = np.zeros((F, slots), dtype=np.int32)
    match = np.full((F, slots), -1, dtype=np.int32)
    live = np.zeros((F, slots, 4))
    counts = np.zeros((F, 4), dtype=np.int32)
    for f in range(F):
        n = B if n_boxes is None else min(max(int(n_boxes[f]), 0), B)
        det = detections(boxes[f], n, conf)
        born = ended = dropped = 0
        frame_count += 1
        tb = {}
        for s, t in enumerate(trk):
            if t is None:
                continue
            if t["x"][6] + t["x"][2] <= 0:
                t["x"][6] = 0.0
            t["x"] = F7 @ t["x"]
            t["P"] = F7 @ t["P"] @ F7.T + Q7
            if t["tsu"] > 0:
                t["streak"] = 0
            t["tsu"] += 1
            bx = _box64(t["x"])
            if not np.isfinite(bx).all():
                trk[s] = None
                ended += 1
            else:
                tb[s] = bx
        rows = sorted(tb)
        G = np.array([[_iou64(tb[s], boxes[f, j, :4]) for j in det] for s in rows]).reshape(len(rows), len(det))
        took = np.full(len(rows), -1)
        if rows and det:
            assert (np.abs(G - thr) >= thr_margin).all(), ("a gain within the margin of the threshold", f, G, thr)
            over = G > thr
            if over.sum(axis=1).max() <= 1 and over.sum(axis=0).max() <= 1:
                for i, j in zip(*np.nonzero(over)):
                    took[i] = j
            else:
                took = best_assignment_f64(G, thr, assign_margin)
        taken = set()
        for i, s in enumerate(rows):
            if took[i] < 0:
                continue
            j = det[took[i]]
            taken.add(j)
            match[f, s] = j
            t = trk[s]
            t["tsu"] = 0
            t["hits"] += 1
            t["streak"] += 1
            P = t["P"]
            S = H7 @ P @ H7.T + R7
            K = P @ H7.T @ np.linalg.inv(S)
            t["x"] = t["x"] + K @ (_z64(boxes[f, j, :4]) - H7 @ t["x"])
            A = np.eye(7) - K @ H7
            t["P"] = A @ P @ A.T + K @ R7 @ K.T
        for j in det:
            if j in taken:
                continue
            free = [s for s in range(slots) if trk[s] is None]
            if not free:
                dropped += 1
                continue
            next_id += 1
            x = np.zeros(7)
            x[:4] = _z64(boxes[f, j, :4])
            trk[free[0]] = dict(id=next_id, tsu=0, hits=0, streak=0, x=x, P=P7.copy())
            match[f, free[0]] = j
            born += 1
        for s, t in enumerate(trk):
            if t is None:
                continue
            ids[f, s] = t["id"]
            bx = _box64(t["x"])
            live[f, s] = bx
            if t["tsu"] < 1 and (t["streak"] >= min_hits or frame_count <= min_hits):
                tracks[f, s, :4] = bx
                tracks[f, s, 4:] = boxes[f, match[f, s], 4:]
            if t["tsu"] > max_age:
                trk[s] = None
                ended += 1
        counts[f] = (born, ended, dropped, n - len(det))
    return tracks, ids, match, live, counts


# ------------------------------------------------------------------ scenes the host and GPU tests share

def scene_rows(F, max_boxes, objects, seed=0, jitter=0.0, score=lambda f, k: 0.9 - 0.1 * k):
    """objects: functions f -> (cx, cy, w, h) or None (missed in that frame).  -> boxes float32 [F, max_boxes, 6] with each frame's
    rows in descending score order as the detector leaves them, n_boxes int32 [F], owner int [F, max_boxes] (the object of a row, -1)."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((F, max_boxes, 6), dtype=np.float32)
    n = np.zeros(F, dtype=np.int32)
    owner = np.full((F, max_boxes), -1)
    for f in range(F):
        rows = []
        for k, obj in enumerate(objects):
            o = obj(f)
            if o is None:
                continue
            cx, cy, w, h = np.asarray(o, dtype=np.float64) + (rng.uniform(-jitter, jitter, 4) if jitter else 0.0)
            rows.append((score(f, k), k, (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)))
        rows.sort(key=lambda r: -r[0])
        for j, (sc, k, b) in enumerate(rows[:max_boxes]):
            boxes[f, j] = (*b, sc, float(k % 3))
            owner[f, j] = k
        n[f] = min(len(rows), max_boxes)
    return boxes, n, owner


def behaviour_scene(F=30, max_boxes=4, min_hits=3, miss=(14, 1), alarm=9):
    """Two objects whose score order swaps every 4 frames; object 1 is missed in frame miss[0] .. miss[0] + miss[1] - 1; a
    one-frame false alarm far from both in frame `alarm` (> min_hits)."""
    assert alarm > min_hits
    a = lambda f: (150.0 + 3.0 * f, 200.0 + 1.0 * f, 80.0, 120.0)
    b = lambda f: None if miss[0] <= f < miss[0] + miss[1] else (450.0 - 2.0 * f, 320.0, 100.0, 60.0)
    c = lambda f: (90.0, 560.0, 50.0, 50.0) if f == alarm else None
    score = lambda f, k: (0.55, 0.8 if (f // 4) % 2 else 0.3, 0.45)[k]
    return scene_rows(F, max_boxes, [a, b, c], score=score)
