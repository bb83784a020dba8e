"""Inputs of tests/test_postproc_f64.py, built from seeds: the CPU tests assert the caps and keep-clear conditions on exactly the
arrays the GPU tests hand to the kernels."""
import functools

import numpy as np

import util


def golden_map(name, sig):
    return np.ascontiguousarray(util.golden(name)["img_lerp_" + sig], dtype=np.float32)


def beam_map(X, Y, seed):
    """A synthetic power map: one to three Gaussian lobes over a rough floor, three to seven decades of range."""
    rng = np.random.default_rng(seed)
    x, y = np.arange(X, dtype=np.float64)[:, None], np.arange(Y, dtype=np.float64)[None, :]
    m = 10.0 ** rng.uniform(-6, -4) * (1.0 + 0.3 * rng.random((X, Y)))
    for _ in range(int(rng.integers(1, 4))):
        cx, cy, w = rng.uniform(0, X), rng.uniform(0, Y), rng.uniform(0.08, 0.3) * max(X, Y, 4)
        m += 10.0 ** rng.uniform(-3, 1) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * w * w))
    return m.astype(np.float32)


def wave_map(das_oracle, name, x0, y0, seed):
    """A synth plane wave from direction (x0, y0) through the delay-and-sum oracle (lerp) at a size of oracle/configs.py."""
    import synth
    c = util.CONFIGS[name]
    d = util.oracle_delays(name)
    orc = das_oracle.Oracle(c["N"], c["X"], c["Y"], c["T"])
    return orc.mimo_lerp(synth.s3_plane_wave(d[x0, y0], c["N"], seed=seed), np.float32(d), np.arange(c["M"], dtype=np.int32))


_COLOR = {}


def color_cases(das_oracle):
    """-> list of dict(name, maps float32 [F, X, Y], threshold, amount, exponent)."""
    if _COLOR:
        return _COLOR["cases"]
    cases = []

    def add(name, maps, threshold=1e-7, amount=0.5, exponent=5):
        cases.append(dict(name=name, maps=np.ascontiguousarray(np.stack(maps), dtype=np.float32), threshold=threshold, amount=amount, exponent=exponent))

    g2 = [golden_map("cfg2", s) for s in ("s1", "s2", "s3")]
    maps = []
    for f in range(190):                                   # every frame a different map; every fifth one quiet (under the threshold)
        m = g2[f % 3] * np.float32(1.7 ** (f // 3 % 9 - 4)) if f % 2 == 0 else beam_map(101, 101, 1000 + f)
        if f % 5 == 3:
            m = m * np.float32(5e-8 / m.max())
        maps.append(m)
    add("101x101 F=190 mixed quiet", maps)
    add("101x101 F=64 threshold 0", [beam_map(101, 101, 2000 + f) if f % 4 else g2[f // 4 % 3] * np.float32(0.37 + f) for f in range(64)], 0.0, 0.25, 2)
    g1 = [golden_map("cfg1", s) for s in ("s1", "s2", "s3")]
    add("11x11 F=7 plane waves", g1 + [wave_map(das_oracle, "cfg1", 2 + 2 * i, 9 - 2 * i, 40 + i) for i in range(4)], 1e-7, 0.75, 1)
    gs = [golden_map("shipped", s) for s in ("s1", "s2", "s3")]
    add("57x32 F=2 exponent 0.5", [gs[0], wave_map(das_oracle, "shipped", 40, 7, 50)], 1e-7, 0.5, 0.5)
    add("57x32 F=3 golden", gs)
    add("57x32 F=1 amount 1.5", [gs[2]], 1e-7, 1.5, 5)
    add("64x64 F=2", [beam_map(64, 64, 3000), beam_map(64, 64, 3001)])
    add("63x65 F=2", [beam_map(63, 65, 3002), beam_map(63, 65, 3003)])
    add("1x1 F=2", [np.full((1, 1), 3.0), np.zeros((1, 1))])
    add("1x40 F=2", [beam_map(1, 40, 3004), beam_map(1, 40, 3005)])
    add("361x361 F=1", [golden_map("cfg5", "s2")])
    add("11x11 F=2 threshold = max of frame 0", [g1[2], g1[2] * np.float32(2.0)], float(g1[2].max()))
    rng = np.random.default_rng(77)
    mixed = beam_map(11, 11, 3006)
    mixed[rng.random((11, 11)) < 0.2] = 0.0
    mixed[rng.random((11, 11)) < 0.1] = -1.0
    inf, nan = beam_map(11, 11, 3007), beam_map(11, 11, 3008)
    inf[3, 4], nan[7, 2] = np.inf, np.nan
    add("11x11 F=7 degenerate", [np.zeros((11, 11)), np.full((11, 11), 3.5), mixed, inf, nan, np.full((11, 11), -2.0), beam_map(11, 11, 3009)])
    _COLOR["cases"] = cases
    return cases


def blob(X, Y, cx, cy, sigma=4.0, floor=1e-3):
    x, y = np.arange(X, dtype=np.float64)[:, None], np.arange(Y, dtype=np.float64)[None, :]
    return (floor + np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def center_cases():
    """-> tuple of (name, maps float32 [frames, X, Y]); frames in {1, 3, 64}.  cfg2 s3 stays out: a smoothed pixel of it lies 8.8e-6 from
    the 95 % line."""
    X = Y = 101
    e = X - 1
    named = [blob(X, Y, 50, 50), blob(X, Y, 0, 47), blob(X, Y, e, 52), blob(X, Y, 45, 0), blob(X, Y, 58, e),
             blob(X, Y, 0, 0), blob(X, Y, 0, e), blob(X, Y, e, 0), blob(X, Y, e, e), blob(X, Y, 1, 1, 2.0),
             blob(X, Y, 30, 40) + blob(X, Y, 70, 40), np.full((X, Y), 2.5, np.float32), np.zeros((X, Y), np.float32),
             golden_map("cfg2", "s1"), golden_map("cfg2", "s2")]
    hot = np.zeros((X, Y), np.float32)
    hot[17, 88] = 4.0
    named.append(hot)
    rng = np.random.default_rng(5)
    while len(named) < 64:
        named.append(blob(X, Y, rng.uniform(0, e), rng.uniform(0, e), rng.uniform(1.5, 9.0)) + np.float32(0.5) * blob(X, Y, rng.uniform(0, e), rng.uniform(0, e), 3.0))
    small = lambda a, b, s: np.random.default_rng(s).uniform(0.1, 1.0, (a, b)).astype(np.float32)
    hot5 = np.zeros((1, 5), np.float32)
    hot5[0, 3] = 1.0
    return (("101x101 x64", np.stack(named)),
            ("57x32 x3 golden", np.stack([golden_map("shipped", s) for s in ("s1", "s2", "s3")])),
            ("32x57 x3", np.stack([blob(32, 57, 31, 20), blob(32, 57, 10, 56, 2.5), np.ascontiguousarray(golden_map("shipped", "s1").T)])),
            ("11x11 x3 golden", np.stack([golden_map("cfg1", s) for s in ("s1", "s2", "s3")])),
            ("2x3 x3", np.stack([small(2, 3, 1), np.full((2, 3), 0.7, np.float32), np.zeros((2, 3), np.float32)])),
            ("1x5 x3", np.stack([small(1, 5, 2), hot5, np.zeros((1, 5), np.float32)])),
            ("361x361 x1", np.stack([golden_map("cfg5", "s1")])))


def letterbox_cases():
    """-> list of (h, w, out_h, out_w, new_h, new_w, top, left, value)."""
    from image_detection.src.yolo_smooth_tracking import letterbox_geometry
    out = []
    for h, w in ((360, 640), (640, 360), (480, 640), (320, 320), (333, 517), (517, 333), (1080, 1920), (8, 8)):
        nh, nw, top, left, oh, ow, _ = letterbox_geometry(h, w)
        out.append((h, w, oh, ow, nh, nw, top, left, 114))
    out += [(37, 53, 64, 96, 45, 71, 3, 5, 0), (37, 53, 64, 96, 45, 71, 3, 5, 255)]       # a hand-made placement, top and left odd
    return out


DECODE_LEVELS = (((80, 80), (40, 40), (20, 20)), ((48, 80), (24, 40), (12, 20)), ((7, 5), (3, 9), (1, 2)))
DECODE_CASES = [(nc, lv, B) for nc, lv, B in ((1, 0, 1), (3, 1, 3), (80, 1, 1), (80, 2, 3), (3, 0, 1), (1, 2, 3), (3, 2, 1))]
DECODE_CONF = 0.1


@functools.lru_cache(maxsize=None)
def decode_raw(nc, lv, B):
    """Head maps float32 [B, 3 * (5 + nc), h, w] on a 1/64 lattice inside [-8, 8] (exact in float16; two class logits are equal --
    a tie, which argmax gives to the lower id -- or 1/64 apart, which no float32 sigmoid confuses)."""
    rng = np.random.default_rng(nc * 100 + lv * 10 + B)
    raw = []
    for h, w in DECODE_LEVELS[lv]:
        r = np.clip(np.rint(rng.normal(0, 1.5, (B, 3, 5 + nc, h, w)) * 64) / 64, -8, 8)
        r[:, :, 4] = np.clip(np.rint(rng.normal(-1.0, 2.0, (B, 3, h, w)) * 64) / 64, -8, 8)
        if nc > 1:
            r[:, :, 5, ::2, :] = r[:, :, 5 + nc - 1, ::2, :]           # planted ties between the first and the last class
        raw.append(np.ascontiguousarray(r.reshape(B, 3 * (5 + nc), h, w), dtype=np.float32))
    return tuple(raw)


NMS_CASES = [  # (K, counts per image, max_det, iou_thres)
    (1, (1, 0), 1, 0.45),
    (63, (63, 0, 17), 300, 0.45),
    (64, (64, 1, 33), 64, 0.0),
    (65, (65, 64, 0, 1), 1, 0.45),
    (1000, (1000, 0, 1, 999, 937, 64, 500, 130), 300, 0.45),
    (1024, (1024, 1000), 1024, 1.0),
    (4000, (4000, 3970), 300, 0.45),
    (4096, (4096, 0, 4033), 4096, 0.45),
    (4096, (4096,), 300, 0.0),
]


@functools.lru_cache(maxsize=None)
def nms_inputs(case):
    """Sorted candidates of NMS_CASES[case]: clusters of boxes on a quarter-pixel lattice (sides 12 .. 40 pixels), shuffled so that the members
    of a cluster lie anywhere in the score order; image 0 has clusters of two (many survivors: max_det cuts), the others of about six
    (chains).  A box of a pair whose IoU comes within 1e-5 of the threshold is widened by a quarter pixel until none is left.
    -> boxes [B, K, 4], scores [B, K] (descending, -1 past counts[b]), cls [B, K] int32, counts [B] int32."""
    import detect_np as D
    K, counts, max_det, thr = NMS_CASES[case]
    B = len(counts)
    rng = np.random.default_rng(1000 + case)
    boxes = np.full((B, K, 4), 1e4, dtype=np.float32)                 # entries past counts[b] are never read: far-away sentinels
    scores = np.full((B, K), -1.0, dtype=np.float32)
    for b, n in enumerate(counts):
        if n == 0:
            continue
        per = 2 if b == 0 else 6
        centre = rng.uniform(40, 600, ((n + per - 1) // per, 2))
        c = (np.repeat(centre, per, axis=0)[:n] + rng.uniform(-9, 9, (n, 2)))[rng.permutation(n)]
        wh = rng.uniform(12, 40, (n, 2))
        bx = np.rint(np.concatenate([c - wh / 2, c + wh / 2], axis=1) * 4) / 4
        for _ in range(20):
            iou = D.iou_matrix_f64(bx)
            near = np.triu(np.abs(iou - thr) < 1e-5, 1) & ((iou > 0) if thr == 0.0 else (thr < 1.0))
            if not near.any():
                break
            bx[np.unique(np.nonzero(near)[1]), 2] += 0.25
        boxes[b, :n] = bx
        scores[b, :n] = np.linspace(0.99, 0.02, n, dtype=np.float32) if n > 1 else 0.5
    cls = rng.integers(0, 80, (B, K)).astype(np.int32)
    return boxes, scores, cls, np.asarray(counts, dtype=np.int32)


def nms_keeps_clear(boxes, thr):
    """The condition under which float32 and float64 take the same greedy decisions: no pair's IoU within 1e-5 of the threshold.  Two
    thresholds are decided exactly on the lattice in either precision and are judged by that instead: at 0 a pair overlaps or it does
    not (the intersection of quarter-pixel boxes is exact; disjoint pairs, IoU = 0, are therefore not counted), at 1 nothing exceeds it
    (intersection <= union holds exactly)."""
    import detect_np as D
    if thr >= 1.0:
        return True
    iou = D.iou_matrix_f64(boxes)
    near = np.triu(np.abs(iou - thr) < 1e-5, 1)
    if thr == 0.0:
        near &= iou > 0
    return not near.any()
