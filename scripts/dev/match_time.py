#!/usr/bin/env python3
"""Time bf_match_boxes_device beside what it replaces and beside the launch it precedes (dev tool; GPU box, no CPU fallback):
  match    one replay of a captured graph holding the bf_match_boxes_device launch on the smoother's state rows   (the code under test)
  pair     ... holding that launch and the bf_smooth_boxes_device launch behind it                                (one frame of SmoothDetections)
  track    ... holding the bf_track_boxes_device launch on the smoother's output                                  (the neighbour in the chain)
  d2h      the current image, the previous image and the state .cpu()                                             (the host round trip it removes:
  numpy    the NumPy restatement of tests/match_np.py on those                                                     copy down, match on the host,
  h2d      the moved boxes and scores .cuda()                                                                      copy up)
at two points on a 640 x 640 frame: the streaming use (8 previous boxes of about 80 x 160 on 16 slots; their templates are decimated
by 2) and a deliberately heavy one (16 boxes of 212 x 212, templates of 254 x 254 at the cap: q = 2, P = 16129).  The current image is
the previous one rolled by (4, -2) over random texture (on the lattice of q = 2).  The detector rows repeat the state's boxes as 0.5 candidates, so the state
is the same after every replay.  The first call's outputs are compared with the restatement, byte for byte, before anything is timed.
Device events around back-to-back graph replays after a warm-up, ROUNDS alternating rounds in one process, medians and minima; the
host parts are timed with a host clock around work that ends in a synchronise.  The rate reported is the byte multiply-adds of the
sums of products alone (positions x P x 3 per box, counted from the shapes) over the match launch's time; the launch also sums
squares and channels per position, which the count leaves out.  Nothing is asserted about time.
usage: python scripts/dev/match_time.py [--rounds 9] [--out profiles/match_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from lib import _native as nat
import match_np as mn

IMG, MAX_BOXES, T_PCT, S_PCT = 640, 300, 120, 150
LOW, HIGH, IOU, CORR = 0.3, 0.7, 0.5, 0.8
SIZES = [dict(name="streaming", boxes=8, w=80, h=160, slots=16, replays=200),
         dict(name="heavy", boxes=16, w=212, h=212, slots=16, replays=20)]


def scene(boxes, w, h, seed=7):
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, 256, (IMG, IMG, 3), dtype=np.uint8)
    cur = np.roll(prev, (-2, 4), axis=(0, 1))
    mx, my = int(0.75 * w) + 8, int(0.75 * h) + 8          # the search area stays on the frame
    x1 = rng.uniform(mx - w / 2, IMG - mx - w / 2, boxes)
    y1 = rng.uniform(my - h / 2, IMG - my - h / 2, boxes)
    rows = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)
    return prev, cur, rows


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def timed_replays(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / replays * 1e3        # us per replay


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def one_size(name, boxes, w, h, slots, replays, rounds):
    lib = nat.lib
    S, B = slots, MAX_BOXES
    h_prev, h_cur, rows = scene(boxes, w, h)
    h_state = np.zeros(mn.state_words(S), dtype=np.int32)
    h_state[0] = boxes
    h_state[4:4 + 4 * boxes] = rows.ravel().view(np.int32)
    h_det = np.zeros((B, 6), dtype=np.float32)
    h_det[:boxes, :4], h_det[:boxes, 4] = rows, 0.5
    prev, cur, det = (torch.from_numpy(a).cuda() for a in (h_prev, h_cur[None].copy(), h_det))
    state = torch.from_numpy(h_state).cuda()
    moved = torch.empty((S, 4), dtype=torch.float32, device="cuda")
    score = torch.empty((S,), dtype=torch.float32, device="cuda")
    status = torch.empty((S,), dtype=torch.int32, device="cuda")
    out = torch.empty((1, B, 6), dtype=torch.float32, device="cuda")
    t_state = torch.zeros((lib.bf_box_track_state_words(S),), dtype=torch.int32, device="cuda")
    tracks = torch.empty((1, S, 6), dtype=torch.float32, device="cuda")
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def match():
        rc = lib.bf_match_boxes_device(cur.data_ptr(), prev.data_ptr(), 1, IMG, IMG, state.data_ptr() + 16, 4, state.data_ptr(), S, T_PCT, S_PCT, moved.data_ptr(),
                                       score.data_ptr(), None, status.data_ptr(), stream())
        assert rc == 0, lib.bf_last_error()

    def pair():
        match()
        rc = lib.bf_smooth_boxes_device(det.data_ptr(), None, B, LOW, HIGH, IOU, CORR, S, moved.data_ptr(), score.data_ptr(), status.data_ptr(), state.data_ptr(),
                                        out.data_ptr(), None, None, stream())
        assert rc == 0, lib.bf_last_error()

    def track():
        rc = lib.bf_track_boxes_device(out.data_ptr(), None, 1, B, 0.1, S, 0.3, 1, 3, t_state.data_ptr(), tracks.data_ptr(), None, None, None, None, stream())
        assert rc == 0, lib.bf_last_error()

    pair()
    torch.cuda.synchronize()
    info = []
    want = mn.match_boxes_np(h_cur[None], h_prev, rows[None], None, T_PCT, S_PCT, info)
    assert moved.cpu().numpy()[:boxes].tobytes() == want[0][0].tobytes() and score.cpu().numpy()[:boxes].tobytes() == want[1][0].tobytes(), \
        "the launch and the restatement disagree"
    assert (want[2][0] == (4, -2)).all() and (want[1][0] == 1).all() and state.cpu().numpy().tobytes() == h_state.tobytes()
    macs = sum(n["nu"] * n["nv"] * n["P"] * 3 for n in info)
    g_match, g_pair, g_track = graph_of(match), graph_of(pair), graph_of(track)
    for _ in range(2):
        timed_replays(g_match, replays); timed_replays(g_pair, replays); timed_replays(g_track, replays)
    t = {"match": [], "pair": [], "track": [], "d2h": [], "numpy": [], "h2d": []}
    for _ in range(rounds):
        t["match"].append(timed_replays(g_match, replays))
        t["pair"].append(timed_replays(g_pair, replays))
        t["track"].append(timed_replays(g_track, replays))
        dt, (hc, hp, hs) = host_clock(lambda: (cur.cpu().numpy(), prev.cpu().numpy(), state.cpu().numpy()))
        t["d2h"].append(dt)
        dt, res = host_clock(lambda: mn.match_boxes_np(hc, hp, hs[4:].view(np.float32).reshape(1, S, 4), hs[:1], T_PCT, S_PCT))
        t["numpy"].append(dt)
        dt, _ = host_clock(lambda: (torch.from_numpy(res[0]).cuda(), torch.from_numpy(res[1]).cuda()))
        t["h2d"].append(dt)
    med = {k: statistics.median(v) for k, v in t.items()}
    host = med["d2h"] + med["numpy"] + med["h2d"]
    us = lambda k, nd=2: {"median": round(med[k], nd), "min": round(min(t[k]), nd)}
    rec = {"point": name, "image": [IMG, IMG], "boxes": boxes, "box_w_h": [w, h], "slots": S, "t_pct": T_PCT, "s_pct": S_PCT,
           "q": sorted({n["q"] for n in info}), "template_pixels_P": sorted({n["P"] for n in info}), "positions_per_box": sorted({n["nu"] * n["nv"] for n in info}),
           "byte_multiply_adds_of_the_products": macs, "rounds": rounds, "replays_per_round": replays,
           "match_us": us("match"), "pair_us": us("pair"), "track_us": us("track"), "d2h_us": us("d2h", 1), "numpy_us": us("numpy", 1), "h2d_us": us("h2d", 1),
           "host_round_trip_us": round(host, 1), "copies_alone_us": round(med["d2h"] + med["h2d"], 1),
           "byte_multiply_adds_per_second": round(macs / (med["match"] * 1e-6), -6),
           "ratio_match_over_track": round(med["match"] / med["track"], 2), "ratio_host_over_match": round(host / med["match"], 1),
           "ratio_copies_over_match": round((med["d2h"] + med["h2d"]) / med["match"], 2),
           "timing": "device events around back-to-back graph replays (match, pair, track); host clock around each host part, ending in a synchronise"}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("match_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("match_time: no usable HIP device; this measurement has no CPU fallback")
    recs = [one_size(rounds=args.rounds, **sz) for sz in SIZES]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": recs}, f, indent=1)
            f.write("\n")
