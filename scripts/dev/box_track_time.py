#!/usr/bin/env python3
"""Time bf_track_boxes_device beside what it replaces and beside the launch it feeds (dev tool; GPU box, no CPU fallback):
  track    one replay of a captured graph holding the bf_track_boxes_device launch                  (the code under test)
  fuse     one replay of a captured graph holding the bf_fuse_boxes_device launch on its d_tracks  (the neighbour in the chain)
  d2h      boxes.cpu() and n_boxes.cpu()                                                           (the host round trip it removes:
  numpy    the plain NumPy loop of tests/box_track_np.py on those                                   copy down, track on the host,
  h2d      the [F, slots, 6] tracked rows .cuda()                                                   copy up)
at two points: the streaming use (one frame, 8 detections in a [1, 300, 6] detector output, 16 slots) and a deliberately heavy one
(64 frames of 300 detections each, 64 slots: drifting, densely overlapping boxes, so most frames run the assignment).  The
tracker's state carries from replay to replay as it does in a stream; the result of the first call from a zeroed state is compared
with the NumPy loop, byte for byte, before anything is timed.
Device events around back-to-back graph replays after a warm-up, ROUNDS alternating rounds in one process, medians and minima; the
host parts are timed with a host clock around work that ends in a synchronise.  The kernel is one workgroup and latency-bound: no
rate or share of peak is derived.  Nothing is asserted about time.
usage: python scripts/dev/box_track_time.py [--rounds 9] [--out profiles/box_track_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from lib import _native as nat
import box_track_np as bt

ROWS, COLS, PER, IMG = 57, 32, 256, 640
SIZES = [dict(name="streaming", frames=1, max_boxes=300, detections=8, slots=16, replays=200),
         dict(name="heavy", frames=64, max_boxes=300, detections=300, slots=64, replays=3)]
CONF, IOU, MAX_AGE, MIN_HITS = 0.1, 0.3, 1, 3


def scene(frames, max_boxes, detections, seed=7):
    """`detections` boxes drifting over a 640 x 640 frame, each frame's rows in descending score order as the detector leaves them."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(60, IMG - 60, (detections, 2))
    vel = rng.uniform(-3, 3, (detections, 2))
    wh = rng.uniform(30, 90, (detections, 2))
    boxes = np.zeros((frames, max_boxes, 6), dtype=np.float32)
    for f in range(frames):
        cc = c + vel * f + rng.uniform(-1, 1, (detections, 2))
        order = np.argsort(-rng.uniform(0.2, 0.95, detections))
        boxes[f, :detections, 0:2] = (cc - wh / 2)[order]
        boxes[f, :detections, 2:4] = (cc + wh / 2)[order]
        boxes[f, :detections, 4] = np.sort(rng.uniform(0.2, 0.95, detections))[::-1]
        boxes[f, :detections, 5] = (order % 3).astype(np.float32)
    return boxes, np.full(frames, detections, dtype=np.int32)


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


def one_size(name, frames, max_boxes, detections, slots, replays, rounds):
    lib = nat.lib
    F, B, S = frames, max_boxes, slots
    h_boxes, h_n = scene(F, B, detections)
    boxes, n = torch.from_numpy(h_boxes).cuda(), torch.from_numpy(h_n).cuda()
    state = torch.zeros((lib.bf_box_track_state_words(S),), dtype=torch.int32, device="cuda")
    tracks = torch.empty((F, S, 6), dtype=torch.float32, device="cuda")
    ids, match = (torch.empty((F, S), dtype=torch.int32, device="cuda") for _ in range(2))
    live = torch.empty((F, S, 4), dtype=torch.float32, device="cuda")
    counts = torch.empty((F, 4), dtype=torch.int32, device="cuda")
    maps = torch.rand((F, ROWS * COLS), generator=torch.Generator().manual_seed(3)).cuda()
    peak = torch.empty((F, S), dtype=torch.int32, device="cuda")

    def track():
        rc = lib.bf_track_boxes_device(boxes.data_ptr(), n.data_ptr(), F, B, CONF, S, IOU, MAX_AGE, MIN_HITS, state.data_ptr(), tracks.data_ptr(), ids.data_ptr(),
                                       match.data_ptr(), live.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.bf_last_error()

    def fuse():
        rc = lib.bf_fuse_boxes_device(maps.data_ptr(), F, ROWS * COLS, ROWS, COLS, PER, tracks.data_ptr(), None, S, IMG, IMG, CONF, None, 0, peak.data_ptr(), None,
                                      None, None, None, None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.bf_last_error()

    track()
    torch.cuda.synchronize()
    branches = []
    want = bt.track_boxes_np(h_boxes, h_n, S, CONF, IOU, MAX_AGE, MIN_HITS, branches=branches)
    for got, w in zip((tracks, ids, match, live, counts, state), want):
        assert got.cpu().numpy().tobytes() == w.tobytes(), "the launch and the NumPy loop disagree"
    g_track, g_fuse = graph_of(track), graph_of(fuse)
    for _ in range(2):
        timed_replays(g_track, replays); timed_replays(g_fuse, replays)
    t = {"track": [], "fuse": [], "d2h": [], "numpy": [], "h2d": []}
    for _ in range(rounds):
        t["track"].append(timed_replays(g_track, replays))
        t["fuse"].append(timed_replays(g_fuse, replays))
        dt, (hb, hn) = host_clock(lambda: (boxes.cpu().numpy(), n.cpu().numpy()))
        t["d2h"].append(dt)
        dt, res = host_clock(lambda: bt.track_boxes_np(hb, hn, S, CONF, IOU, MAX_AGE, MIN_HITS))
        t["numpy"].append(dt)
        dt, _ = host_clock(lambda: torch.from_numpy(res[0]).cuda())
        t["h2d"].append(dt)
    med = {k: statistics.median(v) for k, v in t.items()}
    host = med["d2h"] + med["numpy"] + med["h2d"]
    rec = {"point": name, "frames": F, "max_boxes": B, "detections_per_frame": detections, "slots": S, "iou_threshold": IOU, "max_age": MAX_AGE,
           "min_hits": MIN_HITS, "frames_through_the_assignment_in_first_call": branches.count("assignment"),
           "tracks_born_in_first_call": int(want[4][:, 0].sum()), "rounds": rounds, "replays_per_round": replays,
           "track_us": {"median": round(med["track"], 2), "min": round(min(t["track"]), 2)}, "track_us_per_frame": round(med["track"] / F, 2),
           "fuse_us": {"median": round(med["fuse"], 2), "min": round(min(t["fuse"]), 2)},
           "d2h_us": {"median": round(med["d2h"], 1), "min": round(min(t["d2h"]), 1)},
           "numpy_us": {"median": round(med["numpy"], 1), "min": round(min(t["numpy"]), 1)},
           "h2d_us": {"median": round(med["h2d"], 1), "min": round(min(t["h2d"]), 1)},
           "host_round_trip_us": round(host, 1), "copies_alone_us": round(med["d2h"] + med["h2d"], 1),
           "ratio_track_over_fuse": round(med["track"] / med["fuse"], 2), "ratio_host_over_track": round(host / med["track"], 1),
           "ratio_copies_over_track": round((med["d2h"] + med["h2d"]) / med["track"], 2),
           "timing": "device events around back-to-back graph replays (track, fuse); host clock around each host part, ending in a synchronise"}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("box_track_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("box_track_time: no usable HIP device; this measurement has no CPU fallback")
    recs = [one_size(rounds=args.rounds, **sz) for sz in SIZES]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": recs}, f, indent=1)
            f.write("\n")
