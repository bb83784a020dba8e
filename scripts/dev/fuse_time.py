#!/usr/bin/env python3
"""Time bf_fuse_boxes_device beside a neighbour in the chain and beside the host round trip it replaces (dev tool; GPU box, no CPU
fallback):
  fuse     one replay of a captured graph holding the bf_fuse_boxes_device call, every output asked for    (the code under test)
  peaks    one replay of a captured graph holding the bf_peaks_device launch on the same maps            (the neighbour in the chain)
  host     boxes, counts, sources and maps .cpu(), the NumPy restatement of tests/fuse_np.py (its whole-array form), the [F, 300]
           peak offsets .cuda()                                                                            (the alternative)
at the pipeline's shape: 64 frames, 300 rows of boxes on a 640 x 640 frame, maps of 101 x 101 (staged into LDS) and 57 x 32 (as
shipped).  The maps are lobes plus noise; the boxes are seeded, scores descending and straddling conf = 0.5, counts random per frame
as after NMS; 4 sources per frame come from the bf_peaks_device launch that is timed.  The result of the first call is compared with
the restatement before anything is timed.
Device events around REPLAYS back-to-back graph replays after a warm-up, ROUNDS alternating rounds in one process, medians and
minima; the host alternative is timed with a host clock around work that ends in a synchronise, and most of it is the restatement's
Python loop over boxes, not the copies (copies_us times the four .cpu() and the .cuda() alone).  Nothing is asserted about time.
usage: python scripts/dev/fuse_time.py [--rounds 9] [--out profiles/fuse_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from lib import _native as nat
import fuse_cases
import fuse_np

F, B, W, H, PER, K, CONF = 64, 300, 640, 640, 256, 4, 0.5
GRIDS = [(101, 101), (57, 32)]
REPLAYS = 50


def maps_for(rows, cols):
    g = torch.Generator(device="cpu").manual_seed(rows * 1000 + cols + F)
    x = torch.arange(rows, dtype=torch.float32)[None, :, None] / rows
    y = torch.arange(cols, dtype=torch.float32)[None, None, :] / cols
    t = torch.arange(F, dtype=torch.float32)[:, None, None]
    m = torch.zeros((F, rows, cols))
    for amp, x0, y0, dx, dy in ((1.0, 0.15, 0.2, 0.004, 0.001), (0.9, 0.8, 0.8, -0.003, -0.001), (0.8, 0.5, 0.5, 0.0, 0.0)):
        m += amp * torch.exp(-((x - x0 - dx * t) ** 2 + (y - y0 - dy * t) ** 2) / (2 * 0.05 ** 2))
    m += 0.05 * torch.rand((F, rows, cols), generator=g)
    return m.reshape(F, rows * cols).contiguous().cuda()


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def timed_replays(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPLAYS * 1e3        # us per replay


def one_grid(rows, cols, rounds):
    D = rows * cols
    lib = nat.lib
    rng = np.random.default_rng(rows * cols)
    maps = maps_for(rows, cols)
    boxes = torch.from_numpy(fuse_cases.random_boxes(rng, F, B, W, H, CONF)).cuda()
    counts = torch.from_numpy(rng.integers(0, B + 1, F).astype(np.int32)).cuda()
    src = torch.empty((F, K), dtype=torch.int32, device="cuda")
    peak, center = (torch.empty((F, B), dtype=torch.int32, device="cuda") for _ in range(2))
    power = torch.empty((F, B), dtype=torch.float32, device="cuda")
    rects = torch.empty((F, B, 4), dtype=torch.int32, device="cuda")
    src_box = torch.empty((F, K), dtype=torch.int32, device="cuda")
    out_counts = torch.empty((F, 3), dtype=torch.int32, device="cuda")

    host_peak = np.zeros((F, B), dtype=np.int32)

    def peaks():
        rc = lib.bf_peaks_device(maps.data_ptr(), F, D, rows, cols, 4, K, 0.25, 0.0, PER, src.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.bf_last_error()

    def fuse():
        rc = lib.bf_fuse_boxes_device(maps.data_ptr(), F, D, rows, cols, PER, boxes.data_ptr(), counts.data_ptr(), B, W, H, CONF, src.data_ptr(), K,
                                      peak.data_ptr(), power.data_ptr(), center.data_ptr(), rects.data_ptr(), src_box.data_ptr(), out_counts.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.bf_last_error()

    def copies():
        h = [t.cpu().numpy() for t in (maps, boxes, counts, src)]
        return h, torch.from_numpy(host_peak).cuda()

    def host():
        m, b, c, s = (t.cpu().numpy() for t in (maps, boxes, counts, src))
        return torch.from_numpy(fuse_np.fuse(m, rows, cols, PER, b, c, W, H, CONF, s, fast=True)[0]).cuda()

    peaks()
    fuse()
    torch.cuda.synchronize()
    want = fuse_np.fuse(maps.cpu().numpy(), rows, cols, PER, boxes.cpu().numpy(), counts.cpu().numpy(), W, H, CONF, src.cpu().numpy(), fast=True)
    for got, w in zip((peak, power, center, rects, src_box, out_counts), want):
        assert got.cpu().numpy().tobytes() == w.tobytes(), "the launch and the restatement disagree"
    g_peaks, g_fuse = graph_of(peaks), graph_of(fuse)
    for _ in range(3):
        timed_replays(g_peaks); timed_replays(g_fuse)
    t = {"fuse": [], "peaks": [], "host": [], "copies": []}
    for _ in range(rounds):
        t["fuse"].append(timed_replays(g_fuse))
        t["peaks"].append(timed_replays(g_peaks))
        for name, fn in (("host", host), ("copies", copies)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e6)
    med = {n: statistics.median(v) for n, v in t.items()}
    area = (want[3][..., 1] - want[3][..., 0] + 1) * (want[3][..., 3] - want[3][..., 2] + 1)
    rec = {"frames": F, "max_boxes": B, "rows": rows, "cols": cols, "img_w": W, "img_h": H, "n_src": K, "conf": CONF,
           "map_read": "staged in LDS" if D <= fuse_np.STAGE_MAX else "through L2",
           "boxes_per_frame": round(float(want[5][:, 0].mean()), 1), "cells_per_footprint": round(float(area[want[3][..., 0] >= 0].mean()), 1),
           "sources_with_a_box_per_frame": round(float(want[5][:, 2].mean()), 2), "rounds": rounds,
           "fuse_us": {"median": round(med["fuse"], 2), "min": round(min(t["fuse"]), 2)},
           "peaks_us": {"median": round(med["peaks"], 2), "min": round(min(t["peaks"]), 2)},
           "host_us": {"median": round(med["host"], 1), "min": round(min(t["host"]), 1)},
           "copies_us": {"median": round(med["copies"], 1), "min": round(min(t["copies"]), 1)},
           "ratio_fuse_over_peaks": round(med["fuse"] / med["peaks"], 2), "ratio_host_over_fuse": round(med["host"] / med["fuse"], 1),
           "ratio_copies_over_fuse": round(med["copies"] / med["fuse"], 1),
           "timing": "device events around %d back-to-back graph replays (fuse, peaks); host clock around .cpu() + NumPy restatement + .cuda() + synchronise "
                     "(host) and around the copies alone (copies)" % REPLAYS}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("fuse_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("fuse_time: no usable HIP device; this measurement has no CPU fallback")
    recs = [one_grid(rows, cols, args.rounds) for rows, cols in GRIDS]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": recs}, f, indent=1)
            f.write("\n")
