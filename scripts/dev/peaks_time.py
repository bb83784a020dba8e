#!/usr/bin/env python3
"""Time bf_peaks_device (k = 4, radius = 4) against its floor and against what a user had without it (dev tool; GPU box, no CPU fallback):
  peaks    one call of bf_peaks_device                                                        (the code under test)
  argmax   one call of bf_peak_offsets_device: reads the same bytes, finds one source           (the floor)
  torch    max_pool2d with a (2r+1)^2 window, an equality mask, torch.topk                      (the formulation available before)
on 190-frame batches of config 2 (101 x 101) and as-shipped (57 x 32) maps and a 4-frame batch of config 5 (361 x 361, the tiled form).
The maps are three lobes plus noise, the same tensor for all three; before timing, the torch formulation's sources above the threshold
are checked against the call's (the noise leaves no ties).
Device events around back-to-back enqueues after a warm-up; PAIRS alternating rounds of the three in one process; one JSON object per
size: medians, minima, the ratios, and the call's achieved bytes/s over the bytes the job has to move (the maps read once, the three
outputs written) as a share of the HBM peak bench.py uses.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats`.
Exit status 1 when, at any size, the call's median is not below the torch formulation's minimum.
usage: python scripts/dev/peaks_time.py [--pairs 9] [--out profiles/peaks_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import torch
from lib import _native as nat

HBM_PEAK_GBS = 8000.0          # as bench.py: HBM3E 8 TB/s (spec)
SIZES = [("cfg2", 101, 101, 190), ("shipped", 57, 32, 190), ("cfg5", 361, 361, 4)]
K, RADIUS, FLOOR_REL, PER = 4, 4, 0.5, 64


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3        # us per call


def maps_for(rows, cols, F):
    g = torch.Generator(device="cpu").manual_seed(rows * 1000 + cols + F)
    x = torch.arange(rows, dtype=torch.float32)[:, None] / rows
    y = torch.arange(cols, dtype=torch.float32)[None, :] / cols
    c = torch.rand((F, 3, 2), generator=g)
    amp = torch.tensor([1.0, 0.7, 0.4])
    m = torch.zeros((F, rows, cols))
    for j in range(3):
        m += amp[j] * torch.exp(-((x[None] - c[:, j, 0, None, None]) ** 2 + (y[None] - c[:, j, 1, None, None]) ** 2) / (2 * 0.06 ** 2))
    m += 0.05 * torch.rand((F, rows, cols), generator=g)
    return m.reshape(F, rows * cols).contiguous().cuda()


def one_size(name, rows, cols, F, pairs):
    D = rows * cols
    maps = maps_for(rows, cols, F)
    offs = torch.empty((F, K), dtype=torch.int32, device="cuda")
    vals = torch.empty((F, K), dtype=torch.float32, device="cuda")
    cnt = torch.empty((F, 3), dtype=torch.int32, device="cuda")
    one = torch.empty((F, 1), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    lib = nat.lib
    neg = torch.full((), float("-inf"), device="cuda")
    kept = {}

    def peaks():
        lib.bf_peaks_device(maps.data_ptr(), F, D, rows, cols, RADIUS, K, FLOOR_REL, 0.0, PER, offs.data_ptr(), vals.data_ptr(), cnt.data_ptr(), s)

    def argmax():
        lib.bf_peak_offsets_device(maps.data_ptr(), F, D, D, PER, one.data_ptr(), s)

    def torch_form():
        img = maps.view(F, 1, rows, cols)
        pooled = torch.nn.functional.max_pool2d(img, 2 * RADIUS + 1, stride=1, padding=RADIUS)
        kept["v"], kept["i"] = torch.topk(torch.where(pooled == img, img, neg).view(F, D), K)

    for _ in range(3):
        peaks(); argmax(); torch_form()
    torch.cuda.synchronize()
    nat.check()
    # the same sources: torch's top K local maxima, cut at the threshold, are the call's
    tv, ti = kept["v"], kept["i"]
    want = torch.where(tv >= FLOOR_REL * tv[:, :1], ti.to(torch.int32) * PER, torch.full_like(ti, -1, dtype=torch.int32))
    assert torch.equal(want, offs), "the torch formulation and bf_peaks_device disagree"
    assert torch.equal(one[:, 0], offs[:, 0]), "argmax and the first source disagree"
    t = {"peaks": [], "argmax": [], "torch": []}
    for _ in range(pairs):
        t["peaks"].append(timed(peaks, 100))
        t["argmax"].append(timed(argmax, 100))
        t["torch"].append(timed(torch_form, 20))
    nat.check()
    bytes_moved = 4 * F * D + 4 * F * (2 * K + 3)
    med = {n: statistics.median(v) for n, v in t.items()}
    rate = bytes_moved / (med["peaks"] * 1e-6)
    rec = {"size": name, "rows": rows, "cols": cols, "frames": F, "k": K, "radius": RADIUS, "floor_rel": FLOOR_REL, "pairs": pairs,
           "form": "one workgroup per frame" if D * 12 <= 160 * 1024 - 256 else "tiled, three launches",
           "peaks_us": {"median": round(med["peaks"], 2), "min": round(min(t["peaks"]), 2)},
           "argmax_us": {"median": round(med["argmax"], 2), "min": round(min(t["argmax"]), 2)},
           "torch_us": {"median": round(med["torch"], 2), "min": round(min(t["torch"]), 2)},
           "ratio_peaks_over_argmax": round(med["peaks"] / med["argmax"], 2), "ratio_torch_over_peaks": round(med["torch"] / med["peaks"], 2),
           "bytes_per_call": bytes_moved, "peaks_bytes_per_s": round(rate, 0), "hbm_peak_gbs": HBM_PEAK_GBS,
           "share_of_hbm_peak": round(rate / (HBM_PEAK_GBS * 1e9), 5),
           "peaks_median_below_torch_min": med["peaks"] < min(t["torch"]),
           "timing": "device events around back-to-back enqueues, 100 peaks / 100 argmax / 20 torch calls per sample"}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pairs < 5:
        sys.exit("peaks_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("peaks_time: no usable HIP device; this measurement has no CPU fallback")
    recs = [one_size(*sz, args.pairs) for sz in SIZES]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": recs}, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r["peaks_median_below_torch_min"] for r in recs) else 1)
