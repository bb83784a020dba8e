#!/usr/bin/env python3
"""Time the batched stream ingest against the only other way of doing the same job (dev tool; GPU box, no CPU fallback):
  loop     F calls of bf_ingest_device, each writing one frame of the batch         (the baseline)
  batched  one call of bf_ingest_stream_device for the F frames, header report on    (the code under test)
at config 2 (64 x 256) and the as-shipped size (256 x 256) with F = 190, and config 5 (256 x 1024) with F = 4; hop = N_SAMPLES, no
mask, m_total = N_MICROPHONES, so both write the same bytes (checked bit for bit before timing).
Device events around back-to-back enqueues after a warm-up; PAIRS alternating (loop, batched) pairs in one process; one JSON object
per size: medians, minima, their ratio, and the batched call's achieved bytes/s over the bytes the job has to move,
F*N*(8 + 4*N_MICROPHONES) read + 4*F*m_total*N written, as a share of the HBM peak bench.py uses.
Exit status 1 when, at any size, the batched median is not below the loop's minimum.
usage: python scripts/dev/ingest_time.py [--pairs 9] [--out profiles/ingest_stream_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import torch
from interface import config
from lib import _native as nat

HBM_PEAK_GBS = 8000.0          # as bench.py: HBM3E 8 TB/s (spec)
SIZES = [("cfg2", 64, 256, 190), ("shipped", 256, 256, 190), ("cfg5", 256, 1024, 4)]


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3        # us per call


def one_size(name, M, N, F, pairs):
    config.configure(N_MICROPHONES=M, N_SAMPLES=N, ACTIVE_TILES=M // 64)
    n_arrays, stride = M // 64, 8 + 4 * M
    g = torch.Generator(device="cpu").manual_seed(F + M + N)
    d_pk = torch.randint(0, 256, (F * N, stride), dtype=torch.uint8, generator=g).cuda()
    a = torch.full((F, M, N), float("nan"), dtype=torch.float32, device="cuda")
    b = torch.full((F, M, N), float("nan"), dtype=torch.float32, device="cuda")
    status = torch.empty((F, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    lib = nat.lib
    pk_ptrs = [d_pk[f * N:].data_ptr() for f in range(F)]
    a_ptrs = [a[f].data_ptr() for f in range(F)]

    def loop():
        for f in range(F):
            lib.bf_ingest_device(pk_ptrs[f], n_arrays, 8, 8, a_ptrs[f], s)

    def batched():
        lib.bf_ingest_stream_device(d_pk.data_ptr(), F * N, n_arrays, 8, 8, N, F, M, None, 2, b.data_ptr(), status.data_ptr(), s)

    for _ in range(3):
        loop(); batched()
    torch.cuda.synchronize()
    nat.check()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the two paths disagree"
    t_loop, t_batched = [], []
    for _ in range(pairs):
        t_loop.append(timed(loop, 5))
        t_batched.append(timed(batched, 100))
    nat.check()
    bytes_moved = F * N * stride + 4 * F * M * N
    med_l, med_b = statistics.median(t_loop), statistics.median(t_batched)
    rate = bytes_moved / (med_b * 1e-6)
    rec = {"size": name, "n_microphones": M, "n_samples": N, "frames": F, "pairs": pairs,
           "loop_us": {"median": round(med_l, 2), "min": round(min(t_loop), 2)},
           "batched_us": {"median": round(med_b, 2), "min": round(min(t_batched), 2)},
           "ratio_loop_over_batched": round(med_l / med_b, 2), "bytes_per_call": bytes_moved,
           "batched_bytes_per_s": round(rate, 0), "hbm_peak_gbs": HBM_PEAK_GBS, "share_of_hbm_peak": round(rate / (HBM_PEAK_GBS * 1e9), 4),
           "batched_median_below_loop_min": med_b < min(t_loop),
           "timing": "device events around back-to-back enqueues, 5 loops / 100 batched calls per sample"}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pairs < 5:
        sys.exit("ingest_time: at least five alternating pairs")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("ingest_time: no usable HIP device; this measurement has no CPU fallback")
    recs = [one_size(*sz, args.pairs) for sz in SIZES]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": recs}, f, indent=1)
            f.write("\n")
    sys.exit(0 if all(r["batched_median_below_loop_min"] for r in recs) else 1)
