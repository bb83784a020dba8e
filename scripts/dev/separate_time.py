#!/usr/bin/env python3
"""Time the subtraction step of BeamListener.separate against the map launch it sits beside (dev tool; GPU box, no CPU fallback):
  remove     one bf_remove_sources_device launch, one beam per frame, in place                      (the code under test)
  das        one bf_das_device launch of the same batch: existing code                               (the yardstick)
  iteration  one whole round of separate: maps -> sources (k = 1) -> listen -> remove, through BeamListener, output tensors included
  copy       torch's device-to-device copy of a buffer of the batch's size, and of 1 GiB             (the box's copy bandwidth)
on a 190-frame batch of config 2 (64 microphones x 256 samples, 101 x 101 directions), lerp.  The frames are noise; the beams are the
ones bf_miso_device forms at each frame's loudest direction, so the launch does what the loop's launch does.
Device events around back-to-back enqueues after a warm-up; PAIRS alternating rounds in one process; medians and minima.  The
kernel's bytes are what the job has to move: every frame element read and written once (8 * F * M * N) plus the beams read once.
A batch of this size (12 MB) stays in the Infinity Cache between launches, so its rate is compared with the copy of the same size
as well as with the 1 GiB copy that has to go to HBM.  Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`.
No ratio is asserted: the file records whether the removal launch costs more than a tenth of the map launch.
usage: python scripts/dev/separate_time.py [--pairs 9] [--out profiles/separate_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
from interface import config
from lib import _native as nat
import listen

M, N, X, Y, F = 64, 256, 101, 101, 190


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3        # us per call


def main(pairs, out):
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=8)
    from lib.directions import calculate_delays
    table = np.ascontiguousarray(np.float32(calculate_delays()).ravel())
    assert table.size == X * Y * M
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    mics = np.arange(M, dtype=np.int32)
    bl = listen.BeamListener("lerp", mics=mics)
    g = torch.Generator(device="cpu").manual_seed(190)
    frames = (torch.randn((F, M, N), generator=g) * 0.125).cuda()
    work = frames.clone()
    power = bl.maps(frames)
    offs, _, _ = bl.sources(power, 1, max(X, Y), 0.0, 0.0)
    beams, st = bl.listen(frames, offs)
    assert int(st.abs().sum()) == 0
    status = torch.empty((F, 1), dtype=torch.int32, device="cuda")
    img = torch.empty((F, X * Y), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    lib = nat.lib
    big_a = torch.empty((1 << 28,), dtype=torch.float32, device="cuda")     # 1 GiB
    big_b = torch.empty_like(big_a)
    small_b = torch.empty_like(frames)

    def remove():
        lib.bf_remove_sources_device(nat.LERP, work.data_ptr(), M, F, nat.iptr(mics), M, offs.data_ptr(), 1, beams.data_ptr(), N, 1.0, work.data_ptr(),
                                     status.data_ptr(), s)

    def das():
        lib.bf_das_device(nat.LERP, frames.data_ptr(), M, img.data_ptr(), X * Y, F, nat.iptr(mics), M, 0, X * Y, s)

    def iteration():
        p = bl.maps(work)
        o, _, _ = bl.sources(p, 1, max(X, Y), 0.0, 0.0)
        b, _ = bl.listen(work, o)
        bl.remove(work, o, b, 1.0, out=work)

    def copy_small():
        small_b.copy_(frames)

    def copy_big():
        big_b.copy_(big_a)

    for _ in range(3):
        remove(); das(); iteration(); copy_small(); copy_big()
    torch.cuda.synchronize()
    nat.check()
    # one removal really removes: the residual of the loudest direction's beam carries less energy than the frames
    work.copy_(frames); remove(); torch.cuda.synchronize()
    assert float((work.double() ** 2).sum()) < float((frames.double() ** 2).sum())
    t = {"remove": [], "das": [], "iteration": [], "copy_small": [], "copy_big": []}
    for _ in range(pairs):
        work.copy_(frames)
        t["remove"].append(timed(remove, 200))
        t["das"].append(timed(das, 20))
        work.copy_(frames)
        t["iteration"].append(timed(iteration, 10))
        t["copy_small"].append(timed(copy_small, 200))
        t["copy_big"].append(timed(copy_big, 10))
    nat.check()
    med = {n: statistics.median(v) for n, v in t.items()}
    frame_bytes = 4 * F * M * N
    kernel_bytes = 2 * frame_bytes + 4 * F * N + 8 * F          # frames in and out, beams, offsets and status
    rate = kernel_bytes / (med["remove"] * 1e-6)
    copy_small_rate = 2 * frame_bytes / (med["copy_small"] * 1e-6)
    copy_big_rate = 2 * big_a.numel() * 4 / (med["copy_big"] * 1e-6)
    rec = {"device": torch.cuda.get_device_name(0), "size": "cfg2", "mics": M, "samples": N, "rows": X, "cols": Y, "frames": F, "algo": "lerp",
           "beams": 1, "pairs": pairs}
    for n in t:
        rec[n + "_us"] = {"median": round(med[n], 2), "min": round(min(t[n]), 2), "max": round(max(t[n]), 2)}
    rec.update({"remove_bytes_per_call": kernel_bytes, "remove_bytes_per_s": round(rate, 0),
                "copy_same_size_bytes_per_s": round(copy_small_rate, 0), "copy_1gib_bytes_per_s": round(copy_big_rate, 0),
                "remove_rate_over_copy_same_size": round(rate / copy_small_rate, 3), "remove_rate_over_copy_1gib": round(rate / copy_big_rate, 3),
                "ratio_remove_over_das": round(med["remove"] / med["das"], 4), "ratio_iteration_over_das": round(med["iteration"] / med["das"], 3),
                "remove_over_a_tenth_of_das": med["remove"] > 0.1 * med["das"],
                "timing": "device events around back-to-back enqueues: 200 remove / 20 das / 10 iteration / 200 + 10 copy calls per sample"})
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pairs < 5:
        sys.exit("separate_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("separate_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.pairs, args.out)
