#!/usr/bin/env python3
"""Time bf_lcmv_design_device beside what it replaces and beside the launch it feeds (dev tool; GPU box, no CPU fallback):
  design   one bf_lcmv_design_device call (two launches: gains, taps), as FilterSumListener.retarget enqueues it   (the code under test)
  host     what a moving source cost before: the device -> host read of the row of offsets, filtersum.design_slots on the host
           (NumPy float64), the upload of the taps into the tensor the beams read; the three parts and their sum         (baseline 1)
  filter   one bf_filter_sum_device launch of the same beams, at one frame (the live case) and at 190 frames              (baseline 2)
at 4 slots (the scene of tests/filtersum_np.py plus cell (5, 3)), 64 microphones, 65 taps, 3-8 kHz, and at 8 slots.
The device calls are timed by graph replay: INNER calls captured into one graph, device events around one replay, so the figure is
what the call costs inside a captured chain, not what Python takes to enqueue it.  The host path is timed with a host clock around
work that ends in a device synchronise.  ROUNDS alternating rounds in one process; median, minimum, maximum.  The device taps are
checked against the host design (one float32 ulp of each beam's largest tap) before anything is timed.
No time is asserted anywhere and no threshold is set: the claim is "no host round trip", the file records what each side costs.
usage: python scripts/dev/lcmv_design_time.py [--rounds 9] [--out profiles/lcmv_design_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat

GRID = (41, 23)
CELLS = [(20, 11), (28, 14), (23, 11), (5, 3), (35, 4), (10, 19), (2, 12), (38, 20)]
M, N, T, HOP, BAND, RHO = 64, 256, 65, 128, (3000.0, 8000.0), 0.95
INNER = 20


def stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def replay_us(fn):
    """fn enqueues one call on the current stream -> a function that times one replay of INNER captured calls, in us per call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(INNER):
            fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER * 1e3
    return once


def one_size(slots, rounds):
    import filtersum
    from lib.directions import calculate_delays
    tau = calculate_delays().reshape(-1, M)
    offsets = np.array([c[0] * GRID[1] + c[1] for c in CELLS[:slots]], dtype=np.int32) * M
    fl = filtersum.FilterSumListener.for_slots(tau, slots, M, hop=HOP, n_taps=T, band=BAND, rho=RHO)
    d_off = torch.from_numpy(offsets).cuda()
    status, kept = fl.retarget(d_off)
    torch.cuda.synchronize()
    want, want_kept, want_status = filtersum.design_slots(tau, offsets, M, n_taps=T, band=BAND, rho=RHO)
    got = fl.taps_host()
    assert np.array_equal(status.cpu().numpy(), want_status) and np.array_equal(kept.cpu().numpy(), want_kept)
    assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want).max(axis=(1, 2), keepdims=True)).all()

    def host_path():
        t0 = time.perf_counter()
        offs = d_off.cpu().numpy()                                     # synchronises
        t1 = time.perf_counter()
        taps, _, _ = filtersum.design_slots(tau, offs, M, n_taps=T, band=BAND, rho=RHO)
        t2 = time.perf_counter()
        fl.d_taps.copy_(torch.from_numpy(taps))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return [(b - a) * 1e6 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t0, t3))]

    gen = torch.Generator(device="cpu").manual_seed(190)
    frames = (torch.randn((190, M, N), generator=gen) * 0.125).cuda()
    prev = (torch.randn((M, N), generator=gen) * 0.125).cuda()
    mics = np.arange(M, dtype=np.int32)
    outs = {F: torch.empty((F, slots, N), dtype=torch.float32, device="cuda") for F in (1, 190)}

    def filt(F):
        rc = nat.lib.bf_filter_sum_device(frames.data_ptr(), M, F, HOP, prev.data_ptr(), nat.iptr(mics), M, fl.d_taps.data_ptr(), T, slots, outs[F].data_ptr(), N,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0

    timers = {"design": replay_us(lambda: fl.retarget(d_off)), "filter_1_frame": replay_us(lambda: filt(1)), "filter_190_frames": replay_us(lambda: filt(190))}
    for _ in range(3):
        for once in timers.values():
            once()
        host_path()
    t = {name: [] for name in timers}
    host = []
    for _ in range(rounds):
        for name, once in timers.items():
            t[name].append(once())
        host.append(host_path())
    nat.check()
    rec = {"slots": slots, "in_band_bins": int(fl.bins.size), "kept_nulls": int(want_kept.sum()), "null_decisions": slots * (slots - 1) * int(fl.bins.size)}
    for name in timers:
        rec[name + "_us"] = stats(t[name])
    for i, name in enumerate(("host_read_offsets_us", "host_design_slots_us", "host_upload_taps_us", "host_total_us")):
        rec[name] = stats([h[i] for h in host])
    rec["host_total_over_design"] = round(rec["host_total_us"]["median"] / rec["design_us"]["median"], 1)
    rec["design_over_filter_1_frame"] = round(rec["design_us"]["median"] / rec["filter_1_frame_us"]["median"], 2)
    return rec


def main(rounds, out):
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=GRID[0], MAX_RES_Y=GRID[1], N_TAPS=8)
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "mics": M, "samples": N, "n_taps": T, "band_hz": list(BAND), "rho": RHO, "hop": HOP,
           "timing": "device calls: device events around one replay of a graph of %d captured calls, per call; host path: host clock around work that ends "
                     "in a device synchronise" % INNER,
           "cases": [one_size(slots, rounds) for slots in (4, 8)]}
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("lcmv_design_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("lcmv_design_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
