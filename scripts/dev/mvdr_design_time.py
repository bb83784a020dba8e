#!/usr/bin/env python3
"""Time bf_mvdr_design_device beside its neighbours and beside what it replaces (dev tool; GPU box, no CPU fallback):
  adapt    one bf_mvdr_design_device call (four launches: snapshots, covariance, factor and solve, taps), as
           FilterSumListener.adapt enqueues it                                                                  (the code under test)
  design   one bf_lcmv_design_device call for the same slots (FilterSumListener.retarget), the geometric designer      (neighbour 1)
  filter   one bf_filter_sum_device launch of the same beams at one frame, the live case                                (neighbour 2)
  host     what adaptive taps cost without the call: the device -> host copy of the frames, filtersum.design_mvdr_slots in NumPy
           float64, the upload of the taps into the tensor the beams read; the three parts and their sum                (baseline)
at 4 slots, 65 taps, 3-8 kHz, 14 frames of 256 samples at hop 128 (8 segments a frame, 112 snapshots), for the 64 microphones of the
scene of tests/filtersum_np.py and for 256 microphones with random delays (no geometry is needed to time a design).
The device calls are timed by graph replay: INNER calls captured into one graph, device events around one replay, so the figure is
what the call costs inside a captured chain.  The host path is timed with a host clock around work that ends in a device
synchronise.  ROUNDS alternating rounds in one process; median, minimum, maximum.  The device taps are checked against the host
design (one float32 ulp of each beam's largest tap) before anything is timed.
No time is asserted anywhere and no threshold is set: the file records what each side costs.
usage: python scripts/dev/mvdr_design_time.py [--rounds 9] [--out profiles/mvdr_design_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat

GRID = (41, 23)
CELLS = [(20, 11), (28, 14), (23, 11), (5, 3)]
N, T, HOP, F, BAND, LOADING, SEG_HOP, SLOTS = 256, 65, 128, 14, (3000.0, 8000.0), 0.1, 16, 4
INNER = 10


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


def one_size(M, rounds):
    import filtersum
    if M == 64:
        from lib.directions import calculate_delays
        tau = calculate_delays().reshape(-1, M)
        offsets = np.array([c[0] * GRID[1] + c[1] for c in CELLS], dtype=np.int32) * M
    else:
        tau = np.random.default_rng(M).uniform(-8.0, 8.0, size=(12, M))
        offsets = np.array([3, 7, 0, 10], dtype=np.int32) * M
    mics = np.arange(M, dtype=np.int32)
    fl = filtersum.FilterSumListener.for_slots(tau, SLOTS, M, hop=HOP, n_taps=T, band=BAND, mics=mics)
    geo = filtersum.FilterSumListener.for_slots(tau, SLOTS, M, hop=HOP, n_taps=T, band=BAND, mics=mics)
    d_off = torch.from_numpy(offsets).cuda()
    gen = torch.Generator(device="cpu").manual_seed(M)
    frames = (torch.randn((F, M, N), generator=gen) * 0.125).cuda()
    prev = (torch.randn((M, N), generator=gen) * 0.125).cuda()
    seg_first = max(0, N - HOP - T + 1)
    segs = (N - seg_first - T) // SEG_HOP + 1
    design = dict(n_taps=T, band=BAND, loading=LOADING, seg_first=seg_first, seg_hop=SEG_HOP, segs=segs)

    status, fallback = fl.adapt(frames, d_off, loading=LOADING, seg_hop=SEG_HOP)
    torch.cuda.synchronize()
    want, want_fallback, want_status = filtersum.design_mvdr_slots(frames.cpu().numpy(), mics, tau, offsets, M, **design)
    got = fl.taps_host()
    assert np.array_equal(status.cpu().numpy(), want_status) and np.array_equal(fallback.cpu().numpy(), want_fallback)
    assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want).max(axis=(1, 2), keepdims=True)).all()

    def host_path():
        t0 = time.perf_counter()
        x = frames.cpu().numpy()                                       # synchronises
        t1 = time.perf_counter()
        offs = d_off.cpu().numpy()
        taps, _, _ = filtersum.design_mvdr_slots(x, mics, tau, offs, M, **design)
        t2 = time.perf_counter()
        fl.d_taps.copy_(torch.from_numpy(taps))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return [(b - a) * 1e6 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t0, t3))]

    out = torch.empty((1, SLOTS, N), dtype=torch.float32, device="cuda")

    def filt():
        rc = nat.lib.bf_filter_sum_device(frames.data_ptr(), M, 1, HOP, prev.data_ptr(), nat.iptr(mics), M, fl.d_taps.data_ptr(), T, SLOTS, out.data_ptr(), N,
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0

    timers = {"adapt": replay_us(lambda: fl.adapt(frames, d_off, loading=LOADING, seg_hop=SEG_HOP)), "lcmv_design": replay_us(lambda: geo.retarget(d_off)),
              "filter_1_frame": replay_us(filt)}
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
    rec = {"mics": M, "slots": SLOTS, "frames": F, "segments_per_frame": segs, "snapshots": F * segs, "in_band_bins": int(fl.bins.size)}
    for name in timers:
        rec[name + "_us"] = stats(t[name])
    for i, name in enumerate(("host_read_frames_us", "host_design_mvdr_slots_us", "host_upload_taps_us", "host_total_us")):
        rec[name] = stats([h[i] for h in host])
    rec["host_total_over_adapt"] = round(rec["host_total_us"]["median"] / rec["adapt_us"]["median"], 1)
    rec["adapt_over_lcmv_design"] = round(rec["adapt_us"]["median"] / rec["lcmv_design_us"]["median"], 1)
    rec["adapt_over_filter_1_frame"] = round(rec["adapt_us"]["median"] / rec["filter_1_frame_us"]["median"], 1)
    return rec


def main(rounds, out):
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=GRID[0], MAX_RES_Y=GRID[1], N_TAPS=8)
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "samples": N, "n_taps": T, "band_hz": list(BAND), "hop": HOP, "loading": LOADING,
           "seg_hop": SEG_HOP,
           "timing": "device calls: device events around one replay of a graph of %d captured calls, per call; host path: host clock around work that ends "
                     "in a device synchronise" % INNER,
           "cases": [one_size(M, rounds) for M in (64, 256)]}
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
        sys.exit("mvdr_design_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("mvdr_design_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
