#!/usr/bin/env python3
"""Time bf_mvdr_learn_device beside bf_mvdr_design_device (dev tool; GPU box, no CPU fallback), mvdr_design_time.py's method:
  learn_14 / adapt_14   FilterSumListener.learn (weights given, forget 0.9) and .adapt on 14 frames of 256 samples at hop 128
                        (8 segments a frame, 112 snapshots)
  reaim                 FilterSumListener.reaim: the call with no frames (accumulate, factor and solve, taps)
  learn_1 / adapt_1     the two on ONE frame: the streaming use, a frame learned as it arrives
at 4 slots, 65 taps, 3-8 kHz, for the 64 microphones of the scene of tests/filtersum_np.py and for 256 microphones with random delays.
What is expected: learn about adapt (the same work and one read of the state), reaim = adapt less its first two launches.
The calls are timed by graph replay: INNER calls captured into one graph, device events around one replay.  A replay of learn advances
the state like any call; with forget 0.9 it settles, and nothing timed depends on its values.  ROUNDS alternating rounds in one
process; median, minimum, maximum.  Before anything is timed, learn from an empty state with unit weights and forget 1 is checked to
give adapt's taps byte for byte.  No time is asserted and no threshold is set.
usage: python scripts/dev/mvdr_learn_time.py [--rounds 9] [--out profiles/mvdr_learn_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat

GRID = (41, 23)
CELLS = [(20, 11), (28, 14), (23, 11), (5, 3)]
N, T, HOP, F, BAND, LOADING, SEG_HOP, SLOTS, FORGET = 256, 65, 128, 14, (3000.0, 8000.0), 0.1, 16, 4, 0.9
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
    # one listener per timed call: each keeps the workspaces of its own frame count, so no captured graph's buffers are replaced
    ls = {name: filtersum.FilterSumListener.for_slots(tau, SLOTS, M, hop=HOP, n_taps=T, band=BAND, mics=mics)
          for name in ("learn_14", "adapt_14", "reaim", "learn_1", "adapt_1")}
    d_off = torch.from_numpy(offsets).cuda()
    gen = torch.Generator(device="cpu").manual_seed(M)
    frames = (torch.randn((F, M, N), generator=gen) * 0.125).cuda()
    one = frames[:1].contiguous()
    weights = torch.tensor([1.0, 0.0, 0.5, 1.0, 2.0, 1.0, 0.0, 1.0, 1.0, 0.25, 1.0, 1.0, 1.0, 1.0], dtype=torch.float64).cuda()
    one_weight = weights[:1].contiguous()

    ls["learn_14"].learn(frames, d_off, forget=1.0, loading=LOADING, seg_hop=SEG_HOP)
    ls["adapt_14"].adapt(frames, d_off, loading=LOADING, seg_hop=SEG_HOP)
    torch.cuda.synchronize()
    assert ls["learn_14"].taps_host().tobytes() == ls["adapt_14"].taps_host().tobytes() and ls["learn_14"].d_used.tolist() == [F, 0]
    ls["reaim"].learn(frames, d_off, weights=weights, forget=FORGET)                   # a state to aim from
    ls["learn_14"].forget_all()

    timers = {"learn_14": replay_us(lambda: ls["learn_14"].learn(frames, d_off, weights=weights, forget=FORGET, loading=LOADING, seg_hop=SEG_HOP)),
              "adapt_14": replay_us(lambda: ls["adapt_14"].adapt(frames, d_off, loading=LOADING, seg_hop=SEG_HOP)),
              "reaim": replay_us(lambda: ls["reaim"].reaim(d_off, loading=LOADING)),
              "learn_1": replay_us(lambda: ls["learn_1"].learn(one, d_off, weights=one_weight, forget=FORGET, loading=LOADING, seg_hop=SEG_HOP)),
              "adapt_1": replay_us(lambda: ls["adapt_1"].adapt(one, d_off, loading=LOADING, seg_hop=SEG_HOP))}
    for _ in range(3):
        for once in timers.values():
            once()
    t = {name: [] for name in timers}
    for _ in range(rounds):
        for name, once in timers.items():
            t[name].append(once())
    nat.check()
    for name in ("learn_14", "learn_1", "reaim"):
        assert np.isfinite(ls[name].taps_host()).all() and not ls[name].d_fallback.any().item(), name
    segs = (N - max(0, N - HOP - T + 1) - T) // SEG_HOP + 1
    rec = {"mics": M, "slots": SLOTS, "frames": F, "segments_per_frame": segs, "in_band_bins": int(ls["reaim"].bins.size), "forget": FORGET}
    for name in timers:
        rec[name + "_us"] = stats(t[name])
    med = lambda name: rec[name + "_us"]["median"]
    rec["learn_14_over_adapt_14"] = round(med("learn_14") / med("adapt_14"), 2)
    rec["learn_1_over_adapt_1"] = round(med("learn_1") / med("adapt_1"), 2)
    rec["reaim_over_adapt_14"] = round(med("reaim") / med("adapt_14"), 2)
    return rec


def main(rounds, out):
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=GRID[0], MAX_RES_Y=GRID[1], N_TAPS=8)
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "samples": N, "n_taps": T, "band_hz": list(BAND), "hop": HOP, "loading": LOADING,
           "seg_hop": SEG_HOP,
           "timing": "device events around one replay of a graph of %d captured calls, per call" % INNER,
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
        sys.exit("mvdr_learn_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("mvdr_learn_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
