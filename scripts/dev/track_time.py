#!/usr/bin/env python3
"""Time bf_track_sources_device beside the launch that feeds it and beside doing the association on the host (dev tool; GPU box, no
CPU fallback):
  track    one replay of a captured graph holding the bf_track_sources_device launch                (the code under test)
  peaks    one replay of a captured graph holding the bf_peaks_device launch that feeds it         (the neighbour in the chain)
  host     offsets .cpu(), the plain NumPy loop of tests/track_np.py, the [F, slots] result .cuda() (the alternative: a host round trip)
at (frames, k, slots) = (190, 4, 4) and (190, 64, 64) on as-shipped maps (57 x 32).  The maps are moving lobes plus noise; k = 4 takes
radius 4 and a floor (a handful of sources), k = 64 radius 1 and no floor (every local maximum of the noise: all 64 columns filled, the
association's worst case).  The tracker's state carries from replay to replay as it does in a stream, and the result of the first
call from a zeroed state is compared with the NumPy loop before anything is timed.
Device events around REPLAYS back-to-back graph replays after a warm-up, ROUNDS alternating rounds in one process, medians and minima;
the host alternative is timed with a host clock around work that ends in a synchronise.  The kernel is one wave and latency-bound:
no rate or share of peak is derived.  Nothing is asserted about time.
usage: python scripts/dev/track_time.py [--rounds 9] [--out profiles/track_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from lib import _native as nat
import track_np

ROWS, COLS, F, PER = 57, 32, 190, 256
SIZES = [dict(k=4, slots=4, radius=4, floor_rel=0.25), dict(k=64, slots=64, radius=1, floor_rel=0.0)]
GATE, MAX_MISS, MIN_HITS, Q, R = 3.0, 5, 3, 0.1, 0.1
REPLAYS = 50


def maps_for():
    g = torch.Generator(device="cpu").manual_seed(ROWS * 1000 + COLS + F)
    x = torch.arange(ROWS, dtype=torch.float32)[None, :, None]
    y = torch.arange(COLS, dtype=torch.float32)[None, None, :]
    t = torch.arange(F, dtype=torch.float32)[:, None, None]
    m = torch.zeros((F, ROWS, COLS))
    for amp, x0, y0, dx, dy in ((1.0, 8.0, 6.0, 0.20, 0.05), (0.9, 45.0, 25.0, -0.15, -0.04), (0.8, 28.0, 16.0, 0.0, 0.0)):
        level = amp * (1.0 + 0.2 * torch.sin(t * 0.7 + x0))                  # levels cross: the loudest-first order keeps changing
        m += level * torch.exp(-((x - x0 - dx * t) ** 2 + (y - y0 - dy * t) ** 2) / (2 * 2.5 ** 2))
    m += 0.05 * torch.rand((F, ROWS, COLS), generator=g)
    return m.reshape(F, ROWS * COLS).contiguous().cuda()


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


def one_size(maps, k, slots, radius, floor_rel, rounds):
    D = ROWS * COLS
    lib = nat.lib
    src = torch.empty((F, k), dtype=torch.int32, device="cuda")
    state = torch.zeros((lib.bf_track_state_words(slots),), dtype=torch.int32, device="cuda")
    out = torch.empty((F, slots), dtype=torch.int32, device="cuda")
    ids, match = torch.empty_like(out), torch.empty_like(out)
    pos = torch.empty((F, slots, 4), dtype=torch.float32, device="cuda")
    counts = torch.empty((F, 4), dtype=torch.int32, device="cuda")

    def peaks():
        rc = lib.bf_peaks_device(maps.data_ptr(), F, D, ROWS, COLS, radius, k, floor_rel, 0.0, PER, src.data_ptr(), None, None,
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.bf_last_error()

    def track():
        rc = lib.bf_track_sources_device(src.data_ptr(), F, k, ROWS, COLS, PER, slots, GATE, MAX_MISS, MIN_HITS, Q, R, state.data_ptr(), out.data_ptr(),
                                         ids.data_ptr(), pos.data_ptr(), match.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.bf_last_error()

    def host():
        t_off = track_np.track(src.cpu().numpy(), ROWS, COLS, PER, slots, GATE, MAX_MISS, MIN_HITS, Q, R)[0]
        return torch.from_numpy(t_off).cuda()

    peaks()
    track()
    torch.cuda.synchronize()
    want = track_np.track(src.cpu().numpy(), ROWS, COLS, PER, slots, GATE, MAX_MISS, MIN_HITS, Q, R)
    for got, w in zip((out, ids, pos, match, counts, state), want):
        assert got.cpu().numpy().tobytes() == w.tobytes(), "the launch and the NumPy loop disagree"
    filled = float((src >= 0).sum().item()) / F
    g_peaks, g_track = graph_of(peaks), graph_of(track)
    for _ in range(3):
        timed_replays(g_peaks); timed_replays(g_track)
    t = {"track": [], "peaks": [], "host": []}
    for _ in range(rounds):
        t["track"].append(timed_replays(g_track))
        t["peaks"].append(timed_replays(g_peaks))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        torch.cuda.synchronize()
        t["host"].append((time.perf_counter() - t0) * 1e6)
    med = {n: statistics.median(v) for n, v in t.items()}
    rec = {"frames": F, "k": k, "slots": slots, "rows": ROWS, "cols": COLS, "radius": radius, "floor_rel": floor_rel, "gate": GATE, "max_miss": MAX_MISS,
           "min_hits": MIN_HITS, "detections_per_frame": round(filled, 2), "tracks_born_in_first_call": int(want[4][:, 0].sum()), "rounds": rounds,
           "track_us": {"median": round(med["track"], 2), "min": round(min(t["track"]), 2)},
           "track_us_per_frame": round(med["track"] / F, 3),
           "peaks_us": {"median": round(med["peaks"], 2), "min": round(min(t["peaks"]), 2)},
           "host_us": {"median": round(med["host"], 1), "min": round(min(t["host"]), 1)},
           "ratio_track_over_peaks": round(med["track"] / med["peaks"], 2), "ratio_host_over_track": round(med["host"] / med["track"], 1),
           "timing": "device events around %d back-to-back graph replays (track, peaks); host clock around .cpu() + NumPy loop + .cuda() + synchronise (host)" % REPLAYS}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("track_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("track_time: no usable HIP device; this measurement has no CPU fallback")
    maps = maps_for()
    recs = [one_size(maps, rounds=args.rounds, **sz) for sz in SIZES]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": recs}, f, indent=1)
            f.write("\n")
