#!/usr/bin/env python3
"""Time the map at listed directions against the full map (dev tool; GPU box, no CPU fallback), lerp:
  full_map  one bf_das_device launch over the whole grid                               (what a peak search needed before)
  scan      CoarseToFine.scan: one shared-list bf_das_select_device call on the lattice of every step-th direction
  locate    CoarseToFine.locate with k = 4, coarse radius 2: scan, bf_peaks_device, the windows in torch, one per-frame-list call on
            [F, 4 * (2 step + 1)^2], bf_peaks_device on the windows
on config 2 (64 x 256, 101 x 101, 190 frames, step 4) and config 5 (256 x 1024, 361 x 361, 4 frames, step 16), white-noise frames
(every slot of `locate` is filled: floor_rel 0).
Baseline = ANOTHER build of the library, normally the parent commit's (--parent-lib; loaded through BF_NATIVE_LIB in a child process
of its own): its full_map.  The in-tree build's full_map is measured too -- the same code, so the two show the process-to-process spread.
Every callable is captured in a graph after a warm-up call; a sample is the device-event time of `inner` back-to-back replays; the
full map is sampled on its own (the same procedure in both processes), then scan and locate alternate sample by sample; medians of
--rounds samples (9).  Nothing is asserted about the times.
usage: python scripts/dev/select_time.py --parent-lib <libbeamformer_hip.so of the parent> [--out profiles/select_time.json]"""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [("cfg2", 190, 4, 10), ("cfg5", 4, 16, 3)]      # size, frames, lattice step, replays per sample
K, RADIUS_C = 4, 2


def stats(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def child(rounds):
    """Runs in a process of its own with the library $BF_NATIVE_LIB names (or the in-tree one): one JSON object on the last line."""
    import numpy as np, torch
    from lib import _native as nat
    import listen, synth, util
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("select_time: no usable HIP device; this measurement has no CPU fallback")
    has_select = getattr(nat.lib, "bf_das_select_device", None) is not None and nat.lib.bf_das_select_device.argtypes is not None

    def graphed(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = fn()
        g.replay()
        torch.cuda.synchronize()
        nat.check()
        return g, keep

    def timed(g, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3        # us per replay

    recs = []
    for name, F, step, inner in SIZES:
        c = util.configure(name)
        M, N, X, Y = c["M"], c["N"], c["X"], c["Y"]
        table = util.table_for("lerp", name)
        nat.lib.load_coefficients_lerp(nat.fptr(table), table.size)
        nat.check()
        x = torch.from_numpy(synth.frame_batch(M, N, F)).cuda()
        bl = listen.BeamListener("lerp", mics=np.arange(M))
        fns = {"full_map": lambda: bl.maps(x)}
        rec = {"size": name, "mics": M, "samples": N, "grid": [X, Y], "frames": F, "directions": X * Y}
        if has_select:
            import zoom
            ctf = zoom.CoarseToFine(bl, step)
            fns["scan"] = lambda: ctf.scan(x)
            fns["locate"] = lambda: ctf.locate(x, K, RADIUS_C, 0.0)
            lattice, window = ctf.coarse_shape[0] * ctf.coarse_shape[1], K * (2 * ctf.radius + 1) ** 2
            rec.update({"step": step, "lattice_directions": lattice, "locate_list_entries": lattice + window, "k": K, "coarse_radius": RADIUS_C})
        graphs = {n: graphed(fn) for n, fn in fns.items()}
        if has_select:
            offs, _, counts = graphs["locate"][1]
            rec["locate_slots_filled_mean"] = round(float((offs >= 0).sum()) / F, 2)
            full = graphs["full_map"][1]
            assert torch.equal(graphs["scan"][1], full[:, torch.div(ctf.lattice, bl.offset_per_dir, rounding_mode="floor").long()]), "scan is not the full map at the lattice"
        t = {n: [] for n in graphs}
        for _ in range(rounds):                              # the full map on its own first: the same procedure in both libraries' processes
            t["full_map"].append(timed(graphs["full_map"][0], inner))
        for _ in range(rounds):
            for n, (g, _) in graphs.items():
                if n != "full_map":
                    t[n].append(timed(g, inner))
        nat.check()
        for n in graphs:
            rec[n + "_us"] = stats(t[n])
        rec["full_map_ns_per_direction"] = round(rec["full_map_us"]["median"] * 1e3 / (F * X * Y), 3)
        if has_select:
            rec["scan_ns_per_direction"] = round(rec["scan_us"]["median"] * 1e3 / (F * lattice), 3)
            rec["locate_ns_per_list_entry"] = round(rec["locate_us"]["median"] * 1e3 / (F * (lattice + window)), 3)
        recs.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "results": recs}))


def run_child(lib_path, rounds):
    env = dict(os.environ)
    env.pop("BF_NATIVE_LIB", None)
    if lib_path:
        env["BF_NATIVE_LIB"] = lib_path
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(rounds)], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        sys.exit("select_time: the child with library %s failed (exit %d)" % (lib_path or "in-tree", p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libbeamformer_hip.so of the parent commit (the baseline)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.rounds)
        sys.exit(0)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("select_time: --parent-lib must name the parent commit's build of the library")
    parent = run_child(os.path.abspath(args.parent_lib), args.rounds)
    tree = run_child(None, args.rounds)
    base = {r["size"]: r for r in parent["results"]}
    for r in tree["results"]:
        p = base[r["size"]]["full_map_us"]
        r["parent_full_map_us"] = p
        r["ratio_in_tree_full_map_over_parent"] = round(r["full_map_us"]["median"] / p["median"], 3)
        r["speedup_scan_over_parent_full_map"] = round(p["median"] / r["scan_us"]["median"], 2)
        r["speedup_locate_over_parent_full_map"] = round(p["median"] / r["locate_us"]["median"], 2)
        r["scan_cost_per_direction_over_full_map"] = round(r["scan_ns_per_direction"] / (p["median"] * 1e3 / (r["frames"] * r["directions"])), 2)
    out = {"device": tree["device"], "rounds": args.rounds, "timing": "graph replays between device events; full_map sampled on its own, scan and locate alternating sample by sample; medians",
           "results": tree["results"]}
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
