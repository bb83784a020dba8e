#!/usr/bin/env python3
"""Time the continuous-stream calls against the calls they extend (dev tool; GPU box, no CPU fallback):
  1. beams   bf_miso_stream_device against bf_miso_device: config 2 (64 x 256) and the as-shipped size (256 x 256), 190 frames, 1 and 16
             beams, hop = N and N / 2, pad and lerp.  The new staging moves (N + H) / N of the bytes.
  2. maps    bf_das_stream_device against bf_das_device at config 1, config 2 and as shipped, 190 frames, pad and lerp: the price of the
             strided kernel the stream maps always take.  Floor: real time -- with hop = N / 2 the stream delivers SAMPLE_RATE / hop
             windows per second (as shipped 48828 / 128 = 381.5); the measured rate must be above it.
  3. bench   `python bench.py` (the flagship line) with each library, alternating, `--bench-runs` times each.
Baseline = ANOTHER build of the library, normally the parent commit's (--parent-lib; loaded through BF_NATIVE_LIB in a child process of
its own, as scripts/dev/bench_line.sh does).  The child that loads the in-tree library also times ITS bf_miso_device / bf_das_device,
alternating with the stream call sample by sample: the same code as the parent's, so the two figures show the process-to-process spread.
Device events around back-to-back enqueues after a warm-up; every figure is the median / min / max over --samples samples.
Exit status 1 when a stream map rate is not above real time.
usage: python scripts/dev/stream_time.py --parent-lib <libbeamformer_hip.so of the parent> [--out profiles/stream_time.json]"""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = 190
SAMPLE_RATE = 48828.0          # config.json, as shipped
BEAM_SIZES, MAP_SIZES = ["cfg2", "shipped"], ["cfg1", "cfg2", "shipped"]


def stats(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def child(samples):
    """Runs in a process of its own with the library $BF_NATIVE_LIB names (or the in-tree one): one JSON object on the last line."""
    import numpy as np, torch
    from lib import _native as nat
    import synth, util
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("stream_time: no usable HIP device; this measurement has no CPU fallback")
    lib = nat.lib
    has_stream = getattr(lib, "bf_miso_stream_device", None) is not None and lib.bf_miso_stream_device.argtypes is not None
    s = torch.cuda.current_stream().cuda_stream

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3        # us per call

    def measure(fns, inner):
        """Alternate the callables sample by sample -> one list of us per callable."""
        for fn in fns:
            for _ in range(3):
                assert fn() == 0, lib.bf_last_error()
        torch.cuda.synchronize()
        nat.check()
        out = [[] for _ in fns]
        for _ in range(samples):
            for i, fn in enumerate(fns):
                out[i].append(timed(fn, inner))
        nat.check()
        return out

    def load(algo, name):
        table = util.table_for(algo, name)
        if algo == "pad":
            lib.load_coefficients_pad(nat.iptr(table), table.size)
        else:
            lib.load_coefficients_lerp(nat.fptr(table), table.size)
        nat.check()

    recs = []
    for name in MAP_SIZES:
        c = util.configure(name)
        M, N, D = c["M"], c["N"], c["X"] * c["Y"]
        mics = np.arange(M, dtype=np.int32)
        x = torch.from_numpy(synth.frame_batch(M, N, FRAMES)).cuda()
        prev = x[-1].clone()
        img = torch.empty((FRAMES, D), dtype=torch.float32, device="cuda")
        for algo in ("pad", "lerp"):
            load(algo, name)
            a = util.ALGOS[algo]
            H = lib.bf_stream_history(a) if has_stream else None
            plain = lambda: lib.bf_das_device(a, x.data_ptr(), M, img.data_ptr(), D, FRAMES, nat.iptr(mics), M, 0, D, s)
            if name in BEAM_SIZES:
                for B in (1, 16):
                    offs = (torch.randint(0, D, (FRAMES, B), dtype=torch.int32, device="cuda") * M).contiguous()
                    out = torch.empty((FRAMES, B, N), dtype=torch.float32, device="cuda")
                    miso = lambda: lib.bf_miso_device(a, x.data_ptr(), M, FRAMES, nat.iptr(mics), M, offs.data_ptr(), B, 0.0, out.data_ptr(), N, None, s)
                    fns = [miso]
                    if has_stream:
                        for hop in (N, N // 2):
                            fns.append(lambda hop=hop: lib.bf_miso_stream_device(a, x.data_ptr(), M, FRAMES, hop, prev.data_ptr(), nat.iptr(mics), M,
                                                                                 offs.data_ptr(), B, 0.0, out.data_ptr(), N, None, s))
                    t = measure(fns, 50)
                    rec = {"what": "beams", "size": name, "algo": algo, "frames": FRAMES, "beams": B, "history": H, "bf_miso_device_us": stats(t[0])}
                    if has_stream:
                        rec["bf_miso_stream_device_us"] = {"hop_N": stats(t[1]), "hop_N_half": stats(t[2])}
                    recs.append(rec)
                    print(json.dumps(rec), file=sys.stderr, flush=True)
            fns = [plain]
            if has_stream:
                for hop in (N, N // 2):
                    fns.append(lambda hop=hop: lib.bf_das_stream_device(a, x.data_ptr(), M, img.data_ptr(), D, FRAMES, hop, prev.data_ptr(), nat.iptr(mics), M,
                                                                        0, D, s))
            t = measure(fns, 5 if name == "cfg1" else 2)
            rec = {"what": "maps", "size": name, "algo": algo, "frames": FRAMES, "directions": D, "history": H, "bf_das_device_us": stats(t[0])}
            if has_stream:
                rec["bf_das_stream_device_us"] = {"hop_N": stats(t[1]), "hop_N_half": stats(t[2])}
            recs.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "results": recs}))


def run_child(lib_path, samples):
    env = dict(os.environ)
    env.pop("BF_NATIVE_LIB", None)
    if lib_path:
        env["BF_NATIVE_LIB"] = lib_path
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(samples)], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        sys.exit("stream_time: the child with library %s failed (exit %d)" % (lib_path or "in-tree", p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def run_bench(lib_path):
    env = dict(os.environ)
    env.pop("BF_NATIVE_LIB", None)
    if lib_path:
        env["BF_NATIVE_LIB"] = lib_path
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.DEVNULL, text=True, timeout=600, cwd=ROOT)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        sys.exit("stream_time: bench.py with library %s failed (exit %d)" % (lib_path or "in-tree", p.returncode))
    return json.loads(lines[-1])["value"]


def key(r):
    return (r["what"], r["size"], r["algo"], r.get("beams"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libbeamformer_hip.so of the parent commit (the baseline)")
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.samples < 5:
        sys.exit("stream_time: at least five samples")
    if args.child:
        child(args.samples)
        sys.exit(0)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("stream_time: --parent-lib must name the parent commit's build of the library")
    parent = run_child(os.path.abspath(args.parent_lib), args.samples)
    new = run_child(None, args.samples)
    base = {key(r): r for r in parent["results"]}
    results, ok = [], True
    for r in new["results"]:
        b = base[key(r)]
        call = "bf_miso_device_us" if r["what"] == "beams" else "bf_das_device_us"
        stream_call = "bf_miso_stream_device_us" if r["what"] == "beams" else "bf_das_stream_device_us"
        N = 256
        rec = {k: r[k] for k in ("what", "size", "algo", "frames", "history") if k in r}
        if r["what"] == "beams":
            rec["beams"] = r["beams"]
        else:
            rec["directions"] = r["directions"]
        rec["parent_" + call] = b[call]
        rec["in_tree_" + call] = r[call]
        rec[stream_call] = r[stream_call]
        pm = b[call]
        rec["parent_spread_max_over_median"] = round(pm["max"] / pm["median"], 3)
        rec["ratio_stream_over_parent"] = {h: round(v["median"] / pm["median"], 3) for h, v in r[stream_call].items()}
        if r["what"] == "beams":
            rec["bytes_factor_N_plus_H_over_N"] = round((N + r["history"]) / N, 3)
        else:
            rate = {h: round(r["frames"] / (v["median"] * 1e-6), 1) for h, v in r[stream_call].items()}
            rec["stream_windows_per_s"] = rate
            rec["real_time_windows_per_s"] = {"hop_N": round(SAMPLE_RATE / N, 1), "hop_N_half": round(SAMPLE_RATE / (N // 2), 1)}
            rec["above_real_time"] = all(rate[h] > rec["real_time_windows_per_s"][h] for h in rate)
            ok = ok and rec["above_real_time"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
    bench = {"parent_frames_per_s": [], "in_tree_frames_per_s": []}
    for _ in range(args.bench_runs):
        bench["parent_frames_per_s"].append(round(run_bench(os.path.abspath(args.parent_lib)), 1))
        bench["in_tree_frames_per_s"].append(round(run_bench(None), 1))
    if args.bench_runs:
        p, n = bench["parent_frames_per_s"], bench["in_tree_frames_per_s"]
        bench["parent_spread"] = round((max(p) - min(p)) / statistics.median(p), 4)
        bench["in_tree_median_over_parent_median"] = round(statistics.median(n) / statistics.median(p), 4)
        bench["command"] = "python bench.py --gpus 1 --steps 20 --warmup 3, alternating libraries"
        print(json.dumps(bench), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": new["device"], "samples": args.samples,
                       "timing": "device events around back-to-back enqueues (50 per sample for beams, 2 - 5 for maps), median / min / max over the samples",
                       "results": results, "bench": bench}, f, indent=1)
            f.write("\n")
    sys.exit(0 if ok else 1)
