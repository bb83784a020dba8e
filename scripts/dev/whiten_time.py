#!/usr/bin/env python3
"""Time bf_whiten_device against the map launch it feeds and against what a user had before (dev tool; GPU box, no CPU fallback):
  whiten   one bf_whiten_device launch: K bands, Hann window, beta = 1, on every row of the batch                    (the code under test)
  rfft     the same weighting with torch.fft.rfft / irfft on the same tensors (window, |X|, band rms, floor, divide,
           mask, inverse, gain), K bands in one batched irfft                                                        (baseline 1)
  das      one bf_das_device launch (lerp) of the same batch: existing code                                          (baseline 2)
at config 2 (190 frames x 64 microphones x 256 samples, 101 x 101 directions) and config 5 (4 x 256 x 1024, 361 x 361), K = 1 and 3.
The rfft formulation is checked against the call to 1e-3 of the output's RMS before anything is timed.
Every sample is one replay of a captured graph that holds `inner` back-to-back calls, between two device events; ROUNDS alternating
rounds in one process; median, minimum, maximum.  By work the call is (1 + K) transforms of N points per row against D * N adds per
row for the map, so it should be a small fraction of the map launch; no time is asserted anywhere, the file records the ratio.
usage: python scripts/dev/whiten_time.py [--rounds 9] [--out profiles/whiten_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat
import whiten

SIZES = {"cfg2": dict(F=190, M=64, N=256, X=101, Y=101, tiles=1), "cfg5": dict(F=4, M=256, N=1024, X=361, Y=361, tiles=4)}
BANDS = [(1000.0, 12000.0), (300.0, 3000.0), (3000.0, 8000.0)]
INNER = {"whiten": 20, "rfft": 10, "das": 3}


def graphed(fn, inner):
    """A captured graph of `inner` back-to-back calls -> a function that replays it once and returns us per call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                             # eager warm-up (the map's digest and adaptive array; the fft plans)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sample():
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3
    return sample


def stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def one_size(name, rounds):
    z = SIZES[name]
    F, M, N, X, Y = z["F"], z["M"], z["N"], z["X"], z["Y"]
    D = X * Y
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=z["tiles"], N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=8)
    from lib.directions import calculate_delays
    table = np.ascontiguousarray(np.float32(calculate_delays()).ravel())
    assert table.size == D * M
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    mics = np.arange(M, dtype=np.int32)
    g = torch.Generator(device="cpu").manual_seed(190)
    frames = (torch.randn((F, M, N), generator=g) * 0.125).cuda()
    img = torch.empty((F, D), dtype=torch.float32, device="cuda")
    lib = nat.lib

    def das():
        lib.bf_das_device(nat.LERP, frames.data_ptr(), M, img.data_ptr(), D, F, nat.iptr(mics), M, 0, D, torch.cuda.current_stream().cuda_stream)

    samplers, errs = {"das": graphed(das, INNER["das"])}, {}
    for K in (1, 3):
        wh = whiten.Whitener(BANDS[:K])
        out = torch.empty((K, F, M, N), dtype=torch.float32, device="cuda")
        d_w = torch.from_numpy(wh.window).cuda()
        k = torch.arange(N // 2 + 1, device="cuda")
        inside = torch.stack([(k >= lo) & (k < hi) for lo, hi in wh.bins.tolist()])[:, None, None, :]        # [K, 1, 1, bins]
        count = torch.tensor([hi - lo for lo, hi in wh.bins.tolist()], dtype=torch.float32, device="cuda")[:, None, None, None]
        gain = torch.from_numpy(wh.gain).cuda()[:, None, None, None]

        def call(wh=wh, K=K, out=out, d_w=d_w):
            lib.bf_whiten_device(frames.data_ptr(), M, F, d_w.data_ptr(), nat.iptr(wh.bins), nat.fptr(wh.beta), nat.fptr(wh.gain), K, wh.floor_rel,
                                 wh.floor_abs, out.data_ptr(), torch.cuda.current_stream().cuda_stream)

        def rfft(wh=wh, d_w=d_w, inside=inside, count=count, gain=gain):
            Xf = torch.fft.rfft(frames * d_w)                                                                # [F, M, bins]
            mag = Xf.abs()
            rms = ((mag * mag)[None] * inside).sum(-1, keepdim=True).div(count).sqrt()                        # [K, F, M, 1]
            d = torch.maximum(mag[None], wh.floor_rel * rms)
            return torch.fft.irfft(torch.where(inside, Xf[None] / d, torch.zeros((), dtype=Xf.dtype, device="cuda")), n=N) * gain

        call()
        torch.cuda.synchronize()
        nat.check()
        ref = rfft()
        errs[K] = float((ref - out).abs().max() / out.pow(2).mean().sqrt())
        assert errs[K] <= 1e-3, (name, K, errs[K])
        samplers[("whiten", K)] = graphed(call, INNER["whiten"])
        samplers[("rfft", K)] = graphed(rfft, INNER["rfft"])
    for s in samplers.values():
        s()
    t = {key: [] for key in samplers}
    for _ in range(rounds):
        for key, s in samplers.items():
            t[key].append(s())
    nat.check()
    das_med = statistics.median(t["das"])
    rec = {"frames": F, "mics": M, "samples": N, "rows": X, "cols": Y, "das_lerp_us": stats(t["das"]), "cases": []}
    for K in (1, 3):
        w_med, r_med = statistics.median(t[("whiten", K)]), statistics.median(t[("rfft", K)])
        rec["cases"].append({"bands": K, "whiten_us": stats(t[("whiten", K)]), "rfft_us": stats(t[("rfft", K)]), "rfft_max_err_over_rms": errs[K],
                             "rfft_over_whiten": round(r_med / w_med, 2), "whiten_over_das": round(w_med / das_med, 5),
                             "bytes_per_call": 4 * F * M * N * (1 + K)})
    return rec


def main(rounds, out):
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds,
           "timing": "one replay of a captured graph of %(whiten)d whiten / %(rfft)d rfft / %(das)d das calls per sample, between device events" % INNER,
           "sizes": {name: one_size(name, rounds) for name in SIZES}}
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
        sys.exit("whiten_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("whiten_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
