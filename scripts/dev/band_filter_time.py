#!/usr/bin/env python3
"""Time bf_band_filter_device against what a user had before and against the map launch it feeds (dev tool; GPU box, no CPU fallback):
  filter   one bf_band_filter_device launch: K bands of T taps on every row of a 190-frame batch, hop = N / 2       (the code under test)
  conv1d   torch.nn.functional.conv1d on the same tensors, the T - 1 history samples concatenated in front of every row
           (the concatenation is part of what the user had to do, and is timed)                                      (baseline 1)
  das      one bf_das_device launch (lerp) of the same batch: existing code                                          (baseline 2)
at config 2 (64 microphones x 256 samples, 101 x 101 directions) and the as-shipped size (256 x 256, 57 x 32), T = 65 and 129,
K = 1 and 4.  conv1d is checked against the call to 1e-5 of the largest output before anything is timed.
Device events around back-to-back enqueues after a warm-up; ROUNDS alternating rounds in one process; median, minimum, maximum.
Rates: F*R*N*T*K fused multiply-adds against the 78.65 T lane-operations/s fp32 vector peak, and 4*F*R*N*(1 + K) bytes against the
8 TB/s HBM peak.  The batches fit the Infinity Cache, so the byte rate is a rate of this benchmark.
No time is asserted anywhere: the file records whether the call costs more than a tenth of its map launch at K = 1.
usage: python scripts/dev/band_filter_time.py [--rounds 9] [--out profiles/band_filter_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat
import band

F = 190
SIZES = {"cfg2": dict(M=64, N=256, X=101, Y=101, tiles=1), "shipped": dict(M=256, N=256, X=57, Y=32, tiles=4)}
VALU_PEAK, HBM_PEAK = 78.65e12, 8e12


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3        # us per call


def stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def one_size(name, rounds):
    z = SIZES[name]
    M, N, X, Y = z["M"], z["N"], z["X"], z["Y"]
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=z["tiles"], N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=8)
    from lib.directions import calculate_delays
    table = np.ascontiguousarray(np.float32(calculate_delays()).ravel())
    assert table.size == X * Y * M
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    mics = np.arange(M, dtype=np.int32)
    hop = N // 2
    g = torch.Generator(device="cpu").manual_seed(190)
    frames = (torch.randn((F, M, N), generator=g) * 0.125).cuda()
    prev = (torch.randn((M, N), generator=g) * 0.125).cuda()
    img = torch.empty((F, X * Y), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    lib = nat.lib

    def das():
        lib.bf_das_device(nat.LERP, frames.data_ptr(), M, img.data_ptr(), X * Y, F, nat.iptr(mics), M, 0, X * Y, s)

    runs = {}
    for T in (65, 129):
        for K in (1, 4):
            bands = [(3000.0, 8000.0), (300.0, 3000.0), (8000.0, 16000.0), (0.0, 300.0)][:K]
            bf = band.BandFilter(bands, n_taps=T, hop=hop)
            bf.advance(prev[None])
            w = bf.d_taps.flip(1).unsqueeze(1).contiguous()                      # conv1d correlates: [K, 1, T], taps reversed
            out = torch.empty((K, F, M, N), dtype=torch.float32, device="cuda")

            def filt(T=T, K=K, h=bf.d_taps, out=out):
                lib.bf_band_filter_device(frames.data_ptr(), M, F, hop, prev.data_ptr(), h.data_ptr(), T, K, out.data_ptr(), s)

            def conv(T=T, w=w):
                before = torch.cat([prev[None], frames[:-1]], dim=0)[:, :, hop - (T - 1):hop]
                ext = torch.cat([before, frames], dim=2).view(F * M, 1, T - 1 + N)
                return torch.nn.functional.conv1d(ext, w)                         # [F * M, K, N]

            filt()
            torch.cuda.synchronize()
            nat.check()
            ref = conv().view(F, M, K, N).permute(2, 0, 1, 3)
            err = float((ref - out).abs().max() / out.abs().max())
            assert err <= 1e-5, (name, T, K, err)
            runs[(T, K)] = (filt, conv, err)
    for _ in range(3):
        das()
        for filt, conv, _ in runs.values():
            filt(); conv()
    torch.cuda.synchronize()
    t = {"das": []}
    for key in runs:
        t[("filter",) + key], t[("conv1d",) + key] = [], []
    for _ in range(rounds):
        t["das"].append(timed(das, 10))
        for key, (filt, conv, _) in runs.items():
            t[("filter",) + key].append(timed(filt, 100))
            t[("conv1d",) + key].append(timed(conv, 20))
    nat.check()
    das_med = statistics.median(t["das"])
    rec = {"mics": M, "samples": N, "rows": X, "cols": Y, "frames": F, "hop": hop, "das_lerp_us": stats(t["das"]), "cases": []}
    for (T, K), (_, _, err) in runs.items():
        f_med = statistics.median(t[("filter", T, K)])
        c_med = statistics.median(t[("conv1d", T, K)])
        fma, nbytes = F * M * N * T * K, 4 * F * M * N * (1 + K)
        rec["cases"].append({"n_taps": T, "bands": K, "filter_us": stats(t[("filter", T, K)]), "conv1d_us": stats(t[("conv1d", T, K)]),
                             "conv1d_max_err_rel": err, "conv1d_over_filter": round(c_med / f_med, 2), "filter_over_das": round(f_med / das_med, 4),
                             "fma_per_call": fma, "fraction_of_fp32_vector_peak": round(fma / (f_med * 1e-6) / VALU_PEAK, 4),
                             "bytes_per_call": nbytes, "fraction_of_hbm_peak": round(nbytes / (f_med * 1e-6) / HBM_PEAK, 4)})
    rec["filter_over_a_tenth_of_das_at_one_band"] = any(c["bands"] == 1 and c["filter_over_das"] > 0.1 for c in rec["cases"])
    return rec


def main(rounds, out):
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds,
           "timing": "device events around back-to-back enqueues: 100 filter / 20 conv1d / 10 das calls per sample",
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
        sys.exit("band_filter_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("band_filter_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
