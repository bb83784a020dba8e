#!/usr/bin/env python3
"""Time bf_filter_sum_device against what a user had before and against the plain listen call (dev tool; GPU box, no CPU fallback):
  filter   one bf_filter_sum_device launch: B beams of T taps per microphone, hop = N / 2, as the launch chooses its waves, and
           with the waves of a workgroup pinned to 1, 4 and 16 (bf_filter_sum_waves)                                (the code under test)
  conv1d   torch.nn.functional.conv1d with the microphones as input channels and the beams as output channels, the T - 1 history
           samples concatenated in front of every row (the concatenation is part of what the user had to do, and is timed)   (baseline 1)
  miso     one bf_miso_device launch (lerp) of the same number of beams: existing code, what a delay-and-sum listen costs    (baseline 2)
for a batch of F = 190 frames and for the live case F = 1, T = 65 and 129, B = 1, 2 and 16, at config 2 (64 microphones x 256 samples)
and the as-shipped size (256 x 256).  conv1d is checked against the call to 1e-5 of the largest output before anything is timed.
Device events around back-to-back enqueues after a warm-up; ROUNDS alternating rounds in one process; median, minimum, maximum.
Rate: F*B*M*N*T fused multiply-adds against the 78.65 T lane-operations/s fp32 vector peak.
No time is asserted anywhere: the file records what null steering costs over a plain listen call, and whether splitting the
microphones over more waves pays at F = 1.
usage: python scripts/dev/filter_sum_time.py [--rounds 9] [--out profiles/filter_sum_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat

SIZES = {"cfg2": dict(M=64, N=256, X=101, Y=101, tiles=1), "shipped": dict(M=256, N=256, X=57, Y=32, tiles=4)}
FRAMES, TAPS, BEAMS, WAVES = (190, 1), (65, 129), (1, 2, 16), (0, 1, 4, 16)
VALU_PEAK = 78.65e12


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
    gen = torch.Generator(device="cpu").manual_seed(190)
    all_frames = (torch.randn((max(FRAMES), M, N), generator=gen) * 0.125).cuda()
    prev = (torch.randn((M, N), generator=gen) * 0.125).cuda()
    s = torch.cuda.current_stream().cuda_stream
    lib = nat.lib

    runs = {}
    for F in FRAMES:
        frames = all_frames[:F].contiguous()
        for T in TAPS:
            for B in BEAMS:
                taps = (torch.randn((B, M, T), generator=gen) / T).cuda()
                w = taps.flip(2).contiguous()                                     # conv1d correlates: [B, M, T], taps reversed
                out = torch.empty((F, B, N), dtype=torch.float32, device="cuda")
                offs = (torch.arange(B, dtype=torch.int32) * (X * Y // B) * M).repeat(F, 1).contiguous().cuda()      # [F, B]: every frame's offsets
                status = torch.empty((F, B), dtype=torch.int32, device="cuda")
                beams = torch.empty((F, B, N), dtype=torch.float32, device="cuda")

                def filt(waves, frames=frames, F=F, T=T, B=B, taps=taps, out=out):
                    lib.bf_filter_sum_waves(waves)
                    rc = lib.bf_filter_sum_device(frames.data_ptr(), M, F, hop, prev.data_ptr(), nat.iptr(mics), M, taps.data_ptr(), T, B, out.data_ptr(), N, s)
                    lib.bf_filter_sum_waves(0)
                    assert rc == 0

                def conv(frames=frames, F=F, T=T, w=w):
                    before = torch.cat([prev[None], frames[:-1]], dim=0)[:, :, hop - (T - 1):hop]
                    return torch.nn.functional.conv1d(torch.cat([before, frames], dim=2), w)      # [F, B, N]

                def miso(frames=frames, F=F, B=B, offs=offs, beams=beams, status=status):
                    rc = lib.bf_miso_device(nat.LERP, frames.data_ptr(), M, F, nat.iptr(mics), M, offs.data_ptr(), B, 0.0, beams.data_ptr(), N,
                                            status.data_ptr(), s)
                    assert rc == 0

                filt(0); miso()
                torch.cuda.synchronize()
                nat.check()
                assert int(status.abs().max()) == 0, (name, F, T, B)
                err = float((conv() - out).abs().max() / out.abs().max())
                assert err <= 1e-5, (name, F, T, B, err)
                runs[(F, T, B)] = (filt, conv, miso, err)
    for _ in range(3):
        for filt, conv, miso, _ in runs.values():
            for waves in WAVES:
                filt(waves)
            conv(); miso()
    torch.cuda.synchronize()
    t = {}
    for key in runs:
        for what in ("conv1d", "miso") + tuple("waves%d" % v for v in WAVES):
            t[(what,) + key] = []
    for _ in range(rounds):
        for key, (filt, conv, miso, _) in runs.items():
            inner = 20 if key[0] > 1 else 100
            for waves in WAVES:
                t[("waves%d" % waves,) + key].append(timed(lambda: filt(waves), inner))
            t[("conv1d",) + key].append(timed(conv, 10))
            t[("miso",) + key].append(timed(miso, inner))
    nat.check()
    rec = {"mics": M, "samples": N, "hop": hop, "cases": []}
    for key, (_, _, _, err) in runs.items():
        F, T, B = key
        med = {what: statistics.median(t[(what,) + key]) for what in ("conv1d", "miso", "waves0", "waves1", "waves4", "waves16")}
        fma = F * B * M * N * T
        rec["cases"].append({"frames": F, "n_taps": T, "beams": B, "filter_us": stats(t[("waves0",) + key]),
                             "filter_1_wave_us": stats(t[("waves1",) + key]), "filter_4_waves_us": stats(t[("waves4",) + key]),
                             "filter_16_waves_us": stats(t[("waves16",) + key]), "conv1d_us": stats(t[("conv1d",) + key]),
                             "miso_lerp_us": stats(t[("miso",) + key]), "conv1d_max_err_rel": err,
                             "conv1d_over_filter": round(med["conv1d"] / med["waves0"], 2), "filter_over_miso": round(med["waves0"] / med["miso"], 2),
                             "one_wave_over_16_waves": round(med["waves1"] / med["waves16"], 2), "four_waves_over_16_waves": round(med["waves4"] / med["waves16"], 2),
                             "fma_per_call": fma, "fraction_of_fp32_vector_peak": round(fma / (med["waves0"] * 1e-6) / VALU_PEAK, 4)})
    return rec


def main(rounds, out):
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds,
           "timing": "device events around back-to-back enqueues: 20 calls per sample at 190 frames, 100 at 1 frame, 10 for conv1d",
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
        sys.exit("filter_sum_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("filter_sum_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
