#!/usr/bin/env python3
"""Time bf_resample_device beside the launch that feeds it and beside what it replaces (dev tool; GPU box, no CPU fallback):
  resample  one bf_resample_device call (its two launches), 48828 -> 48000 Hz (4000 / 4069, 32 taps), float32 + PCM   (the code under test)
  miso      the bf_miso_device launch (lerp, 64 microphones x 256 samples) that produces the same rows                  (what feeds it)
  host      what a user had before: the device-to-host copy of the beams, a vectorised float64 NumPy polyphase loop over the
            taps, and the upload of the result                                                                          (what it replaces)
for three shapes: the streaming use (one window, hop 128, 4 beams), a batch (190 windows, 4 beams) and a wide one (190 windows,
64 rows).  The device calls are timed as graph replays -- INNER calls captured into one graph, device events around a replay --
so the figure is the device's, without the host's enqueue cost; the host path is wall time around a synchronised copy, the loop and
the upload.  ROUNDS alternating rounds in one process; median, minimum, maximum.  The NumPy loop is checked against the call to 1e-5
of the largest output before anything is timed.  No time is asserted anywhere.
usage: python scripts/dev/resample_time.py [--rounds 9] [--out profiles/resample_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat
import audio_out

M, N, X, Y, HOP = 64, 256, 11, 11, 128
SHAPES = {"streaming": dict(frames=1, rows=4, inner=50), "batch": dict(frames=190, rows=4, inner=20), "wide": dict(frames=190, rows=64, inner=10)}


def stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def graph_of(fn, inner):
    """`inner` calls of fn captured back to back; returns a function that replays them once and gives microseconds per call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                             # eager warm-up (the miso launch uploads its adaptive array once)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def replay():
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3
    return replay


def polyphase64(x, h64, L, Mdown):
    """x float64 [R, S] from the start of a stream (silence before it) -> float64 [R, ceil(S L / M)]: a loop over the taps, all outputs at once."""
    R, S = x.shape
    T = h64.shape[1]
    k = np.arange(-(-(S * L) // Mdown), dtype=np.int64)
    a = k * Mdown
    i, p = a // L + (T - 1), a % L
    ext = np.concatenate([np.zeros((R, T - 1)), x], axis=1)
    y = np.zeros((R, k.size))
    for t in range(T):
        y += h64[p, t][None, :] * ext[:, i - t]
    return y


def one_shape(name, rounds):
    z = SHAPES[name]
    F, B, inner = z["frames"], z["rows"], z["inner"]
    lib = nat.lib
    g = torch.Generator(device="cpu").manual_seed(F * 100 + B)
    frames = (torch.randn((F, M, N), generator=g) * 0.125).cuda()
    mics = np.arange(M, dtype=np.int32)
    offs = ((torch.arange(F * B, dtype=torch.int32).view(F, B) * 7) % (X * Y) * M).cuda()
    beams = torch.empty((F, B, N), dtype=torch.float32, device="cuda")
    status = torch.empty((F, B), dtype=torch.int32, device="cuda")
    ao = audio_out.AudioOut(48000, rows=B, hop=HOP, gain=1.0 / M)
    S = F * HOP
    cap = lib.bf_resample_capacity(S, ao.up, ao.down)
    audio = torch.empty((B, cap), dtype=torch.float32, device="cuda")
    pcm = torch.empty((cap, B), dtype=torch.int16, device="cuda")
    prev = torch.zeros((B, N), dtype=torch.float32, device="cuda")

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def miso():
        return lib.bf_miso_device(nat.LERP, frames.data_ptr(), M, F, nat.iptr(mics), M, offs.data_ptr(), B, 0.0, beams.data_ptr(), N, status.data_ptr(), stream())

    def resample():
        return lib.bf_resample_device(beams.data_ptr(), B, F, N, N, HOP, prev.data_ptr(), ao.d_taps.data_ptr(), ao.up, ao.down, ao.T, ao.state.data_ptr(), ao.gain,
                                      audio.data_ptr(), cap, pcm.data_ptr(), ao.clip.data_ptr(), ao.count.data_ptr(), stream())

    rec = {"frames": F, "rows": B, "samples": N, "hop": HOP, "stream_samples_per_row": S, "cap": int(cap), "calls_per_graph": inner}
    miso_ok = miso() == 0
    torch.cuda.synchronize()
    if not miso_ok:                                      # (more beams than one miso launch takes: the rows are then noise, the time is still the call's)
        rec["miso_refused"] = lib.bf_last_error().decode()
        lib.bf_clear_error()
        beams.copy_((torch.randn((F, B, N), generator=g) * 0.125).cuda())
    assert resample() == 0, lib.bf_last_error()
    torch.cuda.synchronize()
    nat.check()
    count = int(ao.count.cpu()[0])
    h64 = ao.taps.astype(np.float64)

    def host():
        x = beams.cpu().numpy()                          # the device-to-host copy (synchronises)
        t1 = time.perf_counter()
        joined = x[:, :, N - HOP:].transpose(1, 0, 2).reshape(B, S).astype(np.float64)
        y = (polyphase64(joined, h64, ao.up, ao.down) * ao.gain).astype(np.float32)
        t2 = time.perf_counter()
        up = torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        return y, up, t1, t2

    y, _, _, _ = host()
    got = audio.cpu().numpy()
    err = float(np.abs(got[:, :count] - y[:, :count]).max() / np.abs(got).max())
    assert err <= 1e-5 and count == cap, (name, err, count, cap)
    rec["numpy_max_err_rel"] = err
    replays = {"resample": graph_of(resample, inner)}
    if miso_ok:
        replays["miso"] = graph_of(miso, inner)
    t = {k: [] for k in list(replays) + ["host_copy", "host_numpy", "host_upload", "host_total"]}
    for _ in range(rounds):
        for k, fn in replays.items():
            t[k].append(fn())
        t0 = time.perf_counter()
        _, _, t1, t2 = host()
        t3 = time.perf_counter()
        for k, v in (("host_copy", t1 - t0), ("host_numpy", t2 - t1), ("host_upload", t3 - t2), ("host_total", t3 - t0)):
            t[k].append(v * 1e6)
    nat.check()
    for k, v in t.items():
        rec[k + "_us"] = stats(v)
    r = statistics.median(t["resample"])
    rec["host_over_resample"] = round(statistics.median(t["host_total"]) / r, 1)
    if miso_ok:
        rec["resample_over_miso"] = round(r / statistics.median(t["miso"]), 3)
    rec["fma_per_call"] = int(cap) * B * ao.T
    return rec


def main(rounds, out):
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=8)
    from lib.directions import calculate_delays
    table = np.ascontiguousarray(np.float32(calculate_delays()).ravel())
    assert table.size == X * Y * M
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "ratio": "48828 -> 48000 Hz = 4000 / 4069, 32 taps, float32 + PCM",
           "timing": "device calls: graph replays of calls_per_graph captured calls, device events around a replay, microseconds per call; "
                     "host path: wall time around the synchronised device-to-host copy, the float64 NumPy loop over the taps, and the upload",
           "shapes": {name: one_shape(name, rounds) for name in SHAPES}}
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
        sys.exit("resample_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("resample_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
