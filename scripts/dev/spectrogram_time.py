#!/usr/bin/env python3
"""Time bf_spectrogram_device beside the launch that feeds it and beside what a user would otherwise write (dev tool; GPU box, no CPU
fallback):
  spectrogram  one bf_spectrogram_device call (its two launches): n_fft 512, Hann 400, hop 160, 80 mel bands, log10, its length read
               from the resampler's device count                                                              (the code under test)
  resample     the bf_resample_device call (48828 -> 16000 Hz, 32 taps, float32 only) that produces its input    (what feeds it)
  torch        the same values by torch: the carried tail concatenated in front, torch.stft, |.|^2, the bank as a matmul, clamp,
               log10 -- with every shape fixed, as a graph needs it (the count is taken to be cap)            (what it replaces)
  *_wall       eager calls, wall time to a finished result: the call under test (nothing reaches the host), and the torch formulation
               when the count has to reach the host first (count.cpu(), then slicing, framing and the new tail by that count)
for two shapes: the streaming use (one 256-sample window at hop 128, 4 beams: 42 or 43 samples a push, a frame every fourth push) and
a batch (190 windows, 64 rows: 7969 samples and 49 or 50 frames a row).  The device calls are timed as graph replays -- INNER calls captured
into one graph, device events around a replay -- so the figure is the device's, without the host's enqueue cost.  ROUNDS alternating
rounds in one process; median, minimum, maximum.  The torch formulation is checked against the call before anything is timed.  No time
is asserted anywhere.
usage: python scripts/dev/spectrogram_time.py [--rounds 9] [--out profiles/spectrogram_time.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
import numpy as np
import torch
from interface import config
from lib import _native as nat
import audio_out
import features

N, HOP, SR = 256, 128, 16000
N_FFT, N_WIN, HOP_S, N_MELS, FLOOR = 512, 400, 160, 80, 1e-10
SHAPES = {"streaming": dict(frames=1, rows=4, inner=48, checks=24), "batch": dict(frames=190, rows=64, inner=10, checks=4)}


def stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def graph_of(fn, inner):
    """`inner` calls of fn captured back to back; returns a function that replays them once and gives microseconds per call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                             # eager warm-up
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


class TorchFrames:
    """The formulation a user would write.  torch.stft centres a 400-sample window in its 512-sample frame, so the stream is framed 56
    samples early (zeros in front of the first call, and behind every call for the last frame's 56); the power is the same."""
    PAD = (N_FFT - N_WIN) // 2

    def __init__(self, rows, bank):
        self.window = torch.from_numpy(features.hann(N_WIN)).cuda()
        self.bank = torch.from_numpy(bank).cuda()
        self.zeros = torch.zeros((rows, self.PAD), dtype=torch.float32, device="cuda")
        self.tail = torch.zeros((rows, 0), dtype=torch.float32, device="cuda")

    def frames_of(self, buf):
        x = torch.cat([self.zeros, buf, self.zeros], dim=1)
        X = torch.stft(x, N_FFT, hop_length=HOP_S, win_length=N_WIN, window=self.window, center=False, return_complex=True)     # [rows, 257, frames]
        power = X.real * X.real + X.imag * X.imag
        return torch.log10(torch.clamp(torch.matmul(self.bank, power), min=FLOOR)).transpose(1, 2)

    def push(self, audio, count):
        """audio [rows, cap] with `count` samples there (a host int: the count has reached the host) -> [rows, frames, 80] or None."""
        buf = torch.cat([self.tail, audio[:, :count]], dim=1)
        n = (buf.shape[1] - N_WIN) // HOP_S + 1 if buf.shape[1] >= N_WIN else 0
        out = self.frames_of(buf[:, :(n - 1) * HOP_S + N_WIN]) if n else None
        self.tail = buf[:, n * HOP_S:].clone()
        return out


def one_shape(name, rounds):
    z = SHAPES[name]
    F, B, inner = z["frames"], z["rows"], z["inner"]
    lib = nat.lib
    g = torch.Generator(device="cpu").manual_seed(F * 100 + B)
    beams = (torch.randn((F, B, N), generator=g) * 0.125).cuda()
    prev = torch.zeros((B, N), dtype=torch.float32, device="cuda")
    ao = audio_out.AudioOut(SR, rows=B, hop=HOP, pcm=False)
    bank, support = features.design_mel(SR, N_FFT, N_MELS)
    bf = features.BeamFeatures(SR, B, bank=bank, support=support, floor=FLOOR)
    S = F * HOP
    cap = int(lib.bf_resample_capacity(S, ao.up, ao.down))
    capf = int(lib.bf_spectrogram_capacity(cap, HOP_S))
    audio = torch.empty((B, cap), dtype=torch.float32, device="cuda")
    feat = torch.empty((B, capf, N_MELS), dtype=torch.float32, device="cuda")

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def resample():
        return lib.bf_resample_device(beams.data_ptr(), B, F, N, N, HOP, prev.data_ptr(), ao.d_taps.data_ptr(), ao.up, ao.down, ao.T, ao.state.data_ptr(), ao.gain,
                                      audio.data_ptr(), cap, None, None, ao.count.data_ptr(), stream())

    def spectrogram():
        return lib.bf_spectrogram_device(audio.data_ptr(), B, cap, cap, ao.count.data_ptr(), bf.hist.data_ptr(), bf.state.data_ptr(), bf.d_window.data_ptr(),
                                         N_WIN, N_FFT, HOP_S, bf.d_bank.data_ptr(), bf.d_support.data_ptr(), N_MELS, 1.0, FLOOR, feat.data_ptr(), capf,
                                         bf.count.data_ptr(), stream())

    rec = {"windows": F, "rows": B, "samples_in": S, "cap_samples": cap, "cap_frames": capf, "calls_per_graph": inner}
    # the check: pushes of the same beams through both formulations, frame for frame (the streaming shape completes its first frame in the tenth)
    tf = TorchFrames(B, bank)
    worst, frames_seen, samples_seen = 0.0, 0, 0
    for _ in range(z["checks"]):
        assert resample() == 0 and spectrogram() == 0, lib.bf_last_error()
        torch.cuda.synchronize()
        n_audio, n_frames = int(ao.count.cpu()[0]), int(bf.count.cpu()[0])
        want = tf.push(audio, n_audio)
        assert (0 if want is None else want.shape[1]) == n_frames, (name, n_frames, None if want is None else want.shape)
        if n_frames:
            worst = max(worst, float((feat[:, :n_frames] - want).abs().max()))
        frames_seen += n_frames
        samples_seen += n_audio
    assert frames_seen > 0 and worst < 1e-3, (name, frames_seen, worst)                 # (log10 units; float32 on both sides)
    rec["torch_max_abs_diff_log10"] = worst
    rec["frames_per_call"] = round(frames_seen / float(z["checks"]), 2)
    rec["samples_per_call"] = round(samples_seen / float(z["checks"]), 2)
    nat.check()

    fixed_tail = torch.zeros((B, N_WIN - 1), dtype=torch.float32, device="cuda")

    def torch_fixed():                                   # every shape fixed: the count is taken to be cap, the tail 399 samples
        buf = torch.cat([fixed_tail, audio], dim=1)
        n = (buf.shape[1] - N_WIN) // HOP_S + 1
        out = tf.frames_of(buf[:, :(n - 1) * HOP_S + N_WIN])
        fixed_tail.copy_(buf[:, buf.shape[1] - (N_WIN - 1):])
        return out

    def spectrogram_wall():
        t0 = time.perf_counter()
        spectrogram()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def torch_wall():
        t0 = time.perf_counter()
        tf.push(audio, int(ao.count.cpu()[0]))           # the count reaches the host: a synchronising copy
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    replays = {"spectrogram": graph_of(spectrogram, inner), "resample": graph_of(resample, inner)}
    try:
        replays["torch"] = graph_of(torch_fixed, inner)
        rec["torch_frames_per_call"] = int(((N_WIN - 1 + cap) - N_WIN) // HOP_S + 1)
    except Exception as e:                               # (a library that does not capture: the eager figures remain)
        rec["torch_graph_error"] = repr(e)[:200]
        torch.cuda.synchronize()
    walls = {"spectrogram_wall": spectrogram_wall, "torch_count_on_host_wall": torch_wall}
    t = {k: [] for k in list(replays) + list(walls)}
    for _ in range(rounds):
        for k, fn in replays.items():
            t[k].append(fn())
        resample()
        torch.cuda.synchronize()
        for k, fn in walls.items():
            t[k].append(fn())
    nat.check()
    for k, v in t.items():
        rec[k + "_us"] = stats(v)
    s = statistics.median(t["spectrogram"])
    rec["spectrogram_over_resample"] = round(s / statistics.median(t["resample"]), 3)
    if "torch" in t:
        rec["torch_over_spectrogram"] = round(statistics.median(t["torch"]) / s, 3)
    rec["torch_count_on_host_wall_over_spectrogram_wall"] = round(statistics.median(t["torch_count_on_host_wall"]) / statistics.median(t["spectrogram_wall"]), 2)
    return rec


def main(rounds, out):
    config.configure(N_MICROPHONES=4, N_SAMPLES=N, MAX_RES_X=2, MAX_RES_Y=1, N_TAPS=8)
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds,
           "what": "48828 -> 16000 Hz (32 taps), then n_fft 512, Hann 400, hop 160, 80 mel bands, log10; the spectrogram's length is the resampler's device count",
           "timing": "spectrogram, resample, torch: graph replays of calls_per_graph captured calls, device events around a replay, microseconds per call; "
                     "*_wall: eager, wall time from the call to a synchronised device, microseconds",
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
        sys.exit("spectrogram_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("spectrogram_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
