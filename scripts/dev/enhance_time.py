#!/usr/bin/env python3
"""Time bf_enhance_device beside the launch that feeds it and beside what a user would otherwise write (dev tool; GPU box, no CPU
fallback):
  enhance  one bf_enhance_device call (its four launches) through enhance.Enhancer.push: n_fft 256, hop_s 128, root-Hann windows, the
           tracker past its learning stretch                                                                  (the code under test)
  miso     the bf_miso_device launch (64 microphones x 256 samples, lerp) that produces its input            (what feeds it)
  torch    the same values by torch: the carried history concatenated in front, torch.stft, the header's gain recursion as a Python
           loop over the frames of elementwise torch operations, torch.fft.irfft, the synthesis window and an overlap-add by
           torch.nn.functional.fold (torch.istft refuses the root-Hann pair without centring: its envelope is zero at the first
           sample), with every shape fixed, as a graph needs it                                              (what it replaces)
for two shapes: the streaming use (one 256-sample window at hop 128, 4 beams: 128 samples and one frame a push) and a batch (190
windows, 64 rows: 24320 samples and 190 frames a row).  The calls are timed as graph replays -- INNER calls captured into one graph,
device events around a replay -- so the figure is the device's, without the host's enqueue cost.  ROUNDS alternating rounds in one
process; median, minimum, maximum.  The torch formulation is checked against the call, push by push from the start of a stream,
before anything is timed.  No time is asserted anywhere.
usage: python scripts/dev/enhance_time.py [--rounds 9] [--out profiles/enhance_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from lib import _native as nat
import enhance
import synth
import util

N, HOP, N_FFT, HOP_S = 256, 128, 256, 128
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
SHAPES = {"streaming": dict(frames=1, rows=4, inner=48, checks=24), "batch": dict(frames=190, rows=64, inner=4, checks=3)}


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


class TorchEnhance:
    """The formulation a user would write, for pushes of a multiple of hop_s samples from the start of a stream (c stays 0)."""

    def __init__(self, en, rows, device):
        self.en = en
        z = lambda n: torch.zeros((rows, n), dtype=torch.float32, device=device)
        self.hist, self.ola, self.lam, self.prior = z(N_FFT - 1), z(N_FFT), z(N_FFT // 2 + 1), z(N_FFT // 2 + 1)
        self.wa, self.ws = en.d_win_a.to(device), en.d_win_s.to(device)
        self.seen = 0                                    # a host value: it is the same for every stream

    def gains(self, P):
        """P [rows, bins, count] -> G of the same shape: the header's recursion, frame by frame."""
        e = self.en
        lam, prior, out = self.lam, self.prior, []
        for i in range(P.shape[2]):
            p = P[:, :, i]
            if self.seen < e.n_init:
                lam = p if self.seen == 0 else lam + (p - lam) / float(self.seen + 1)
                self.seen += 1
            else:
                g = p / lam.clamp(min=FLT_MIN)
                w = ((g - e.g0) / (e.g1 - e.g0)).clamp(0.0, 1.0)
                a = e.a_noise + (1.0 - e.a_noise) * w
                lam = lam + (1.0 - a) * (p - lam)
            den = lam.clamp(min=FLT_MIN)
            xi = e.alpha * (prior / den).clamp(max=FLT_MAX) + (1.0 - e.alpha) * (p / den - 1.0).clamp(min=0.0)
            g_i = (1.0 - 1.0 / (1.0 + xi)).clamp(min=e.g_min)
            prior = g_i * g_i * p
            out.append(g_i)
        self.lam.copy_(lam)
        self.prior.copy_(prior)
        return torch.stack(out, dim=2)

    def push(self, x):
        """x [rows, S], S a multiple of hop_s -> [rows, S]."""
        S = x.shape[1]
        buf = torch.cat([self.hist, x], dim=1)
        X = torch.stft(buf[:, HOP_S - 1:], N_FFT, hop_length=HOP_S, win_length=N_FFT, window=self.wa, center=False, return_complex=True)   # [rows, bins, count]
        Y = self.gains(X.real * X.real + X.imag * X.imag) * X
        v = torch.fft.irfft(Y, n=N_FFT, dim=1) * self.ws[None, :, None]                    # [rows, n_fft, count]
        count = v.shape[2]
        span = (count - 1) * HOP_S + N_FFT
        folded = torch.nn.functional.fold(v, output_size=(1, span), kernel_size=(1, N_FFT), stride=(1, HOP_S))[:, 0, 0]
        acc = torch.cat([self.ola, torch.zeros_like(x)], dim=1)
        acc[:, HOP_S:HOP_S + span] += folded
        self.ola.copy_(acc[:, S:])
        self.hist.copy_(buf[:, S:])
        return acc[:, :S]


def stream_of(beams):
    """[F, B, N] -> [B, F * HOP]: the last HOP samples of every window."""
    return beams[:, :, N - HOP:].permute(1, 0, 2).reshape(beams.shape[1], -1).contiguous()


def one_shape(name, rounds):
    z = SHAPES[name]
    F, B, inner = z["frames"], z["rows"], z["inner"]
    c = util.configure("cfg2")
    M, D = c["M"], c["X"] * c["Y"]
    assert c["N"] == N
    table = util.table_for("lerp", "cfg2")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size)
    nat.check()
    mics = np.arange(M, dtype=np.int32)
    frames = torch.from_numpy(synth.frame_batch(M, N, F)).cuda()
    g = torch.Generator(device="cpu").manual_seed(F * 100 + B)
    offs = (torch.randint(0, D, (F, B), generator=g, dtype=torch.int32) * M).cuda().contiguous()
    beams = torch.empty((F, B, N), dtype=torch.float32, device="cuda")
    status = torch.empty((F, B), dtype=torch.int32, device="cuda")

    def miso():
        return nat.lib.bf_miso_device(util.ALGOS["lerp"], frames.data_ptr(), M, F, nat.iptr(mics), M, offs.data_ptr(), B, 0.0, beams.data_ptr(), N,
                                      status.data_ptr(), torch.cuda.current_stream().cuda_stream)

    assert miso() == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    en = enhance.Enhancer(rows=B, hop=HOP, n_fft=N_FFT, hop_s=HOP_S)
    rec = {"windows": F, "rows": B, "samples": F * HOP, "frames_per_call": F * HOP // HOP_S, "calls_per_graph": inner,
           "workspace_floats": int(nat.lib.bf_enhance_workspace(B, F * HOP, N_FFT, HOP_S))}
    # the check: the same pushes through both formulations from the start of a stream (noise of another seed every push)
    te = TorchEnhance(en, B, "cuda")
    worst, scale = 0.0, float(beams.abs().max())
    for k in range(z["checks"]):
        noisy = beams + 0.05 * scale * torch.randn(beams.shape, generator=torch.Generator(device="cpu").manual_seed(k)).cuda()
        clean, count = en.push(noisy)
        want = te.push(stream_of(noisy))
        torch.cuda.synchronize()
        assert count.cpu().tolist() == [F * HOP // HOP_S, 0]
        worst = max(worst, float((clean - want).abs().max()))
    assert worst < 1e-3 * scale, (name, worst, scale)
    assert te.seen == en.n_init == int(en.state.cpu()[1])
    rec["torch_max_abs_diff_over_peak"] = worst / scale
    nat.check()

    flat = stream_of(beams)
    replays = {"enhance": graph_of(lambda: en.push(beams), inner), "miso": graph_of(miso, inner)}
    try:
        replays["torch"] = graph_of(lambda: te.push(flat), inner)
    except Exception as e:                               # (a library that does not capture: the device figures remain)
        rec["torch_graph_error"] = repr(e)[:200]
        torch.cuda.synchronize()
    t = {k: [] for k in replays}
    for _ in range(rounds):
        for k, fn in replays.items():
            t[k].append(fn())
    nat.check()
    for k, v in t.items():
        rec[k + "_us"] = stats(v)
    e = statistics.median(t["enhance"])
    rec["enhance_over_miso"] = round(e / statistics.median(t["miso"]), 3)
    if "torch" in t:
        rec["torch_over_enhance"] = round(statistics.median(t["torch"]) / e, 2)
    return rec


def main(rounds, out):
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds,
           "what": "n_fft 256, hop_s 128, root-Hann windows, the default Wiener recursion past its learning stretch, on the last 128 samples of every 256-sample beam window",
           "timing": "graph replays of calls_per_graph captured calls, device events around a replay, microseconds per call",
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
        sys.exit("enhance_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("enhance_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
