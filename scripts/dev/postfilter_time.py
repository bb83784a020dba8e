#!/usr/bin/env python3
"""Time bf_postfilter_device beside its neighbours in the chain and beside what a user would otherwise write (dev tool; GPU box, no CPU
fallback):
  postfilter  one bf_postfilter_device call (its four launches) through postfilter.SpatialPostFilter.gains: n_fft 256, hop_s 128, the
              root-Hann analysis window, beta 0.8, the microphones' denominator, 4 slots                     (the code under test)
  miso        the bf_miso_device launch (lerp) that makes the 4 beams of the same windows                    (the `listen` beside it)
  enhance     the bf_enhance_device call, with the post-filter's gains given, that applies them              (what it feeds)
  torch       the same gains by torch: the carried history concatenated in front, torch.stft of the microphones' rows, the steering
              as an einsum over the microphones, and the recursion as a Python loop over the frames of elementwise torch operations,
              with every shape fixed, as a graph needs it                                                    (what it replaces)
for two shapes: the streaming use (one 256-sample window at hop 128: 128 samples and one frame a call) and a batch (190 windows: 24320
samples and 190 frames).  The calls are timed as graph replays -- INNER calls captured into one graph, device events around a replay --
so the figure is the device's, without the host's enqueue cost.  ROUNDS alternating rounds in one process; median, minimum, maximum.
The torch formulation is checked against the call, call by call from the start of a stream, before anything is timed.  No time is
asserted anywhere.
usage: python scripts/dev/postfilter_time.py [--rounds 9] [--out profiles/postfilter_time.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from lib import _native as nat
import enhance
import postfilter
import synth
import util

N, HOP, N_FFT, HOP_S, SLOTS = 256, 128, 256, 128, 4
SHAPES = {"streaming": dict(frames=1, inner=48, checks=24), "batch": dict(frames=190, inner=4, checks=3)}


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


class TorchPostfilter:
    """The formulation a user would write, for calls of a multiple of hop_s samples from the start of a stream (c stays 0, lag 0)."""

    def __init__(self, pf, dirs):
        self.pf = pf
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
        self.hist, self.N, self.D = z(pf.n, N_FFT - 1), z(pf.slots, pf.n_bins), z(pf.slots, pf.n_bins)
        self.tau = pf.d_tau[torch.as_tensor(dirs, device="cuda")]                             # [slots, M] float64
        self.k = torch.arange(pf.n_bins, dtype=torch.float64, device="cuda")
        self.seen = False                                # a host value: it is the same for every slot

    def gains(self, x):
        """x [M, S], S a multiple of hop_s -> G [slots, count, bins]."""
        pf, n = self.pf, self.pf.n
        buf = torch.cat([self.hist, x], dim=1)
        X = torch.stft(buf[:, HOP_S - 1:], N_FFT, hop_length=HOP_S, win_length=N_FFT, window=pf.d_window, center=False, return_complex=True)   # [M, bins, count]
        phase = (-2.0 * np.pi / N_FFT) * self.tau[:, :, None] * self.k[None, None, :]          # [slots, M, bins]
        a = torch.polar(torch.ones_like(phase), phase).to(torch.complex64)
        Y = torch.einsum("bmk,mkc->bkc", a, X)
        Q = (X.real * X.real + X.imag * X.imag).sum(dim=0)                                     # [bins, count]
        num = (Y.real * Y.real + Y.imag * Y.imag - Q[None]) / float(n * (n - 1))
        den = (Q / float(n))[None].expand_as(num)
        Ns, Ds, out = self.N, self.D, []
        for i in range(num.shape[2]):
            if not self.seen:
                Ns, Ds, self.seen = num[:, :, i], den[:, :, i], True
            else:
                Ns = num[:, :, i] + pf.beta * (Ns - num[:, :, i])
                Ds = den[:, :, i] + pf.beta * (Ds - den[:, :, i])
            ratio = (Ns.clamp(min=0.0) / Ds.clamp(min=1e-37)).clamp(pf.g_min, 1.0)
            out.append(torch.where(Ds > 0, ratio, torch.full_like(ratio, pf.g_min)))
        self.N.copy_(Ns)
        self.D.copy_(Ds)
        self.hist.copy_(buf[:, x.shape[1]:])
        return torch.stack(out, dim=1)


def stream_of(frames):
    """[F, M, N] -> [M, F * HOP]: the last HOP samples of every window."""
    return frames[:, :, N - HOP:].permute(1, 0, 2).reshape(frames.shape[1], -1).contiguous()


def one_shape(name, rounds):
    z = SHAPES[name]
    F, inner = z["frames"], z["inner"]
    c = util.configure("cfg2")
    M, D = c["M"], c["X"] * c["Y"]
    assert c["N"] == N
    table = util.table_for("lerp", "cfg2")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size)
    nat.check()
    mics = np.arange(M, dtype=np.int32)
    tau = np.asarray(util.oracle_delays("cfg2"), dtype=np.float64).reshape(D, M)
    dirs = [(7 * b + 3) * D // 31 for b in range(SLOTS)]
    frames = torch.from_numpy(synth.frame_batch(M, N, F)).cuda()
    row = torch.tensor([d * M for d in dirs], dtype=torch.int32, device="cuda")
    offs = row[None].expand(F, -1).contiguous()
    beams = torch.empty((F, SLOTS, N), dtype=torch.float32, device="cuda")
    status = torch.empty((F, SLOTS), dtype=torch.int32, device="cuda")

    def miso():
        return nat.lib.bf_miso_device(util.ALGOS["lerp"], frames.data_ptr(), M, F, nat.iptr(mics), M, offs.data_ptr(), SLOTS, 0.0, beams.data_ptr(), N,
                                      status.data_ptr(), torch.cuda.current_stream().cuda_stream)

    assert miso() == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    pf = postfilter.SpatialPostFilter(tau, mics, SLOTS, M, HOP, m_total=M, n_fft=N_FFT, hop_s=HOP_S)
    en = enhance.Enhancer(rows=SLOTS, hop=HOP, n_fft=N_FFT, hop_s=HOP_S)
    rec = {"windows": F, "microphones": M, "slots": SLOTS, "samples": F * HOP, "frames_per_call": F * HOP // HOP_S, "calls_per_graph": inner,
           "workspace_floats": int(nat.lib.bf_postfilter_workspace(SLOTS, F * HOP, N_FFT, HOP_S))}
    # the check: the same calls through both formulations from the start of a stream (noise of another seed every call)
    tp = TorchPostfilter(pf, dirs)
    worst, scale = 0.0, float(frames.abs().max())
    for k in range(z["checks"]):
        noisy = frames + 0.05 * scale * torch.randn(frames.shape, generator=torch.Generator(device="cpu").manual_seed(k)).cuda()
        g, count, st = pf.gains(noisy, row)
        want = tp.gains(stream_of(noisy))
        torch.cuda.synchronize()
        assert count.cpu().tolist() == [F * HOP // HOP_S, 0] and st.cpu().tolist() == [0] * SLOTS
        worst = max(worst, float((g - want).abs().max()))
    assert worst < 1e-3, (name, worst)
    rec["torch_max_abs_gain_diff"] = worst
    nat.check()

    g, _, _ = pf.gains(frames, row)
    flat = stream_of(frames)
    replays = {"postfilter": graph_of(lambda: pf.gains(frames, row), inner), "miso": graph_of(miso, inner),
               "enhance": graph_of(lambda: en.push(beams, gains=g), inner)}
    try:
        replays["torch"] = graph_of(lambda: tp.gains(flat), inner)
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
    p = statistics.median(t["postfilter"])
    rec["postfilter_over_miso"] = round(p / statistics.median(t["miso"]), 3)
    rec["postfilter_over_enhance"] = round(p / statistics.median(t["enhance"]), 3)
    if "torch" in t:
        rec["torch_over_postfilter"] = round(statistics.median(t["torch"]) / p, 2)
    return rec


def main(rounds, out):
    rec = {"device": torch.cuda.get_device_name(0), "rounds": rounds,
           "what": "n_fft 256, hop_s 128, root-Hann analysis window, beta 0.8, the microphones' denominator, 4 slots over 64 microphones, on the last 128 "
                   "samples of every 256-sample window",
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
        sys.exit("postfilter_time: at least five alternating rounds")
    if not torch.cuda.is_available() or not nat.gpu_available():
        sys.exit("postfilter_time: no usable HIP device; this measurement has no CPU fallback")
    main(args.rounds, args.out)
