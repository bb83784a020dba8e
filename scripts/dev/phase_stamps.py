#!/usr/bin/env python3
"""Dev tool: where the waves of the batched pad / lerp kernel spend their time.

  build (here or on the GPU box):  python3 scripts/dev/phase_stamps.py build [hipcc flags]   -> scripts/dev/bin/libbeamformer_hip_stamps.so
  run (GPU box):                   python3 scripts/dev/phase_stamps.py run [lerp|pad] [workload] [frames]

The profiling library is the production source compiled with -DBF_STAMPS: every wave of das_pair_kernel reads s_memtime at
its phase boundaries (all next to barriers) and the per-phase totals are summed over the launch.  Beside the totals the run prints
one row per wave index of the workgroup: the SIMDs it ran on (HW_ID; the first wave's SIMD differs from workgroup to workgroup),
in how many workgroups it shared the SIMD of wave (index & 3), its sweep and its wait for the staged chunk, each as a share of the
mean wave lifetime, and the waits of the waves w, w + 4, w + 8, w + 12 side by side -- whether the four waves of a SIMD finish a
half as a staircase.
$BF_STAMPS_LIB: another path for the profiling library (to keep two builds side by side)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.environ.get("BF_STAMPS_LIB") or os.path.join(ROOT, "scripts", "dev", "bin", "libbeamformer_hip_stamps.so")
sys.path.insert(0, ROOT)


def build():
    import __graft_entry__ as ge
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    srcs = [os.path.join(ge.CSRC, s) for s in ge.SOURCES]
    cmd = ["/opt/rocm/bin/hipcc"] + ge.HIPCC_FLAGS + ["-shared", "-DBF_STAMPS"] + sys.argv[2:] + srcs + ["-o", OUT]
    subprocess.check_call(cmd)
    print("built", OUT)


def run(algo="lerp", workload="cfg2", frames=190):
    os.environ["BF_NATIVE_LIB"] = OUT
    import ctypes as C
    import numpy as np
    import torch
    import bench
    sys.path.insert(0, bench.PKG)
    from interface import config
    from lib import _native as nat, directions
    import synth
    M, tiles, N, X, Y, T = bench.WORKLOADS[workload]
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=tiles, N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=T)
    delays = directions.calculate_delays()
    if algo == "pad":
        t = np.ascontiguousarray(delays.astype(int).astype(np.int32)).ravel()
        nat.lib.load_coefficients_pad(nat.iptr(t), t.size)
    else:
        t = np.ascontiguousarray(np.float32(delays)).ravel()
        nat.lib.load_coefficients_lerp(nat.fptr(t), t.size)
    nat.check()
    D = X * Y
    mics = np.arange(M, dtype=np.int32)
    sig = torch.from_numpy(synth.frame_batch(M, N, frames)).cuda()
    img = torch.empty((frames, D), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    go = lambda: nat.lib.bf_das_device(nat.ALGOS[algo] if hasattr(nat, "ALGOS") else {"pad": 0, "lerp": 1}[algo], sig.data_ptr(), M, img.data_ptr(), D, frames,
                                       nat.iptr(mics), M, 0, D, stream)
    for _ in range(3):
        assert go() == 0, nat.check()
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * 16)()
    assert nat.lib.bf_read_phase_stamps(buf, 1) == 0
    reps = 10
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        go()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    assert nat.lib.bf_read_phase_stamps(buf, 1) == 0
    v = [int(x) for x in buf]
    names = ["sweep", "wait (chunk free)", "staging", "wait (chunk staged)", "wait (rows free)", "parking", "wait (rows parked)", "ordered sum (+ its idle)"]
    tot = sum(v[:8])
    print("%s %s %d frames: %.4f ms per launch (%.0f frames/s), %d waves stamped per launch" % (algo, workload, frames, ms, frames / ms * 1e3, v[8] // reps))
    for n, x in zip(names, v[:8]):
        print("  %-26s %6.2f %%" % (n, 100.0 * x / max(tot, 1)))
    print("  mean wave lifetime %.1f ticks; ticks per ms of launch per wave slot: %.0f" % (tot / max(v[8], 1), tot / reps / ms / 4096.0))
    if getattr(nat.lib, "bf_read_wave_stamps", None) is None:
        return
    wbuf = (C.c_ulonglong * 128)()
    assert nat.lib.bf_read_wave_stamps(wbuf, 1) == 0
    rows = [[int(x) for x in wbuf[8 * w:8 * w + 8]] for w in range(16)]
    life = tot / max(v[8], 1)                 # every wave of a workgroup lives as long as the workgroup: the mean is each row's lifetime
    print("  per wave index (sweep and wait: shares of the mean wave lifetime; SIMD 0/1/2/3: where HW_ID placed it, by workgroups;")
    print("  with w & 3: the recorded workgroups in which it ran on the SIMD of wave (index & 3)):")
    print("  wave   on SIMD 0 / 1 / 2 / 3 (%)    with w & 3    sweep    wait (chunk staged)")
    waits = {}
    for w, r in enumerate(rows):
        n = sum(r[2:6])
        if n == 0:
            continue
        waits[w] = 100.0 * r[1] / n / life
        print("  %4d   %5.1f %5.1f %5.1f %5.1f       %6.1f %%     %6.2f %%   %6.2f %%" % (
            (w,) + tuple(100.0 * x / n for x in r[2:6]) + (100.0 * r[6] / max(r[7], 1), 100.0 * r[0] / n / life, waits[w])))
    if waits:
        mean = sum(waits.values()) / len(waits)
        print("  waits: mean %.2f %%, min %.2f %%, max %.2f %%, (max - min) / mean = %.2f  (%d workgroups of the last launch recorded)" % (
            mean, min(waits.values()), max(waits.values()), (max(waits.values()) - min(waits.values())) / mean, rows[0][7]))
    for q in range(4):
        ws = [w for w in range(q, 16, 4) if w in waits]
        print("  waves %s (oldest first): waits %s" % (", ".join("%d" % w for w in ws), ", ".join("%.2f %%" % waits[w] for w in ws)))

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
    else:
        a = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "run" else sys.argv[1:]
        run(a[0] if a else "lerp", a[1] if len(a) > 1 else "cfg2", int(a[2]) if len(a) > 2 else 190)
