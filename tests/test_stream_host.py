"""CPU: the host-side contract of the continuous-stream calls (bf_stream_history, bf_miso_stream_device, bf_das_stream_device,
bf_get_pad_table), StreamBeamformer's argument checks and the gfx950 resources of das_miso_kernel / das_mimo_kernel with HIST.

Every argument is checked before device bring-up, so the refusals run without a GPU.  One refusal is not here: `H > hop` (and the
clamped-table refusal) needs a loaded table, and a table can only be loaded onto a device -- tests/test_stream.py has both."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import util
from support import FAKE, nat_cfg1 as nat, refused

N = 256


def _miso(nat, **kw):
    a = dict(algo=nat.PAD, d_signals=FAKE, m_total=8, frames=2, hop=N, d_prev=None, adaptive_array=np.arange(4, dtype=np.int32), n=4, d_offsets=FAKE,
             beams=3, mic_gain=0.0, d_out=FAKE, out_stride=N, d_status=FAKE)
    a.update(kw)
    mics = a["adaptive_array"]
    return nat.lib.bf_miso_stream_device(a["algo"], a["d_signals"], a["m_total"], a["frames"], a["hop"], a["d_prev"], None if mics is None else nat.iptr(mics),
                                         a["n"], a["d_offsets"], a["beams"], a["mic_gain"], a["d_out"], a["out_stride"], a["d_status"], None)


def _das(nat, **kw):
    a = dict(algo=nat.LERP, d_signals=FAKE, m_total=8, d_images=FAKE, image_stride=121, frames=2, hop=N, d_prev=FAKE,
             adaptive_array=np.arange(4, dtype=np.int32), n=4, dir_begin=0, dir_end=121)
    a.update(kw)
    mics = a["adaptive_array"]
    return nat.lib.bf_das_stream_device(a["algo"], a["d_signals"], a["m_total"], a["d_images"], a["image_stride"], a["frames"], a["hop"], a["d_prev"],
                                        None if mics is None else nat.iptr(mics), a["n"], a["dir_begin"], a["dir_end"], None)


def test_new_symbols_exist(native):
    for name in ("bf_stream_history", "bf_miso_stream_device", "bf_das_stream_device", "bf_get_pad_table"):
        assert getattr(native.lib, name, None) is not None, name


CAUSAL = "reads ahead of the window's end, which a causal stream cannot supply"
COMMON = [
    (dict(algo=2), "algo BF_HYBRID " + CAUSAL),
    (dict(algo=3), "algo BF_FIR_NAIVE " + CAUSAL),
    (dict(algo=4), "algo BF_FIR_VEC " + CAUSAL),
    (dict(algo=7), "unknown algo 7"),
    (dict(algo=-1), "unknown algo -1"),
    (dict(d_signals=None), "d_signals is null"),
    (dict(adaptive_array=None), "adaptive_array is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(hop=0), "hop = 0 < 1"),
    (dict(hop=-128), "hop = -128 < 1"),
    (dict(hop=N + 1), "hop = 257 > N_SAMPLES = 256"),
    (dict(n=0), "n = 0 < 1"),
    (dict(adaptive_array=np.array([0, 1, 8, 2], dtype=np.int32)), r"adaptive_array\[2\] = 8 is not a row of frames with m_total = 8"),
    (dict(adaptive_array=np.array([0, -1, 2, 3], dtype=np.int32)), r"adaptive_array\[1\] = -1"),
]


@pytest.mark.parametrize("kw,match", COMMON + [
    (dict(d_offsets=None), "d_offsets is null"),
    (dict(d_out=None), "d_out is null"),
    (dict(beams=0), "beams = 0 < 1"),
    (dict(out_stride=N - 1), "out_stride = 255 < N_SAMPLES = 256"),
    (dict(mic_gain=math.inf), "mic_gain = inf is not finite"),
    (dict(mic_gain=math.nan), "mic_gain = -?nan is not finite"),
])
def test_miso_stream_argument_errors(nat, kw, match):
    refused(nat, _miso(nat, **kw), "bf_miso_stream_device: " + match)


@pytest.mark.parametrize("kw,match", COMMON + [
    (dict(d_images=None), "d_images is null"),
    (dict(dir_begin=-1), r"bad direction range \[-1,121\) of 121"),
    (dict(dir_end=122), r"bad direction range \[0,122\) of 121"),
    (dict(dir_begin=7, dir_end=7), r"bad direction range \[7,7\) of 121"),
    (dict(image_stride=120), "image_stride 120 < 121 directions"),
])
def test_das_stream_argument_errors(nat, kw, match):
    refused(nat, _das(nat, **kw), "bf_das_stream_device: " + match)


def test_history_of_nothing_loaded(nat):
    nat.lib.unload_coefficients_pad()
    nat.lib.unload_coefficients_lerp()
    for algo in range(-1, 6):
        assert nat.lib.bf_stream_history(algo) == -1
    nat.check()                            # a query, not a failure: no error recorded
    one = np.zeros(1, dtype=np.int32)
    refused(nat, nat.lib.bf_get_pad_table(nat.iptr(one), 1), "bf_get_pad_table: 1 requested, 0 loaded")
    refused(nat, nat.lib.bf_get_pad_table(None, 1), "bf_get_pad_table: whole is null")


def test_valid_arguments_without_gpu(nat):
    if nat.gpu_available():
        pytest.skip("without a GPU only")
    refused(nat, _miso(nat), "no usable HIP device")
    refused(nat, _miso(nat, algo=nat.LERP, hop=1, d_prev=FAKE, d_status=None, mic_gain=128.0), "no usable HIP device")
    refused(nat, _das(nat), "no usable HIP device")
    refused(nat, _das(nat, algo=nat.PAD, hop=N // 2, d_prev=None, dir_begin=100, dir_end=121, image_stride=21), "no usable HIP device")


def test_stream_beamformer_arguments(nat):
    import stream
    for algo in ("hybrid", "fir_naive", "fir_vec", "miso_pad2"):
        with pytest.raises(ValueError, match="causal stream"):
            stream.StreamBeamformer(algo)
    for hop in (0, -1, N + 1):
        with pytest.raises(ValueError, match=r"hop must be in \[1, N_SAMPLES = 256\]"):
            stream.StreamBeamformer("pad", hop=hop, mics=[0, 1])
    sb = stream.StreamBeamformer("lerp", mics=[0, 1, 2])
    assert sb.hop == N and sb.n == 3 and sb.offset_per_dir == 3
    assert stream.StreamBeamformer("pad", hop=100, mics=np.arange(5)).hop == 100
    nat.lib.unload_coefficients_lerp()
    with pytest.raises(nat.BeamformerError, match="the lerp table is not loaded"):
        sb.history
    import torch
    with pytest.raises(ValueError, match=r"out must be \[F, B, 256\]"):
        sb.audio(torch.zeros((2, 3, 255)))
    # audio(): the last `hop` samples of every window, joined per beam
    half = stream.StreamBeamformer("pad", hop=N // 2, mics=[0])
    out = torch.arange(3 * 2 * N, dtype=torch.float32).reshape(3, 2, N)
    a = half.audio(out)
    assert a.shape == (2, 3 * N // 2)
    assert torch.equal(a[1], torch.cat([out[f, 1, N // 2:] for f in range(3)]))
    if not nat.gpu_available():
        for call in (lambda: sb.listen(torch.zeros((1, 3, N)), [0]), lambda: sb.maps(torch.zeros((1, 3, N))), lambda: sb.advance(torch.zeros((1, 3, N)))):
            with pytest.raises((nat.BeamformerError, ValueError)):
                call()


# ------------------------------------------------------------------ gfx950 resources of the two new kernels

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("check_inflight_copies", os.path.join(util.ROOT, "scripts", "dev", "check_inflight_copies.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    path = str(tmp_path_factory.mktemp("stream_isa") / "das_strided.s")
    chk.compile_asm(path, units=["das_strided.hip"])
    return chk, path


def test_stream_kernels_fit_sixteen_waves_without_scratch(asm):
    """das_miso_kernel<ALGO, NC, true> and das_mimo_kernel<ALGO, NC, DPW, true> (HIST: the continuous-stream mode), pad and lerp only,
    NC 1, 2, 4, 8, 16 (maps: DPW 1 and 4): compiled with the build's flags, no scratch, no spills, at most 128 VGPRs, and a 1024-thread
    workgroup allowed."""
    chk, path = asm
    md = chk.metadata(path)
    text = open(path).read()
    wg = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        size = re.search(r"\.max_flat_workgroup_size:\s+(\d+)", blk)
        if name and size:
            wg[name.group(1)] = int(size.group(1))
    names = list(md)
    short = dict(zip(chk.demangle(names), names))
    want = ["bf::das_miso_kernel<%d, %d, true>" % (a, nc) for a in (0, 1) for nc in (1, 2, 4, 8, 16)]
    want += ["bf::das_mimo_kernel<%d, %d, %d, true>" % (a, nc, dpw) for a in (0, 1) for nc in (1, 2, 4, 8, 16) for dpw in (1, 4)]
    hist = [n for n in short if re.match(r"bf::das_mi[sm]o_kernel<.*, true>$", n)]
    assert sorted(hist) == sorted(want)                 # the exact list: no other instantiation with history exists
    for w in want:
        m = md[short[w]]
        assert m["spill"] == 0 and m["scratch"] == 0, (w, m)
        assert m["vgprs"] <= 128, (w, m)
        assert wg[short[w]] >= 1024, (w, wg[short[w]])
