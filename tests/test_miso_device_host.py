"""CPU: the host-side contract of bf_miso_device / bf_peak_offsets_device (every argument is checked before device bring-up,
so these run without a GPU) and the gfx950 resources of every das_miso_kernel instantiation."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import util
from support import entry, FAKE, refused


def _miso(nat, **kw):
    a = dict(algo=nat.PAD, d_signals=FAKE, m_total=8, frames=2, adaptive_array=np.arange(4, dtype=np.int32), n=4, d_offsets=FAKE, beams=3,
             mic_gain=0.0, d_out=FAKE, out_stride=None, d_status=FAKE)
    a.update(kw)
    stride = _n_samples(nat) if a["out_stride"] is None else a["out_stride"]
    mics = a["adaptive_array"]
    return nat.lib.bf_miso_device(a["algo"], a["d_signals"], a["m_total"], a["frames"], None if mics is None else nat.iptr(mics), a["n"], a["d_offsets"],
                                  a["beams"], a["mic_gain"], a["d_out"], stride, a["d_status"], None)


_peak = entry("bf_peak_offsets_device", d_power=FAKE, frames=2, image_stride=10, n_dirs=10, offset_per_dir=4, d_offsets=FAKE)


def _n_samples(nat):
    cfg = (C.c_int * 5)()
    nat.lib.bf_get_config(cfg)
    return cfg[1]


@pytest.mark.parametrize("kw,match", [
    (dict(algo=3), "BF_FIR_NAIVE has no MISO form"),
    (dict(algo=7), "unknown algo 7"),
    (dict(algo=-1), "unknown algo -1"),
    (dict(d_signals=None), "d_signals is null"),
    (dict(adaptive_array=None), "adaptive_array is null"),
    (dict(d_offsets=None), "d_offsets is null"),
    (dict(d_out=None), "d_out is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(beams=0), "beams = 0 < 1"),
    (dict(beams=-3), "beams = -3 < 1"),
    (dict(adaptive_array=np.array([0, 1, 8, 2], dtype=np.int32)), r"adaptive_array\[2\] = 8 is not a row of frames with m_total = 8"),
    (dict(adaptive_array=np.array([0, -1, 2, 3], dtype=np.int32)), r"adaptive_array\[1\] = -1"),
    (dict(mic_gain=math.inf), "mic_gain = inf is not finite"),
    (dict(mic_gain=-math.inf), "mic_gain = -inf is not finite"),
    (dict(mic_gain=math.nan), "mic_gain = -?nan is not finite"),
])
def test_miso_device_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _miso(native, **kw), match)


def test_miso_device_out_stride_and_n(native):
    N = _n_samples(native)
    refused(native, _miso(native, out_stride=N - 1), "out_stride = %d < N_SAMPLES = %d" % (N - 1, N))
    refused(native, _miso(native, n=0), "n = 0 < 1")


@pytest.mark.parametrize("kw,match", [
    (dict(d_power=None), "d_power is null"),
    (dict(d_offsets=None), "d_offsets is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(n_dirs=0), "n_dirs = 0 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(image_stride=9), "image_stride = 9 < n_dirs = 10"),
    (dict(n_dirs=3, image_stride=3, offset_per_dir=2 ** 30), r"\(n_dirs - 1\) \* offset_per_dir = 2147483648 does not fit"),
])
def test_peak_offsets_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _peak(native, **kw), match)


def test_peak_offsets_largest_offset_that_fits_passes_the_checks(native):
    """(n_dirs - 1) * offset_per_dir == INT_MAX is accepted by the argument checks (and then needs a device)."""
    if native.gpu_available():
        pytest.skip("without a GPU only: with one, valid arguments would enqueue")
    refused(native, _peak(native, n_dirs=2, image_stride=2, offset_per_dir=2 ** 31 - 1), "no usable HIP device")


def test_valid_arguments_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only")
    refused(native, _miso(native), "no usable HIP device")
    refused(native, _miso(native, algo=native.FIR_VEC, d_status=None, mic_gain=128.0), "no usable HIP device")
    refused(native, _peak(native), "no usable HIP device")


def test_beam_listener_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only")
    import torch
    import listen
    bl = listen.BeamListener("pad", mics=[0, 1, 2])
    assert bl.n == 3 and bl.offset_per_dir == 3
    with pytest.raises(native.BeamformerError, match="no usable HIP device"):
        bl.listen(torch.zeros((1, 3, 8)), [0])
    with pytest.raises(native.BeamformerError, match="no usable HIP device"):
        bl.loudest(torch.zeros((1, 4)))


def test_beam_listener_offsets_per_direction(native):
    import listen
    from interface import config
    assert listen.BeamListener("fir_vec", mics=np.arange(5)).offset_per_dir == 5 * config.N_TAPS
    assert listen.BeamListener("lerp", mics=np.arange(5)).offset_per_dir == 5
    with pytest.raises(ValueError):
        listen.BeamListener("miso_pad2")


# ------------------------------------------------------------------ gfx950 resources of the generalised kernel

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("check_inflight_copies", os.path.join(util.ROOT, "scripts", "dev", "check_inflight_copies.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    path = str(tmp_path_factory.mktemp("miso_isa") / "das_strided.s")
    chk.compile_asm(path, units=["das_strided.hip"])
    return chk, path


def test_every_miso_instantiation_fits_sixteen_waves_without_scratch(asm):
    """das_miso_kernel<ALGO, NC, HIST>, 5 algorithms x NC 1, 2, 4, 8, 16 without history and pad / lerp x NC with it (25 + 10, and no
    other): compiled, no scratch, a 1024-thread workgroup allowed and at most 128 VGPRs (16 waves of one workgroup share the CU's four
    SIMDs: four waves per SIMD)."""
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
    want = ["bf::das_miso_kernel<%d, %d, false>" % (a, nc) for a in range(5) for nc in (1, 2, 4, 8, 16)]
    want += ["bf::das_miso_kernel<%d, %d, true>" % (a, nc) for a in (0, 1) for nc in (1, 2, 4, 8, 16)]
    assert sorted(n for n in short if n.startswith("bf::das_miso_kernel<")) == sorted(want)
    for w in want:
        m = md[short[w]]
        assert m["spill"] == 0 and m["scratch"] == 0, (w, m)
        assert m["vgprs"] <= 128, (w, m)
        assert wg[short[w]] >= 1024, (w, wg[short[w]])
