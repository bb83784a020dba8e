"""GPU (-m gpu): the C-ABI's refusals that sit AFTER device bring-up -- return code, the exact bf_last_error text and, on the
host-pointer calls, the all-NaN output.  None of them launches a kernel: the device sees table and adaptive-array uploads only.

Sizes: 16 microphones, 64 samples, 5 x 5 directions, 8 taps; torch tensors serve as device pointers."""
import ctypes as C

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

M, N, X, Y, T = 16, 64, 5, 5, 8
D = X * Y
MICS = np.arange(M, dtype=np.int32)


class Ctx:
    def __init__(self, nat):
        import torch
        assert torch.cuda.is_available()
        self.nat, self.lib = nat, nat.lib
        rng = np.random.default_rng(11)
        self.whole = rng.integers(0, 11, size=D * M).astype(np.int32)
        self.delays = (rng.random(D * M) * 10).astype(np.float32)
        self.taps = rng.standard_normal(D * M * T).astype(np.float32)
        self.sig = torch.zeros((1, M, N), dtype=torch.float32, device="cuda")
        self.img = torch.zeros((1, D), dtype=torch.float32, device="cuda")
        self.out = torch.zeros((1, 1, N), dtype=torch.float32, device="cuda")
        self.residual = torch.zeros((1, M, N), dtype=torch.float32, device="cuda")
        self.offsets = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
        self.big = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")       # stands in wherever a call is refused on its sizes alone
        torch.cuda.synchronize()

    def load(self, *names):
        lib, nat = self.lib, self.nat
        for unload in (lib.unload_coefficients_pad, lib.unload_coefficients_lerp, lib.unload_coefficients_convolve, lib.unload_coefficients_convolve_hybrid):
            unload()
        if "pad" in names:
            lib.load_coefficients_pad(nat.iptr(self.whole), self.whole.size)
        if "lerp" in names:
            lib.load_coefficients_lerp(nat.fptr(self.delays), self.delays.size)
        if "fir" in names:
            lib.load_coefficients_convolve(nat.fptr(self.taps), self.taps.size)
        nat.check()

    def refused(self, rc, text, want_rc=-1):
        assert rc == want_rc
        got = self.lib.bf_last_error().decode()
        self.lib.bf_clear_error()
        assert got == text

    def das(self, algo=0, m_total=M, image_stride=D, frames=1, mics=MICS, n=None, dir_begin=0, dir_end=D):
        mics = np.ascontiguousarray(mics, dtype=np.int32)
        return self.lib.bf_das_device(algo, self.sig.data_ptr(), m_total, self.img.data_ptr(), image_stride, frames, self.nat.iptr(mics),
                                      mics.size if n is None else n, dir_begin, dir_end, None)


@pytest.fixture(scope="module")
def ctx(native):
    assert native.gpu_available(), "these tests need the MI355X"
    assert native.lib.bf_configure(M, 32, X, Y, T) == 0 and native.lib.bf_configure(M, N, X, Y, T) == 0   # (a change of N_SAMPLES drops every table)
    native.lib.bf_clear_error()
    yield Ctx(native)
    native.lib.bf_clear_error()
    util.configure("cfg1")


@pytest.mark.parametrize("kw,text", [
    (dict(dir_begin=-1), "bf_das_device: bad direction range [-1,25) of 25"),
    (dict(dir_end=26), "bf_das_device: bad direction range [0,26) of 25"),
    (dict(dir_begin=7, dir_end=7), "bf_das_device: bad direction range [7,7) of 25"),
    (dict(dir_begin=9, dir_end=2, image_stride=0), "bf_das_device: bad direction range [9,2) of 25"),
    (dict(image_stride=24), "bf_das_device: image_stride 24 < 25 directions"),
    (dict(dir_begin=3, dir_end=10, image_stride=6), "bf_das_device: image_stride 6 < 7 directions"),
    (dict(mics=list(range(15)) + [16]), "bf_das_device: adaptive_array names row 16 but frames have 16 rows"),
    (dict(mics=list(range(15)) + [16], dir_begin=-1), "bf_das_device: adaptive_array names row 16 but frames have 16 rows"),
    (dict(mics=[0, 1, 2, -2] + list(range(4, 16))), "adaptive_array[3] = -2 is negative"),
    (dict(mics=[-1] * 16, m_total=0), "adaptive_array[0] = -1 is negative"),
    (dict(mics=MICS[:8]), "load_coefficients_pad loaded 400 coefficients but MAX_RES_X*MAX_RES_Y*n = 5*5*8 = 200"),
    (dict(mics=MICS[:8], dir_end=26), "load_coefficients_pad loaded 400 coefficients but MAX_RES_X*MAX_RES_Y*n = 5*5*8 = 200"),
    (dict(algo=4, mics=MICS[:8]), "load_coefficients_convolve loaded 3200 coefficients but MAX_RES_X*MAX_RES_Y*n*N_TAPS = 5*5*8*T = 1600"),
    (dict(algo=3, mics=MICS[:3]), "load_coefficients_convolve loaded 3200 coefficients but MAX_RES_X*MAX_RES_Y*n*N_TAPS = 5*5*3*T = 600"),
    (dict(algo=1), "load_coefficients_lerp has not been called"),
    (dict(algo=2, dir_begin=-1), "load_coefficients_convolve_hybrid has not been called"),
])
def test_das_device(ctx, kw, text):
    ctx.load("pad", "fir")
    ctx.refused(ctx.das(**kw), text)


def test_das_device_table_unloaded(ctx):
    ctx.load()
    ctx.refused(ctx.das(), "load_coefficients_pad has not been called")
    ctx.refused(ctx.das(algo=4), "load_coefficients_convolve has not been called")


def test_miso_host_offset_past_the_table(ctx):
    nat, lib = ctx.nat, ctx.lib
    ctx.load("pad", "fir")
    sig = np.zeros(M * N, dtype=np.float32)
    for fn, offset, text in ((lib.miso_pad, D * M - M + 1, "offset 385 + n 16 exceeds the 400 loaded coefficients"),
                             (lib.miso_pad, -1, "offset -1 + n 16 exceeds the 400 loaded coefficients"),
                             (lib.miso_convolve_vectorized, (D * M - M + 1) * T, "offset 385 + n 16 exceeds the 3200 loaded coefficients"),
                             (lib.miso_lerp, 0, "load_coefficients_lerp has not been called"),
                             (lib.miso_convolve_hybrid, 0, "load_coefficients_convolve_hybrid has not been called")):
        out = np.zeros(N, dtype=np.float32)
        ctx.refused(fn(nat.fptr(sig), nat.fptr(out), nat.iptr(MICS), M, offset), text, None)
        assert np.isnan(out).all(), text
    bad = MICS.copy()
    bad[5] = -3
    out = np.zeros(N, dtype=np.float32)
    ctx.refused(lib.miso_pad(nat.fptr(sig), nat.fptr(out), nat.iptr(bad), M, 0), "adaptive_array[5] = -3 is negative", None)
    assert np.isnan(out).all()
    image = np.zeros(D, dtype=np.float32)
    ctx.refused(lib.mimo_lerp(nat.fptr(sig), nat.fptr(image), nat.iptr(MICS), M), "load_coefficients_lerp has not been called", None)
    assert np.isnan(image).all()
    out = np.zeros(N, dtype=np.float32)
    ctx.refused(lib.pad_delay(nat.fptr(sig), nat.fptr(out), -2), "negative delay -2", None)
    assert np.isnan(out).all()


def test_device_beams_with_the_table_unloaded(ctx):
    nat, lib = ctx.nat, ctx.lib
    ctx.load("fir")
    p = lambda t: t.data_ptr()
    gain = C.c_float(1.0)
    ctx.refused(lib.bf_miso_device(0, p(ctx.sig), M, 1, nat.iptr(MICS), M, p(ctx.offsets), 1, gain, p(ctx.out), N, None, None),
                "bf_miso_device: load_coefficients_pad has not been called")
    ctx.refused(lib.bf_miso_device(2, p(ctx.sig), M, 1, nat.iptr(MICS), M, p(ctx.offsets), 1, gain, p(ctx.out), N, None, None),
                "bf_miso_device: load_coefficients_convolve_hybrid has not been called")
    ctx.refused(lib.bf_remove_sources_device(1, p(ctx.sig), M, 1, nat.iptr(MICS), M, p(ctx.offsets), 1, p(ctx.out), N, gain, p(ctx.residual), None, None),
                "bf_remove_sources_device: load_coefficients_lerp has not been called")
    ctx.refused(lib.bf_remove_sources_device(0, p(ctx.sig), M, 1, nat.iptr(MICS), M, p(ctx.offsets), 1, p(ctx.out), N, gain, p(ctx.residual), None, None),
                "bf_remove_sources_device: load_coefficients_pad has not been called")
    ctx.refused(lib.bf_miso_stream_device(0, p(ctx.sig), M, 1, N, None, nat.iptr(MICS), M, p(ctx.offsets), 1, gain, p(ctx.out), N, None, None),
                "bf_miso_stream_device: load_coefficients_pad has not been called")
    ctx.refused(lib.bf_das_stream_device(1, p(ctx.sig), M, p(ctx.img), D, 1, N, None, nat.iptr(MICS), M, 0, D, None),
                "bf_das_stream_device: load_coefficients_lerp has not been called")


def test_frequency_domain_and_nms_limits(ctx):
    nat, lib = ctx.nat, ctx.lib
    b = ctx.big.data_ptr()
    ctx.refused(lib.bf_fd_dft_device(b, M, 1, nat.iptr(MICS), M, 30, 4, b, b, b, b, None), "bf_fd_dft_device: bins [30,34) exceed N_SAMPLES/2+1 = 33")
    ctx.refused(lib.bf_fd_dft_device(b, M, 1, nat.iptr(MICS), M, 33, 1, b, b, b, b, None), "bf_fd_dft_device: bins [33,34) exceed N_SAMPLES/2+1 = 33")
    bad = MICS.copy()
    bad[15] = 16
    ctx.refused(lib.bf_fd_dft_device(b, M, 1, nat.iptr(bad), M, 0, 4, b, b, b, b, None), "bf_fd_dft_device: adaptive_array names row 16 but frames have 16 rows")
    ctx.refused(lib.bf_fd_cholesky_inverse_device(b, b, 257, 1, C.c_float(1e-3), b, b, b, None),
                "bf_fd_cholesky_inverse_device: 257 mics; the blocked factorisation handles at most 256")
    ctx.refused(lib.bf_fd_mvdr_power_device(b, b, b, b, 257, D, 1, b, None), "bf_fd_mvdr_power_device: 257 mics; at most 256")
    ctx.refused(lib.bf_nms_device(b, b, b, b, 1, 4097, C.c_float(0.45), 300, b, b, b, None), "bf_nms_device: k = 4097 candidates; at most 4096")
