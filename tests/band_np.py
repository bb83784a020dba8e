"""bf_band_filter_device's definition (include/beamformer_hip.h) restated in NumPy: over all outputs at once, with a Python loop
over the taps t = 0 .. T-1 in order, every step one single-rounding float32 fused multiply-add

    acc_{t+1} = fmaf(h[b][t], x~_f[r][j - t], acc_t),      acc_0 = 0.0f.

The fused step is a real fmaf: tests/band_fma.c (its loop over an array of outputs), compiled on first use with the host compiler
into a temporary directory, else libm's fmaf through ctypes, one call per output.  A float64 product-and-add rounded to float32 is
NOT this operation (it rounds twice) and is not used."""
import ctypes as C
import ctypes.util
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_step = None


def _load():
    global _step
    if _step is not None:
        return _step
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        so = os.path.join(tempfile.mkdtemp(prefix="band_fma_"), "band_fma.so")
        try:
            subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(_HERE, "band_fma.c"), "-o", so, "-lm"])
            fn = C.CDLL(so).band_fma_step
            fn.restype = None
            fn.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_long]

            def step(h, x, acc):
                x = np.ascontiguousarray(x, dtype=np.float32)
                assert acc.dtype == np.float32 and acc.flags.c_contiguous and x.shape == acc.shape
                fn(C.c_float(float(h)), x.ctypes.data_as(C.POINTER(C.c_float)), acc.ctypes.data_as(C.POINTER(C.c_float)), acc.size)
            _step = step
        except (OSError, subprocess.CalledProcessError):
            _step = None
    if _step is None:
        libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.fmaf.restype = C.c_float
        libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
        each = np.frompyfunc(libm.fmaf, 3, 1)

        def step(h, x, acc):
            acc[...] = each(np.float32(h), np.asarray(x, dtype=np.float32), acc).astype(np.float32)
        _step = step
    # the step must be fused: 1 + 2^-12 squared is 1 + 2^-11 + 2^-24; minus (1 + 2^-11) a fused step leaves 2^-24, a product rounded first leaves 0
    a = np.array([1.0 + 2.0 ** -12], dtype=np.float32)
    acc = np.array([-(1.0 + 2.0 ** -11)], dtype=np.float32)
    _step(a[0], a, acc)
    assert acc[0] == np.float32(2.0 ** -24), "fmaf is not fused here: %r" % acc[0]
    return _step


def extended(x, T, hop, prev=None):
    """x float32 [F, R, N] -> [F, R, T - 1 + N]: every row behind the T - 1 samples that precede it (x~ of the definition)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    F, R, N = x.shape
    ext = np.zeros((F, R, T - 1 + N), dtype=np.float32)
    ext[:, :, T - 1:] = x
    if hop > 0 and T > 1:
        assert T - 1 <= hop <= N
        for f in range(F):
            src = x[f - 1] if f > 0 else prev
            if src is not None:
                ext[f, :, :T - 1] = np.asarray(src, dtype=np.float32)[:, hop - (T - 1):hop]
    return ext


def band_filter(x, taps, hop=0, prev=None):
    """x float32 [F, R, N], taps float32 [K, T], hop (0: independent windows), prev float32 [R, N] or None -> float32 [K, F, R, N]."""
    step = _load()
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    K, T = taps.shape
    F, R, N = np.shape(x)
    ext = extended(x, T, hop, prev)
    out = np.zeros((K, F, R, N), dtype=np.float32)
    for b in range(K):
        acc = out[b]
        for t in range(T):                      # in this order: the chain of every output
            step(taps[b, t], ext[:, :, T - 1 - t:T - 1 - t + N], acc)
    return out
