"""Shared helpers for the parity tests (sizes, golden vectors, oracle tables)."""
import functools
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

from configs import CONFIGS  # oracle/configs.py (on sys.path via conftest)

REL_TOL = 1e-5   # BASELINE.json north_star: "within 1e-5 relative for float32 beam power"

ALGOS = {"pad": 0, "lerp": 1, "hybrid": 2, "fir_naive": 3, "fir_vec": 4}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


@functools.lru_cache(maxsize=None)
def oracle_delays(name):
    """float64 [X, Y, M] from the NumPy restatement (itself pinned by test_oracle_golden)."""
    import directions_np as D
    c = CONFIGS[name]
    return D.calculate_delays(c["X"], c["Y"], arrays=c["arrays"])


def inputs(name):
    """The S1/S2/S3 blocks of a size, regenerated from their definitions and checked against the golden hashes."""
    import synth
    c = CONFIGS[name]
    g = golden(name)
    d = oracle_delays(name)
    x0, y0 = [int(v) for v in g["s3_dir"]]
    out = {"s1": synth.s1_tone(c["M"], c["N"]), "s2": synth.s2_noise(c["M"], c["N"]), "s3": synth.s3_plane_wave(d[x0, y0], c["N"])}
    return out


def table_for(algo, name):
    """The table each reference wrapper loads (benchmark.pyx): int32 whole for pad, float32 delays for lerp/hybrid,
    get_h2 taps of the full delay for the two FIR flavours."""
    import directions_np as D
    d = oracle_delays(name)
    if algo == "pad":
        return D.whole_samples(d)
    if algo in ("lerp", "hybrid"):
        return np.float32(d)
    g = golden(name)
    if "taps_get_h2" in g.files:
        return g["taps_get_h2"]
    return D.compute_convolve_h(d, CONFIGS[name]["T"])


def max_rel(got, want):
    got = np.asarray(got, dtype=np.float64).ravel()
    want = np.asarray(want, dtype=np.float64).ravel()
    denom = np.maximum(np.abs(want), np.finfo(np.float32).tiny)
    return float(np.max(np.abs(got - want) / denom))


def bits_differ(got, want, nan_is_nan=False):
    """An empty string where float32 `got` equals `want` bit for bit; otherwise what to say: the first differing flat direction, both values
    as hex bits, the number of differing entries and the largest distance in float32 steps.  nan_is_nan: an entry that is NaN on
    both sides counts as equal whatever its payload (a NaN on one side only never does)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32).ravel(), np.ascontiguousarray(want, dtype=np.float32).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = g != w
    if nan_is_nan:
        bad &= ~(np.isnan(got) & np.isnan(want))
    if not bad.any():
        return ""
    # distance in steps: the bit patterns mapped to a line on which neighbouring floats are neighbouring integers
    line = lambda u: np.where(u >> 31 != 0, -(u & 0x7FFFFFFF).astype(np.int64), (u & 0x7FFFFFFF).astype(np.int64))
    d = int(np.flatnonzero(bad)[0])
    return "first differing flat direction %d: got 0x%08x (%r), want 0x%08x (%r); %d of %d entries differ, by at most %d float32 steps" % (
        d, g[d], float(got[d]), w[d], float(want[d]), int(bad.sum()), bad.size, int(np.abs(line(g[bad]) - line(w[bad])).max()))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = bits_differ(got, want)
    assert not diff, diff


def same_named(names, got, want, what):
    """Tuples of 4-byte arrays, one per name, equal in dtype, shape and every bit; an entry of `got` that is None is not compared."""
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert g.tobytes() == w.tobytes()


def wild(rng, shape):
    """Floats whose magnitudes spread over 2^-12 .. 2^12: a chain summed in another order rounds differently."""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-12, 13, size=shape))).astype(np.float32)


def stream_windows(rng, R, N, hop, F):
    """A stream cut into F windows of N every `hop` samples, and the window that began `hop` samples before the first."""
    step = hop if hop > 0 else N
    S = wild(rng, (R, step * F + N))
    frames = np.ascontiguousarray(np.stack([S[:, (f + 1) * step:(f + 1) * step + N] for f in range(F)]))
    return frames, np.ascontiguousarray(S[:, :N])


def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    return torch


def place(a, off):
    """A device copy of `a` that starts `off` floats past a 16-byte boundary (torch allocations are 256-byte aligned)."""
    torch = torch_gpu()
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    return buf, view


def place_words(a, off):
    """A device copy of `a`, in its own 4-byte dtype, that starts `off` words past a 16-byte boundary; the view keeps its buffer alive."""
    torch = torch_gpu()
    t = torch.from_numpy(np.ascontiguousarray(a).ravel())
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    view = buf[off:off + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off
    return view


CANARY = 64                 # elements in front of and behind every device output
CANARY_VALUE = -1234.5      # floats; the int outputs carry int(CANARY_VALUE) = -1234


def canaried(shape, dtype):
    """A device buffer of canaries and the view of `shape` elements in its middle that a kernel is to write."""
    torch = torch_gpu()
    total = int(np.prod(shape))
    buf = torch.full((CANARY + total + CANARY,), CANARY_VALUE if dtype.is_floating_point else int(CANARY_VALUE), dtype=dtype, device="cuda")
    return buf, buf[CANARY:CANARY + total]


def intact(buf, total):
    """Whether the canaries on both sides of canaried()'s view of `total` elements survived."""
    host = buf.cpu().numpy()
    want = host.dtype.type(CANARY_VALUE)
    return bool((host[:CANARY] == want).all() and (host[CANARY + total:] == want).all())


def audio_power(listener, out):
    import mvdr_np
    return mvdr_np.power(listener.audio(out).cpu().numpy()[0])


def configure_small(N):
    """The smallest sizes the row-wise kernels' tests need: 4 microphones, 2 x 1 directions, 8 taps and N samples."""
    from interface import config
    config.configure(N_MICROPHONES=4, N_SAMPLES=N, MAX_RES_X=2, MAX_RES_Y=1, N_TAPS=8)


def configure(name, **extra):
    """Switch the product package (interface.config + native library) to a size of oracle/configs.py."""
    from interface import config
    c = CONFIGS[name]
    kw = dict(N_MICROPHONES=c["M"], ACTIVE_TILES=c["arrays"], N_SAMPLES=c["N"], MAX_RES_X=c["X"], MAX_RES_Y=c["Y"], N_TAPS=c["T"])
    kw.update(extra)
    config.configure(**kw)
    return c
