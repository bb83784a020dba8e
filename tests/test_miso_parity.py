"""GPU (-m gpu): the one-direction path, bit for bit against the oracle.

Every miso_* entry point and every single-signal helper (pad_delay, lerp_delay, convolve_*_delay*) runs
das_miso_kernel<ALGO, NC> (csrc/das_strided.hip), NC in {1, 2, 4, 8, 16} by N, with the microphones staged through LDS in
one or several chunks.  The oracle (oracle/das_oracle.c) is pinned to the compiled reference by test_oracle_golden.py, and
the kernels keep the reference's microphone order and operation order, so the raw blocks must be BIT-IDENTICAL.

Every output buffer carries 16 NaN floats past its N samples: the call must write all N and none of the 16.
test_host_side.py::test_miso_cases_reach_every_kernel_instantiation checks, without a GPU, that MISO_CASES reaches every
NC and chunked staging for every algorithm."""
import ctypes as C

import numpy as np
import pytest

from support import nat

pytestmark = pytest.mark.gpu

SENTINEL = 16
MISO_ALGOS = ["pad", "lerp", "hybrid", "convolve_vectorized", "pad2"]

MISO_CASES = [
    # M_total n_active    N   T  dirs   pmax  edges   what it exercises
    (8,     5,   37,  8,  3,   30.0, True),    # NC 1; N not a multiple of 4 (scalar staging loads); delays 0, N - 1, past N
    (16,   16,   64, 16,  3,   12.0, False),   # NC 1; identity list, 16 taps
    (12,    9,  100,  8,  4,   99.0, True),    # NC 2; permuted subset, N not a multiple of 64
    (64,   64,  128, 16,  3,   20.0, False),   # NC 2; all mics, 16 taps
    (24,   20,  200,  8,  3,  150.0, True),    # NC 4; partial last segment
    (80,   70,  256,  8,  5,   47.0, False),   # NC 4; pad / lerp plans stage 32 mics at a time: three chunks
    (32,   27,  450, 16,  3,  300.0, True),    # NC 8; 16 taps, large delays
    (40,   33,  512,  8,  3,   60.0, False),   # NC 8; several chunks for pad / lerp (long rows)
    (16,   13, 1000,  8,  3,  999.0, True),    # NC 16; N not a multiple of 64, delays up to the block length
    (320, 300, 1024,  8,  3,  100.0, False),   # NC 16; 300 mics: many chunks for every algorithm
    (40,   33, 1024, 16,  3, 1100.0, True),    # NC 16; delays past the block lengthen every row: chunks of a few mics
]


def case_id(c):
    return "M%d_n%d_N%d_T%d_D%d_p%g%s" % (c[:6] + ("_edges" if c[6] else "",))


def case_tables(case):
    """Seeded inputs of one case: signals [M_total, N], the microphone list, delays [D, n] (float64), FIR taps [D, n, T] and the
    pad2 table [M_total] (by microphone id).  With `edges`, every direction has delays 0, N - 1 + 0.25, N + 5.5 and 7 (a lerp
    weight of exactly 1) on its first four mics, and the pad2 table the same on the list's first four mics."""
    M_total, n, N, T, D, pmax, edges = case
    rng = np.random.default_rng(list(case[:5]))
    sig = (rng.standard_normal((M_total, N)) * 0.25).astype(np.float32)
    mics = (np.arange(M_total) if n == M_total else rng.choice(M_total, n, replace=False)).astype(np.int32)
    delays = rng.uniform(0, pmax, size=(D, n))
    taps = rng.uniform(-0.5, 0.5, size=(D, n, T)).astype(np.float32)
    by_mic = np.floor(rng.uniform(0, pmax, size=M_total)).astype(np.int32)
    if edges:
        special = [0.0, N - 1 + 0.25, N + 5.5, 7.0]
        delays[:, :4] = special
        by_mic[mics[:4]] = np.floor(special).astype(np.int32)
    return sig, mics, delays, taps, by_mic


def miso_max_whole(algo, case):
    """The largest whole-sample delay the product's loader keeps for `algo` (values past N are clamped to N), i.e. what
    run_miso_host plans with (plain FIRs: none)."""
    N = case[2]
    _, mics, delays, _, by_mic = case_tables(case)
    if algo == "convolve_vectorized":
        return 0
    whole = by_mic[mics] if algo == "pad2" else np.floor(np.float32(delays)).astype(np.int64)
    return int(min(whole.max(), N))


def _configure(case):
    from interface import config
    M_total, n, N, T, D = case[:5]
    config.configure(N_MICROPHONES=M_total, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=T)


def _buffer(n, head=None):
    buf = np.full(n + SENTINEL, np.nan, dtype=np.float32)
    if head is not None:
        buf[:n] = head
    return buf


def _assert_written(buf, want, n):
    """All n samples written, bit for bit; the 16-float tail still NaN."""
    assert buf[:n].tobytes() == want.tobytes(), np.flatnonzero(buf[:n].view(np.int32) != want.view(np.int32))[:8]
    assert buf[n:].tobytes() == np.full(SENTINEL, np.nan, dtype=np.float32).tobytes()


# ------------------------------------------------------------------ miso_*: every NC, one and several chunks

@pytest.mark.parametrize("case", MISO_CASES, ids=case_id)
@pytest.mark.parametrize("algo", MISO_ALGOS)
def test_miso_matches_oracle(nat, oracle_lib, algo, case):
    M_total, n, N, T, D, pmax, edges = case
    sig, mics, delays, taps, by_mic = case_tables(case)
    _configure(case)
    orc = oracle_lib.Oracle(N, D, 1, T)
    d32 = np.ascontiguousarray(np.float32(delays)).ravel()
    whole = np.floor(d32).astype(np.int32)
    h = np.ascontiguousarray(taps).ravel()
    if algo == "pad":
        nat.lib.load_coefficients_pad(nat.iptr(whole), whole.size)
    elif algo == "lerp":
        nat.lib.load_coefficients_lerp(nat.fptr(d32), d32.size)
    elif algo == "hybrid":
        nat.lib.load_coefficients_convolve_hybrid(nat.fptr(d32), d32.size)
    elif algo == "convolve_vectorized":
        nat.lib.load_coefficients_convolve(nat.fptr(h), h.size)
    else:
        nat.lib.load_coefficients_pad2(nat.iptr(by_mic), by_mic.size)
    nat.check()
    for d in sorted({0, D // 2, D - 1}):
        off = d * n * (T if algo == "convolve_vectorized" else 1)
        buf = _buffer(N)
        if algo == "pad":
            nat.lib.miso_pad(nat.fptr(sig), nat.fptr(buf), nat.iptr(mics), n, off)
            want = orc.miso_pad(sig, whole, mics, off)
        elif algo == "lerp":
            nat.lib.miso_lerp(nat.fptr(sig), nat.fptr(buf), nat.iptr(mics), n, off)
            want = orc.miso_lerp(sig, d32, mics, off)
        elif algo == "hybrid":
            nat.lib.miso_convolve_hybrid(nat.fptr(sig), nat.fptr(buf), nat.iptr(mics), n, off)
            want = orc.miso_hybrid(sig, d32, mics, off)
        elif algo == "convolve_vectorized":
            nat.lib.miso_convolve_vectorized(nat.fptr(sig), nat.fptr(buf), nat.iptr(mics), n, off)
            want = orc.miso_convolve_vectorized(sig, h, mics, off)
        else:
            nat.lib.miso_pad2(nat.fptr(sig), nat.fptr(buf), nat.iptr(mics), n, off)
            want = orc.miso_pad2(sig, by_mic, mics, off)
        nat.check()
        assert np.isfinite(want).all()
        _assert_written(buf, want, N)


# ------------------------------------------------------------------ the single-signal helpers

HELPER_SIZES = [(37, 8), (64, 16), (100, 8), (128, 16), (200, 8), (256, 16), (450, 8), (512, 16), (1000, 8), (1024, 16)]


@pytest.mark.parametrize("N,T", HELPER_SIZES)
def test_delay_helpers_match_oracle(nat, oracle_lib, N, T):
    """pad_delay / lerp_delay / convolve_hybrid_delay_add at pads 0, 1, N - 1, N, N + 5 (lerp weights 0, 0.3125, 1) and the four
    plain FIR helpers, from a non-zero `out`: the *_add helpers (and pad_delay, lerp_delay, convolve_delay_naive) accumulate
    into it, convolve_delay_vectorized overwrites it."""
    from interface import config
    config.configure(N_MICROPHONES=4, N_SAMPLES=N, MAX_RES_X=2, MAX_RES_Y=2, N_TAPS=T)
    rng = np.random.default_rng(1000 * N + T)
    sig = rng.standard_normal(N).astype(np.float32)
    base = rng.standard_normal(N).astype(np.float32)
    h = rng.uniform(-0.5, 0.5, T).astype(np.float32)
    orc = oracle_lib.Oracle(N, 2, 2, T)
    s, hp = nat.fptr(sig), nat.fptr(h)

    def check(call, want, start=base):
        buf = _buffer(N, start)
        call(nat.fptr(buf))
        nat.check()
        _assert_written(buf, want, N)

    for p in (0, 1, N - 1, N, N + 5):
        check(lambda o: nat.lib.pad_delay(s, o, p), orc.pad_delay(sig, base, p))
        for w in (0.0, 0.3125, 1.0):
            check(lambda o: nat.lib.lerp_delay(s, o, C.c_float(w), p), orc.lerp_delay(sig, base, w, p))
        check(lambda o: nat.lib.convolve_hybrid_delay_add(s, hp, p, o), orc.convolve_hybrid_delay_add(sig, h, p, base))
    for p in (N, N + 5):     # nothing to add: `out` comes back as it went in
        assert orc.pad_delay(sig, base, p).tobytes() == base.tobytes()
    check(lambda o: nat.lib.convolve_delay_naive(s, o, hp), orc.convolve_delay_naive(sig, base, h))
    check(lambda o: nat.lib.convolve_delay_naive_add(s, hp, o), orc.convolve_delay_naive_add(sig, h, base))
    check(lambda o: nat.lib.convolve_delay_vectorized_add(s, hp, o), orc.convolve_delay_vectorized_add(sig, h, base))
    fresh = orc.convolve_delay_vectorized(sig, h, base)
    assert fresh.tobytes() == orc.convolve_delay_vectorized(sig, h, np.zeros(N, dtype=np.float32)).tobytes()
    check(lambda o: nat.lib.convolve_delay_vectorized(s, hp, o), fresh)
    check(lambda o: nat.lib.convolve_delay_vectorized(s, hp, o), fresh, start=np.full(N, np.nan, dtype=np.float32))


# ------------------------------------------------------------------ api.h shims

def test_convolve_shims_match_mimo_on_published_frame(nat):
    """convolve_mimo_naive / convolve_mimo_vectorized (api.h) on a frame handed over with bf_publish_frame == mimo_convolve_*
    on the frame get_data returns (the reference's 122 dead-microphone rows zeroed)."""
    from interface import config
    M, N, X, Y, T = 256, 256, 5, 4, 8
    config.configure(N_MICROPHONES=M, N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=T)
    rng = np.random.default_rng(29)
    sig = (rng.standard_normal((M, N)) * 0.25).astype(np.float32)
    taps = rng.uniform(-0.5, 0.5, X * Y * M * T).astype(np.float32)
    mics = np.arange(M, dtype=np.int32)
    nat.lib.load_coefficients_convolve(nat.fptr(taps), taps.size)
    nat.lib.bf_publish_frame(nat.fptr(sig)); nat.check()
    seen = np.zeros_like(sig)
    nat.lib.get_data(nat.fptr(seen)); nat.check()
    assert np.count_nonzero(~seen.any(axis=1)) == 122
    for shim, mimo in ((nat.lib.convolve_mimo_naive, nat.lib.mimo_convolve_naive),
                       (nat.lib.convolve_mimo_vectorized, nat.lib.mimo_convolve_vectorized)):
        a = np.full(X * Y, np.nan, dtype=np.float32)
        b = np.full(X * Y, np.nan, dtype=np.float32)
        shim(nat.fptr(a), nat.iptr(mics), M); nat.check()
        mimo(nat.fptr(seen), nat.fptr(b), nat.iptr(mics), M); nat.check()
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ error contract: an error is set and `out` is all NaN

def test_miso_errors_poison_out(nat):
    from interface import config
    M, N, D, T = 8, 128, 3, 8
    n = M
    config.configure(N_MICROPHONES=M, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=T)
    rng = np.random.default_rng(31)
    sig = rng.standard_normal((M, N)).astype(np.float32)
    mics = np.arange(n, dtype=np.int32)
    whole = rng.integers(0, 20, D * n).astype(np.int32)
    d32 = rng.uniform(0, 20, D * n).astype(np.float32)
    taps = rng.uniform(-0.5, 0.5, D * n * T).astype(np.float32)
    by_mic = rng.integers(0, 20, 4).astype(np.int32)           # pad2 table for mics 0..3 only
    nat.lib.bf_clear_error()

    def fails(call, match, ids=mics):
        buf = np.full(N + SENTINEL, 7.0, dtype=np.float32)
        call(nat.fptr(buf), nat.iptr(ids))
        with pytest.raises(nat.BeamformerError, match=match):
            nat.check()
        assert np.isnan(buf[:N]).all() and (buf[N:] == 7.0).all()

    def loaders():
        nat.lib.load_coefficients_pad(nat.iptr(whole), whole.size)
        nat.lib.load_coefficients_lerp(nat.fptr(d32), d32.size)
        nat.lib.load_coefficients_convolve_hybrid(nat.fptr(d32), d32.size)
        nat.lib.load_coefficients_convolve(nat.fptr(taps), taps.size)
        nat.lib.load_coefficients_pad2(nat.iptr(by_mic), by_mic.size)
        nat.check()

    s = nat.fptr(sig)
    per_entry = {"pad": (nat.lib.miso_pad, 1), "lerp": (nat.lib.miso_lerp, 1), "hybrid": (nat.lib.miso_convolve_hybrid, 1),
                 "convolve": (nat.lib.miso_convolve_vectorized, T)}
    loaders()
    for name, (fn, per) in per_entry.items():
        fails(lambda o, m: fn(s, o, m, n, ((D - 1) * n + 1) * per), "exceeds")      # offset + n past the table
        fails(lambda o, m: fn(s, o, m, n, -n * per), "exceeds")                     # negative offset
        buf = np.full(N, np.nan, dtype=np.float32)
        fn(s, nat.fptr(buf), nat.iptr(mics), n, (D - 1) * n * per); nat.check()    # the last direction itself is fine
        assert np.isfinite(buf).all(), name
    fails(lambda o, m: nat.lib.miso_convolve_vectorized(s, o, m, n, T + 3), "multiple of N_TAPS")
    fails(lambda o, m: nat.lib.miso_pad2(s, o, m, 4, 0), "outside", ids=np.array([0, 1, 4, 2], dtype=np.int32))
    buf = np.full(N, np.nan, dtype=np.float32)
    nat.lib.miso_pad2(s, nat.fptr(buf), nat.iptr(mics), 4, 0); nat.check()
    assert np.isfinite(buf).all()

    unloads = [(nat.lib.unload_coefficients_pad, nat.lib.miso_pad, 1, "has not been called"),
               (nat.lib.unload_coefficients_pad2, nat.lib.miso_pad2, 1, "outside"),
               (nat.lib.unload_coefficients_lerp, nat.lib.miso_lerp, 1, "has not been called"),
               (nat.lib.unload_coefficients_convolve, nat.lib.miso_convolve_vectorized, T, "has not been called"),
               (nat.lib.unload_coefficients_convolve_hybrid, nat.lib.miso_convolve_hybrid, 1, "has not been called")]
    for unload, fn, per, match in unloads:
        unload()
        fails(lambda o, m: fn(s, o, m, 4 if fn is nat.lib.miso_pad2 else n, 0), match)
    loaders()
