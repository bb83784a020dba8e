"""Cases for test_batched_plan_branches.py (GPU) and test_batched_cases_host.py (CPU): frame batches that reach every kernel family
plan_das (csrc/das_plan.cpp) routes a bf_das_device call to, with more frame rows than active microphones, and a NumPy
restatement of the routing rule so that a case's expected family is checked on the CPU before a GPU sees it.  hostile(name, algo)
gives every case a second batch, of samples that N(0, 0.25) never draws.
TEST INFRASTRUCTURE ONLY.

Three table kinds:
  random   independent uniform delays per (direction, microphone), as test_gpu_parity._random_case draws them: the whole-sample
           delay changes at nearly every direction step, so pad / lerp with 16 waves replan to the direction-outer variant (3)
  smooth   delays[d, m] = c_m + s_m * d / D over the flat direction index d, c_m uniform in [0, pmax - span], s_m uniform in
           [-span, span], clipped at 0, with span = min(D / 8, pmax / 2).  A microphone's whole-sample delay then changes at most
           span + 1 times over the D - 1 steps (under 1/4 of them at every D used here, span / 2D on average), so the sweep
           kernels (2, 5, 6, 8) are what runs.
  folded   (tests/pair_cases.py) smooth along a grid row of Y directions, delays[d, m] = c_m + s_m * (d % Y) / Y with span = min(Y / 4,
           pmax / 2), and back to c_m at every row end, as a real grid's delays are: most microphones change there at once, so where no
           run of 8 divides Y the sweep-order rule (csrc/sweep_order.h) walks every other row backwards and the pad / lerp pair kernels
           store through an order that is not the identity."""
import collections
import functools
import zlib

import numpy as np

import sweep_order_np as SO
from util import ALGOS

PLAIN = ("pad", "lerp")
FIRS = ("hybrid", "fir_naive", "fir_vec")
ALL = PLAIN + FIRS

Case = collections.namedtuple("Case", "name family algos M_total n N X Y T pmax kind rows F")


def _c(name, family, algos, M_total, n, N, X, Y, T, pmax, kind, rows="sorted", F=3):
    return Case(name, family, algos, M_total, n, N, X, Y, T, pmax, kind, rows, F)


# `family`: bf_last_das_variant() of the batched call (include/beamformer_hip.h), one number or one per algorithm.
CASES = [
    # ---- 0: the strided kernel das_mimo_kernel
    _c("strided_nc1_odd_n", 0, ALL, 8, 5, 64, 3, 3, 8, 63.9, "random", rows="reversed"),   # nc = 1, odd n, delays up to the block
    _c("strided_masked_tail", 0, ALL, 16, 13, 100, 5, 3, 8, 20.0, "random"),               # N not a multiple of 64
    _c("strided_chunked_dpw4", 0, PLAIN, 300, 280, 128, 4, 3, 8, 47.0, "random"),          # mics chunked, 4 accumulators carried across chunks
    _c("strided_fir_16_taps", 0, FIRS, 40, 32, 256, 4, 4, 16, 9.0, "random"),              # T = 16: no shifted-copies layout
    _c("strided_fir_512", 0, FIRS, 24, 20, 512, 5, 4, 8, 60.0, "random"),                  # FIR beyond 256 samples, nc = 8
    # ---- 2: the one-frame sweep das_copies_kernel walking the frames
    _c("sweep_8_waves", 2, PLAIN, 64, 37, 256, 7, 5, 8, 30.0, "random"),                   # fewer than 256 directions, n % 16 != 0 (8 waves count no re-reads: random stays in the sweep)
    _c("sweep_16_waves_odd_n", 2, PLAIN, 64, 37, 256, 17, 16, 8, 30.0, "smooth", rows="reversed"),   # 272 directions, n % 16 != 0
    _c("sweep_scalar_staging", 2, PLAIN, 20, 16, 202, 17, 16, 8, 30.0, "smooth"),          # N % 4 != 0
    _c("sweep_runtime_stride", 2, PLAIN, 20, 16, 256, 17, 16, 8, 200.0, "smooth"),         # lead > 56; n and N otherwise pair-eligible
    # ---- 3: the direction-outer variant of das_copies_kernel
    _c("direct_m_total", 3, PLAIN, 20, 16, 256, 17, 16, 8, 40.0, "random", rows="reversed"),
    _c("direct_four_segments", 3, PLAIN, 40, 24, 1024, 9, 8, 8, 40.0, "random"),
    # ---- 4: the FIR one-frame kernel walking the frames
    _c("fir_one_frame_odd_n", 4, FIRS, 64, 37, 256, 7, 5, 8, 30.0, "random", rows="reversed"),
    # ---- 6: das_long_kernel
    _c("long_two_segments", 6, PLAIN, 40, 32, 512, 17, 16, 8, 40.0, "smooth", rows="reversed"),   # fixed row stride
    _c("long_partial_third", 6, PLAIN, 64, 48, 700, 17, 16, 8, 20.0, "smooth"),            # third segment partial, fourth empty
    # four segments, run-time row stride.  lerp: rows of (sample, difference) pairs behind a 304-float prefix are 2 * 1328 floats; two
    # copies of 8 microphones are 169984 bytes, more than the 160 KiB of LDS, so plan_das keeps das_copies_kernel (2) for it
    _c("long_runtime_stride", {"pad": 6, "lerp": 2}, PLAIN, 20, 16, 1000, 9, 8, 8, 300.0, "smooth"),
    _c("sweep_two_segments_odd_n", 2, PLAIN, 12, 9, 450, 9, 8, 8, 30.0, "smooth"),         # n % half != 0: das_copies_kernel at two segments
    # ---- 5 / 8 and 7: the pair kernels with out-of-order rows
    _c("pair_reversed_rows", {"pad": 5, "lerp": 8}, PLAIN, 20, 16, 256, 17, 16, 8, 30.0, "smooth", rows="reversed"),
    _c("fir_pair_reversed_rows", 7, FIRS, 40, 32, 256, 17, 16, 8, 30.0, "smooth", rows="reversed"),
    # the same two with a microphone count that is no power of two: the mean over the microphones divides (csrc/das_device.h, mic_mean)
    _c("pair_divided_mean", {"pad": 5, "lerp": 8}, PLAIN, 56, 48, 256, 17, 16, 8, 30.0, "smooth", rows="reversed"),
    _c("fir_pair_divided_mean", 7, FIRS, 56, 48, 256, 17, 16, 8, 30.0, "smooth", rows="reversed"),
    # ---- two frames: the smallest batch the pair kernels take, no workgroup row with a single frame
    _c("pair_two_frames", {"pad": 5, "lerp": 8}, PLAIN, 20, 16, 256, 17, 16, 8, 30.0, "smooth", F=2),
    # ---- 8 on rows of 16-byte cells (das_pair2_cells_kernel, bf_last_das_rows() == 2): lerp with a multiple of 32 microphones
    _c("cells_reversed_rows", 8, ("lerp",), 40, 32, 256, 17, 16, 8, 30.0, "smooth", rows="reversed"),   # two halves of 16
    _c("cells_divided_mean_masked", 8, ("lerp",), 100, 96, 252, 17, 16, 8, 30.0, "smooth"),           # six halves, the mean divides, sample 252 .. 255 masked
    _c("cells_two_frames_short", 8, ("lerp",), 40, 32, 132, 17, 16, 8, 30.0, "smooth", F=2),           # round 1 of the power pass is one quad
]
BY_NAME = {c.name: c for c in CASES}
PARAMS = [(c.name, a) for c in CASES for a in c.algos]

# the cases of the digest-cache eviction tests
EVICT_PLAIN, EVICT_FIR, EVICT_CELLS = "pair_reversed_rows", "fir_pair_reversed_rows", "cells_reversed_rows"

# Cases of other modules (tests/pair_cases.py) that draw their data with the generators below: name -> Case.  They are no part of
# CASES, PARAMS or the hostile batch.
EXTRA = {}


def case_of(name):
    return BY_NAME[name] if name in BY_NAME else EXTRA[name]


def family_of(case, algo):
    return case.family[algo] if isinstance(case.family, dict) else case.family


def rows_of(case, algo):
    """bf_last_das_rows() of the batched call: 2 where the lerp pair sweep runs on cell rows, 1 on rows of sample pairs, 0 for every
    other family."""
    if family_of(case, algo) != 8:
        return 0
    return 2 if case.name.startswith("cells_") else 1


def shard(case):
    """The direction range [lo, hi) of the batched call."""
    return 3, case.X * case.Y - 2


def span_of(case):
    return min(case.X * case.Y / 8.0, case.pmax / 2.0)


Data = collections.namedtuple("Data", "frames mics delays taps")


@functools.lru_cache(maxsize=None)
def data(name):
    """frames float32 [F, M_total, N], mics int32 [n] (rows of a frame; column i of a table pairs with mics[i]), delays float64
    [D, n], taps float32 [D, n, T].  Seeded by the case's name; read-only, shared by every test that asks."""
    c = case_of(name)
    D = c.X * c.Y
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    frames = (rng.standard_normal((c.F, c.M_total, c.N)) * 0.25).astype(np.float32)
    mics = np.sort(rng.choice(c.M_total, c.n, replace=False)).astype(np.int32)
    if c.rows == "reversed":
        mics = np.ascontiguousarray(mics[::-1])
    if c.kind == "random":
        delays = rng.uniform(0, c.pmax, size=(D, c.n))
    elif c.kind == "folded":
        span = min(c.Y / 4.0, c.pmax / 2.0)
        c_m = rng.uniform(0, c.pmax - span, size=c.n)
        s_m = rng.uniform(-span, span, size=c.n)
        delays = np.maximum(c_m[None, :] + s_m[None, :] * ((np.arange(D) % c.Y)[:, None] / c.Y), 0.0)
    else:
        span = span_of(c)
        c_m = rng.uniform(0, c.pmax - span, size=c.n)
        s_m = rng.uniform(-span, span, size=c.n)
        delays = np.maximum(c_m[None, :] + s_m[None, :] * (np.arange(D)[:, None] / D), 0.0)
    taps = rng.uniform(-0.5, 0.5, size=(D, c.n, c.T)).astype(np.float32)
    for a in (frames, mics, delays, taps):
        a.setflags(write=False)
    return Data(frames, mics, delays, taps)


def _oracle_maps(name, algo, frames):
    """Oracle maps float32 [len(frames), D] over the full direction range (oracle/libdas_oracle.so has to be built: the tests
    that come here ask for the oracle_lib fixture first)."""
    import das_oracle
    c, d = case_of(name), data(name)
    orc = das_oracle.Oracle(c.N, c.X, c.Y, c.T)
    orc.load(ALGOS[algo], table(name, algo))
    return np.stack([orc.mimo_range(ALGOS[algo], f, d.mics, 0, c.X * c.Y) for f in frames])


# ---- hostile samples -----------------------------------------------------------------------------------------------------

KINDS = ("quiet", "one bad sample", "plain", "loud", "saturated", "sparse", "poison in the unread tail")
QUIET, BAD, PLAIN_F, LOUD, SATURATED, SPARSE, POISON = range(7)
HOSTILE_FRAMES = len(KINDS)
QUIET_LOG2 = -138       # where the median of the quiet frame's map is put: 12 binades below the smallest normal float32, 11 above the smallest subnormal

# frame BAD: (case, algo) whose tables let the one NaN reach every direction although the algorithm delays by whole samples --
# hybrid at T = 16 reads T / 2 = 8 samples past the whole-sample split, and that table's whole-sample delays span 0 .. 8
BAD_REACHES_ALL = {("strided_fir_16_taps", "hybrid")}
# frame POISON: (case, algo) whose tables leave no sample unread -- every microphone has whole-sample delay 0 in some direction
# (hybrid: a delay of at most T / 2).  The plain FIRs read everything in every case and are not listed.
POISON_NOTHING = {("direct_m_total", "pad"), ("direct_m_total", "lerp"),
                  ("strided_masked_tail", "hybrid"), ("strided_fir_16_taps", "hybrid"), ("fir_one_frame_odd_n", "hybrid")}

Hostile = collections.namedtuple("Hostile", "frames clean want info")


def _seven_plain(name):
    c, d = BY_NAME[name], data(name)
    rng = np.random.default_rng(zlib.crc32((name + "/hostile").encode()))
    f = (rng.standard_normal((HOSTILE_FRAMES, c.M_total, c.N)) * 0.25).astype(np.float32)
    f[QUIET] = d.frames[0]                                      # "the case's plain frame"
    return f


@functools.lru_cache(maxsize=None)
def hostile(name, algo):
    """Seven frames on the tables, microphone list and shapes of data(name) -- so the family of a batched call is the case's --
    that a kernel can get wrong while every N(0, 0.25) frame passes.  The pair kernels make partners of (0, 1), (2, 3), (4, 5);
    frame 6 runs alone.  In every frame the rows the microphone list does not name are NaN throughout.

      0 quiet      frames[0] of data(name) * 2^e, e such that the median of the oracle map is 2^QUIET_LOG2: a subnormal map
      1 one bad    a plain frame with one NaN, at row mics[m*], index N - 1 - q: m* the microphone whose whole-sample delay
                   varies most over the directions, q the median of its delays -- about half of the directions read it.  The
                   plain FIRs have no whole-sample rows (m* = 0, q = N / 2): every direction reads every sample
      2 plain      N(0, 0.25)
      3 loud       a plain frame * 2^e, e the largest at which the largest sum of squares the oracle forms (N times the map) stays
                   below 2^128: all finite, in [2^126, 2^128), less than a factor 4 from overflow.  (The map itself cannot come
                   nearer than 1/N to the largest float32: it is that sum divided by N.)
      4 saturated  frame 3 * 4: the sums are 16 times as large, and a map's smallest is within 2.6 of its largest, so all overflow
      5 sparse     a plain frame whose active rows i = 0, 3, 6 ... of the microphone list are +0.0 and i = 1, 4, 7 ... are -0.0
      6 poison     a plain frame, active row mics[m] NaN from index N - min_d whole[d][m] (hybrid: + T / 2) on: what no direction
                   reads.  The plain FIRs read everything: untouched

    -> Hostile(frames float32 [7, M_total, N], clean = the frames before NaNs went in (inactive rows 0: NaN), want = the oracle maps
    float32 [7, D] of `frames`, info = dict(e_quiet, e_loud, bad = (row, index), poisoned = number of samples)).  Read-only."""
    c, d = BY_NAME[name], data(name)
    D = c.X * c.Y
    w = whole(name, algo)
    f = _seven_plain(name)
    inactive = np.setdiff1d(np.arange(c.M_total), d.mics)
    f[:, inactive] = 0.0
    base = _oracle_maps(name, algo, f[[QUIET, LOUD]])           # of the plain frames, before scaling
    e_quiet = int(np.round((QUIET_LOG2 - np.log2(np.median(base[0].astype(np.float64)))) / 2))
    e_loud = int(np.floor((128 - np.log2(base[1].astype(np.float64).max() * c.N)) / 2 - 1e-9))
    f[QUIET] = np.ldexp(f[QUIET], e_quiet)
    f[LOUD] = np.ldexp(f[LOUD], e_loud)
    f[SATURATED] = f[LOUD] * np.float32(4)
    active = d.mics
    f[SPARSE, active[0::3]] = 0.0
    f[SPARSE, active[1::3]] = -0.0
    clean = f.copy()
    clean[:, inactive] = np.nan
    if w is None:
        m_star, q = 0, c.N // 2
    else:
        m_star = int(np.argmax(w.max(axis=0) - w.min(axis=0)))
        q = int(np.sort(w[:, m_star])[D // 2])
    bad = (int(active[m_star]), c.N - 1 - q)
    f[BAD, bad[0], bad[1]] = np.nan
    poisoned = 0
    if w is not None:
        first = c.N - w.min(axis=0) + (c.T // 2 if algo == "hybrid" else 0)
        for m in range(c.n):
            if first[m] < c.N:
                f[POISON, active[m], first[m]:] = np.nan
                poisoned += c.N - int(first[m])
    f[:, inactive] = np.nan
    want = _oracle_maps(name, algo, f)
    for a in (f, clean, want):
        a.setflags(write=False)
    return Hostile(f, clean, want, dict(e_quiet=e_quiet, e_loud=e_loud, bad=bad, poisoned=poisoned))


def table(name, algo):
    """What load_coefficients_* takes for `algo`, shaped [X, Y, n(, T)]."""
    c, d = case_of(name), data(name)
    if algo == "pad":
        t = d.delays.astype(int).astype(np.int32)
    elif algo in ("lerp", "hybrid"):
        t = np.float32(d.delays)
    else:
        return np.ascontiguousarray(d.taps.reshape(c.X, c.Y, c.n, c.T))
    return np.ascontiguousarray(t.reshape(c.X, c.Y, c.n))


def whole(name, algo):
    """The whole-sample rows int32 [D, n] the library keeps for `algo` (values beyond N clamp to N); None for the plain FIRs."""
    c, d = case_of(name), data(name)
    if algo in ("fir_naive", "fir_vec"):
        return None
    w = d.delays.astype(int).astype(np.int32) if algo == "pad" else SO.whole_of(d.delays)
    return np.minimum(w, c.N)


# ---- the routing rule, restated ---------------------------------------------------------------------------------------------

def reload_share(w, lo, hi, dpw, order=None):
    """(changes, steps) as bf_last_das_reloads defines them for directions [lo, hi) swept in `order` (default: flat): steps =
    the positions of every run of dpw but its first (a partial last run padded to dpw), times the microphones; changes = those
    at which the whole-sample delay differs from the position before."""
    order = np.arange(lo, hi) if order is None else order
    steps = -(-(hi - lo) // dpw) * (dpw - 1) * w.shape[1]
    return SO.run_changes(w, order, dpw), steps


def _round_up(v, m):
    return (v + m - 1) // m * m


def plan(algo, n, N, T, dirs, frames, max_whole):
    """What plan_das decides before any digest is counted: dict(nc, layout, lead, waves, dpw, pair, cells, long_rows).  cells: the
    lerp pair sweep runs on rows of 16-byte cells (das_pair2_cells_kernel), which takes whole pairs of 16-microphone halves."""
    nc = -(-N // 64)
    nc = 1 if nc <= 1 else 2 if nc <= 2 else 4 if nc <= 4 else 8 if nc <= 8 else 16
    plain = algo in PLAIN
    if not (nc >= 4 if plain else (nc == 4 and T == 8)):
        return dict(nc=nc, layout=0)
    nseg = nc // 4
    fixed_lead = 56 if nseg == 1 else 64
    back = max_whole + 1 + T // 2 if algo == "hybrid" else T // 2 if not plain else max_whole + 1
    lead = max(_round_up(back + 1, 4), fixed_lead)
    waves = 8 if plain and nseg == 1 and dirs < 256 else 16
    dpw = 4 if nseg == 4 else 8
    pair = nseg == 1 and waves == 16 and lead == fixed_lead and n % 16 == 0 and N % 4 == 0 and frames >= 2
    cells = pair and algo == "lerp" and n % 32 == 0 and N > 128
    long_rows = False
    if plain and nseg > 1:
        half = 16 // nseg
        slot_bytes = (2 if algo == "lerp" else 1) * 2 * (lead + nseg * 256) * 4      # two shifted copies of a microphone's row(s)
        long_rows = n % half == 0 and N % 4 == 0 and slot_bytes * 2 * half <= 160 * 1024
    return dict(nc=nc, layout=2, lead=lead, waves=waves, dpw=dpw, pair=pair, cells=cells, long_rows=long_rows)


def predict_family(algo, n, N, T, w, lo, hi, frames):
    """bf_last_das_variant() of a launch over directions [lo, hi) of a table whose whole-sample rows are `w` (None: the plain
    FIRs), following plan_das and ensure_digest (csrc/beamformer_api.cpp)."""
    max_whole = 0 if w is None else int(w.max())
    p = plan(algo, n, N, T, hi - lo, frames, max_whole)
    if p["layout"] == 0:
        return 0
    if algo not in PLAIN:
        return 7 if p["pair"] else 4
    if p["waves"] == 16:
        # the digest build counts the re-reads in the order the launch sweeps (the pair kernels: bf_sweep_order) and hands a table
        # that re-reads at more than half of the shareable steps to the direction-outer variant
        order = SO.sweep_order(w, lo, hi, p["dpw"])[0] if p["pair"] else None
        changes, steps = reload_share(w, lo, hi, p["dpw"], order)
        if steps > 0 and 2 * changes > steps:
            return 3
    if p["pair"]:
        return 8 if algo == "lerp" else 5
    return 6 if p["long_rows"] else 2


_WANT = {}


def want(oracle_lib, name, algo):
    """Oracle maps float32 [F, D] of every frame over the full direction range: computed once per (case, algo), read-only."""
    if (name, algo) not in _WANT:
        c, d = case_of(name), data(name)
        orc = oracle_lib.Oracle(c.N, c.X, c.Y, c.T)
        orc.load(ALGOS[algo], table(name, algo))
        w = np.stack([orc.mimo_range(ALGOS[algo], d.frames[f], d.mics, 0, c.X * c.Y) for f in range(c.F)])
        w.setflags(write=False)
        _WANT[(name, algo)] = w
    return _WANT[(name, algo)]
