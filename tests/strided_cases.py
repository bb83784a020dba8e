"""Cases for test_strided_cases.py (GPU) and test_strided_cases_host.py (CPU): one row per instantiation and tiling class of the three
kernel templates of csrc/das_strided.hip that the stream and listed-direction calls run on,

    das_mimo_kernel<ALGO, NC, DPW, true>    pad / lerp, NC 1 2 4 8 16, DPW 1 4 (HIST = true: the stream maps)            20
    das_select_kernel<ALGO, NC, DPW, HIST>  pad / lerp / hybrid / fir_vec without HIST, pad / lerp with it; DPW 1 4,
                                            2 in place of 4 for hybrid at NC 16                                     40 + 20
    das_miso_kernel<ALGO, NC, true>         pad / lerp (HIST = true: the stream beams)                                   10

with the sizes that reach each, a restatement of the two planner functions they depend on (size_strided and tile_strided of
csrc/das_plan.cpp), the deterministic inputs of every row and their expected outputs from the committed C checker.
TEST INFRASTRUCTURE ONLY.

What a row's sizes are for (all at 256 compute units, the MI355X):
  NC      N_SAMPLES 64, 100, 256, 320 (no multiple of 64), 1024 -> 1, 2, 4, 8, 16 segments of 64 samples
  DPW     1 while the n microphone rows fit LDS beside the power scratch, 4 (hybrid at NC 16: 2) once they are staged in chunks;
          CHUNKED_N[NC] microphones need chunks under every algorithm's row stride here
  tile    with group = 16 waves x DPW: `small` while count x frames < 256 x group (a tile is a fraction of a group), else
          k = clamp(count x frames / (1024 x group), 1, 8) groups per tile, k = 1 for a chunked plan.  2100 x 16 gives k = 2 at DPW 1;
          2100 = 65 x 32 + 20, so the last tile holds one whole group and a ragged one of 4.  A chunked plan never has a tile
          beyond one group (k = 1; small tiles are fractions), so no DPW > 1 instantiation can make a second trip through its
          group loop: those rows take 2053 x 8 = 32 whole-group tiles and one of 5 entries (waves 5 .. 15 idle, waves 0 .. 4 with one
          of their DPW entries).
Stream rows that share sizes (`twin`) share table, stream and expectation: the select-stream row lists directions of the map row's grid."""
import collections
import functools
import types

import numpy as np

import select_np
import test_stream
from util import ALGOS

CUS = 256
LDS_BYTES = 160 * 1024
KERNELS = ("map", "select", "select_hist", "beam")            # bf_last_strided_plan's out[10]: 0, 1, 2, 3
PLAIN = ("pad", "lerp")
N_OF = {1: 64, 2: 100, 4: 256, 8: 320, 16: 1024}
CHUNKED_N = {1: 470, 2: 240, 4: 96, 8: 50, 16: 27}             # microphones that need several chunks at NC, for every algorithm here
HOP_OF_NC = {1: "half", 2: "N", 4: "half", 8: "N", 16: "H"}     # NC 16: the history fills the hop
MAXD = 20                                                       # largest whole-sample delay of every table unless a row says otherwise

Row = collections.namedtuple("Row", "name kernel algo NC DPW HIST chunks tile M_total n N D T maxd F count hop d0 tags")


def _row(name, kernel, algo, NC, DPW, chunks, tile, n, D, F, count, hop="N", T=8, maxd=MAXD, d0=0, tags=(), N=None):
    return Row(name, kernel, algo, NC, DPW, kernel in ("map", "select_hist", "beam"), chunks, tile, n + 2 if n < 16 else n + 3, n, N or N_OF[NC], D, T, maxd,
               F, count, hop, d0, frozenset(tags))


def _rows():
    rows = []
    for NC in (1, 2, 4, 8, 16):
        # ---- every instantiation of the map and select kernels: DPW 1 in a tile of two groups, DPW > 1 in whole-group tiles and a ragged one
        for algo in PLAIN:
            rows.append(_row("map_%s_nc%d_dpw1" % (algo, NC), "map", algo, NC, 1, "one", "k2+", 5, 2100, 16, 2100, HOP_OF_NC[NC]))
            rows.append(_row("map_%s_nc%d_dpw4" % (algo, NC), "map", algo, NC, 4, "several", "k1", CHUNKED_N[NC], 2053, 8, 2053, HOP_OF_NC[NC]))
            # the same sizes, tables and streams as the two map rows: directions of their grids, listed
            rows.append(_row("selh_%s_nc%d_dpw1" % (algo, NC), "select_hist", algo, NC, 1, "one", "k2+", 5, 2100, 16, 2100, HOP_OF_NC[NC], tags=["twin"]))
            rows.append(_row("selh_%s_nc%d_dpw4" % (algo, NC), "select_hist", algo, NC, 4, "several", "k1", CHUNKED_N[NC], 2053, 8, 2053, HOP_OF_NC[NC],
                             tags=["twin"]))
        for algo in ("pad", "lerp", "hybrid", "fir_vec"):
            dpw = 2 if (algo == "hybrid" and NC == 16) else 4
            rows.append(_row("sel_%s_nc%d_dpw1" % (algo, NC), "select", algo, NC, 1, "one", "k2+", 5, 12, 16, 2100))
            rows.append(_row("sel_%s_nc%d_dpw%d" % (algo, NC, dpw), "select", algo, NC, dpw, "several", "k1", CHUNKED_N[NC], 12, 8, 2053))
        # ---- das_miso_kernel<.., true>: NC 1 / 2 on the strided geometry, NC 4 .. 16 on the shifted-copies geometry (chunks of at most 16 microphones;
        # lerp at NC 16 holds 4 rows per chunk unless n is a multiple of 4, so one chunk is 3 microphones)
        for algo in PLAIN:
            rows.append(_row("beam_%s_nc%d_one" % (algo, NC), "beam", algo, NC, None, "one", None, 3, 6, 2, None, "all"))
            rows.append(_row("beam_%s_nc%d_several" % (algo, NC), "beam", algo, NC, None, "several", None, CHUNKED_N[NC] if NC <= 2 else 20, 6, 2, None, "all"))
    for algo in PLAIN:
        # ---- the tile classes a k2+ / chunked k1 row above does not give: small and one-chunk k1, per kernel
        for kernel, short, D in (("map", "map", None), ("select", "sel", 12), ("select_hist", "selh", None)):
            tw = ["twin"] if kernel == "select_hist" else []
            rows.append(_row("%s_%s_small" % (short, algo), kernel, algo, 1, 1, "one", "small", 5, D or 301, 3, 301, "half", tags=tw))
            rows.append(_row("%s_%s_k1" % (short, algo), kernel, algo, 1, 1, "one", "k1", 5, D or 600, 8, 600, "N", tags=tw))
        # ---- eight groups per tile (the planner's cap): a wave carries `filled` and its row head across seven group edges
        rows.append(_row("map_%s_k8" % algo, "map", algo, 1, 1, "one", "k2+", 5, 8300, 16, 8300, "half", tags=["k8"]))
        # ---- maps of a direction shard, written at the shard's origin
        rows.append(_row("map_%s_shard_k1" % algo, "map", algo, 1, 1, "one", "k1", 5, 750, 8, 600, "half", d0=150, tags=["shard"]))
        rows.append(_row("map_%s_shard_k2" % algo, "map", algo, 1, 1, "one", "k2+", 5, 2300, 16, 2100, "N", d0=200, tags=["shard"]))
        # ---- the beam kernel's history inside a zero prefix far longer than it: delays up to 3 under the fixed 64-column prefix of NC 16
        rows.append(_row("beam_%s_nc16_short_history" % algo, "beam", algo, 16, None, "one", None, 3, 6, 2, None, "all", maxd=3, tags=["lead_gt_hist"]))
        # ---- hostile samples through stage_chunk_stream
        rows.append(_row("map_%s_hostile" % algo, "map", algo, 2, 1, "one", "small", 5, 40, 5, 40, "half", tags=["hostile"]))
        rows.append(_row("selh_%s_hostile" % algo, "select_hist", algo, 2, 1, "one", "small", 5, 40, 5, 40, "half", tags=["hostile", "twin"]))
        rows.append(_row("beam_%s_hostile" % algo, "beam", algo, 2, None, "one", None, 5, 6, 5, None, "all", tags=["hostile"]))
    # ---- tap counts other than 8 in the window-local call: the zero columns in front of and behind a row follow N_TAPS
    for algo, T in (("hybrid", 5), ("hybrid", 64), ("fir_vec", 16), ("fir_vec", 64)):
        rows.append(_row("sel_%s_taps%d" % (algo, T), "select", algo, 2, 1, "one", "small", 5, 12, 3, 37, T=T, tags=["taps"]))
    return rows


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


def instantiation(row):
    """(kernel, algo, NC, DPW) as bf_last_strided_plan tells them; the beam kernel has no DPW argument."""
    return (row.kernel, row.algo, row.NC, None if row.kernel == "beam" else row.DPW)


def all_instantiations():
    want = set()
    for NC in (1, 2, 4, 8, 16):
        for algo in PLAIN:
            want |= {("map", algo, NC, 1), ("map", algo, NC, 4), ("select_hist", algo, NC, 1), ("select_hist", algo, NC, 4), ("beam", algo, NC, None)}
        for algo in ("pad", "lerp", "hybrid", "fir_vec"):
            want |= {("select", algo, NC, 1), ("select", algo, NC, 2 if (algo == "hybrid" and NC == 16) else 4)}
    assert len(want) == 90
    return want


# (kernel, algo, chunks, tile) every kernel with tiles must be launched in, (algo, NC, chunks) for the beams, and the tagged rows
def all_classes():
    want = set()
    for algo in PLAIN:
        for kernel in ("map", "select", "select_hist"):
            want |= {(kernel, algo, "one", "small"), (kernel, algo, "one", "k1"), (kernel, algo, "one", "k2+"), (kernel, algo, "several", "k1")}
        for NC in (1, 2, 4, 8, 16):
            want |= {("beam", algo, NC, "one"), ("beam", algo, NC, "several")}
        want |= {("tag", algo, "shard", "k1"), ("tag", algo, "shard", "k2+"), ("tag", algo, "lead_gt_hist", "beam"), ("tag", algo, "hist_eq_hop", 16)}
        want |= {("tag", algo, "hostile", k) for k in ("map", "select_hist", "beam")}
    want |= {("tag", "hybrid", "taps", 5), ("tag", "hybrid", "taps", 64), ("tag", "fir_vec", "taps", 16), ("tag", "fir_vec", "taps", 64)}
    return want


def classes_of(row):
    got = set()
    if row.kernel == "beam":
        got.add(("beam", row.algo, row.NC, row.chunks))
    elif row.algo in PLAIN:
        got.add((row.kernel, row.algo, row.chunks, row.tile))
    if "shard" in row.tags and row.d0 > 0 and row.d0 + row.count == row.D:
        got.add(("tag", row.algo, "shard", row.tile))
    if "lead_gt_hist" in row.tags:
        got.add(("tag", row.algo, "lead_gt_hist", row.kernel))
    if "hostile" in row.tags:
        got.add(("tag", row.algo, "hostile", row.kernel))
    if "taps" in row.tags:
        got.add(("tag", row.algo, "taps", row.T))
    if row.HIST and row.NC == 16 and row.kernel != "beam" and hop_of(row) == history(row):
        got.add(("tag", row.algo, "hist_eq_hop", 16))
    return got


def history(row):
    return row.maxd + (1 if row.algo == "lerp" else 0)


def hops(row):
    """The hops a row runs with: one for the map and select rows, N, N / 2 and H for the beams."""
    N, H = row.N, max(history(row), 1)
    kinds = {"N": N, "half": N // 2, "H": H}
    return [kinds["N"], kinds["half"], kinds["H"]] if row.hop == "all" else [kinds[row.hop]]


def hop_of(row):
    assert row.hop != "all"
    return hops(row)[0]


def plan_max_whole(row):
    return 0 if row.algo == "fir_vec" else row.maxd


# ------------------------------------------------------------------ size_strided / tile_strided restated (csrc/das_plan.cpp)

PLAN_KEYS = ("nc", "lead", "row_stride", "mic_chunk", "n_chunks", "waves", "dpw", "tile_dirs", "n_tiles", "lds")


def _round_up(v, m):
    return (v + m - 1) // m * m


def size_strided(N, n_mics, lead, tail):
    """The LDS image of the strided layout: rows of lead + 64 NC + tail floats beside 16 waves x pbw scratch rows of 64 NC + 4; the
    microphones in one chunk (DPW 1) while they fit 160 KiB - scratch - 16 bytes, else in chunks of a multiple of 4 (DPW 4).  None:
    not even one row fits."""
    segs = -(-N // 64)
    nc = 1 if segs <= 1 else 2 if segs <= 2 else 4 if segs <= 4 else 8 if segs <= 8 else 16
    p = dict(nc=nc, lead=lead, row_stride=lead + nc * 64 + tail, waves=16)
    srow = nc * 64 + 4
    pbw = 4 if nc <= 4 else 2 if nc <= 8 else 1
    scratch = 16 * pbw * srow * 4
    budget = LDS_BYTES - scratch - 16
    row_bytes = p["row_stride"] * 4
    if row_bytes * n_mics <= budget:
        p.update(mic_chunk=n_mics, n_chunks=1, dpw=1)
    else:
        mc = budget // row_bytes
        if mc < 1:
            return None
        if mc >= 4:
            mc &= ~3
        p.update(mic_chunk=mc, n_chunks=-(-n_mics // mc), dpw=4)
    p["lds"] = _round_up(p["mic_chunk"] * p["row_stride"], 4) * 4 + scratch
    return p


def tile_strided(p, dirs, frames, n_cus=CUS):
    group = p["waves"] * p["dpw"]
    work = dirs * frames
    if work < n_cus * group:
        td = _round_up(max(1, -(-work // n_cus)), p["dpw"])
    else:
        k = 1 if p["n_chunks"] > 1 else work // (n_cus * 4 * group)
        td = min(max(k, 1), 8) * group
    p["tile_dirs"], p["n_tiles"] = td, -(-dirs // td)
    return p


def plan_stream(algo, N, n, frames, dirs, max_whole, n_cus=CUS):
    p = size_strided(N, n, _round_up(max_whole + 1, 4), 0)
    return None if p is None else tile_strided(p, dirs, frames, n_cus)


def plan_select(algo, N, n, T, frames, count, max_whole, stream, n_cus=CUS):
    if stream:
        p = size_strided(N, n, _round_up(max_whole + 1, 4), 0)
    else:
        taps = T if algo in ("hybrid", "fir_vec") else 0
        shift = 0 if algo == "fir_vec" else max_whole
        p = size_strided(N, n, _round_up(shift + 1 + taps // 2, 4), _round_up(taps, 4))
    if p is None:
        return None
    if p["dpw"] == 4 and algo == "hybrid" and p["nc"] == 16:
        p["dpw"] = 2
    return tile_strided(p, count, frames, n_cus)


def tile_class(p, dirs, frames, n_cus=CUS):
    group = p["waves"] * p["dpw"]
    if dirs * frames < n_cus * group:
        return "small"
    assert p["tile_dirs"] % group == 0
    return "k1" if p["tile_dirs"] == group else "k2+"


def export(lib, row):
    """The row's plan from the library's own exports: bf_plan_das_stream, bf_plan_das_select, or bf_plan_das's one-beam plan."""
    import ctypes as C
    out = (C.c_longlong * 10)()
    assert lib.bf_configure(row.M_total, row.N, row.D, 1, row.T) == 0
    a, mw = ALGOS[row.algo], plan_max_whole(row)
    if row.kernel == "map":
        rc = lib.bf_plan_das_stream(a, row.n, row.F, row.d0, row.d0 + row.count, mw, CUS, out)
    elif row.kernel == "beam":
        rc = lib.bf_plan_das(a, row.n, 1, 0, 1, mw, CUS, out)
    else:
        rc = lib.bf_plan_das_select(a, row.n, row.F, row.count, mw, int(row.HIST), CUS, out)
    assert rc == 0, lib.bf_last_error()
    return dict(zip(PLAN_KEYS, out))


# ------------------------------------------------------------------ a row's inputs

def _seed(row):
    """Rows that share sizes (a map row and its select-stream twin) share the seed, so table, stream and expectation are shared."""
    return [row.M_total, row.n, row.N, row.D, row.T, row.maxd, row.F, len(row.algo), hops(row)[0], int("hostile" in row.tags)]


class Stream(test_stream.Stream):
    """tests/test_stream.py's seeded stream and its windows; `window` names a frame's samples in S, so that a row can plant values in
    them, and `sealed` rebuilds the zero-prefixed copy ext() reads after S was written to."""

    def window(self, f):
        s = self.start + f * self.hop
        return slice(s, s + self.N)

    def sealed(self):
        self.Sz = np.concatenate([np.zeros((self.S.shape[0], self.P), np.float32), self.S], axis=1)
        return self


def make_stream(row, hop, with_prev, mics):
    """The row's stream.  A hostile row (5 frames) gets the pattern of test_das_select.test_hostile_samples in the windows of frames 0 .. 2
    and hostile values where only a history read finds them: in the previous frame (with_prev) and in the last `hist` samples in front
    of frames 3 and 4, at the far end of the history (reached by the largest delay alone) and at its near end."""
    st = Stream(_seed(row) + [hop, int(with_prev)], row.M_total, row.N, hop, row.F, with_prev)
    if "hostile" in row.tags:
        S, N, H = st.S, row.N, max(history(row), 1)
        w = [st.window(f).start for f in range(row.F)]
        S[:, w[0]:w[0] + N:7] = np.float32(1e-41)
        S[2, w[0] + 5:w[0] + 9] = [0.0, -0.0, np.float32(-1e-44), 0.0]
        S[mics[1], w[1] + 17] = np.nan
        S[mics[3], w[1] + 60] = np.inf
        S[mics[0], w[2] + 3] = -np.inf
        S[mics[4], w[2]:w[2] + N] = -0.0
        S[mics[2], w[3] - 1] = np.float32(1e-41)
        S[mics[4], w[4] - H] = np.inf
        S[mics[0], w[4] - 1] = -0.0
        if with_prev:
            S[mics[1], w[0] - H] = np.nan
            S[mics[3], w[0] - 1] = np.float32(-1e-44)
    return st.sealed()


@functools.lru_cache(maxsize=None)
def _tables(seed, M_total, n, D, T, maxd, fir):
    rng = np.random.default_rng(list(seed))
    mics = rng.permutation(M_total)[:n].astype(np.int32)
    delays = rng.uniform(0.0, maxd + 0.99, size=(D, n))
    delays[rng.integers(0, D), rng.integers(0, n)] = maxd + 0.5        # the largest whole-sample delay is maxd exactly
    delays[0, 0] = 0.25                                                  # ... and the smallest 0
    taps = rng.uniform(-0.5, 0.5, size=(D, n, T)).astype(np.float32) if fir else np.zeros(1, np.float32)
    return mics, delays, taps


@functools.lru_cache(maxsize=None)
def tables(row):
    """(mics int32 [n], delays float64 [D, n], taps float32 [D, n, T] for fir_vec) and the flat table arrays select_np.powers reads."""
    mics, delays, taps = _tables(tuple(_seed(row)[:6] + [len(row.algo), int("hostile" in row.tags)]), row.M_total, row.n, row.D, row.T, row.maxd,
                                 row.algo == "fir_vec")
    d32 = np.ascontiguousarray(np.float32(delays)).ravel()
    whole = np.floor(d32).astype(np.int32)
    assert row.algo == "fir_vec" or (whole.max() == row.maxd and whole.min() == 0)
    per = row.T if row.algo == "fir_vec" else 1
    tab = types.SimpleNamespace(algo=row.algo, n=row.n, T=row.T, d32=d32, whole=whole, h=np.ascontiguousarray(taps, dtype=np.float32).ravel(), per=per,
                                entries=(taps.size if row.algo == "fir_vec" else d32.size))
    return mics, delays, taps, tab


def listed(row):
    """The list of a select row: int64 offsets [F, count] with rejected entries among them, and the directions they name [F, count]."""
    _, _, _, tab = tables(row)
    rng = np.random.default_rng(_seed(row) + [77])
    dirs = rng.integers(0, row.D, (row.F, row.count))
    dirs[:, 0], dirs[:, -1] = 0, row.D - 1
    offs = dirs.astype(np.int64) * row.n * tab.per
    offs[:, 5::37] = -1
    offs[:, 11] = tab.entries - row.n * tab.per + 1
    return offs, dirs


def beam_offsets(row, B):
    """int64 [F, B]: the first and last direction, then directions that change with the frame; with 16 beams or more one rejected entry."""
    _, _, _, tab = tables(row)
    dirs = np.array([[0, row.D - 1] + [(3 * b + f) % row.D for b in range(B)] for f in range(row.F)])[:, :B]
    offs = dirs.astype(np.int64) * row.n
    if B >= 16:
        offs[:, 9] = tab.entries
    return offs


def window_frames(row):
    """Frames [F, M_total, N] of a window-local select row."""
    rng = np.random.default_rng(_seed(row) + [5])
    return (rng.standard_normal((row.F, row.M_total, row.N)) * 0.25).astype(np.float32)


# ------------------------------------------------------------------ a row's expected outputs (the committed C checker)

def stream_beams(oracle_lib, row, st, offsets, f0=0):
    """The extended-window restatement: for every frame f (counted from f0) the checker runs on N + P samples, ext(f), at the accepted
    offsets of offsets [F, B]; the last N samples of each result are the beam.  -> (float32 [F, B, N], quiet NaN rows at rejected entries; status)."""
    mics, _, _, tab = tables(row)
    offsets = np.asarray(offsets, dtype=np.int64)
    status = select_np.verdicts(row.algo, offsets, row.n, row.T, tab.entries)
    out = np.empty(offsets.shape + (row.N,), dtype=np.float32)
    out.view(np.uint32)[...] = select_np.NAN_BITS
    orc = oracle_lib.Oracle(row.N + st.P, row.D, 1, row.T)
    a = ALGOS[row.algo]
    orc.load(a, tab.whole if row.algo == "pad" else tab.d32)
    for f in range(offsets.shape[0]):
        ok = np.flatnonzero(status[f] == 0)
        uniq, inverse = np.unique(offsets[f, ok], return_inverse=True)
        out[f, ok] = orc.miso_many(a, st.ext(f0 + f), mics, uniq)[:, st.P:][inverse]
    return out, status


def beam_power(beams, n, N):
    """float32(sum over t of (o / n)^2 in t order) / N of beams [.., N]: every square rounded before it is added."""
    q = np.asarray(beams, dtype=np.float32) / np.float32(n)
    sq = q * q
    assert sq.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        return np.add.accumulate(sq, axis=-1, dtype=np.float32)[..., -1] / np.float32(N)


_MAPS = {}


def stream_map(oracle_lib, row, with_prev=True):
    """The full stream map float32 [F, D] of a map or select-stream row's table and stream, computed once per shared seed."""
    key = (tuple(_seed(row)), with_prev)
    if key not in _MAPS:
        mics, _, _, _ = tables(row)
        st = make_stream(row, hop_of(row), with_prev, mics)
        offs = (np.arange(row.D, dtype=np.int64) * row.n)[None, :]
        full = np.empty((row.F, row.D), dtype=np.float32)
        for f in range(row.F):                                  # frame by frame: the beams of 16 frames x 2100 directions need not all be held
            beams, status = stream_beams(oracle_lib, row, st, offs, f0=f)
            assert not status.any()
            full[f] = beam_power(beams[0], row.n, row.N)
        _MAPS[key] = (st, full)
        _MAPS[key][1].setflags(write=False)
    return _MAPS[key]


def want_listed(oracle_lib, row):
    """Expected (power float32 [F, count], status int32 [F, count]) of a select or select-stream row."""
    mics, _, _, tab = tables(row)
    offs, dirs = listed(row)
    if row.kernel == "select":
        return select_np.powers(oracle_lib, tab, window_frames(row), mics, offs, row.N)
    _, full = stream_map(oracle_lib, row)
    status = select_np.verdicts(row.algo, offs, row.n, row.T, tab.entries)
    power = np.take_along_axis(full, dirs, axis=1).copy()
    power.view(np.uint32)[status != 0] = select_np.NAN_BITS
    return power, status
