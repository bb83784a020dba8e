"""The table of tests/test_topk.py: rows (name, B, T, K, population), inputs built from seeds, and what each row covers.

`population` is a tuple of B names from POPULATIONS, one per image: several populations share one launch.  The key map below (and
its inverse) restates score_key of csrc/nms_kernels.hip; it is used to construct inputs whose K-th largest key has chosen bytes and
to assert what the table covers (tests/test_topk_host.py) -- never for an expectation, which comes from topk_np's float comparisons."""
import functools
import zlib

import numpy as np

MAX_SCORES = 5 * 40001           # per row
TOTALS = (1, 63, 65, 1023, 1025, 8191, 8192, 8193, 16384, 16385, 32768, 32769, 33793, 40001)
KS = (1, 2, 63, 64, 65, 300, 1000, 1023, 1024)
FAMILY_TOTALS = (1025, 8193, 16385, 33793)       # one total per kernel for the populations that aim at a code path


def kernel_of(total):
    """launch_topk_candidates' rule: keys in 8, 16 or 32 registers per thread of the 1024, else re-read from memory."""
    if total <= 8 * 1024:
        return "reg8"
    if total <= 16 * 1024:
        return "reg16"
    if total <= 32 * 1024:
        return "reg32"
    return "generic"


# ---------------------------------------------------------------- the key map, for construction and coverage only

def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def key_of(x):
    """uint32 keys of float32 scores: a > b <=> key(a) > key(b); NaN -> 0; both zeros -> 0x80000000."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    k = np.where((u >> np.uint32(31)) != 0, ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(x), np.uint32(0), k).astype(np.uint32)


def float_of(key):
    """The float32 a key comes from (keys under 0x007FFFFF give negative NaN patterns, keys over 0xFF800000 positive ones: callers discard them)."""
    key = np.ascontiguousarray(key, dtype=np.uint32)
    return from_bits(np.where((key >> np.uint32(31)) != 0, key & np.uint32(0x7FFFFFFF), ~key))


def key_bytes(key):
    return [(int(key) >> (8 * p)) & 255 for p in range(4)]         # [pass 0 .. pass 3]; the select walks pass 3 first


def from_bytes(b):
    return np.uint32(b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24))


def bits_of_key(key):
    return int(bits(float_of(np.asarray([key], dtype=np.uint32)))[0])


PINF, NINF, FLT_MAX = 0x7F800000, 0xFF800000, 0x7F7FFFFF
PZERO, NZERO = 0x00000000, 0x80000000
NANS_POS, NANS_NEG = (0x7FC00000, 0x7F800001, 0x7FABCDEF, 0x7FFFFFFF), (0xFFC00000, 0xFF800001, 0xFFABCDEF, 0xFFFFFFFF)
SUBS_POS, SUBS_NEG = (0x00000001, 0x00012345, 0x007FFFFF), (0x80000001, 0x80012345, 0x807FFFFF)
SPECIAL_KINDS = ("pinf", "ninf", "nan_pos", "nan_neg", "flt_max", "sub_pos", "sub_neg", "pzero", "nzero")


def special_kind(u):
    """uint32 bit patterns -> dict kind -> bool mask."""
    u = np.asarray(u, dtype=np.uint32)
    mag = u & np.uint32(0x7FFFFFFF)
    neg = (u >> np.uint32(31)) != 0
    nan, sub = mag > 0x7F800000, (mag > 0) & (mag < 0x00800000)
    return dict(pinf=u == PINF, ninf=u == NINF, nan_pos=nan & ~neg, nan_neg=nan & neg, flt_max=u == FLT_MAX, sub_pos=sub & ~neg, sub_neg=sub & neg,
                pzero=u == PZERO, nzero=u == NZERO)


# ---------------------------------------------------------------- populations: (rng, T, K) -> float32 [T]

def _near_keys(rng, kk, n):
    """Keys that share 0 .. 3 leading bytes with kk and are random below: every radix pass sees rivals in the K-th key's bin and around it."""
    share = rng.integers(0, 4, n).astype(np.uint64)
    keep = (np.uint64(0xFFFFFFFF) << (np.uint64(8) * (np.uint64(4) - share))) & np.uint64(0xFFFFFFFF)
    rnd = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    keys = ((np.uint64(int(kk)) & keep) | (rnd & ~keep & np.uint64(0xFFFFFFFF))).astype(np.uint32)
    f = float_of(keys)
    return f[~np.isnan(f)]


def _around(rng, T, kk, n_above, tie_bits):
    """A row whose keys hold `n_above` entries above kk, the bit patterns `tie_bits` (all of key kk) at ascending indices in that order, and
    entries below kk elsewhere.  Where nothing lies above kk (+inf) or below it (NaN) the ties take those places, cycling through tie_bits."""
    kk = int(kk)
    pool = _near_keys(rng, kk, 4 * T + 256)
    pk = key_of(pool)
    above, below = pool[pk > kk], pool[pk < kk]
    tie_bits = list(tie_bits)
    n_tie = min(len(tie_bits), T)
    n_above = max(0, min(n_above, T - n_tie))
    if above.size == 0:
        n_tie, n_above = n_tie + n_above, 0
    n_below = T - n_tie - n_above
    if kk == 0:
        n_tie, n_below = n_tie + n_below, 0
    ties = np.asarray([tie_bits[i % len(tie_bits)] for i in range(n_tie)], dtype=np.uint32)
    assert (key_of(from_bits(ties)) == kk).all()
    lower = rng.choice(below, n_below) if below.size else from_bits(rng.choice(np.asarray(NANS_POS + NANS_NEG, dtype=np.uint32), n_below))
    out = np.empty(T, dtype=np.float32)
    perm = rng.permutation(T)
    out[np.sort(perm[:n_tie])] = from_bits(ties)
    out[perm[n_tie:n_tie + n_above]] = rng.choice(above, n_above) if n_above else np.empty(0, np.float32)
    out[perm[n_tie + n_above:]] = lower
    return out


def _byte_key(rng, p, val):
    """A key whose byte p is val, the other bytes in 2 .. 253, and which is no NaN's bit pattern."""
    b = [int(v) for v in rng.integers(2, 254, 4)]
    b[p] = val
    if p == 3 and val == 255:
        b[2] = int(rng.integers(0, 0x80))           # 2^127 .. FLT_MAX: under +inf (0xFF800000)
    if p == 3 and val == 0:
        b[2] = int(rng.integers(0x80, 0x100))       # -FLT_MAX .. -2^127: over -inf (0x007FFFFF)
    return from_bytes(b)


def _bytes_pop(p, val):
    def pop(rng, T, K):
        kk = _byte_key(rng, p, val)
        return _around(rng, T, kk, min(K, T) - 2, [bits_of_key(kk)] * 4)
    return pop


def _residue_pop(r):
    def pop(rng, T, K):
        b = [4 * int(m) + (r + 3) % 4 for m in rng.integers(1, 63, 4)]          # (b + 1) & 3 == r, 4 <= b <= 251: never the nb == 256 arm
        kk = from_bytes(b)
        return _around(rng, T, kk, min(K, T) // 2, [bits_of_key(kk)] * 3)
    return pop


def _straddle_pop(tie_bits):
    """The K-th place falls among copies of a special: up to four are admitted, the others are not."""
    def pop(rng, T, K):
        kk = int(key_of(from_bits(np.asarray(tie_bits[:1], dtype=np.uint32)))[0])
        return _around(rng, T, kk, min(K, T) - 4, [tie_bits[i % len(tie_bits)] for i in range(max(8, len(tie_bits)))])
    return pop


def _uniform(rng, T, K):
    return (rng.random(T) * 1.7 + 1e-3).astype(np.float32)          # rounded from float64: the whole mantissa varies


def _random_keys(rng, T, K):
    out = np.empty(0, dtype=np.float32)
    while out.size < T:
        f = float_of(rng.integers(0, 2 ** 32, 2 * T + 16, dtype=np.uint64).astype(np.uint32))
        out = np.concatenate([out, f[~np.isnan(f)]])
    return out[:T]


def _negatives(rng, T, K):
    """Distinct negatives over 2^-20 .. 2^20 under fewer than K positives: the K-th place is a negative."""
    out = (-np.exp2(rng.uniform(-20, 20, T))).astype(np.float32)
    n_pos = min(K, T) // 2
    out[rng.permutation(T)[:n_pos]] = _uniform(rng, n_pos, K)
    return out


_POOL = np.asarray((PINF, NINF, FLT_MAX, FLT_MAX | 0x80000000, PZERO, NZERO) + NANS_POS + NANS_NEG + SUBS_POS + SUBS_NEG, dtype=np.uint32)


def _specials_mix(rng, T, K):
    """Half specials of every kind, half numbers of both signs over 2^-12 .. 2^12."""
    out = (rng.standard_normal(T) * np.exp2(rng.integers(-12, 13, T))).astype(np.float32)
    pick = rng.random(T) < 0.5
    out[pick] = from_bits(rng.choice(_POOL, int(pick.sum())))
    return out


def _specials_sparse(rng, T, K):
    """Positives with one special in fifty: with K well under T everything but +inf and FLT_MAX stays outside the selection."""
    out = (rng.random(T) * 0.9 + 0.1).astype(np.float32)
    pick = rng.random(T) < 0.02
    out[pick] = from_bits(rng.choice(_POOL, int(pick.sum())))
    return out


def _all_nan(rng, T, K):
    return from_bits(rng.choice(np.asarray(NANS_POS + NANS_NEG, dtype=np.uint32), T))


def _few_numbers(rng, T, K):
    """min(K, T) // 2 numbers, the rest NaN: NaNs are admitted in index order."""
    out = _all_nan(rng, T, K)
    n = min(K, T) // 2
    out[rng.permutation(T)[:n]] = (rng.standard_normal(n) * 3).astype(np.float32)
    return out


TIE = np.float32(0.25)


def _tie_fill(rng, T, tie_at, n_greater):
    """TIE at the indices tie_at, n_greater distinct larger scores at random other places, distinct smaller positive scores and -1 elsewhere."""
    out = (rng.random(T) * 0.2 + 0.01).astype(np.float32)
    out[rng.random(T) < 0.3] = -1.0
    free = np.setdiff1d(np.arange(T), tie_at)
    n_greater = min(n_greater, free.size)
    out[rng.permutation(free)[:n_greater]] = (0.5 + rng.permutation(2048)[:n_greater] / 4096.0).astype(np.float32)
    out[tie_at] = TIE
    return out


def _all_equal(rng, T, K):
    return np.full(T, 0.375, dtype=np.float32)


def _every_97th(rng, T, K):
    return _tie_fill(rng, T, np.arange(0, T, 97), min(10, min(K, T) // 4))


def _exact_ties(rng, T, K):
    k = min(K, T)
    g = k // 3
    return _tie_fill(rng, T, np.sort(rng.permutation(T)[:k - g]), g)


def _last_tie_ragged(rng, T, K):
    """The last admitted tie sits in the final, ragged round of 1024; where that round has room, one more tie follows it and stays out."""
    k = min(K, T)
    g = k // 2
    need = k - g
    last = max(T - 3, (T // 1024) * 1024) if T % 1024 else T - 3
    last = max(last, need - 1)
    at = np.concatenate([np.sort(rng.permutation(last)[:need - 1]), [last], [T - 1] if last < T - 1 else []]).astype(np.int64)
    return _tie_fill(rng, T, at, g)


def _greater(which):
    def pop(rng, T, K):
        k = min(K, T)
        g = {"0": 0, "k-1": k - 1, ">=k": k + 5}[which]
        n_tie = min(2 * k, max(T - g, 1)) if which == "0" else min(5, max(T - g, 1))
        return _tie_fill(rng, T, np.sort(rng.permutation(T)[:n_tie]), g)
    return pop


def _fold_one_bin(rng, T, K):
    return (rng.random(T) * 0.5 + 0.5).astype(np.float32).clip(0.5, np.float32(1.0) - np.float32(2.0 ** -24))


def _fold_two_bins(rng, T, K):
    out = _fold_one_bin(rng, T, K)
    out[1::2] *= np.float32(4.0)              # [2, 4): the next top byte of the key
    return out


def _fold_64_bins(rng, T, K):
    top = (0x82 + np.arange(T) % 64).astype(np.uint32) << np.uint32(24)
    return float_of(top | rng.integers(0, 2 ** 24, T).astype(np.uint32))


def _flood(rng, T, K):
    out = rng.integers(1, 400, T).astype(np.float32) / np.float32(512.0)
    out[rng.random(T) < 0.3] = -1.0
    return out


def _no_candidate(rng, T, K):
    return np.full(T, -1.0, dtype=np.float32)


def _dominated(rng, T, K):
    out = _flood(rng, T, K)
    out[: T // 2] = 0.5
    return out


POPULATIONS = {
    "uniform": _uniform, "random keys": _random_keys, "negatives": _negatives,
    "specials mix": _specials_mix, "specials sparse": _specials_sparse, "all nan": _all_nan, "few numbers": _few_numbers,
    "straddle +inf": _straddle_pop([PINF]), "straddle -inf": _straddle_pop([NINF]), "straddle flt_max": _straddle_pop([FLT_MAX]),
    "straddle nan": _straddle_pop([v for pair in zip(NANS_POS, NANS_NEG) for v in pair]),
    "straddle sub+": _straddle_pop([SUBS_POS[1]]), "straddle sub-": _straddle_pop([SUBS_NEG[1]]),
    "straddle zeros -+": _straddle_pop([NZERO, PZERO]), "straddle zeros +-": _straddle_pop([PZERO, NZERO]),
    "straddle zeros --+": _straddle_pop([NZERO, NZERO, PZERO, PZERO, NZERO, PZERO]),
    "all equal": _all_equal, "every 97th": _every_97th, "exact ties": _exact_ties, "last tie ragged": _last_tie_ragged,
    "greater 0": _greater("0"), "greater k-1": _greater("k-1"), "greater >=k": _greater(">=k"),
    "fold one bin": _fold_one_bin, "fold two bins": _fold_two_bins, "fold 64 bins": _fold_64_bins,
    "flood": _flood, "no candidate": _no_candidate, "dominated": _dominated,
}
for _p in range(4):
    for _v in (0, 1, 254, 255):
        POPULATIONS["byte %d = %d" % (_p, _v)] = _bytes_pop(_p, _v)
for _r in range(4):
    POPULATIONS["residue %d" % _r] = _residue_pop(_r)

BYTES = tuple("byte %d = %d" % (p, v) for p in range(4) for v in (0, 1, 254, 255))
RESIDUES = tuple("residue %d" % r for r in range(4))
SPECIALS = ("specials mix", "specials sparse", "all nan", "few numbers", "straddle +inf", "straddle -inf", "straddle flt_max", "straddle nan", "straddle sub+",
            "straddle sub-", "straddle zeros -+", "straddle zeros +-", "straddle zeros --+")
TIES = ("all equal", "every 97th", "exact ties", "last tie ragged", "greater 0", "greater k-1", "greater >=k")
FOLDS = ("fold one bin", "fold two bins", "fold 64 bins")
MIXED = ("uniform", "random keys", "negatives", "specials mix", "flood")


def _rows():
    rows = []

    def add(name, T, K, pops):
        per = max(1, min(16, MAX_SCORES // T))              # images per launch: under the size cap, at most 16
        chunks = [pops[i:i + per] for i in range(0, len(pops), per)]
        for i, c in enumerate(chunks):
            rows.append(("%s T=%d K=%d%s" % (name, T, K, " #%d" % i if len(chunks) > 1 else ""), len(c), T, K, tuple(c)))

    # every total, either side of every dispatch edge, with every K; K > T, K == T; one image and a batch
    sweep = {1: (1, 2), 63: (63, 64, 1024), 65: (64, 65), 1023: (1023, 1024, 1), 1025: (1024, 300), 8191: (300,), 8192: (1000,), 8193: (1, 1024),
             16384: (2, 1000), 16385: (1023,), 32768: (1024,), 32769: (65, 1024), 33793: (63,), 40001: (1024, 1)}
    for T in TOTALS:
        for K in sweep[T]:
            add("mixed", T, K, MIXED + ("last tie ragged", "straddle zeros -+"))
    for T, K in ((1, 1), (65, 64), (1025, 2), (8192, 1023), (16385, 300), (32768, 1000), (40001, 1024)):
        add("one image", T, K, ("random keys",))
    for T, K in ((1, 2), (63, 64), (1023, 1024)):
        add("all inside", T, K, ("specials mix", "straddle zeros +-", "few numbers", "all nan"))
    # populations aimed at a code path, on one total per kernel
    for T in FAMILY_TOTALS:
        add("bytes", T, 65, BYTES)
        add("residues", T, 300, RESIDUES)
        add("specials", T, 64, SPECIALS)
        add("ties", T, 300 if T > 16385 else 65, TIES)
        add("folding", T, 1024, FOLDS)
    add("ties", 40001, 1000, ("every 97th", "last tie ragged", "exact ties"))
    add("ties", 8191, 63, ("every 97th", "last tie ragged", "exact ties"))
    # the populations of test_gpu_topk_candidates_match_numpy (tests/test_detector.py), one row each
    add("existing", 25200, 1024, ("flood", "no candidate", "dominated"))
    return rows


ROWS = _rows()
NAMES = [r[0] for r in ROWS]


@functools.lru_cache(maxsize=8)
def inputs(name):
    """-> scores float32 [B, T], boxes float32 [B, T, 4] (coordinate 0 = the box's index), cls int32 [B, T]."""
    _, B, T, K, pops = ROWS[NAMES.index(name)]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    scores = np.stack([POPULATIONS[p](rng, T, K) for p in pops]).astype(np.float32, copy=False)
    assert scores.shape == (B, T) and scores.dtype == np.float32
    boxes = rng.standard_normal((B, T, 4)).astype(np.float32)
    boxes[..., 0] = np.arange(T, dtype=np.float32)[None, :]
    cls = rng.integers(0, 80, (B, T)).astype(np.int32)
    for a in (scores, boxes, cls):
        a.setflags(write=False)
    return scores, boxes, cls


# ---------------------------------------------------------------- what a row covers

def covers(name):
    """The coverage classes of a row, read off its data: a set of strings (see REQUIRED)."""
    _, B, T, K, pops = ROWS[NAMES.index(name)]
    scores, _, _ = inputs(name)
    kern = kernel_of(T)
    fam = "generic" if kern == "generic" else "reg"
    keff = min(K, T)
    out = {"kernel " + kern, "total %d" % T, "k %d" % K, "one image" if B == 1 else "batch"}
    out.add("k > total" if K > T else "k == total" if K == T else "k < total")
    if T % 1024:
        out.add(kern + " lanes past total")
    for b in range(B):
        s = scores[b]
        u, key = bits(s), key_of(s)
        desc = np.sort(key)[::-1]
        kth = int(desc[keff - 1])
        greater, equal = int((key > kth).sum()), int((key == kth).sum())
        need = keff - greater
        for p, byte in enumerate(key_bytes(kth)):
            if byte in (0, 1, 254, 255):
                out.add("%s pass %d byte %d" % (fam, p, byte))
            if byte != 255:                                # (bin 255 takes the nb == 256 arm, which picks nothing)
                out.add("%s pass %d residue %d" % (fam, p, (byte + 1) & 3))
        # tie shapes
        tied = np.flatnonzero(key == kth)
        last = int(tied[need - 1])
        if equal == T and T > 1:
            out.add(fam + " tie all equal")
        if equal == need and need > 1 and equal < T:
            out.add(fam + " tie exactly need_eq")
        if need > 1 and last // 1024 >= 5:
            out.add(fam + " tie many rounds")
        if T % 1024 and T > 1024 and last >= (T // 1024) * 1024 and need > 1:
            out.add(fam + " tie last in ragged round")
        if T > K and equal > 1:
            if greater == 0:
                out.add(fam + " greater 0")
            if greater == keff - 1:
                out.add(fam + " greater k-1")
        vals, cnt = np.unique(key[key < kth], return_counts=True)
        if T > K and (cnt[vals != 0] > 1).any():             # a tied value with K or more scores above it: wholly outside
            out.add(fam + " greater >= k")
        # specials on either side of the K-th place (rank by the restated key, index ascending among equals)
        rank = np.empty(T, dtype=np.int64)
        rank[np.lexsort((np.arange(T), -key.astype(np.int64)))] = np.arange(T)
        chosen = rank < keff
        for kind, m in special_kind(u).items():
            if (m & chosen).any():
                out.add("%s selected" % kind)
            if (m & ~chosen).any():
                out.add("%s not selected" % kind)
        sel = np.flatnonzero(chosen & ((u == PZERO) | (u == NZERO)))
        if sel.size:
            neg, pos = sel[u[sel] == NZERO], sel[u[sel] == PZERO]
            if neg.size and pos.size and neg.min() < pos.max():
                out.add(fam + " selected -0.0 before +0.0")
            if neg.size and pos.size and pos.min() < neg.max():
                out.add(fam + " selected +0.0 before -0.0")
            if kth == 0x80000000 and equal > need and neg.size and pos.size:
                out.add(fam + " zeros straddle")
        if np.isnan(s).all():
            out.add("all nan")
        if 0 < int((~np.isnan(s)).sum()) < keff and T > K:
            out.add("nan admitted in index order")
        if kth < 0x80000000 and kth > 0x007FFFFF and int((s > 0).sum()) > 0 and np.unique(s[s < 0]).size > keff:
            out.add("k-th among distinct negatives")
        if np.unique(key & 0xFF).size > 200 and np.unique((key >> 8) & 0xFF).size > 200:
            out.add("all four bytes vary")
        # pass 3's histogram folding, reg kernels: wave w of slab j holds the indices j * 1024 + 64 w .. + 63
        if fam == "reg":
            top = (key >> np.uint32(24)).astype(np.int64)
            pad = np.full((-T) % 64, -1, dtype=np.int64)
            waves = np.concatenate([top, pad]).reshape(-1, 64)
            full = waves[(waves >= 0).all(axis=1)]
            if full.size:
                distinct = np.asarray([np.unique(w).size for w in full])
                if (distinct == 1).any():
                    out.add("fold one bin")
                if (distinct == 64).any():
                    out.add("fold 64 bins")
                two = full[distinct == 2]
                if any((w[0::2] == w[0]).all() and (w[1::2] == w[1]).all() for w in two):
                    out.add("fold two alternating bins")
            if pad.size:
                out.add("fold lanes past total")
    return out


REQUIRED = (
    ["kernel " + k for k in ("reg8", "reg16", "reg32", "generic")] + ["total %d" % t for t in TOTALS] + ["k %d" % k for k in KS]
    + ["one image", "batch", "k > total", "k == total", "k < total"] + [k + " lanes past total" for k in ("reg8", "reg16", "reg32", "generic")]
    + ["%s pass %d byte %d" % (f, p, v) for f in ("reg", "generic") for p in range(4) for v in (0, 1, 254, 255)]
    + ["%s pass %d residue %d" % (f, p, r) for f in ("reg", "generic") for p in range(4) for r in range(4)]
    + ["%s %s" % (f, t) for f in ("reg", "generic") for t in ("tie all equal", "tie exactly need_eq", "tie many rounds", "tie last in ragged round",
                                                             "greater 0", "greater k-1", "greater >= k", "selected -0.0 before +0.0",
                                                             "selected +0.0 before -0.0", "zeros straddle")]
    + ["%s %s" % (k, side) for k in SPECIAL_KINDS for side in ("selected", "not selected")]
    + ["all nan", "nan admitted in index order", "k-th among distinct negatives", "all four bytes vary",
       "fold one bin", "fold two alternating bins", "fold 64 bins", "fold lanes past total"]
)


# ---------------------------------------------------------------- the chained test's head maps

CHAIN_CASE = (1, 2, 3)          # postproc_cases.DECODE_CASES: one class, levels 7 x 5, 3 x 9, 1 x 2 (192 boxes), three images
CHAIN_K, CHAIN_IOU, CHAIN_MAX_DET = 64, 0.45, 300
