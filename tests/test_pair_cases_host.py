"""CPU: the rows of tests/pair_cases.py checked on their own, before a GPU sees them -- the data are the same on every run, every
frame has more rows than active microphones, the family and the row layout written beside a row are what the restated routing rule
(batched_cases.predict_family / plan) gives for the row's own table, whose geometry is the native planner's (bf_plan_das); the rows
take every exit of both lerp drains, behind a trip of the loop and without one; a power sum that leaves its drain a quad early gives
other bits in every direction looked at; and the many-microphone rows do pass the 64 halves or chunks whose microphone ids a lane
holds."""
import ctypes as C

import numpy as np
import pytest

import batched_cases as BC
import pair_cases as PC
import util

LERP_ROWS = [r for r in PC.ROWS if r.algo == "lerp" and PC.BY_NAME[r.case].N % 4 == 0]      # (all but edge130, whose last two squares the oracle fuses)


def test_rows_are_deterministic_and_complete():
    names = [c.name for c in PC.CASES if c.name.startswith(("len132", "edge", "cells160", "chunks"))]
    first = {n: BC.data(n) for n in names}
    BC.data.cache_clear()
    for n in names:
        for a, b in zip(first[n], BC.data(n)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), n
    assert len(PC.BY_NAME) == len(PC.CASES) and not set(PC.BY_NAME) & set(BC.BY_NAME)      # (the names seed the data: no two alike)
    assert len(PC.IDS) == len(set(PC.IDS)) == len(PC.ROWS)
    assert sorted(PC.MANY_MICS + PC.BLOCK_LENGTHS) == sorted(PC.ROWS)
    # every block length on every pair kernel and FIR flavour, three frames
    for N in PC.LENGTHS:
        for case, algo, family, rows in (("len%d_16of20", "pad", 5, 0), ("len%d_16of20", "lerp", 8, 1), ("len%d_32of40", "lerp", 8, 2),
                                         ("len%d_32of40", "hybrid", 7, 0), ("len%d_32of40", "fir_naive", 7, 0), ("len%d_32of40", "fir_vec", 7, 0)):
            assert PC.Row(case % N, algo, family, rows) in PC.ROWS and PC.BY_NAME[case % N].F == 3
    assert PC.LENGTHS == tuple(N for N in range(129, 257) if N % 4 == 0) and len(PC.LENGTHS) == 32
    for N in PC.SHORT:
        for case, rows in (("len%d_16of20_f2", 1), ("len%d_32of40_f2", 2)):
            assert PC.Row(case % N, "lerp", 8, rows) in PC.ROWS and PC.BY_NAME[case % N].F == 2
    # rows out of order in at least one row per kernel
    kernels = {}
    for r in PC.ROWS:
        if PC.kernel_of(r):
            kernels.setdefault(PC.kernel_of(r), set()).add(PC.BY_NAME[r.case].rows)
    assert sorted(kernels) == ["das_hybrid_pair_kernel", "das_pair2_cells_kernel", "das_pair2_kernel", "das_pair_kernel"]
    for k, orders in kernels.items():
        assert orders == {"reversed", "sorted"}, k


@pytest.mark.parametrize("case", [c.name for c in PC.CASES])
def test_rows_and_shapes(case):
    c, d = PC.BY_NAME[case], BC.data(case)
    D = c.X * c.Y
    assert c.M_total > c.n and d.frames.shape == (c.F, c.M_total, c.N) and d.frames.dtype == np.float32
    assert d.mics.dtype == np.int32 and len(set(d.mics.tolist())) == c.n and 0 <= d.mics.min() and d.mics.max() < c.M_total
    step = np.diff(d.mics)
    assert (step < 0).all() if c.rows == "reversed" else (step > 0).all()
    assert not np.array_equal(d.mics, np.arange(c.n))            # a real subset: a kernel that read row i for column i would be wrong
    assert c.kind == ("folded" if case.startswith("order") else "smooth") and c.pmax == 30.0 and c.T == 8
    assert d.delays.shape == (D, c.n) and d.delays.min() >= 0 and d.delays.max() <= c.pmax
    assert (c.X, c.Y) == ((9, 8) if c.N == 1024 else (13, 21) if case.startswith("order") else (17, 16))
    lo, hi = BC.shard(c)
    assert 0 < lo < hi < D
    # the fixed prefix holds for every algorithm of the case: the furthest look-back (hybrid: max_whole + 1 + T / 2) + 1 within it
    for algo in c.algos:
        w = BC.whole(case, algo)
        if w is not None:
            assert int(w.max()) + 2 + (c.T // 2 if algo == "hybrid" else 0) <= (56 if c.N <= 256 else 64), algo


@pytest.mark.parametrize("row", PC.ROWS, ids=PC.IDS)
def test_expected_family_follows_the_routing_rule(native, row):
    """The family and the row layout beside the row == the restated rule on the row's own table, for the shard and the full range;
    the rule's geometry == the native planner's."""
    c = PC.BY_NAME[row.case]
    algo = row.algo
    w = BC.whole(row.case, algo)
    D = c.X * c.Y
    max_whole = 0 if w is None else int(w.max())
    out = (C.c_longlong * 10)()
    assert row.family == BC.family_of(c, algo)
    assert native.lib.bf_configure(c.M_total, c.N, c.X, c.Y, c.T) == 0
    try:
        for lo, hi in (BC.shard(c), (0, D)):
            assert BC.predict_family(algo, c.n, c.N, c.T, w, lo, hi, c.F) == row.family, (lo, hi)
            p = BC.plan(algo, c.n, c.N, c.T, hi - lo, c.F, max_whole)
            assert native.lib.bf_plan_das(util.ALGOS[algo], c.n, c.F, lo, hi, max_whole, 256, out) == 0
            nc, lead, rs, mc, nch, waves, dpw, tile, ntiles, lds = list(out)
            assert nc == p["nc"] and lds <= 160 * 1024 and mc * nch >= c.n
            assert row.rows == ((2 if p["cells"] else 1) if row.family == 8 else 0)
            assert bool(p.get("cells")) == (PC.kernel_of(row) == "das_pair2_cells_kernel")
            if p["layout"] == 2:
                assert (lead, waves, dpw) == (p["lead"], p["waves"], p["dpw"])
                assert bool(p["pair"]) == (row.family in (5, 7, 8))
                if p["long_rows"]:                              # two halves of 16 / segments microphones
                    assert mc == 2 * 16 // (nc // 4)
                if p["pair"]:
                    assert mc == (16 if algo in BC.PLAIN else 32)
            else:
                assert row.family == 0
            # more than 64 halves of the pair kernels, more than 64 chunks of the one-frame sweep: the ids beyond come from memory
            if row.case in PC.MANY_HALVES:
                half = 8 if algo == "pad" else 16
                assert p["pair"] and c.n % half == 0 and c.n // half == PC.MANY_HALVES[row.case] > 64
            if row.case in PC.MANY_CHUNKS:
                assert row.family == 2 and not p["long_rows"] and (mc, nch) == (4, PC.MANY_CHUNKS[row.case]) and nch > 64
                assert c.n - mc * (nch - 1) == 1                # the last chunk holds one microphone
    finally:
        util.configure("cfg1")
    if row.family == 8 and row.rows == 2:
        assert c.n % 32 == 0 and c.n // 16 in (2, 8, 10, 16)


@pytest.mark.parametrize("row", PC.ORDERED, ids=["%s-%s" % (r.case, r.algo) for r in PC.ORDERED])
def test_ordered_rows_sweep_in_another_order(row):
    """The shard and the full range of an ORDERED row are swept in an order that is not the identity: rows of the grid walked backwards."""
    import sweep_order_np as SO
    c = PC.BY_NAME[row.case]
    w = BC.whole(row.case, row.algo)
    assert [r.algo for r in PC.ORDERED] == ["pad", "lerp", "lerp"] and [r.rows for r in PC.ORDERED] == [0, 1, 2]
    for lo, hi in (BC.shard(c), (0, c.X * c.Y)):
        order, info = SO.sweep_order(w, lo, hi)
        print("%s %s [%d, %d): %s" % (row.case, row.algo, lo, hi, info))
        assert sorted(order.tolist()) == list(range(lo, hi)) and not info["identity"] and info["reversed"] >= c.X // 2 - 1
        assert info["changes"] < info["changes_identity"]


def test_many_microphone_rows_are_all_there():
    assert sorted(PC.MANY_HALVES) == sorted(c.name for c in PC.CASES if c.name.startswith("mics"))
    assert {r.case for r in PC.ROWS if r.case in PC.MANY_HALVES and r.algo == "pad"} == {"mics528_n256", "mics528_n252"}
    assert {(r.case, r.algo) for r in PC.ROWS if r.case.startswith("mics1040")} == {(n, a) for n in ("mics1040_n256", "mics1040_n252") for a in ("hybrid", "fir_vec")}
    cells = sorted((PC.BY_NAME[r.case].n, PC.BY_NAME[r.case].N) for r in PC.MANY_MICS if r.rows == 2)
    assert cells == sorted((n, N) for n in (128, 160, 256) for N in PC.MANY)
    assert 160 & (160 - 1) != 0                                  # no power of two: the mean over the microphones divides


def test_every_drain_exit_is_taken_with_and_without_a_trip():
    """Round 1 of the lerp kernels' power pass: every (kernel, exit, trip or not) that a block length can ask for has a row, and the
    rows leave none out."""
    table = PC.drain_table()
    can_occur = {(k,) + PC.drain(N) for k in ("das_pair2_kernel", "das_pair2_cells_kernel") for N in PC.LENGTHS}
    assert len(can_occur) == 2 * 8 * 2                           # two kernels, eight exits, behind a trip or not
    print()
    for key in sorted(can_occur):
        rows = table.get(key, [])
        print("%-22s exit %d, %-12s %2d rows: %s" % (key[0], key[1], "after a trip" if key[2] else "no trip", len(rows),
                                                     " ".join(sorted({"%d/F%d" % (PC.BY_NAME[r.case].N, PC.BY_NAME[r.case].F) for r in rows}))))
    assert set(table) == can_occur, sorted(can_occur - set(table))
    for key in can_occur:
        assert table[key], key
        if not key[2]:                                           # without a trip: a three-frame row and a two-frame one
            assert {PC.BY_NAME[r.case].F for r in table[key]} >= {2, 3}, key
    # the formula against the drain's own loop: trips of 8 while more than 8 quads are left, then exit = what is left
    for N in PC.LENGTHS:
        nq, trips = (N - 128) // 4, 0
        while nq > 8:
            nq, trips = nq - 8, trips + 1
        assert PC.drain(N) == (nq, trips > 0), N


def _k_ordered(sq, upto):
    s = np.zeros(sq.shape[0], dtype=np.float32)
    for k in range(upto):
        s = s + sq[:, k]
    return s


@pytest.mark.parametrize("row", LERP_ROWS, ids=["%s-%s" % (r.case, r.algo) for r in LERP_ROWS])
def test_a_drain_left_one_quad_early_changes_the_bits(oracle_lib, row):
    """Teeth, on the oracle alone: for the first 64 directions of frame 0 the float32 k-ordered sum of the N squared means (which,
    divided by N, is the oracle's map bit for bit) differs in bits from the same sum stopped at N - 4 -- in all 64."""
    c, d = PC.BY_NAME[row.case], BC.data(row.case)
    orc = oracle_lib.Oracle(c.N, c.X, c.Y, c.T)
    orc.load(util.ALGOS["lerp"], BC.table(row.case, "lerp"))
    beams = orc.miso_many(util.ALGOS["lerp"], d.frames[0], d.mics, np.arange(64, dtype=np.int32) * c.n)
    mean = beams / np.float32(c.n)
    sq = mean * mean
    assert sq.dtype == np.float32 and sq.shape == (64, c.N)
    whole, early = _k_ordered(sq, c.N), _k_ordered(sq, c.N - 4)
    want = BC.want(oracle_lib, row.case, "lerp")[0, :64]
    assert (whole / np.float32(c.N)).tobytes() == want.tobytes()            # the restated sum is the oracle's
    differ = int((whole.view(np.uint32) != early.view(np.uint32)).sum())
    differ_map = int(((early / np.float32(c.N)).view(np.uint32) != want.view(np.uint32)).sum())
    print("%s: the sum stopped at %d differs from the sum over %d in %d of 64 directions (the maps in %d)" % (row.case, c.N - 4, c.N, differ, differ_map))
    assert differ == 64 and differ_map == 64
