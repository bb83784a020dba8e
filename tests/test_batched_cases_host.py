"""CPU: the case module of the batched planner-branch tests (tests/batched_cases.py) checked on its own -- the data are the same on
every run, every frame has more rows than active microphones, the smooth tables stay far below the share of re-reads at which the
digest build hands a launch to the direction-outer variant and the random ones far above it, the family written beside a case is
what the restated routing rule gives (whose geometry is in turn the native planner's, bf_plan_das), and the oracle runs them all."""
import ctypes as C

import numpy as np
import pytest

import batched_cases as BC
import util


def test_cases_are_deterministic():
    first = {c.name: BC.data(c.name) for c in BC.CASES}
    BC.data.cache_clear()
    for c in BC.CASES:
        again = BC.data(c.name)
        for a, b in zip(first[c.name], again):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), c.name
    assert len(BC.BY_NAME) == len(BC.CASES)                     # (the names seed the data: no two alike)


@pytest.mark.parametrize("case", [c.name for c in BC.CASES])
def test_rows_and_shapes(case):
    c, d = BC.BY_NAME[case], BC.data(case)
    D = c.X * c.Y
    assert c.M_total > c.n and d.frames.shape == (c.F, c.M_total, c.N) and d.frames.dtype == np.float32
    assert d.mics.dtype == np.int32 and len(set(d.mics.tolist())) == c.n and 0 <= d.mics.min() and d.mics.max() < c.M_total
    step = np.diff(d.mics)
    assert (step < 0).all() if c.rows == "reversed" else (step > 0).all()
    assert not np.array_equal(d.mics, np.arange(c.n))            # a real subset: a kernel that read row i for column i would be wrong
    assert d.delays.shape == (D, c.n) and d.delays.min() >= 0 and d.delays.max() <= c.pmax
    lo, hi = BC.shard(c)
    assert 0 < lo < hi < D
    if c.kind == "smooth":
        assert BC.span_of(c) <= D / 4


def test_every_family_has_out_of_order_rows():
    fams = {}
    for name, algo in BC.PARAMS:
        c = BC.BY_NAME[name]
        fams.setdefault(BC.family_of(c, algo), set()).add(c.rows)
    assert sorted(fams) == [0, 2, 3, 4, 5, 6, 7, 8]
    for fam, rows in fams.items():
        assert "reversed" in rows, fam
    assert {c.F for c in BC.CASES} == {2, 3}


def _shares(name, algo):
    """Share of the shareable steps of the flat order at which the whole-sample delay changes: the shard and the full range."""
    c = BC.BY_NAME[name]
    w = BC.whole(name, algo)
    p = BC.plan(algo, c.n, c.N, c.T, c.X * c.Y - 5, c.F, int(w.max()))
    out = []
    for lo, hi in (BC.shard(c), (0, c.X * c.Y)):
        changes, steps = BC.reload_share(w, lo, hi, p["dpw"])
        out.append(changes / steps)
    return out, p["dpw"]


@pytest.mark.parametrize("case,algo", [(n, a) for n, a in BC.PARAMS if BC.BY_NAME[n].kind == "smooth" and a in BC.PLAIN])
def test_smooth_tables_share_their_reads(case, algo):
    shares, dpw = _shares(case, algo)
    print("%s %s: whole-sample delay changes at %.4f (shard) / %.4f (full range) of the shareable steps, runs of %d" % (case, algo, shares[0], shares[1], dpw))
    for s in shares:
        assert s < 0.25


@pytest.mark.parametrize("case,algo", [(n, a) for n, a in BC.PARAMS if BC.family_of(BC.BY_NAME[n], a) == 3])
def test_random_tables_headed_for_the_direction_outer_variant_re_read(case, algo):
    assert BC.BY_NAME[case].kind == "random"
    shares, dpw = _shares(case, algo)
    print("%s %s: whole-sample delay changes at %.4f (shard) / %.4f (full range) of the shareable steps, runs of %d" % (case, algo, shares[0], shares[1], dpw))
    for s in shares:
        assert s > 0.5


@pytest.mark.parametrize("case,algo", BC.PARAMS)
def test_expected_family_follows_the_routing_rule(native, case, algo):
    """The family beside the case == the restated rule on the case's own table, for the shard and the full range; the rule's
    geometry == the native planner's."""
    c = BC.BY_NAME[case]
    w = BC.whole(case, algo)
    D = c.X * c.Y
    max_whole = 0 if w is None else int(w.max())
    out = (C.c_longlong * 10)()
    assert native.lib.bf_configure(c.M_total, c.N, c.X, c.Y, c.T) == 0
    try:
        for lo, hi in (BC.shard(c), (0, D)):
            assert BC.predict_family(algo, c.n, c.N, c.T, w, lo, hi, c.F) == BC.family_of(c, algo), (lo, hi)
            p = BC.plan(algo, c.n, c.N, c.T, hi - lo, c.F, max_whole)
            assert native.lib.bf_plan_das(util.ALGOS[algo], c.n, c.F, lo, hi, max_whole, 256, out) == 0
            nc, lead, rs, mc, nch, waves, dpw, tile, ntiles, lds = list(out)
            assert nc == p["nc"] and lds <= 160 * 1024 and mc * nch >= c.n
            if p["layout"] == 2:
                assert (lead, waves, dpw) == (p["lead"], p["waves"], p["dpw"])
                if p["long_rows"]:                              # two halves of 16 / segments microphones
                    assert mc == 2 * 16 // (nc // 4)
                if p["pair"]:
                    assert mc == (16 if algo in BC.PLAIN else 32)
        # the one-frame call of the GPU test's first step walks no frames; where it takes another family the test says so
        one = BC.predict_family(algo, c.n, c.N, c.T, w, 0, D, 1)
        fam = BC.family_of(c, algo)
        assert one == ({5: 2, 8: 2, 7: 4}.get(fam, fam))
    finally:
        util.configure("cfg1")


def test_what_the_case_comments_promise():
    """The properties a case is named for, on the data it actually draws."""
    w = BC.whole("sweep_runtime_stride", "lerp")
    assert w.max() + 2 > 56                                      # past the fixed 56-sample prefix
    for algo in BC.PLAIN:
        assert BC.whole("long_runtime_stride", algo).max() + 2 > 64
        assert BC.whole("long_two_segments", algo).max() + 2 <= 64 and BC.whole("long_partial_third", algo).max() + 2 <= 64
    # lerp's long-row image: 8 microphones x two copies x 2 * (lead + 1024) floats must not fit 160 KiB for family 2 to run
    lead = BC.plan("lerp", 16, 1000, 8, 67, 3, int(BC.whole("long_runtime_stride", "lerp").max()))["lead"]
    assert 8 * 2 * 2 * (lead + 1024) * 4 > 160 * 1024
    assert BC.whole("strided_nc1_odd_n", "pad").max() == 63     # delays up to the block


@pytest.mark.parametrize("case,algo", BC.PARAMS)
def test_oracle_runs_every_case(oracle_lib, case, algo):
    c = BC.BY_NAME[case]
    w = BC.want(oracle_lib, case, algo)
    assert w.shape == (c.F, c.X * c.Y) and w.dtype == np.float32
    assert np.isfinite(w).all() and (w > 0).all()
    assert not np.array_equal(w[0], w[1])                       # frames differ: a kernel that read the wrong frame would show
