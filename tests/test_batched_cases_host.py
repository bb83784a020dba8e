"""CPU: the case module of the batched planner-branch tests (tests/batched_cases.py) checked on its own -- the data are the same on
every run, every frame has more rows than active microphones, the smooth tables stay far below the share of re-reads at which the
digest build hands a launch to the direction-outer variant and the random ones far above it, the family written beside a case is
what the restated routing rule gives (whose geometry is in turn the native planner's, bf_plan_das), and the oracle runs them all.
The hostile batch (BC.hostile) is checked here on the oracle alone -- every frame does on the CPU what it is there for -- and one test
shows why the GPU tests compare maps in bits: a wrong summation order stays far under REL_TOL."""
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
    assert len(BC.CASES) == 24 and len(BC.PARAMS) == 56
    # lerp's pair sweep (8) on both row layouts, each with rows out of order, with a count that is no power of two, and with two frames
    layouts = {}
    for name, algo in BC.PARAMS:
        c = BC.BY_NAME[name]
        if BC.family_of(c, algo) == 8:
            layouts.setdefault(BC.rows_of(c, algo), []).append(c)
        else:
            assert BC.rows_of(c, algo) == 0
    assert sorted(layouts) == [1, 2]
    assert sorted(c.name for c in layouts[2]) == ["cells_divided_mean_masked", "cells_reversed_rows", "cells_two_frames_short"]
    for rows, cases in layouts.items():
        assert any(c.rows == "reversed" for c in cases) and any(c.n & (c.n - 1) for c in cases) and any(c.F == 2 for c in cases), rows
    assert {BC.BY_NAME[n].algos for n in (BC.EVICT_PLAIN, BC.EVICT_FIR, BC.EVICT_CELLS)} == {BC.PLAIN, BC.FIRS, ("lerp",)}


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
                # the row layout beside the case: cells for whole pairs of 16-microphone halves beyond 128 samples
                assert BC.rows_of(c, algo) == ((2 if p["cells"] else 1) if BC.family_of(c, algo) == 8 else 0)
                assert bool(p["cells"]) == (p["pair"] and algo == "lerp" and c.n % 32 == 0 and c.N > 128)
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


def test_hostile_batch_is_deterministic(oracle_lib):
    first = {p: BC.hostile(*p) for p in BC.PARAMS}
    BC.hostile.cache_clear()
    for p in BC.PARAMS:
        again = BC.hostile(*p)
        assert again.info == first[p].info, p
        for a, b in zip(first[p][:3], again[:3]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), p


@pytest.mark.parametrize("case,algo", BC.PARAMS)
def test_hostile_frames_on_the_oracle(oracle_lib, case, algo):
    """What each of the seven frames is for, on the oracle alone: the GPU test then only has to ask for the same NaNs and bits.
    Measured over the first 50 (case, algorithm) pairs: quiet exponents -62 .. -65, loud exponents 63 .. 66, the loud frames' largest sum
    of squares 2^126.1 .. 2^127.99 with a map's largest entry at most 2.54 times its smallest, NaN share of the one bad sample
    0.51 .. 0.60 (pad / lerp), 0.56 .. 0.87 (hybrid at 8 taps), 1 for hybrid at 16 taps and the plain FIRs."""
    c, d = BC.BY_NAME[case], BC.data(case)
    h = BC.hostile(case, algo)
    D = c.X * c.Y
    w = h.want
    assert h.frames.shape == (BC.HOSTILE_FRAMES, c.M_total, c.N) and h.frames.dtype == np.float32 and w.shape == (BC.HOSTILE_FRAMES, D)
    inactive = np.setdiff1d(np.arange(c.M_total), d.mics)
    assert inactive.size >= 3 and np.isnan(h.frames[:, inactive]).all()
    assert h.frames[BC.QUIET].tobytes() == np.where(np.isnan(h.clean[0]), np.float32(np.nan), np.ldexp(d.frames[0], h.info["e_quiet"])).astype(np.float32).tobytes()
    print("%s %s: %s, NaN share of frame 1 %.2f, largest sum of squares of frame 3 2^%.2f"
          % (case, algo, h.info, np.isnan(w[BC.BAD]).mean(), np.log2(float(w[BC.LOUD].max()) * c.N)))

    # the rows no microphone names, and the samples no direction reads, are never read: the maps of the frames with zeros in the
    # inactive rows and without the poison are the same bytes
    zeroed = np.where(np.isnan(h.clean), np.float32(0), h.clean)
    assert np.isfinite(zeroed).all()
    base = BC._oracle_maps(case, algo, zeroed)
    for f in (BC.QUIET, BC.PLAIN_F, BC.LOUD, BC.SATURATED, BC.SPARSE, BC.POISON):
        assert w[f].tobytes() == base[f].tobytes(), BC.KINDS[f]
    assert not np.isnan(base[BC.BAD]).any()

    tiny = np.finfo(np.float32).tiny
    assert (w[BC.QUIET] > 0).all() and (w[BC.QUIET] < tiny).all()                       # nonzero and subnormal, every entry
    share = np.isnan(w[BC.BAD]).mean()
    assert np.isnan(h.frames[BC.BAD][d.mics]).sum() == 1
    if algo in ("fir_naive", "fir_vec") or (case, algo) in BC.BAD_REACHES_ALL:
        assert share == 1.0
    else:
        assert 0.1 <= share <= 0.9
        assert np.array_equal(w[BC.BAD][~np.isnan(w[BC.BAD])].view(np.uint32), base[BC.BAD][~np.isnan(w[BC.BAD])].view(np.uint32))
    assert np.isfinite(w[BC.PLAIN_F]).all()
    # loud: the map is the sum of squares over N, so it is that sum -- the number that can overflow -- which sits under the top:
    # less than a factor 4 from 2^128, and N times nearer than a map value of 2^125 could come
    assert np.isfinite(w[BC.LOUD]).all() and float(w[BC.LOUD].max()) * c.N >= 2.0 ** 126
    assert np.isposinf(w[BC.SATURATED]).all()                                           # +inf everywhere, hence no NaN
    assert h.frames[BC.SATURATED][d.mics].tobytes() == (h.frames[BC.LOUD][d.mics] * np.float32(4)).tobytes()
    sp = h.frames[BC.SPARSE][d.mics]
    zero_rows, neg_rows = ~sp.any(axis=1) & ~np.signbit(sp).any(axis=1), ~sp.any(axis=1) & np.signbit(sp).all(axis=1)
    assert zero_rows.sum() == -(-c.n // 3) and neg_rows.sum() == -(-(c.n - 1) // 3)
    assert np.isfinite(w[BC.SPARSE]).all()
    poisoned = int(np.isnan(h.frames[BC.POISON][d.mics]).sum())
    assert poisoned == h.info["poisoned"]
    if algo in ("fir_naive", "fir_vec") or (case, algo) in BC.POISON_NOTHING:
        assert poisoned == 0
    else:
        assert poisoned >= 1


def _pad_restated(case, frame, power_sum="k order", mic_order="table"):
    """pad in NumPy float32, every direction at once: out += the microphone's row shifted by its whole-sample delay, microphone by
    microphone; out /= n; the squares summed one k at a time (the last N % 4 fused, as oracle/das_oracle.c states) and divided by N.
    power_sum="pairwise": the squares summed as a balanced tree.  mic_order="reversed": the microphones from last to first."""
    c, d = BC.BY_NAME[case], BC.data(case)
    w = BC.whole(case, "pad")
    D, N = w.shape[0], c.N
    assert N % 4 == 0                                           # no fused tail to restate at the sizes used here
    k = np.arange(N)
    out = np.zeros((D, N), dtype=np.float32)
    for m in (range(c.n) if mic_order == "table" else range(c.n - 1, -1, -1)):
        src = k[None, :] - w[:, m][:, None]
        out += np.where(src >= 0, frame[d.mics[m]][np.maximum(src, 0)], np.float32(0))
    out /= np.float32(c.n)
    sq = out * out
    assert sq.dtype == np.float32
    if power_sum == "k order":
        s = np.zeros(D, dtype=np.float32)
        for i in range(N):
            s = s + sq[:, i]
    else:
        s = sq
        while s.shape[1] > 1:
            if s.shape[1] % 2:
                s = np.concatenate([s, np.zeros((D, 1), dtype=np.float32)], axis=1)
            s = s[:, 0::2] + s[:, 1::2]
        s = s[:, 0]
    return s / np.float32(N)


@pytest.mark.parametrize("case", ["strided_nc1_odd_n", "strided_masked_tail", "pair_reversed_rows", "long_partial_third"])
def test_a_wrong_order_hides_under_the_tolerance(oracle_lib, case):
    """Why the maps are compared in bits.  A float32 restatement of pad equals the oracle byte for byte; the same restatement with
    the power summed as a tree, or with the microphones swept from last to first, moves a fifth of the map or more and stays a
    factor 7 or more under REL_TOL.  Measured on frame 0 (share of entries moved, largest relative error):
                             tree sum            reversed microphones
      strided_nc1_odd_n      0.222   9.1e-08     0.222   9.1e-08
      strided_masked_tail    0.467   2.4e-07     0.400   2.1e-07
      pair_reversed_rows     0.853   5.6e-07     0.603   2.3e-07
      long_partial_third     0.919   1.3e-06     0.651   3.4e-07"""
    frame = BC.data(case).frames[0]
    want = BC.want(oracle_lib, case, "pad")[0]
    assert _pad_restated(case, frame).tobytes() == want.tobytes()
    for wrong in (dict(power_sum="pairwise"), dict(mic_order="reversed")):
        got = _pad_restated(case, frame, **wrong)
        moved, err = float((got != want).mean()), util.max_rel(got, want)
        print("%s %s: %.3f of the entries differ, largest relative error %.2g" % (case, wrong, moved, err))
        assert moved >= 0.20, wrong
        assert err < util.REL_TOL, wrong


@pytest.mark.parametrize("case,algo", BC.PARAMS)
def test_oracle_runs_every_case(oracle_lib, case, algo):
    c = BC.BY_NAME[case]
    w = BC.want(oracle_lib, case, algo)
    assert w.shape == (c.F, c.X * c.Y) and w.dtype == np.float32
    assert np.isfinite(w).all() and (w > 0).all()
    assert not np.array_equal(w[0], w[1])                       # frames differ: a kernel that read the wrong frame would show
