"""CPU: tests/strided_cases.py against the library's planner exports (bf_plan_das_stream, bf_plan_das_select, bf_plan_das; no GPU).

  * every row's declared (NC, DPW, chunks, tile class) is what the export returns for its sizes at 256 compute units;
  * the rows cover all 90 instantiations of das_mimo_kernel<.., true>, das_select_kernel and das_miso_kernel<.., true> and every class
    strided_cases.all_classes lists; what is missing fails with its name;
  * size_strided and tile_strided restated in Python equal the two exports on a few thousand random legal shapes, no shape leaves the
    90 tuples, DPW > 1 exactly when there are several chunks, LDS <= 160 KiB, lead >= history in stream mode;
  * the expectations of every non-hostile row are finite and positive, and the batched checker entry equals the per-beam one."""
import ctypes as C

import numpy as np
import pytest

import strided_cases as sc
import util
from support import lib
from util import ALGOS


# ------------------------------------------------------------------ the rows against the exports

def check_row(lib, row):
    """What the table says of a row against the export's plan; returns the plan."""
    p = sc.export(lib, row)
    assert p["nc"] == row.NC, (row.name, "NC", p)
    assert (p["n_chunks"] > 1) == (row.chunks == "several"), (row.name, "chunks", p)
    assert p["lds"] <= sc.LDS_BYTES
    if row.kernel == "beam":
        assert row.NC <= 2 or p["mic_chunk"] <= 16
        assert p["lead"] >= sc.history(row)
        if "lead_gt_hist" in row.tags:
            assert p["lead"] > sc.history(row) + 4
        return p
    assert p["dpw"] == row.DPW, (row.name, "DPW", p)
    assert sc.tile_class(p, row.count, row.F) == row.tile, (row.name, "tile", p)
    group = p["waves"] * p["dpw"]
    last = row.count - (p["n_tiles"] - 1) * p["tile_dirs"]
    if row.tile != "small":
        # a whole group, then a ragged one that leaves waves without an entry and (DPW > 1) waves with fewer than DPW
        ragged = last % group
        assert 0 < ragged < p["waves"], (row.name, last, group)
        assert (last > group) if row.tile == "k2+" else (p["n_tiles"] > 1 and last < p["waves"]), (row.name, last, group)
    if row.HIST:
        assert p["lead"] >= sc.history(row) and sc.history(row) <= sc.hop_of(row) <= row.N
    return p


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.name)
def test_row_reaches_what_it_declares(lib, row):
    p = check_row(lib, row)
    # the restatement agrees on the table's own shapes too
    if row.kernel == "map":
        assert p == sc.plan_stream(row.algo, row.N, row.n, row.F, row.count, sc.plan_max_whole(row))
    elif row.kernel != "beam":
        assert p == sc.plan_select(row.algo, row.N, row.n, row.T, row.F, row.count, sc.plan_max_whole(row), row.HIST)


def missing(rows):
    """Names of the instantiations and classes the rows leave out."""
    # an instantiation counts where a tile holds a whole group and then a ragged one: k2+ for DPW 1, whole-group tiles and a ragged one beyond
    inst = sc.all_instantiations() - {sc.instantiation(r) for r in rows if r.kernel == "beam" or r.tile == ("k2+" if r.DPW == 1 else "k1")}
    classes = sc.all_classes() - set().union(*[sc.classes_of(r) for r in rows])
    return sorted(map(str, inst)) + sorted(map(str, classes))


def test_rows_cover_all_90_instantiations_and_every_class():
    assert {sc.instantiation(r) for r in sc.ROWS} <= sc.all_instantiations()
    assert missing(sc.ROWS) == []


def test_the_coverage_check_bites(lib):
    """One row removed: its instantiation is reported missing.  One row with a wrong NC: the export contradicts it."""
    victim = sc.BY_NAME["sel_hybrid_nc16_dpw2"]
    assert missing([r for r in sc.ROWS if r is not victim]) == [str(("select", "hybrid", 16, 2))]
    victim = sc.BY_NAME["map_lerp_shard_k2"]
    assert missing([r for r in sc.ROWS if r is not victim]) == [str(("tag", "lerp", "shard", "k2+"))]
    wrong = sc.BY_NAME["map_pad_nc8_dpw1"]._replace(NC=4)
    with pytest.raises(AssertionError, match="NC"):
        check_row(lib, wrong)


# ------------------------------------------------------------------ the restatement against the exports, on random shapes

def _export_select(lib, algo, n, F, count, mw, stream):
    out = (C.c_longlong * 10)()
    rc = lib.bf_plan_das_select(ALGOS[algo], n, F, count, mw, int(stream), sc.CUS, out)
    return dict(zip(sc.PLAN_KEYS, out)) if rc == 0 else None


def _export_stream(lib, algo, n, F, d0, d1, mw):
    out = (C.c_longlong * 10)()
    rc = lib.bf_plan_das_stream(ALGOS[algo], n, F, d0, d1, mw, sc.CUS, out)
    return dict(zip(sc.PLAN_KEYS, out)) if rc == 0 else None


def test_restatement_equals_the_exports_on_random_shapes(lib):
    rng = np.random.default_rng(90)
    seen, tuples = set(), sc.all_instantiations()
    try:
        for i in range(3000):
            algo = ("pad", "lerp", "hybrid", "fir_vec")[rng.integers(0, 4)]
            N = int(rng.choice([rng.integers(1, 1025), 64, 65, 128, 129, 256, 512, 513, 1024]))
            n = int(rng.choice([rng.integers(1, 513), rng.integers(1, 64)]))
            T = int(rng.integers(1, 9)) * 8 if algo == "fir_vec" else int(rng.integers(1, 65))
            mw = int(rng.integers(0, N + 1))
            F = int(rng.choice([1, 2, 3, 8, 16, 190]))
            count = int(rng.choice([rng.integers(1, 40), rng.integers(1, 5000), rng.integers(1, 70000)]))
            assert lib.bf_configure(max(n, 1), N, 8, 1, T) == 0
            sel = sc.plan_select(algo, N, n, T, F, count, mw, False)
            assert _export_select(lib, algo, n, F, count, mw, False) == sel, (algo, N, n, T, mw, F, count)
            plans = [("select", sel, None)]
            if algo in sc.PLAIN:
                d0 = int(rng.integers(0, 300))
                st = sc.plan_stream(algo, N, n, F, count, mw)
                assert _export_stream(lib, algo, n, F, d0, d0 + count, mw) == st, (algo, N, n, mw, F, count)
                assert _export_select(lib, algo, n, F, count, mw, True) == st
                plans += [("map", st, mw), ("select_hist", st, mw)]
            else:
                assert _export_stream(lib, algo, n, F, 0, count, mw) is None and _export_select(lib, algo, n, F, count, mw, True) is None
            for kernel, p, hist_of in plans:
                if p is None:                                          # one microphone row does not fit: refused by both
                    continue
                assert (kernel, algo, p["nc"], p["dpw"]) in tuples, (kernel, algo, p)
                assert (p["dpw"] > 1) == (p["n_chunks"] > 1)
                assert p["lds"] <= sc.LDS_BYTES and p["mic_chunk"] * p["n_chunks"] >= n
                assert p["tile_dirs"] >= 1 and (p["n_tiles"] - 1) * p["tile_dirs"] < count <= p["n_tiles"] * p["tile_dirs"]
                assert p["n_chunks"] == 1 or p["tile_dirs"] <= p["waves"] * p["dpw"]       # a chunked plan never walks a second group
                if hist_of is not None:
                    assert p["lead"] >= hist_of + (1 if algo == "lerp" else 0)
                seen.add((kernel, algo, p["nc"], p["dpw"]))
        assert len(seen) >= 60, len(seen)                              # the draw is wide enough to mean something
    finally:
        util.configure("cfg1")


def test_plan_das_stream_refuses(lib):
    out = (C.c_longlong * 10)(*([-7] * 10))
    util.configure("cfg1")
    for args, text in [((ALGOS["hybrid"], 8, 1, 0, 4, 3), "continuous mode exists for pad and lerp only"),
                       ((ALGOS["pad"], 0, 1, 0, 4, 3), "empty launch"),
                       ((ALGOS["lerp"], 8, 1, 4, 4, 3), "empty launch")]:
        lib.bf_clear_error()
        assert lib.bf_plan_das_stream(*args, 256, out) == -1
        assert lib.bf_last_error().decode() == "bf_plan_das_stream: " + text and list(out) == [-7] * 10
    lib.bf_clear_error()


# ------------------------------------------------------------------ the expectations

def test_batched_checker_entry_equals_the_per_beam_one(oracle_lib):
    """oracle_miso_many is a loop over oracle_miso_pad / oracle_miso_lerp: the same bits, hostile samples included."""
    rng = np.random.default_rng(7)
    N, D, n, M = 150, 9, 6, 8
    sig = (rng.standard_normal((M, N)) * 0.25).astype(np.float32)
    sig[1, 3], sig[2, 40], sig[3, 7], sig[4, ::5] = np.nan, np.inf, np.float32(1e-41), -0.0
    mics = rng.permutation(M)[:n].astype(np.int32)
    d32 = np.float32(rng.uniform(0, 30, (D, n)))
    orc = oracle_lib.Oracle(N, D, 1, 8)
    offs = np.array([0, 5 * n, 8 * n, 5 * n, 3], dtype=np.int32)
    for a, table, one in ((0, np.floor(d32).astype(np.int32), orc.miso_pad), (1, d32, orc.miso_lerp)):
        orc.load(a, table)
        many = orc.miso_many(a, sig, mics, offs)
        for b, off in enumerate(offs):
            assert util.bits_differ(many[b], one(sig, table, mics, int(off)), nan_is_nan=True) == ""
        assert np.isnan(many).any() and np.isfinite(many).any()


@pytest.mark.parametrize("row", [r for r in sc.ROWS if "hostile" not in r.tags], ids=lambda r: r.name)
def test_expected_values_are_finite_and_positive(oracle_lib, row):
    """No comparison of the GPU file passes on NaN = NaN: a non-hostile row's accepted entries are finite and > 0, its rejected ones the quiet NaN."""
    mics, _, _, _ = sc.tables(row)
    if row.kernel == "beam":
        for hop in sc.hops(row):
            st = sc.make_stream(row, hop, True, mics)
            beams, status = sc.stream_beams(oracle_lib, row, st, sc.beam_offsets(row, 17))
            assert status.sum() == row.F and np.isfinite(beams[status == 0]).all()
            assert (np.abs(beams[status == 0]).max(axis=-1) > 0).all()
            assert (sc.beam_power(beams[status == 0], row.n, row.N) > 0).all()
        return
    if row.kernel == "map":
        _, full = sc.stream_map(oracle_lib, row)
        want = full[:, row.d0:row.d0 + row.count]
        assert want.shape == (row.F, row.count)
    else:
        want, status = sc.want_listed(oracle_lib, row)
        assert 0 < (status != 0).sum() < status.size // 8
        assert (want.view(np.uint32)[status != 0] == 0x7FC00000).all()
        want = want[status == 0]
    assert np.isfinite(want).all() and (want > 0).all()
