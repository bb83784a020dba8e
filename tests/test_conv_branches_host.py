"""CPU: the convolutions' launch planner (plan_conv2d in csrc/conv_kernels.hip, through bf_plan_conv2d) against tests/conv_cases.py.

  * the ladder of conv_cases.find_shape reaches every row of the table at 256 compute units (the MI355X), inside the caps, with live edges;
  * the set of branches the planner returns -- on the table's layers and on a sweep of random legal layers under every setting of the two
    process switches -- equals the table: a branch the table lacks fails here, and so does a table entry nothing reaches;
  * the rows keep the variety the GPU test relies on (slices, residuals, missing bias, both store epilogues, the concatenation's entries);
  * invariants of every plan, and the tile picker's own definition restated: the cost of the tile returned is the least among the allowed shapes.

The A/B environment switches ($BF_CONV_ROW, $BF_CONV_TAP, $BF_CONV_PATCH) are read once per process; the table describes the library with
none of them set, and the plan reports what the process read."""
import random

import pytest

import conv_cases as cc
from support import lib

CUS = 256


def _check_plan(p, eb, M, N, ldy, has_res, ldr, misaligned, n_cus):
    """What must hold of any plan (list of 16) for a layer of M pixels x N channels."""
    b = cc.branch_of(p)
    E = 16 // eb
    assert b.eb == eb and b.family in (cc.REG, cc.DMA, cc.PATCH)
    assert p[12:15] == [0, 1, -1], "BF_CONV_ROW / BF_CONV_TAP / BF_CONV_PATCH are set: the branch table describes the library without them"
    assert p[15] == n_cus
    assert p[9] * b.bm >= M and p[10] * b.bn >= N and p[9] >= 1 and p[10] >= 1
    if b.family != cc.PATCH:
        assert (p[9] - 1) * b.bm < M and (p[10] - 1) * b.bn < N            # no workgroup without work
    assert (b.bn == 32) == (N <= 32)
    assert not (b.cpr == 8 and (b.split or eb == cc.F32))
    assert not (b.fast_tap and b.cat)
    assert not (b.split and (eb != cc.F32 or b.family != cc.DMA))
    assert (p[11] > 0) == (b.family == cc.PATCH) and p[11] <= 64 * 1024
    wide = N % E == 0 and ldy % E == 0 and not (misaligned & 8) and (not has_res or (ldr % E == 0 and not (misaligned & 16)))
    assert b.wide == int(wide)
    return b


def _tile_cost(bm, bn, M, N, n_cus, thin):
    wgs = -(-M // bm) * -(-N // bn)
    return float(-(-wgs // n_cus)) * bm * bn * (1.0 + thin / bm + thin / bn)


def _check_tile_is_cheapest(b, M, N, n_cus):
    """The picker's definition (the comment on pick_dma_tile): among the shapes the output allows -- 32-channel tiles for up to 32 channels and
    only for those -- the one with the least ceil(workgroups / CUs) x area x (1 + thin / rows + thin / columns); thin = 8 beside the float32
    matrix instruction, 160 beside the float16 and bfloat16 ones."""
    thin = 8.0 if (b.eb == cc.F32 and not b.split) else 160.0
    allowed = [t for t in cc.TILES if (t[1] == 32) == (N <= 32)]
    assert (b.bm, b.bn) in allowed
    mine = _tile_cost(b.bm, b.bn, M, N, n_cus, thin)
    assert all(mine <= _tile_cost(bm, bn, M, N, n_cus, thin) for bm, bn in allowed), (b, M, N, n_cus)


def _found(lib, n_cus):
    return {r.index: cc.find_shape(lib, r, n_cus) for r in cc.ROWS}


@pytest.fixture(scope="module")
def found(lib):
    return _found(lib, CUS)


def test_the_table_names_each_branch_once():
    assert len(set(cc.BRANCHES)) == len(cc.BRANCHES) == 142
    assert {r.branch for r in cc.ROWS} == set(cc.BRANCHES)
    assert len({r.id for r in cc.ROWS}) == len(cc.ROWS)
    # every conv_dma_kernel instantiation the default build can launch: 5 tiles x kCat x (float16 64-byte, float32 native, float32 split) + 4 tiles x kCat x 128-byte rows
    inst = {(b.eb, b.bm, b.bn, b.cpr, b.cat, b.split) for b in cc.BRANCHES if b.family == cc.DMA}
    assert len(inst) == 5 * 2 * 3 + 4 * 2


def test_the_ladder_finds_every_row_inside_the_caps(lib, found):
    missing = [r.id for r in cc.ROWS if found[r.index] is None]
    assert not missing, missing
    for r in cc.ROWS:
        (B, H, W), p = found[r.index]
        ho, wo = r.out_hw(H, W)
        M = B * ho * wo
        assert cc.in_caps(r, B, H, W) and M * r.n * r.K <= cc.MAX_MNK
        b = _check_plan(p, r.branch.eb, M, r.n, r.ldy, r.residual, r.n, 0, CUS)
        assert b == r.branch, r.id
        assert M % b.bm != 0 and M > b.bm and r.n % b.bn != 0, r.id            # a ragged last tile both ways, more than one row of tiles
        if b.family == cc.DMA:
            _check_tile_is_cheapest(b, M, r.n, CUS)


def test_a_row_nothing_reaches_and_a_missing_row_are_noticed(lib, found):
    """The two ways the table can drift from the planner, tried once each on copies: 128-byte rows with the split do not exist, so the ladder
    finds no shape for such a row; and a table without its 64 x 128 float16 entries is smaller than the set of branches the planner returns on
    the shapes found (the sweep of test_random_legal_layers_stay_inside_the_table meets such a branch on layers of its own)."""
    ghost = cc.Row(cc.Branch(cc.F32, cc.DMA, 128, 128, 8, 1, 1, 0, 1), 512, 200, 1, 1, 0, "dense")
    ghost.index, ghost.sliced, ghost.residual, ghost.bias, ghost.silu = 999, False, False, True, True
    assert cc.find_shape(lib, ghost, CUS) is None
    fewer = set(cc.BRANCHES) - {b for b in cc.BRANCHES if (b.eb, b.bm, b.bn) == (cc.F16, 64, 128)}
    seen = {cc.branch_of(found[r.index][1]) for r in cc.ROWS}
    assert seen - fewer and seen == set(cc.BRANCHES)


def test_the_rows_keep_their_variety():
    rows = cc.ROWS
    for tile in cc.TILES:
        mine = [r for r in rows if r.branch.family == cc.DMA and (r.branch.bm, r.branch.bn) == tile]
        for eb in (cc.F16, cc.F32):
            assert {(r.sliced, r.residual) for r in mine if r.branch.eb == eb} >= {(True, True), (True, False), (False, True), (False, False)}, (tile, eb)
    for fam in (cc.REG, cc.DMA, cc.PATCH):
        assert any(not r.bias for r in rows if r.branch.family == fam) and any(r.bias for r in rows if r.branch.family == fam)
        assert {r.branch.wide for r in rows if r.branch.family == fam} == {0, 1}
    for r in rows:
        assert (r.n % r.E == 0) == bool(r.branch.wide) and r.ldy >= r.n and (r.ldy > r.n) == r.sliced
        assert (r.ldy % r.E == 0) or not r.branch.wide
    for b in cc.BRANCHES:
        mine = [r for r in rows if r.branch == b]
        if b.family == cc.DMA and b.cat:
            assert {r.src for r in mine} == {"dense", "two", "up"}, b
            for r in mine:
                if r.src != "dense":                      # the sources meet on an edge of the stage this kernel walks
                    assert r.c1 % (b.cpr * r.E) == 0 and 0 < r.c1 < r.c
            if b.eb == cc.F16 and b.cpr == 4 and b.bn >= 64:   # ... and where 128-byte rows were due, a first source that is no whole number of them
                assert any(r.note == "c1-off-row" and r.c1 % (8 * r.E) != 0 and r.c1 % (4 * r.E) == 0 and r.K >= 512 and r.n >= 128 for r in mine), b
        if b.family == cc.REG and b.cat:
            assert any(r.src == "two" and r.dma == 1 and r.c1 % (4 * r.E) != 0 for r in mine), b
    off = [r for r in rows if r.branch.family == cc.DMA and not r.branch.cat and not r.branch.fast_tap]
    assert any(r.c // r.E < 4 for r in off) and any(r.kh * r.kw > 32 for r in off)


@pytest.mark.parametrize("n_cus", [32, 304])
def test_other_compute_unit_counts_give_consistent_plans(lib, n_cus):
    """The shapes move with the device (the picker's ceiling), the branches do not: whatever the ladder finds is the row's branch with a
    consistent plan, and every row is found but those of the 64 x 128 tile, whose windows are one 64-pixel tile wide."""
    got = _found(lib, n_cus)
    for r in cc.ROWS:
        if got[r.index] is None:
            assert (r.branch.bm, r.branch.bn) == (64, 128), r.id
            continue
        (B, H, W), p = got[r.index]
        ho, wo = r.out_hw(H, W)
        b = _check_plan(p, r.branch.eb, B * ho * wo, r.n, r.ldy, r.residual, r.n, 0, n_cus)
        assert b == r.branch
        if b.family == cc.DMA:
            _check_tile_is_cheapest(b, B * ho * wo, r.n, n_cus)
    assert sum(v is not None for v in got.values()) >= len(cc.ROWS) - 8


def _random_layer(rng):
    """A layer the entry points take -> (arguments of bf_plan_conv2d up to `misaligned`, M)"""
    eb = rng.choice((cc.F16, cc.F32))
    E = 16 // eb
    c = rng.choice((4, 8, 8, 16, 32, 32, 64, 64, 128, 256, 512, 1024))
    kh, kw = rng.choice(((1, 1), (1, 1), (3, 3), (3, 3), (2, 2), (4, 4), (6, 6), (5, 5), (1, 16), (3, 1), (4, 8), (6, 2)))
    stride, pad = rng.choice((1, 1, 2)), rng.choice((0, 1, 2))
    W = rng.randint(max(1, kw - 2 * pad), 140)
    if c < E:
        stride, pad, W = 2, rng.choice((0, 2)), W + (W & 1)
        if (kw * c) % E:
            kw += 1
        W = max(W, kw + (kw & 1))
    H = rng.randint(max(1, kh - 2 * pad), 140)
    B = rng.choice((1, 1, 2, 3, 8))
    n = rng.choice((rng.randint(1, 32), rng.randint(33, 127), rng.randint(128, 700), 128, 256, 64, 32))
    ldy = n + rng.choice((0, 0, E, 3))
    has_res = rng.random() < 0.3
    ldr = n + rng.choice((0, E, 1)) if has_res else 0
    mis = rng.choice((0, 0, 0, 8, 16, 24))
    c1, ld1, up1, has_x2, ld2 = c, c, 0, 0, 0
    if (kh, kw, stride, pad) == (1, 1, 1, 0) and c >= 2 * E and rng.random() < 0.6:
        c1 = E * rng.randint(1, c // E)
        ld1 = c1 + E * rng.choice((0, 1, 3))
        has_x2 = int(c1 < c or rng.random() < 0.3)
        ld2 = (c - c1) + E * rng.choice((0, 2)) if c1 < c else 0
        up1 = int(rng.random() < 0.3)
        if up1:
            H, W = H + (H & 1), W + (W & 1)
    ho, wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    return (eb, B, H, W, c, n, kh, kw, stride, pad, ldy, int(has_res), ldr, c1, ld1, up1, has_x2, ld2, mis), B * ho * wo


def test_random_legal_layers_stay_inside_the_table(lib):
    import ctypes as C
    rng = random.Random(20240607)
    seen = set()
    for _ in range(6000):
        args, M = _random_layer(rng)
        dma, mode, n_cus = rng.choice((0, 1, 1, 1, 2)), rng.choice((0, 1)), rng.choice((32, 104, 256, 304))
        out = (C.c_longlong * cc.OUT_LEN)()
        assert lib.bf_plan_conv2d(*args, dma, mode, n_cus, out) == 0, (args, lib.bf_last_error())
        p = list(out)
        eb, n, ldy, has_res, ldr, mis = args[0], args[5], args[10], args[11], args[12], args[18]
        b = _check_plan(p, eb, M, n, ldy, has_res, ldr, mis, n_cus)
        assert b in set(cc.BRANCHES), (b, args)
        kh, kw, stride, pad = args[6:10]
        assert b.cat == int(args[16] or args[15] or args[14] != args[4] or (kh, kw, stride, pad) == (1, 1, 1, 0))
        if dma == 0:
            assert b.family == cc.REG
        if b.family == cc.PATCH:
            assert args[4] == 4 and n <= 32 and (eb == cc.F16 or dma == 2)
        if b.family == cc.DMA:
            assert b.split == (mode if eb == cc.F32 else 0)
            _check_tile_is_cheapest(b, M, n, n_cus)
        seen.add(b)
    assert len(seen) > 100                                # (the sweep reaches most of the table by itself; the ladder reaches all of it)
