"""Rows for test_pair_block_lengths.py (GPU) and test_pair_cases_host.py (CPU): the four two-frame ("pair") delay-and-sum kernels at
every block length they take, and at the microphone counts where their code takes another path.  A row is (case, algorithm) with the
family (bf_last_das_variant) and the row layout (bf_last_das_rows) it has to reach; the data, tables and the restated routing rule are
those of tests/batched_cases.py, which draws a case's data from its name.
TEST INFRASTRUCTURE ONLY.

  das_pair_kernel          pad, family 5                 halves of 8 microphones
  das_pair2_kernel         lerp, family 8, rows 1        halves of 8
  das_pair2_cells_kernel   lerp, family 8, rows 2        halves of 16, microphone counts that are a multiple of 32
  das_hybrid_pair_kernel   hybrid / fir_naive / fir_vec, family 7, halves of 16

Every table is smooth with pmax = 30 (the fixed 56-sample prefix then holds for every algorithm: hybrid looks back max_whole + 6), on
a 17 x 16 grid unless said otherwise: 272 directions are 16 waves, two whole groups of 128 and a ragged one of 16.  (The ORDERED rows:
folded tables on 13 x 21, whose sweep order is not the identity.)  Every frame has more rows than active microphones; the cases whose
N is an odd multiple of 4 take their rows from last to first.

Block lengths: the pair kernels take N % 4 == 0 with 128 < N <= 256, 32 lengths.  What depends on N is hand-written: the staging masks
(4 * lane < N; 128 + l, 192 + l, 129 + l, 193 + l < N on cell rows) and the drains of the two lerp kernels' power pass
(add_in_order_rolling, csrc/das_device.h; add_in_order_linear, csrc/das_cells.hip), whose round 1 sums (N - 128) / 4 quads and
leaves by one of eight exits, entered behind a trip of the loop or without one: drain(N)."""
import collections

import batched_cases as BC

LENGTHS = tuple(range(132, 257, 4))                 # every block length the pair kernels take
SHORT = tuple(range(132, 161, 4))                   # round 1 of the lerp power pass enters its drain without a trip of the loop
MANY = (256, 252)                                   # the lengths of the microphone-count rows
GRID, PMAX, T = (17, 16), 30.0, 8

Row = collections.namedtuple("Row", "case algo family rows")

CASES, ROWS = [], []


def _add(name, M_total, n, N, algos, family, cells=False, F=3, grid=GRID, reversed_rows=None, kind="smooth"):
    """One case and its rows.  family: one number or one per algorithm; cells: lerp runs on cell rows."""
    rev = N % 8 == 4 if reversed_rows is None else reversed_rows
    c = BC.Case(name, family, algos, M_total, n, N, grid[0], grid[1], T, PMAX, kind, "reversed" if rev else "sorted", F)
    assert name not in BC.BY_NAME and name not in BC.EXTRA, name
    BC.EXTRA[name] = c
    CASES.append(c)
    for a in algos:
        fam = BC.family_of(c, a)
        ROWS.append(Row(name, a, fam, (2 if cells else 1) if fam == 8 else 0))


# ---- block lengths: 16 of 20 microphones (pad 5, lerp 8 on rows of sample pairs) and 32 of 40 (lerp 8 on cell rows, the FIRs 7).  Three
# frames: the last workgroup row computes its frame twice.
for _N in LENGTHS:
    _add("len%d_16of20" % _N, 20, 16, _N, BC.PLAIN, {"pad": 5, "lerp": 8})
    _add("len%d_32of40" % _N, 40, 32, _N, ("lerp",) + BC.FIRS, {"lerp": 8, "hybrid": 7, "fir_naive": 7, "fir_vec": 7}, cells=True)
# two frames, no workgroup row with one frame, where round 1 is the drain alone: one exit each
for _N in SHORT:
    _add("len%d_16of20_f2" % _N, 20, 16, _N, ("lerp",), 8, F=2)
    _add("len%d_32of40_f2" % _N, 40, 32, _N, ("lerp",), 8, cells=True, F=2)
# the neighbours on either side leave the pair kernels: two chunks of 64 samples take the strided kernel, N % 4 != 0 the one-frame sweep,
# two segments the long rows
_add("edge128", 20, 16, 128, BC.PLAIN, 0)
_add("edge130", 20, 16, 130, BC.PLAIN, 2)
_add("edge260", 20, 16, 260, BC.PLAIN, 6)
# a sweep order that is not the identity (ORDERED): on a 13 x 21 grid whose delays start over at every row end, the pad / lerp pair kernels
# sweep every other row backwards and their summing waves store through the order -- here into a shard with padded image rows
_add("order13x21_16of20", 20, 16, 252, BC.PLAIN, {"pad": 5, "lerp": 8}, grid=(13, 21), kind="folded")
_add("order13x21_32of40", 40, 32, 256, ("lerp",), 8, cells=True, grid=(13, 21), kind="folded", reversed_rows=True)

# ---- microphone counts.  das_pair_kernel and das_hybrid_pair_kernel keep the microphone ids of the first 64 halves in a register and
# load those of the halves beyond; das_copies_kernel does the same per chunk; the cells kernel wraps to half 0 an iteration ahead.
for _N in MANY:
    _add("mics528_n%d" % _N, 536, 528, _N, ("pad",), 5)                                  # 66 halves of 8
    _add("mics1040_n%d" % _N, 1048, 1040, _N, ("hybrid", "fir_vec"), 7)                   # 65 halves of 16
    for _n in (128, 160, 256):                                                            # 8, 10 (the mean divides) and 16 halves of 16
        _add("cells%d_n%d" % (_n, _N), _n + 8, _n, _N, ("lerp",), 8, cells=True)
# four segments off the long-row path (261 is no multiple of the half of 4): das_copies_kernel walks 66 chunks of 4, the last of one microphone
_add("chunks66_n1024", 270, 261, 1024, ("lerp",), 2, grid=(9, 8), reversed_rows=True)

BY_NAME = {c.name: c for c in CASES}
IDS = ["%s-%s" % (r.case, r.algo) for r in ROWS]

# the rows that enter code no smaller count reaches
MANY_MICS = [r for r in ROWS if r.case.startswith(("mics", "cells", "chunks"))]
BLOCK_LENGTHS = [r for r in ROWS if r.case.startswith(("len", "edge", "order"))]
ORDERED = [r for r in ROWS if r.case.startswith("order")]
MANY_HALVES = {"mics528_n256": 66, "mics528_n252": 66, "mics1040_n256": 65, "mics1040_n252": 65}      # halves of das_pair_kernel (8) / das_hybrid_pair_kernel (16)
MANY_CHUNKS = {"chunks66_n1024": 66}                                                                    # chunks of das_copies_kernel


def kernel_of(row):
    return {5: "das_pair_kernel", 7: "das_hybrid_pair_kernel"}.get(row.family) or \
        {1: "das_pair2_kernel", 2: "das_pair2_cells_kernel"}.get(row.rows)


def drain(N):
    """(exit, trip) of round 1 of a lerp pair kernel's power pass at block length N: it sums q = (N - 128) / 4 quads, in trips of 8
    while more than 8 are left; the drain then ends behind quad 1 .. 7 (BF_*_DONE(1 .. 7)) or falls through (8)."""
    q = (N - 128) // 4
    assert 128 < N <= 256 and N % 4 == 0
    return (q - 1) % 8 + 1, q > 8


def drain_table():
    """(kernel, exit, trip) -> the rows that take it, for the two lerp pair kernels."""
    t = {}
    for r in ROWS:
        if r.family == 8:
            t.setdefault((kernel_of(r),) + drain(BY_NAME[r.case].N), []).append(r)
    return t
