"""CPU only: what the compiler puts around the hand-written sweep of das_pair2_cells_kernel (csrc/das_cells.hip), read off the
gfx950 assembly by scripts/dev/pair2_instruction_budget.py (budget_cells) and scripts/dev/check_inflight_copies.py (scan_cells).
The kernel is bound by the instructions its SIMDs issue, and its hard-wired cells are sound only in a build that
does not spill and copies no register with a read in flight.

The bounds are the necessary work plus a few instructions of slack:
  * staging of a steady-state half (one mic per wave, N = 256): the loop's branch, the two tests of N == 256 and the wait for the
    loads (4); per frame three lanes read, three moves of them, four DPP moves and four subtractions (28); the row address and four
    stores (5); then the next fetch: the row base of two frames from the mic id (six scalar), the two clamped lane offsets (4), eight
    loads, the next half's index (three scalar), its mic id (one load) and the row to stage next (1) -- 60.  The DPP moves and the
    lane reads need their operands two instructions old: up to 10 s_nop where nothing else fits.  Bound 76.
  * from one mic's S2 to the next one's: 64 packed operations, 7 tests and 7 branches, and 13 more: the address, four reads and two
    waits of S1, the two table loads and at most three further scalar instructions (waits and the ladder's s_setprio included) -- 91,
    das_pair2_kernel's own bound.
"""
import importlib.util
import os
import re

import pytest

import util


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(util.ROOT, "scripts", "dev", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def budget():
    m = _load("pair2_instruction_budget")
    b = m.budget_cells()
    print(m.report(b))
    print("ladder %s, in flight %s, entering the power pass at %s, barriers in the half loop %s" %
          (b["ladder"], b["prio_in_flight"], sorted(b["power_entry"]), b["loop_barriers"]))
    return b


def test_staging_path_of_a_steady_state_half(budget):
    st = budget["staging"]
    assert st is not None, "no BF_STAGE_BEGIN / BF_STAGE_END path in das_pair2_cells_kernel"
    assert sum(t.startswith("ds_write_b128") for t in st) == 4, st                 # whole cells, 16 bytes per lane
    assert sum(t.startswith("ds_write") for t in st) == 4, st
    assert sum(t.split()[0] == "global_load_dword" for t in st) == 8, st           # lane l: s f[l + 64 q], through the scalar base
    assert sum(t.startswith(("global_load", "buffer_load", "flat_load")) for t in st) == 8, st
    assert all(re.search(r",\s*s\[\d+:\d+\]", t) for t in st if t.startswith("global_load")), st     # the scalar base, no 64-bit lane pointer
    assert sum(t.startswith("s_barrier") for t in st) == 0
    assert len(st) <= 76, len(st)


def test_from_one_mic_to_the_next(budget):
    gaps = budget["gaps"]
    assert len(gaps) == 15         # sixteen mics of a half, unrolled
    for g in gaps:
        assert g["packed"] == 64, g
        assert g["test/branch"] <= 14, g
        assert g["lds"] == 4 and g["vector"] == 1 and g["table load"] <= 2, g
        assert g["scalar"] + g["wait"] - 2 <= 3, g          # beyond S1's two waits
        assert sum(g.values()) - g["packed"] - g["test/branch"] <= 13, g
        assert sum(g.values()) <= 64 + 14 + 13, g


def test_registers_and_spills(budget):
    r = budget["resources"]
    assert r["scratch"] == 0
    assert r["vgprs"] <= 128
    assert budget["lane_spills"] == 0       # no SGPR spill or reload between the half loop's barriers
    assert budget["loop_barriers"] == 1     # one barrier per 16 mics


def test_the_ladder(budget):
    assert budget["ladder"] == [(3, 0), (2, 4), (1, 8), (0, 12)]     # (priority, mics swept before it)
    assert budget["prio_in_flight"] == []                            # never between a mic's two statements
    assert budget["power_entry"] == {0}                              # every wave enters either power pass at 0


def test_power_pass_keeps_its_shape(budget):
    p = budget["power"]
    assert p is not None and p["barriers"] == 3
    assert p["parking"]["lds store"] == 32 and p["parking"]["packed multiply"] == 64, p["parking"]
    assert len(p["loops"]) == 2
    for lp in p["loops"]:
        assert lp["reads"] == 8 and lp["adds"] == 32 and 0 not in lp["waits"], lp      # strict k order, no full wait inside the loop


def test_no_copy_of_a_register_with_a_read_in_flight():
    r = _load("check_inflight_copies").scan_cells()
    assert r["kernels"] == 1
    assert r["bad"] == [], r["bad"][:5]
    assert r["pairs"] == 16 and r["gaps"] == [], r["gaps"][:5]      # nothing between S1 and S2 touches v96..v120
    assert r["spills"] == {}, r["spills"]
