"""CPU only: the instruction budget of das_pair2_kernel (csrc/das_pair.hip) around its packed arithmetic, read off the gfx950
assembly by scripts/dev/pair2_instruction_budget.py.  The kernel is bound by the instructions its SIMDs issue, so
what the compiler puts around the hand-written sweep is part of its speed.

The bounds are the necessary work plus a few instructions of slack:
  * staging of a steady-state half: the loop's branch, one wait, the row address, the part test, eight subtractions, two DPP
    moves, four stores; then the next fetch: the row base of two frames from the mic id (six scalar), two loads, the next half's
    index (three scalar) and mic id (one load) -- 31, bound 40;
  * from one mic's S2 to the next one's: 64 packed operations, 7 tests and 7 branches, and 13 more: the address, four reads and
    two waits of S1, the two table loads and at most three further scalar instructions (waits included) -- 91."""
import importlib.util
import os

import pytest

import util


@pytest.fixture(scope="module")
def budget():
    spec = importlib.util.spec_from_file_location("pair2_instruction_budget", os.path.join(util.ROOT, "scripts", "dev", "pair2_instruction_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    b = m.budget()
    print(m.report(b))
    return b


def test_staging_path_of_a_steady_state_half(budget):
    st = budget["staging"]
    assert st is not None, "no BF_STAGE_BEGIN / BF_STAGE_END path in das_pair2_kernel"
    assert sum(t.startswith("ds_write_b128") for t in st) == 4 and sum(t.startswith("global_load_dwordx4") for t in st) == 2, st   # the path is the staging
    assert len(st) <= 40, len(st)


def test_from_one_mic_to_the_next(budget):
    gaps = budget["gaps"]
    assert len(gaps) == 7          # eight mics of a half, unrolled
    for g in gaps:
        assert g["packed"] == 64, g
        assert g["test/branch"] <= 14, g
        assert sum(g.values()) - g["packed"] - g["test/branch"] <= 13, g
        assert g["lds"] == 4 and g["vector"] == 1 and g["table load"] <= 2, g
        assert g["scalar"] + g["wait"] - 2 <= 3, g          # beyond S1's two waits
        assert sum(g.values()) <= 64 + 14 + 13, g


def test_registers_and_spills(budget):
    r = budget["resources"]
    assert r["scratch"] == 0
    assert r["vgprs"] <= 128
    assert r["sgpr_spills"] <= 27
    assert budget["lane_spills"] == 0       # no SGPR spill or reload between the half loop's barriers
