"""CPU only: the instruction budget of the k-ordered mean-power pass of das_pair2_kernel (csrc/das_pair.hip), section (d) of
scripts/dev/pair2_instruction_budget.py, read off the gfx950 assembly of the power-of-two path.

Parking, per wave and group of 128 directions, both rounds together.  The necessary work:
  * 64 packed multiplies: 32 register pairs (8 directions x 4 samples, a pair being frames 0 and 1) times the mean and the square;
  * 32 eight-byte stores: 8 directions x 2 frames x 2 rounds, a lane's two samples of a half row each (ds_write2_b32: the two floats
    of a frame sit in two register pairs);
  * addresses: the store's offsets are 8 bits of dwords and reach two rows of 132 floats, so a round needs 8 addresses (4 pairs of
    rows x 2 frames): the lane id (2), the first address (2) and 7 adds -- 11 a round, 22;
  * which waves sum, and that a round's lanes are inside the tile and the frame exists, is decided before the barrier or behind it
    as the compiler likes: at most the wave test, the frame test and their branch in each round -- 8 scalar or branch instructions;
  * the initial value of the running sum: 1.
That is 127; the bound is 135.  No plain v_mul_f32 (the parent's 128) may come back.

The ordered sum: two loops (one a round), each a trip of 32 samples: 8 reads of 16 bytes, 32 v_add_f32, one wait per pair of reads --
and none of them a full one (lgkmcnt(0)): inside the loop the chain never sits through an LDS round trip; only the drain behind it
counts down to 0."""
import importlib.util
import os

import pytest

import util


@pytest.fixture(scope="module")
def power():
    spec = importlib.util.spec_from_file_location("pair2_instruction_budget", os.path.join(util.ROOT, "scripts", "dev", "pair2_instruction_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    b = m.budget()
    print(m.report(b))
    assert b["power"] is not None, "no BF_POWER_POW2 / BF_POWER_END markers in das_pair2_kernel"
    return b["power"]


def test_barriers_of_the_pass(power):
    assert power["barriers"] == 3          # parked, summed, parked; the fourth is the group's first


def test_parking_of_both_rounds(power):
    p = power["parking"]
    assert p["packed multiply"] == 64, p
    assert p["multiply"] == 0, p
    assert p["lds store"] == 32 and p["lds read"] == 0, p
    assert p["wait"] == 0, p               # nothing is waited for between the sweep's last barrier and the stores
    assert p["vector"] <= 22 + 1 + 2, p
    assert p["scalar"] + p["test/branch"] <= 8 + 4, p
    assert sum(p.values()) <= 135, p


def test_ordered_sum_loops_never_wait_for_everything(power):
    loops = power["loops"]
    assert len(loops) == 2, loops
    for lp in loops:
        assert lp["reads"] == 8 and lp["adds"] == 32, lp
        assert len(lp["waits"]) <= 8 and lp["waits"], lp
        assert 0 not in lp["waits"], lp
