"""CPU: plan_das (csrc/das_plan.cpp) alone, in a stand-alone program (tests/plan_table_main.cpp) whose host side is built with
AddressSanitizer + UBSan, over a sweep of 3,290,112 launches: every algorithm, block lengths and microphone counts on both sides of every
threshold, one frame and several, grids from one direction to 130,321, tables with and without structure, two chip sizes.

The sweep reaches each of the nine kernel families (DasFamily, csrc/das_kernels.h), and where tests/batched_cases.plan restates the
routing rule independently -- sweep plans on the full chip -- every accepted launch reports the family the restatement predicts.  No
hash of the table is kept: a planner change shows here as a disagreement with the restated rule, not as a stale file."""
import os
import subprocess

import pytest

import batched_cases as BC
import util
from util import ALGOS

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = {v: k for k, v in ALGOS.items()}
LAUNCHES, REFUSED = 3290112, 387072           # the sweep's size; the vectorized FIR with 1 or 7 taps is refused
# (bf_last_das_variant, bf_last_das_rows) of the nine families, and the launcher of each (plan_table_main.cpp's numbering)
FAMILIES = {(0, 0): 0, (2, 0): 1, (3, 0): 1, (4, 0): 1, (5, 0): 2, (6, 0): 5, (7, 0): 4, (8, 1): 2, (8, 2): 3}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(rows of the restated sub-sweep, {(variant, rows): count} and (launches, refused) of the whole sweep): one sanitized run."""
    import __graft_entry__ as ge
    exe = str(tmp_path_factory.mktemp("plan_table") / "plan_table_main")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + san +
                          ["-I", ge.CSRC, os.path.join(ge.CSRC, "das_plan.cpp"), os.path.join(util.ROOT, "tests", "plan_table_main.cpp"), "-o", exe])
    symbols = subprocess.run(["nm", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "__asan_init" in symbols and "__ubsan_handle" in symbols, "the host side is not instrumented"
    r = subprocess.run([exe, "sub"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows, counts, size = [], {}, None
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] != "#":
            rows.append([int(x) for x in f[:9] + f[10:]])
        elif f[1] == "launches":
            size = (int(f[2]), int(f[4]))
        else:
            counts[(int(f[1]), int(f[2]))] = int(f[3])
    return rows, counts, size


def test_sweep_runs_clean_and_reaches_every_family(table):
    rows, counts, size = table
    assert size == (LAUNCHES, REFUSED)
    assert set(counts) == set(FAMILIES) and all(c > 0 for c in counts.values()), counts
    assert sum(counts.values()) == LAUNCHES - REFUSED
    assert len(rows) == LAUNCHES // 2 // 2 // 3


def test_families_equal_the_restated_rule(table):
    """Every accepted launch of the sub-sweep (digest_direct = 0, 256 CUs, max_whole in {12, 56, 200}): the variant and rows numbers
    of its family are what batched_cases.plan predicts, and launch_das reaches that family's launcher.  A refused launch never asks
    the restatement."""
    rows, _, _ = table
    accepted = refused = 0
    for algo, N, n, T, frames, dirs, mw, direct, n_cus, rc, *plan in rows:
        assert (direct, n_cus) == (0, 256) and mw in (12, 56, 200)
        if rc != 0:
            assert not plan
            refused += 1
            continue
        accepted += 1
        name = NAMES[algo]
        p = BC.plan(name, n, N, T, dirs, frames, min(mw, N))
        if p["layout"] == 0:
            want = (0, 0)
        elif name not in BC.PLAIN:
            want = (7 if p["pair"] else 4, 0)
        elif p["pair"]:
            want = (8, 2 if p["cells"] else 1) if name == "lerp" else (5, 0)
        else:
            want = (6 if p["long_rows"] else 2, 0)
        got = (plan[15], plan[16])
        assert got == want, (name, N, n, T, frames, dirs, mw, got, want)
        assert plan[-1] == FAMILIES[got], (name, N, n, T, frames, dirs, mw, got, plan[-1])
        if p["layout"] == 2:
            assert (plan[0], plan[1], plan[5], plan[9]) == (p["nc"], p["lead"], p["waves"], p["dpw"]), (name, N, n, T, frames, dirs, mw, plan, p)
    assert refused == REFUSED // 2 // 2 // 3 and accepted + refused == len(rows)
