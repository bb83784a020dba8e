"""CPU only: the wave priorities of das_pair2_kernel and das_pair_kernel (csrc/das_pair.hip), read off the gfx950 assembly that
scripts/dev/pair2_instruction_budget.py compiles.

The four waves of a SIMD issue by priority, then by age, so at one priority they finish every half of the sweep as a staircase and
the youngest runs the end of each half alone.  The kernel therefore keys the priority to progress -- the ladder:
  * 3 from the half loop's barrier on, before the staging's first store;
  * 2, 1 and 0 at the start of mic 2, 4 and 6 of the unrolled half, never between a mic's two statements (`;BF_S1_END` to
    `;BF_S2_BEGIN`, where the hard-wired quads are in flight) and never inside the second one;
  * 0 once more behind the half loop: a wave without directions of its own keeps 3 from barrier to barrier (it stages and
    waits), and every wave enters the mean-power pass at priority 0.
What the statements cost is held by tests/test_pair2_budget_host.py; this file holds where they are.
das_pair_kernel (pad), whose mics run as two trips of three and two more, has the ladder at that grain: 3 from the barrier on, 1
behind either trip, 0 before the last two mics and behind the half loop.

The checks walk the kernel's control-flow graph (the tool's own parser: instructions, markers, branch targets) with a small set of
states per instruction instead of enumerating paths -- the 56 out-of-line re-read stubs of a half would make 2^56 of them."""
import importlib.util
import os
import re

import pytest

import util


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("pair2_instruction_budget", os.path.join(util.ROOT, "scripts", "dev", "pair2_instruction_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def asm(tool):
    return tool.compile_asm()


@pytest.fixture(scope="module")
def graph(tool, asm):
    items, labels = tool.parse(tool.kernel_lines(asm))
    return items, labels


@pytest.fixture(scope="module")
def pad_graph(tool, asm):
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN\S*das_pair_kernel\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return tool.parse(lines[start + 1:end])


def _prio(it):
    """the immediate of an s_setprio instruction, None for anything else"""
    m = re.match(r"s_setprio\s+(\d+)$", it.get("text", ""))
    return int(m.group(1)) if m else None


def _succ(items, labels, i):
    it = items[i]
    out = [] if it["next"] is None else [it["next"]]
    return out + [labels[t] for t in it["targets"] if t in labels]


def _flow(items, labels, starts, step, stop=lambda it: False):
    """States reaching every item: a fixed point of `step(state, item) -> state` over the graph, from `starts` = {item: state};
    an item for which `stop` holds receives states and passes none on.  -> {item index: set of states on arrival}"""
    seen = {}
    work = list(starts.items())
    while work:
        i, st = work.pop()
        if st in seen.setdefault(i, set()):
            continue
        seen[i].add(st)
        if stop(items[i]):
            continue
        nxt = step(st, items[i])
        work += [(s, nxt) for s in _succ(items, labels, i)]
    return seen


def _is_barrier(it):
    return it.get("text") == "s_barrier"


def _ladders(items, labels):
    """From every barrier to the next: the priorities a wave sets on the way, a run of equal ones counted once (a loop sets its
    own again on every trip).  -> (sequences arriving at the next barrier from the barriers behind which a 3 is set, how many
    such barriers there are, {sequence on arrival} of every ds_write_b128 behind such a barrier once the 3 is set)"""
    arrivals, stores, entered = set(), set(), 0

    def step(seq, it):
        p = _prio(it)
        return seq if p is None or seq[-1:] == (p,) else seq + (p,)
    for b in [i for i, it in enumerate(items) if _is_barrier(it)]:
        seen = _flow(items, labels, {s: () for s in _succ(items, labels, b)}, step, stop=_is_barrier)
        ends = {seq for i, sts in seen.items() if _is_barrier(items[i]) for seq in sts}
        if not any(3 in seq for seq in ends):
            continue                                    # not a barrier that leads into a half
        entered += 1
        arrivals |= ends
        for i, sts in seen.items():
            if items[i].get("text", "").startswith("ds_write_b128"):
                stores |= {seq for seq in sts if 3 in seq}
    return arrivals, entered, stores


def test_the_ladder_of_a_half(graph):
    """From each barrier that leads into a half (the one before the first half and the loop's own) to the next barrier: a wave
    sets 3, 2, 1, 0 (the sweep) or 3 alone (no directions of its own), or leaves the loop and sets 0; the 3 precedes every
    staging store and the staging markers."""
    items, labels = graph
    arrivals, entered, stores = _ladders(items, labels)
    print("das_pair2_kernel, priorities from a half's barrier to the next:", sorted(arrivals))
    assert entered == 2, entered
    assert arrivals == {(3, 2, 1, 0), (3,), (0,)}, arrivals
    assert stores == {(3,)}, stores
    seen = _flow(items, labels, {0: None}, lambda st, it: st if _prio(it) is None else _prio(it))
    begins = [i for i, it in enumerate(items) if it.get("marker") == "BF_STAGE_BEGIN"]
    assert begins and all(seen.get(i) == {3} for i in begins), [seen.get(i) for i in begins]


def test_the_pad_kernels_ladder_of_a_half(pad_graph):
    """das_pair_kernel: 3, 1, 0 (the sweep), 3 alone (no directions of its own), or 0 on leaving the loop; staged at 3."""
    items, labels = pad_graph
    arrivals, entered, stores = _ladders(items, labels)
    print("das_pair_kernel, priorities from a half's barrier to the next:", sorted(arrivals))
    assert entered == 2, entered
    assert arrivals == {(3, 1, 0), (3,), (0,)}, arrivals
    assert stores and stores == {(3,)}, stores


def test_the_pad_kernel_ends_and_sums_at_priority_zero(pad_graph):
    """das_pair_kernel has no markers around its power pass: only the half loop's own barrier is reached at another priority
    than 0 (by the waves that skipped the sweep), and the kernel ends at 0."""
    items, labels = pad_graph
    seen = _flow(items, labels, {0: 0}, lambda st, it: st if _prio(it) is None else _prio(it))
    high = [i for i, it in enumerate(items) if _is_barrier(it) and seen.get(i, set()) - {0}]
    assert len(high) == 1 and seen[high[0]] == {0, 3}, [(i, seen[i]) for i in high]
    ends = [i for i, it in enumerate(items) if it.get("text") == "s_endpgm"]
    assert ends and all(seen.get(i, {0}) == {0} for i in ends)


def test_no_priority_change_while_the_quads_are_in_flight(tool, asm):
    """None between `;BF_S1_END` and `;BF_S2_BEGIN`, none inside the second statement (its out-of-line stubs included)."""
    where, n_s2 = None, 0
    for line in tool.kernel_lines(asm):
        l = line.strip()
        if "BF_S1_END" in l:
            where = "between"
        elif "BF_S2_BEGIN" in l:
            where, n_s2 = "s2", n_s2 + 1
        elif l.startswith(";;#ASMEND") and where == "s2":
            where = None
        elif where is not None:
            assert not l.split(";")[0].strip().startswith("s_setprio"), (where, n_s2, l)
    assert n_s2 == 8 and where is None


def test_every_wave_enters_the_power_pass_at_priority_zero(graph):
    """The last s_setprio before either power pass, on every path from the kernel's entry, sets 0 (none at all: the priority a
    wave starts with)."""
    items, labels = graph
    seen = _flow(items, labels, {0: 0}, lambda st, it: st if _prio(it) is None else _prio(it))
    passes = [i for i, it in enumerate(items) if it.get("marker") in ("BF_POWER_POW2", "BF_POWER_DIV")]
    assert len(passes) == 2
    for i in passes:
        assert seen.get(i) == {0}, (items[i], seen.get(i))
    assert any(_prio(it) == 3 for it in items)          # (the walk did see the ladder)


def test_no_other_kernel_sets_a_priority(tool, asm):
    """The unit's two kernels have five and four, and no other delay-and-sum unit's source names the instruction."""
    inside = None
    counts = {}
    for l in asm.split("\n"):
        m = re.match(r"(_Z\w+):", l)
        if m:
            inside = m.group(1)
        elif l.startswith(".Lfunc_end"):
            inside = None
        elif inside and l.split(";")[0].strip().startswith("s_setprio"):
            counts[inside] = counts.get(inside, 0) + 1
    assert sorted((("das_pair2_kernel" in k, n) for k, n in counts.items())) == [(False, 4), (True, 5)], counts
    assert all("das_pair_kernel" in k or "das_pair2_kernel" in k for k in counts), counts
    for name in ("das_kernels.hip", "das_strided.hip", "remove_sources.hip", "das_device.h", "das_geometry.h"):
        assert "s_setprio" not in open(os.path.join(tool.CSRC, name)).read(), name
