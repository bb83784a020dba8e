"""Static instruction budget of das_pair2_kernel (csrc/das_pair.hip): what a wave issues around the packed arithmetic.

Compiles the unit to gfx950 assembly with the build's flags (HIPCC_FLAGS of __graft_entry__.py) and reports, for das_pair2_kernel:
  (a) the instructions on the staging path of one steady-state half (1 <= h, h + 2 < n_half, part == 1, N == 256): the longest path
      through the control-flow graph from the source's `;BF_STAGE_BEGIN` marker to `;BF_STAGE_END` that passes none of the markers the
      source puts on the other alternatives (`;BF_STAGE_MASKED`, `;BF_STAGE_PART0`, `;BF_STAGE_WIPE`, `;BF_STAGE_OTHER`);
  (b) the instructions of every kind between one mic's `;BF_S2_BEGIN` and the next one's in the text, the out-of-line `.subsection 1`
      re-read stubs excluded: a mic's steps 1..7, the next mic's address, reads, waits and step 0, and the table loads between;
  (c) VGPRs, SGPRs, spilled SGPRs and scratch bytes from the code-object metadata, and the v_readlane / v_writelane (SGPR spill
      traffic) between the barriers of the half loop;
  (d) the k-ordered mean-power pass of the power-of-two path (`;BF_POWER_POW2` to `;BF_POWER_END`): what every wave issues to park
      its squares, by kind, and the reads, adds and waits of each ordered-sum loop.

usage: python scripts/dev/pair2_instruction_budget.py [das_pair.hip]      (default: the unit in csrc/; another path: a variant of it
       with the same markers, e.g. an older revision)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "zybo-rt-sampler-image-detection_amd", "csrc")
KERNEL = "das_pair2_kernel"
OFF_PATH = ("BF_STAGE_MASKED", "BF_STAGE_PART0", "BF_STAGE_WIPE", "BF_STAGE_OTHER")
KINDS = ("packed", "test/branch", "lds", "wait", "table load", "scalar", "vector")


def compile_asm(src=None, unit="das_pair.hip"):
    """gfx950 assembly text of the unit (device side only), built with the flags the library is built with."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    src = src or os.path.join(CSRC, unit)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "das_pair.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + [f for f in ge.HIPCC_FLAGS if f != "-fPIC"] + [
            "-I", CSRC, "--cuda-device-only", "-S", src, "-o", out]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def kernel_lines(txt, kernel=KERNEL):
    """The text lines of das_pair2_kernel (or of `kernel`), from its symbol to its .Lfunc_end."""
    lines = txt.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN\S*%s\S*:" % kernel, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def kind_of(text):
    op = text.split()[0]
    if op.startswith(("v_pk_fma_f32", "v_pk_add_f32")):
        return "packed"
    if op.startswith(("s_cmp", "s_cbranch", "s_branch", "s_bitcmp")):
        return "test/branch"
    if op.startswith("ds_"):
        return "lds"
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "table load"
    return "scalar" if op.startswith("s_") else "vector"


def parse(lines):
    """-> (items, labels): items are instructions {text, sub, next, targets} and markers {marker, sub, next}, subsection 0 first;
    labels: name -> index of the item behind it."""
    subs, cur = {0: [], 1: []}, 0
    for line in lines:
        l = line.strip()
        m = re.match(r";\s*(BF_\w+)", l)
        if m:
            subs[cur].append({"marker": m.group(1)})
            continue
        l = l.split(";")[0].strip()
        if not l:
            continue
        m = re.match(r"\.subsection\s+(\d+)", l)
        if m:
            cur = int(m.group(1))
            subs.setdefault(cur, [])
            continue
        if l.startswith("."):
            m = re.match(r"(\.[\w$.]+):", l)
            if m:
                subs[cur].append({"label": m.group(1)})
            continue
        subs[cur].append({"text": l})
    items, labels = [], {}
    for sub in sorted(subs):
        pending = []
        for it in subs[sub]:
            if "label" in it:
                pending.append(it["label"])
                continue
            for lab in pending:
                labels[lab] = len(items)
            pending = []
            items.append(dict(it, sub=sub))
    for i, it in enumerate(items):
        nxt = i + 1 if i + 1 < len(items) and items[i + 1]["sub"] == it["sub"] else None
        targets = []
        if "text" in it:
            op = it["text"].split()[0]
            if op == "s_branch":
                targets, nxt = [it["text"].split()[1]], None
            elif op.startswith("s_cbranch"):
                targets = [it["text"].split()[1]]
            elif op in ("s_endpgm", "s_setpc_b64"):
                nxt = None
        it["next"], it["targets"] = nxt, targets
    return items, labels


def staging_path(items, labels):
    """(a): the instructions of the longest BF_STAGE_BEGIN -> BF_STAGE_END path that passes no OFF_PATH marker, in order; None
    where the source has no such markers."""
    begins = [i for i, it in enumerate(items) if it.get("marker") == "BF_STAGE_BEGIN"]
    if not begins:
        return None
    memo = {}

    def longest(i, on_path):
        if i is None or i in on_path:
            return None
        it = items[i]
        if it.get("marker") == "BF_STAGE_END":
            return []
        if it.get("marker") in OFF_PATH:
            return None
        if i in memo:
            return memo[i]
        succ = [it["next"]] + [labels.get(t) for t in it["targets"]]
        best = None
        for s in succ:
            p = longest(s, on_path | {i})
            if p is not None and (best is None or len(p) > len(best)):
                best = p
        if best is not None and "text" in it:
            best = [it["text"]] + best
        memo[i] = best
        return best

    sys.setrecursionlimit(20000)
    paths = [p for p in (longest(b, frozenset()) for b in begins) if p is not None]
    return max(paths, key=len) if paths else None


def mic_gaps(lines):
    """(b): one {kind: count} per pair of consecutive BF_S2_BEGIN markers of the text, `.subsection 1` blocks excluded."""
    gaps, cur, stub = [], None, False
    for line in lines:
        l = line.strip()
        if "BF_S2_BEGIN" in l:
            if cur is not None:
                gaps.append(cur)
            cur = dict.fromkeys(KINDS, 0)
            continue
        l = l.split(";")[0].strip()
        if re.match(r"\.subsection\s+1", l):
            stub = True
        elif re.match(r"\.subsection\s+0", l):
            stub = False
        elif cur is not None and not stub and l and not l.startswith(".") and not l.endswith(":"):
            cur[kind_of(l)] += 1
    return gaps


def resources(txt, kernel=KERNEL):
    """(c): the metadata entry of the kernel."""
    blk = next(b for b in re.split(r"\n\s+- (?=\.agpr_count:)", txt)[1:] if kernel in re.search(r"\.name:\s+(\S+)", b).group(1))
    g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
    return dict(vgprs=g("vgpr_count"), sgprs=g("sgpr_count"), sgpr_spills=g("sgpr_spill_count"), scratch=g("private_segment_fixed_size"))


def lane_spills_in_half_loop(lines):
    """v_readlane / v_writelane from the barrier before the first mic of the half loop's text to the barrier behind its last mic
    (the loop's own barrier); None where the text has no mic."""
    s2 = [i for i, l in enumerate(lines) if "BF_S2_BEGIN" in l]
    bars = [i for i, l in enumerate(lines) if l.split(";")[0].strip() == "s_barrier"]
    if not s2 or not [b for b in bars if b < s2[0]] or not [b for b in bars if b > s2[-1]]:
        return None
    lo, hi = max(b for b in bars if b < s2[0]), min(b for b in bars if b > s2[-1])
    return sum(1 for l in lines[lo:hi] if re.match(r"v_(readlane|writelane)_b32", l.split(";")[0].strip()))


POWER_KINDS = ("packed multiply", "multiply", "lds store", "lds read", "vector", "scalar", "wait", "test/branch")


def power_kind_of(text):
    op = text.split()[0]
    if op.startswith("v_pk_mul_f32"):
        return "packed multiply"
    if op.startswith("v_mul_f32"):
        return "multiply"
    if op.startswith("ds_write"):
        return "lds store"
    if op.startswith("ds_read"):
        return "lds read"
    k = kind_of(text)
    return k if k in ("wait", "test/branch", "scalar") else "vector"


def power_pass(lines):
    """(d): the mean-power pass of the power-of-two path, the text from the source's `;BF_POWER_POW2` marker to the next
    `;BF_POWER_END`; None where the source has no such markers.
      parking: {kind: count} of what every wave issues to park its squares: the text before the pass's first barrier (round 0: the
               means, the squares, the stores) and between its second and its third (round 1), barriers excluded;
      loops:   one entry per loop of the text that reads LDS and adds (the ordered sum of a round): its 16-byte reads, its v_add_f32,
               the lgkmcnt of every wait in it in order -- a 0 among them is a full wait, an LDS round trip the chain sits through."""
    begin = [i for i, l in enumerate(lines) if "BF_POWER_POW2" in l]
    if not begin:
        return None
    end = next((i for i in range(begin[0], len(lines)) if "BF_POWER_END" in lines[i]), len(lines))   # (laid out before the pass: to the kernel's end)
    text = []                                               # instructions and labels of the pass, in text order
    for line in lines[begin[0] + 1:end]:
        l = line.split(";")[0].strip()
        if not l:
            continue
        if l.startswith(".") and not l.endswith(":"):
            continue
        text.append(l)
    bars = [i for i, l in enumerate(text) if l == "s_barrier"]
    parking = dict.fromkeys(POWER_KINDS, 0)
    if len(bars) >= 3:
        for l in text[:bars[0]] + text[bars[1] + 1:bars[2]]:
            if not l.endswith(":"):
                parking[power_kind_of(l)] += 1
    loops = []
    where = {l[:-1]: i for i, l in enumerate(text) if l.endswith(":")}
    for i, l in enumerate(text):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if m and m.group(1) in where and where[m.group(1)] < i:
            body = [t for t in text[where[m.group(1)]:i] if not t.endswith(":")]
            reads = sum(t.startswith("ds_read_b128") for t in body)
            adds = sum(t.startswith("v_add_f32") for t in body)
            if reads and adds and "s_barrier" not in body:
                waits = [int(w) for t in body if t.startswith("s_waitcnt") for w in re.findall(r"lgkmcnt\((\d+)\)", t)]
                loops.append(dict(reads=reads, adds=adds, waits=waits))
    return dict(parking=parking, barriers=len(bars), loops=loops)


def budget(src=None):
    txt = compile_asm(src)
    lines = kernel_lines(txt)
    items, labels = parse(lines)
    return dict(staging=staging_path(items, labels), gaps=mic_gaps(lines), resources=resources(txt), lane_spills=lane_spills_in_half_loop(lines),
                power=power_pass(lines))


# ---- das_pair2_cells_kernel (csrc/das_cells.hip): the same report for the kernel of the same family on rows of 16-byte cells ----
CELLS_UNIT, CELLS_KERNEL = "das_cells.hip", "das_pair2_cells_kernel"


def half_loop_lines(lines):
    """The lines of the half loop, wherever the compiler laid its blocks out (it rotates the loop: the barrier that ends an iteration
    stands in front of the first mic in the text): the compiler's own comment on every block label says which loop the block belongs
    to, and the half loop is the one of depth 2 that holds the mics.  A block without a label belongs to the loop of the one it falls
    out of.  None where the text has no mic."""
    out, inner = [], False
    for i, l in enumerate(lines):
        if re.match(r"\.LBB\d+_\d+:", l):
            note = l + (lines[i + 1] if i + 1 < len(lines) and lines[i + 1].strip().startswith(";") else "")   # (a header's comment takes two lines)
            inner = "Depth=2" in note
        if inner:
            out.append(l)
    return out if any("BF_S2_BEGIN" in l for l in out) else None


def sgpr_spill_traffic_in_half_loop(lines):
    """lane_spills_in_half_loop for a kernel whose staging reads lanes of its own (the cells kernel takes lane 0 of the next register with
    v_readlane) and whose loop is laid out rotated: the registers SGPRs are spilled to are those some v_writelane of the kernel writes;
    counted are, in half_loop_lines, every v_writelane and every v_readlane out of such a register.  None where the text has no mic."""
    loop = half_loop_lines(lines)
    if loop is None:
        return None
    code = lambda ls: [l.split(";")[0].strip() for l in ls]
    spill_regs = set(m.group(1) for m in (re.match(r"v_writelane_b32\s+(v\d+)\s*,", l) for l in code(lines)) if m)
    n = 0
    for l in code(loop):
        m = re.match(r"v_readlane_b32\s+\S+\s*(v\d+)\s*,", l)
        n += 1 if l.startswith("v_writelane_b32") or (m and m.group(1) in spill_regs) else 0
    return n


def barriers_in_half_loop(lines):
    loop = half_loop_lines(lines)
    return None if loop is None else sum(l.split(";")[0].strip() == "s_barrier" for l in loop)


def setprio_sequence_of_a_half(lines):
    """The s_setprio immediates of half_loop_lines in text order from the loop's header on, each with the number of BF_S2_BEGIN markers
    (mics) passed before it: [(immediate, mics before)], the out-of-line `.subsection 1` blocks excluded."""
    loop = half_loop_lines(lines)
    head = next(i for i, l in enumerate(loop) if l.startswith(".LBB") and i + 1 < len(loop) and "Inner Loop Header" in loop[i + 1])
    seq, mics, stub = [], 0, False
    for l in loop[head:] + loop[:head]:
        c = l.split(";")[0].strip()
        if "BF_S2_BEGIN" in l:
            mics += 1
        if re.match(r"\.subsection\s+1", c):
            stub = True
        elif re.match(r"\.subsection\s+0", c):
            stub = False
        elif not stub and c.startswith("s_setprio"):
            seq.append((int(c.split()[1]), mics))
    return seq


def priorities_entering_the_power_pass(items, labels):
    """The priorities a wave can hold where it passes `;BF_POWER_POW2` or `;BF_POWER_DIV`, over every path of the control-flow graph from
    the kernel's entry (priority 0): a set."""
    seen, found, work = set(), set(), [(0, 0)]
    while work:
        i, prio = work.pop()
        while i is not None and (i, prio) not in seen:
            seen.add((i, prio))
            it = items[i]
            if it.get("marker") in ("BF_POWER_POW2", "BF_POWER_DIV"):
                found.add(prio)
            m = re.match(r"s_setprio\s+(\d+)$", it.get("text", ""))
            if m:
                prio = int(m.group(1))
            for t in it["targets"]:
                if labels.get(t) is not None:
                    work.append((labels[t], prio))
            i = it["next"]
    return found


def setprio_between_a_mics_statements(lines):
    """The s_setprio instructions between a `;BF_S1_END` and the next `;BF_S2_BEGIN` (where a mic's cells are in flight): a list."""
    bad, inside = [], False
    for l in lines:
        if "BF_S1_END" in l:
            inside = True
        elif "BF_S2_BEGIN" in l:
            inside = False
        elif inside and l.split(";")[0].strip().startswith("s_setprio"):
            bad.append(l.strip())
    return bad


def budget_cells(src=None):
    txt = compile_asm(src, CELLS_UNIT)
    lines = kernel_lines(txt, CELLS_KERNEL)
    items, labels = parse(lines)
    return dict(staging=staging_path(items, labels), gaps=mic_gaps(lines), resources=resources(txt, CELLS_KERNEL),
                lane_spills=sgpr_spill_traffic_in_half_loop(lines), power=power_pass(lines), ladder=setprio_sequence_of_a_half(lines),
                prio_in_flight=setprio_between_a_mics_statements(lines), power_entry=priorities_entering_the_power_pass(items, labels),
                loop_barriers=barriers_in_half_loop(lines))


def report(b):
    out = []
    st = b["staging"]
    if st is None:
        out.append("(a) staging path of a steady-state half: no BF_STAGE_BEGIN / BF_STAGE_END markers in this source")
    else:
        kinds = dict.fromkeys(KINDS, 0)
        for t in st:
            kinds[kind_of(t)] += 1
        out.append("(a) staging path of a steady-state half: %d instructions  (%s)" % (len(st), ", ".join("%s %d" % (k, kinds[k]) for k in KINDS if kinds[k])))
        out += ["      " + t for t in st]
    out.append("(b) from one mic's S2 to the next one's, stubs excluded: %d gaps" % len(b["gaps"]))
    for i, g in enumerate(b["gaps"]):
        out.append("      gap %d: %3d instructions  (%s)" % (i, sum(g.values()), ", ".join("%s %d" % (k, g[k]) for k in KINDS if g[k])))
    r = b["resources"]
    out.append("(c) VGPRs %d, SGPRs %d, spilled SGPRs %d, scratch %d bytes; v_readlane / v_writelane inside the half loop: %s" %
               (r["vgprs"], r["sgprs"], r["sgpr_spills"], r["scratch"], b["lane_spills"]))
    p = b.get("power")
    if p is None:
        out.append("(d) mean-power pass: no BF_POWER_POW2 / BF_POWER_END markers in this source")
    else:
        pk = p["parking"]
        out.append("(d) mean-power pass, power-of-two path: %d barriers; parking, both rounds: %d instructions  (%s)" %
                   (p["barriers"], sum(pk.values()), ", ".join("%s %d" % (k, pk[k]) for k in POWER_KINDS if pk[k])))
        for i, lp in enumerate(p["loops"]):
            out.append("      ordered-sum loop %d: %d reads of 16 bytes, %d adds, waits lgkmcnt(%s)%s" %
                       (i, lp["reads"], lp["adds"], ", ".join(map(str, lp["waits"])), "  <- a full wait inside the loop" if 0 in lp["waits"] else ""))
    return "\n".join(out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--cells":
        b = budget_cells(sys.argv[2] if len(sys.argv) > 2 else None)
        print(report(b))
        print("(e) s_setprio in the half loop, (immediate, mics before): %s; between a mic's two statements: %d; priorities entering the power pass: %s; "
              "barriers in the half loop: %d" % (b["ladder"], len(b["prio_in_flight"]), sorted(b["power_entry"]), b["loop_barriers"]))
    else:
        print(report(budget(sys.argv[1] if len(sys.argv) > 1 else None)))
