"""Do two gfx950 assembly files hold the same kernels?

Two bars, for two kinds of change:
  * literal (the default), for a MOVE of kernels between translation units: the move must not change a single instruction, register
    numbers included;
  * --renumbered, for a source-level RESTATEMENT of a kernel (the same arithmetic written through a helper, say): the register allocator
    may hand out other numbers for the same program, so every register operand -- v<n>, s<n>, a<n> and tuples such as v[8:11] -- is
    replaced by its register file and tuple width (v, s2, v4) before the comparison.  Mnemonics, modifiers, immediates, offsets, wait
    counts, labels and the order of the instructions are still compared literally, and so are the metadata fields.  It does not show
    that the renumbering is consistent; tests/test_isa_hazards.py checks what depends on which register holds what.

For every kernel (the entries of `.amdgpu_metadata`, identified by their mangled names) this compares
  * the instruction text between the kernel's symbol and its `.Lfunc_end`, after comments and blank lines are dropped and local labels
    (`.L<stem><digits>[_<digits>]`: the numbers count functions and asm statements of the whole file) are renamed to their order of
    first appearance inside the kernel;
  * six fields of the kernel's metadata entry: vgpr_count, sgpr_count, agpr_count, vgpr_spill_count, private_segment_fixed_size and
    group_segment_fixed_size.
It prints the kernels missing on either side and the first differing line of every kernel that differs, and exits non-zero on any
difference.  Either file may be a concatenation of several units' assembly (check_inflight_copies.compile_asm writes one).

--renamed FILE, for kernels whose NAME or parameter list changed (a template argument more, parameters appended): FILE holds one
`OLD -> NEW` line per such kernel, demangled as check_inflight_copies.demangle prints them (`bf::stream_map_kernel<0, 1, 4> ->
bf::das_mimo_kernel<0, 1, 4, true>`).  A renamed kernel is compared with its new name's text, in either mode, and three things are
not differences for it: lines that differ only in the kernel's own symbol, the value of `.amdhsa_kernarg_size`, and the offset of a
scalar load whose base is the kernel-argument pointer's entry registers (an implicit argument that moved behind appended parameters).
Kernels that differ in such offsets alone are listed apart, as "argument offsets only", with the number of loads; everything else about
them, and every kernel the file does not name, is compared as above.

usage: python scripts/dev/isa_equal.py [--renumbered] [--renamed FILE] OLD.s NEW.s"""
import re
import sys

FIELDS = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL_RE = re.compile(r"\.L([A-Za-z_$.]*)\d+(?:_\d+)?\b")
REG_RE = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")


def metadata(txt):
    """{mangled kernel name: {field: value}} from the .amdgpu_metadata blocks (an entry starts at its `- .agpr_count:` line)."""
    out = {}
    for blk in re.split(r"\n\s+- (?=\.agpr_count:)", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            out[name.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in FIELDS}
    return out


def symbols(lines, names):
    """{kernel name: index of its `name:` line} for the kernels the metadata names"""
    out = {}
    for i, l in enumerate(lines):
        if l[:1] not in ("", " ", "\t") and l.split(":")[0] in names:
            out[l.split(":")[0]] = i
    return out


def kernarg_pointer(txt, name):
    """The SGPR pair that holds the kernel-argument pointer on entry, as the operand text `s[a:b]` (the user SGPRs come in the
    descriptor's order: private segment buffer, dispatch pointer, queue pointer, kernel-argument pointer).  None: the kernel has none."""
    m = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), txt, re.S)

    def on(field):
        f = re.search(r"\.amdhsa_user_sgpr_%s\s+(\d+)" % field, m.group(1)) if m else None
        return int(f.group(1)) if f else 0

    if not on("kernarg_segment_ptr"):
        return None
    first = 4 * on("private_segment_buffer") + 2 * on("dispatch_ptr") + 2 * on("queue_ptr")
    return "s[%d:%d]" % (first, first + 1)


def body(lines, start, renumbered=False, own=None, pointer=None, offsets=None):
    """The instruction text of the kernel whose symbol is on line `start`: comments and blank lines dropped, local labels renamed by
    first appearance, with `renumbered` every register operand reduced to its file and tuple width.  None: no such symbol.
    For a renamed kernel: `own` (its mangled name) is replaced by `<kernel>` wherever it is mentioned, and the offset of every scalar
    load whose base is literally `pointer` (kernarg_pointer's pair; a copy of the pointer in other registers is compared like everything
    else) is replaced by `<argument>` and appended to `offsets`."""
    if start is None:
        return None
    seen = {}
    load = re.compile(r"(s_load_\w+\s+[^,]+,\s*%s,\s*)(0x[0-9a-fA-F]+|\d+)\b" % re.escape(pointer)) if pointer else None

    def rename(m):
        return ".L%s#%d" % (m.group(1), seen.setdefault(m.group(0), len(seen)))

    def regfile(m):
        return m.group(1) if m.group(2) else "%s%d" % (m.group(1), int(m.group(4)) - int(m.group(3)) + 1)

    def argument(m):
        offsets.append(int(m.group(2), 0))
        return m.group(1) + "<argument>"

    out = []
    for l in lines[start + 1:]:
        l = l.split(";")[0].strip()
        if not l:
            continue
        if l.startswith(".Lfunc_end"):
            return out
        l = LABEL_RE.sub(rename, l)
        if own:
            l = re.sub(r"^(\.amdhsa_kernarg_size) \d+$", r"\1 <size>", l.replace(own, "<kernel>"))
        if load:
            l = load.sub(argument, l, count=1)
        out.append(REG_RE.sub(regfile, l) if renumbered else l)
    raise ValueError("line %d: the kernel's text has no .Lfunc_end" % (start + 1))


def load_renamed(path, names_old, names_new, demangle):
    """A file of `OLD -> NEW` lines, demangled names as check_inflight_copies.demangle prints them (blank lines and # comments skipped)
    -> {mangled old: mangled new}.  Every name must exist on its side, and no name may appear twice."""
    short_old, short_new = dict(zip(demangle(names_old), names_old)), dict(zip(demangle(names_new), names_new))
    out = {}
    for lineno, l in enumerate(open(path), 1):
        l = l.split("#")[0].strip()
        if not l:
            continue
        where = "%s line %d (%s)" % (path, lineno, l)
        sides = [x.strip() for x in l.split("->")]
        if len(sides) != 2:
            raise ValueError("%s: not `OLD -> NEW`" % where)
        old, new = sides
        if old not in short_old:
            raise ValueError("%s: OLD has no kernel %s" % (where, old))
        if new not in short_new:
            raise ValueError("%s: NEW has no kernel %s" % (where, new))
        if short_old[old] in out or short_new[new] in out.values():
            raise ValueError("%s: named twice" % where)
        out[short_old[old]] = short_new[new]
    return out


def compare(old_txt, new_txt, renumbered=False, renamed=None, argument_offsets=None):
    """-> list of differences, one line of text each (empty: the two files hold the same kernels), and the number of kernels compared.
    renamed {mangled old: mangled new}: those kernels are compared with each other, and for them three things are no differences: a
    mention of the kernel's own symbol, the size of the kernel-argument segment (no field this compares) and the offset of a scalar load
    from the kernel-argument pointer.  argument_offsets (a dict, filled): {new name: number of such loads whose offset moved}."""
    renamed = dict(renamed or {})
    diffs = []
    md_old, md_new = metadata(old_txt), metadata(new_txt)
    pairs = [(n, renamed.get(n, n)) for n in sorted(md_old) if renamed.get(n, n) in md_new]
    for n in sorted(set(md_old) - set(o for o, _ in pairs)):
        diffs.append("only in OLD: %s" % n)
    for n in sorted(set(md_new) - set(w for _, w in pairs)):
        diffs.append("only in NEW: %s" % n)
    lines_old, lines_new = old_txt.split("\n"), new_txt.split("\n")
    sym_old, sym_new = symbols(lines_old, md_old), symbols(lines_new, md_new)
    for n, w in pairs:
        for f in FIELDS:
            if md_old[n][f] != md_new[w][f]:
                diffs.append("%s: .%s %d -> %d" % (n, f, md_old[n][f], md_new[w][f]))
        if n in renamed:
            off_a, off_b = [], []
            a = body(lines_old, sym_old.get(n), renumbered, n, kernarg_pointer(old_txt, n), off_a)
            b = body(lines_new, sym_new.get(w), renumbered, w, kernarg_pointer(new_txt, w), off_b)
        else:
            a, b = body(lines_old, sym_old.get(n), renumbered), body(lines_new, sym_new.get(w), renumbered)
        if a is None or b is None:
            diffs.append("%s: no instruction text in %s" % (n, "OLD" if a is None else "NEW"))
        elif a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            diffs.append("%s: instruction %d of %d / %d: %r -> %r" % (n, i, len(a), len(b), a[i] if i < len(a) else None, b[i] if i < len(b) else None))
        elif n in renamed and off_a != off_b and argument_offsets is not None:   # (equal texts: the loads are the same lines on both sides)
            argument_offsets[w] = sum(x != y for x, y in zip(off_a, off_b))
    return diffs, len(pairs)


if __name__ == "__main__":
    import argparse
    import os
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--renumbered", action="store_true")
    ap.add_argument("--renamed", metavar="FILE")
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    old_txt, new_txt = open(args.old).read(), open(args.new).read()
    renamed, moved = None, {}
    if args.renamed:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from check_inflight_copies import demangle
        renamed = load_renamed(args.renamed, list(metadata(old_txt)), list(metadata(new_txt)), demangle)
    diffs, common = compare(old_txt, new_txt, renumbered=args.renumbered, renamed=renamed, argument_offsets=moved)
    for d in diffs:
        print(d)
    if moved:
        print("argument offsets only (no difference): %d kernels" % len(moved))
        for n, d in zip(moved, demangle(list(moved))):
            print("  %s: %d loads" % (d, moved[n]))
    print("%d kernels on both sides, %d differences" % (common, len(diffs)))
    sys.exit(1 if diffs or common == 0 else 0)
