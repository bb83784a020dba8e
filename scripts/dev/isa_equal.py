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

usage: python scripts/dev/isa_equal.py [--renumbered] OLD.s NEW.s"""
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


def body(lines, start, renumbered=False):
    """The instruction text of the kernel whose symbol is on line `start`: comments and blank lines dropped, local labels renamed by
    first appearance, with `renumbered` every register operand reduced to its file and tuple width.  None: no such symbol."""
    if start is None:
        return None
    seen = {}

    def rename(m):
        return ".L%s#%d" % (m.group(1), seen.setdefault(m.group(0), len(seen)))

    def regfile(m):
        return m.group(1) if m.group(2) else "%s%d" % (m.group(1), int(m.group(4)) - int(m.group(3)) + 1)

    out = []
    for l in lines[start + 1:]:
        l = l.split(";")[0].strip()
        if not l:
            continue
        if l.startswith(".Lfunc_end"):
            return out
        l = LABEL_RE.sub(rename, l)
        out.append(REG_RE.sub(regfile, l) if renumbered else l)
    raise ValueError("line %d: the kernel's text has no .Lfunc_end" % (start + 1))


def compare(old_txt, new_txt, renumbered=False):
    """-> list of differences, one line of text each (empty: the two files hold the same kernels)"""
    diffs = []
    md_old, md_new = metadata(old_txt), metadata(new_txt)
    for n in sorted(set(md_old) - set(md_new)):
        diffs.append("only in OLD: %s" % n)
    for n in sorted(set(md_new) - set(md_old)):
        diffs.append("only in NEW: %s" % n)
    lines_old, lines_new = old_txt.split("\n"), new_txt.split("\n")
    sym_old, sym_new = symbols(lines_old, md_old), symbols(lines_new, md_new)
    for n in sorted(set(md_old) & set(md_new)):
        for f in FIELDS:
            if md_old[n][f] != md_new[n][f]:
                diffs.append("%s: .%s %d -> %d" % (n, f, md_old[n][f], md_new[n][f]))
        a, b = body(lines_old, sym_old.get(n), renumbered), body(lines_new, sym_new.get(n), renumbered)
        if a is None or b is None:
            diffs.append("%s: no instruction text in %s" % (n, "OLD" if a is None else "NEW"))
        elif a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            diffs.append("%s: instruction %d of %d / %d: %r -> %r" % (n, i, len(a), len(b), a[i] if i < len(a) else None, b[i] if i < len(b) else None))
    return diffs, len(set(md_old) & set(md_new))


if __name__ == "__main__":
    files = [a for a in sys.argv[1:] if a != "--renumbered"]
    if len(files) != 2:
        sys.exit(__doc__)
    diffs, common = compare(open(files[0]).read(), open(files[1]).read(), renumbered=len(files) < len(sys.argv) - 1)
    for d in diffs:
        print(d)
    print("%d kernels on both sides, %d differences" % (common, len(diffs)))
    sys.exit(1 if diffs or common == 0 else 0)
