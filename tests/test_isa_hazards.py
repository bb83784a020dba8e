"""The hand-scheduled LDS reads of the shifted-copies kernels (csrc/das_kernels.hip, das_pair.hip) stay sound only while nothing touches a register that has a read in
flight (scripts/dev/check_inflight_copies.py explains).  CPU-only: compiles the kernels to gfx950 assembly, builds the control-
flow graph of every das_copies_kernel / das_pair_kernel instantiation (out-of-line `.subsection 1` stubs and loop back-edges
included), runs the in-flight data-flow over every path, and reads spill / scratch sizes from the code-object metadata."""
import importlib.util
import os
import re

import pytest

import util


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_inflight_copies", os.path.join(util.ROOT, "scripts", "dev", "check_inflight_copies.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def asm(chk, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isa") / "das_units.s")
    chk.compile_asm(path)
    return path


FAKE = """
_ZN2bf12_GLOBAL__N_16copies15das_pair_kernelILi9EEEvPKfPfPKiS7_S4_S4_NS0_5KArgsE:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	ds_read_b64 v[10:11], v1 offset:0
%s
	s_endpgm
.Lfunc_end0:
"""


@pytest.mark.parametrize("body,n_bad", [
    ("\ts_waitcnt lgkmcnt(0)\n\tv_pk_add_f32 v[2:3], v[2:3], v[10:11]", 0),                              # consumed after the wait
    ("\tv_mov_b32_e32 v20, v11\n\ts_waitcnt lgkmcnt(0)", 1),                                              # copied while in flight
    ("\tv_mov_b32_e32 v10, 0\n\ts_waitcnt lgkmcnt(0)", 1),                                                # overwritten while in flight
    ("\tds_write_b64 v1, v[10:11]\n\ts_waitcnt lgkmcnt(0)", 1),                                           # stored while in flight
    ("\tds_read_b64 v[12:13], v1 offset:8\n\ts_waitcnt lgkmcnt(1)\n\tv_mov_b32_e32 v20, v10\n\tv_mov_b32_e32 v21, v12\n\ts_waitcnt lgkmcnt(0)", 1),   # counted wait: the older read has landed, the younger not
    # the hazard sits behind a branch, in an out-of-line stub that the straight-line text never reaches
    ("\ts_cmp_lg_u32 s2, s3\n\ts_cbranch_scc1 .Lstub\n.Lback:\n\ts_waitcnt lgkmcnt(0)\n\tv_pk_add_f32 v[2:3], v[2:3], v[10:11]\n"
     "\t.subsection 1\n.Lstub:\n\tv_add_u32_e32 v20, v10, v1\n\ts_waitcnt lgkmcnt(0)\n\ts_branch .Lback\n\t.subsection 0", 1),
    # a wait inside the not-taken stub must not hide a read that is still in flight on the fall-through path
    ("\ts_cbranch_scc1 .Lstub\n.Lback:\n\tv_mov_b32_e32 v20, v10\n\ts_waitcnt lgkmcnt(0)\n"
     "\t.subsection 1\n.Lstub:\n\ts_waitcnt lgkmcnt(0)\n\ts_branch .Lback\n\t.subsection 0", 1),
    # carried around a loop: in flight at the back-edge, touched at the loop head on the second trip
    (".Lloop:\n\tv_mov_b32_e32 v20, v30\n\tds_read_b64 v[30:31], v1 offset:16\n\ts_add_u32 s2, s2, 1\n\ts_cmp_lt_u32 s2, 4\n\ts_cbranch_scc1 .Lloop\n\ts_waitcnt lgkmcnt(0)", 1),
])
def test_scanner_finds_what_it_should(chk, tmp_path, body, n_bad):
    p = tmp_path / "fake.s"
    p.write_text(FAKE % body)
    kernels, bad = chk.scan(str(p))
    assert kernels == 1 and len(bad) == n_bad, bad


@pytest.fixture(scope="module")
def iseq():
    spec = importlib.util.spec_from_file_location("isa_equal", os.path.join(util.ROOT, "scripts", "dev", "isa_equal.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


FAKE_UNIT = """
_Z5alphaPf:
	s_load_dwordx2 s[0:1], s[4:5], 0x0 ; a comment
.LBB%(n)d_1:

	v_add_f32_e32 v1, %(operand)s, v1
	s_cbranch_scc1 .LBB%(n)d_1
	s_cbranch_scc0 .Lr1_%(stmt)d
.Lb1_%(stmt)d:
	s_endpgm
	.subsection 1
.Lr1_%(stmt)d:
	s_branch .Lb1_%(stmt)d
	.subsection 0
.Lfunc_end%(n)d:
%(second)s
	.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 0
    .name:           _Z5alphaPf
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .vgpr_count:     %(vgprs)d
    .vgpr_spill_count: 0
%(second_md)s...
	.end_amdgpu_metadata
"""
FAKE_SECOND = "_Z4betaPf:\n\ts_endpgm\n.Lfunc_end7:\n"
FAKE_SECOND_MD = """  - .agpr_count:     0
    .group_segment_fixed_size: 1024
    .name:           _Z4betaPf
    .private_segment_fixed_size: 0
    .sgpr_count:     8
    .vgpr_count:     2
    .vgpr_spill_count: 0
"""


@pytest.mark.parametrize("change,n_diff,needle", [
    (dict(n=3, stmt=212), 0, None),                                     # equal but for the label numbers of another unit
    (dict(operand="v3"), 1, "v_add_f32_e32 v1, v3, v1"),                # one changed instruction
    (dict(vgprs=25), 1, ".vgpr_count 24 -> 25"),                        # one changed metadata field
    (dict(second="", second_md=""), 1, "only in OLD: _Z4betaPf"),       # one kernel missing
])
def test_comparator_finds_what_it_should(iseq, change, n_diff, needle):
    base = dict(n=0, stmt=17, operand="v2", vgprs=24, second=FAKE_SECOND, second_md=FAKE_SECOND_MD)
    diffs, common = iseq.compare(FAKE_UNIT % base, FAKE_UNIT % dict(base, **change))
    assert common == (1 if "second" in change else 2)
    assert len(diffs) == n_diff, diffs
    assert needle is None or needle in diffs[0], diffs


def test_renumbered_comparison_forgives_register_numbers_and_nothing_else(iseq):
    base = dict(n=0, stmt=17, operand="v2", vgprs=24, second=FAKE_SECOND, second_md=FAKE_SECOND_MD)
    old = FAKE_UNIT % base
    assert iseq.compare(old, FAKE_UNIT % dict(base, operand="v3"))[0]                          # literal: a difference
    assert not iseq.compare(old, FAKE_UNIT % dict(base, operand="v3"), renumbered=True)[0]     # another number of the same file
    for change, needle in ((dict(operand="s3"), "'v_add_f32_e32 v, v, v' -> 'v_add_f32_e32 v, s, v'"),      # another register file
                           (dict(operand="v[2:3]"), "-> 'v_add_f32_e32 v, v2, v'"),                        # a tuple: another width
                           (dict(operand="1.0"), "-> 'v_add_f32_e32 v, 1.0, v'"),                          # an immediate
                           (dict(vgprs=25), ".vgpr_count 24 -> 25")):                                      # the metadata, as ever
        diffs, _ = iseq.compare(old, FAKE_UNIT % dict(base, **change), renumbered=True)
        assert len(diffs) == 1 and needle in diffs[0], diffs


FAKE_RENAMED = """
%(name)s:
	s_load_dwordx2 s[10:11], %(ptr)s, 0x0
	s_load_dword s12, %(ptr)s, %(implicit)s
	s_load_dword s13, s[10:11], %(other)s
	s_endpgm
	.amdhsa_kernel %(name)s
		.amdhsa_kernarg_size %(size)d
		.amdhsa_user_sgpr_dispatch_ptr %(dispatch)d
		.amdhsa_user_sgpr_queue_ptr %(queue)d
		.amdhsa_user_sgpr_kernarg_segment_ptr 1
	.end_amdhsa_kernel
.Lfunc_end0:
	.size	%(name)s, .Lfunc_end0-%(name)s
	.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 0
    .name:           %(name)s
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .vgpr_count:     4
    .vgpr_spill_count: 0
...
	.end_amdgpu_metadata
"""


@pytest.mark.parametrize("dispatch,queue,ptr", [(0, 0, "s[0:1]"), (1, 0, "s[2:3]"), (0, 1, "s[2:3]"), (1, 1, "s[4:5]")])
def test_renamed_comparison_forgives_symbol_argument_size_and_argument_offsets_only(iseq, dispatch, queue, ptr):
    """(the kernel-argument pointer follows the dispatch and queue pointers where the descriptor enables them)"""
    base = dict(dispatch=dispatch, queue=queue, ptr=ptr)
    old = FAKE_RENAMED % dict(base, name="_Z5alphaPf", implicit="0xb4", other="0x10", size=424)
    moved = dict(base, name="_Z5alphaPfi", implicit="0xc4", other="0x10", size=440)
    new = FAKE_RENAMED % moved
    assert iseq.kernarg_pointer(old, "_Z5alphaPf") == ptr
    if ptr != "s[0:1]":    # the same loads through a pair that is NOT the entry pair of this descriptor keep their offsets
        wrong = dict(moved, dispatch=0, queue=0)
        assert iseq.compare(FAKE_RENAMED % dict(wrong, name="_Z5alphaPf", implicit="0xb4", size=424), FAKE_RENAMED % wrong, renamed={"_Z5alphaPf": "_Z5alphaPfi"})[0]
    diffs, common = iseq.compare(old, new)
    assert common == 0 and len(diffs) == 2, diffs                                  # without the map: two unrelated kernels
    counts = {}
    diffs, common = iseq.compare(old, new, renamed={"_Z5alphaPf": "_Z5alphaPfi"}, argument_offsets=counts)
    assert common == 1 and not diffs, diffs
    assert counts == {"_Z5alphaPfi": 1}                                            # reported apart: one load, its offset only
    for mode in (False, True):
        # a load through any other pointer keeps its offset, and so does everything else
        diffs, _ = iseq.compare(old, FAKE_RENAMED % dict(moved, other="0x14"), renumbered=mode, renamed={"_Z5alphaPf": "_Z5alphaPfi"})
        assert len(diffs) == 1 and "0x10" in diffs[0] and "0x14" in diffs[0], diffs
    same_name = FAKE_RENAMED % dict(moved, name="_Z5alphaPf")
    assert len(iseq.compare(old, same_name)[0]) == 1                               # a kernel that was not renamed gets none of this


@pytest.mark.parametrize("text,needle", [
    ("alpha<0> -> alpha<0, true>\n# a comment\n\nbeta -> beta2  # another\n", None),
    ("alpha<0> alpha<0, true>\n", "not `OLD -> NEW`"),
    ("gamma -> beta2\n", "OLD has no kernel gamma"),
    ("beta -> gamma\n", "NEW has no kernel gamma"),
    ("beta -> beta2\nalpha<0> -> beta2\n", "named twice"),
])
def test_rename_file_errors_name_the_line(iseq, tmp_path, text, needle):
    p = tmp_path / "renamed.txt"
    p.write_text(text)
    demangle = lambda names: [{"_a": "alpha<0>", "_b": "beta", "_a2": "alpha<0, true>", "_b2": "beta2"}[n] for n in names]
    if needle is None:
        assert iseq.load_renamed(str(p), ["_a", "_b"], ["_a2", "_b2"], demangle) == {"_a": "_a2", "_b": "_b2"}
    else:
        with pytest.raises(ValueError, match=needle) as e:
            iseq.load_renamed(str(p), ["_a", "_b"], ["_a2", "_b2"], demangle)
        assert "line %d" % (text.count("\n")) in str(e.value)


def test_no_register_with_a_read_in_flight_is_touched(chk, asm):
    kernels, bad = chk.scan(asm)
    assert kernels >= 43
    assert not bad, bad[:5]


def test_every_default_plan_instantiation_is_scanned_and_none_that_pipelines_reads_spills(chk, asm):
    """launch_das (das_plan.cpp) can pick for the shifted-copies layout: the pair kernel (pad) and its frame-interleaved successor (lerp); the one-frame sweep for 1 / 2 / 4 segments with the fixed or
    the run-time row stride, 16 waves -- one segment also with 8 waves -- and its direction-outer (DIRECT) twin; the three 8-tap FIR
    flavours.  The instantiations that keep LDS reads in flight across asm statements (pair kernel; one-segment sweep; the long-row
    kernel, whose lerp sweep issues a mic's reads behind its predecessor's last step) must not use scratch: a spilled register with a read in flight is reloaded before the data lands."""
    md = chk.metadata(asm)
    names = [n for n in md if any(k in n for k in ("das_copies_kernel", "das_pair_kernel", "das_pair2_kernel", "das_long_kernel", "das_hybrid_pair_kernel"))]
    short = dict(zip(chk.demangle(names), names))
    want = ["bf::copies::das_pair_kernel<0>"]
    for a in (0, 1):
        want += ["bf::copies::das_copies_kernel<%d, 1, %d, %d, %s>" % (a, rs, w, d) for rs in (312, 0) for w, d in ((16, "false"), (8, "false"), (16, "true"))]
        want += ["bf::copies::das_copies_kernel<%d, %d, %d, 16, %s>" % (a, seg, rs, d) for seg, fixed in ((2, 576), (4, 1088)) for rs in (fixed, 0) for d in ("false", "true")]
    want += ["bf::copies::das_copies_kernel<%d, 1, %d, 16, false>" % (a, rs) for a in (2, 3, 4) for rs in (320, 0)]
    want += ["bf::copies::das_long_kernel<%d, %d, %d>" % (a, seg, rs) for a in (0, 1) for seg, fixed in ((2, 576), (4, 1088)) for rs in (fixed, 0)]
    want += ["bf::copies::das_hybrid_pair_kernel<%d>" % a for a in (2, 3, 4)] + ["bf::copies::das_pair2_kernel<1>"]
    missing = [w for w in want if w not in short]
    assert not missing, missing
    kernels, _ = chk.scan(asm)
    assert kernels == len(names)                       # the scan covered every one of them
    pipelined = [w for w in want if "bf::copies::das_pair_kernel" in w or "bf::copies::das_long_kernel" in w or "bf::copies::das_pair2_kernel" in w or
                 "bf::copies::das_hybrid_pair_kernel" in w or
                 (w.startswith("bf::copies::das_copies_kernel<0, 1,") or w.startswith("bf::copies::das_copies_kernel<1, 1,")) and w.endswith("false>")]
    assert len(pipelined) == 1 + 8 + 2 * 4 + 1 + 3     # (their launchers refuse to launch any of these from a build that uses scratch)
    for w in pipelined:
        m = md[short[w]]
        assert m["spill"] == 0 and m["scratch"] == 0, (w, m)
        assert m["vgprs"] <= 128                        # 16 waves per CU


def test_no_instantiation_outside_the_default_plan_is_compiled(chk, asm):
    """Nothing plan_das cannot choose is compiled: the other algorithm of each pair kernel (das_pair_kernel is pad, das_pair2_kernel
    lerp), the quad + DPP strided kernel (it was a trailing `true` where HIST now stands; the exact list below leaves it no room),
    and the strided map kernel for pad / lerp beyond 128 samples (4 / 8 / 16 segments) WITHOUT history -- with it
    (das_mimo_kernel<.., HIST = true>, the continuous-stream maps) every size is the strided kernel's.  No das_mimo_kernel exists
    outside the 58 listed: 38 without history (pad / lerp at NC 1, 2; the three FIR flavours at every NC; DPW 1 and 4) and 20 with."""
    every = chk.demangle(list(chk.metadata(asm)))
    retired = [n for n in every if n in ("bf::copies::das_pair_kernel<1>", "bf::copies::das_pair2_kernel<0>") or
               re.match(r"bf::das_mimo_kernel<[01], (4|8|16), \d+, false>", n)]
    assert not retired, retired
    want = ["bf::das_mimo_kernel<%d, %d, %d, false>" % (a, nc, dpw) for a in range(5) for nc in (1, 2, 4, 8, 16) for dpw in (1, 4) if a >= 2 or nc <= 2]
    want += ["bf::das_mimo_kernel<%d, %d, %d, true>" % (a, nc, dpw) for a in (0, 1) for nc in (1, 2, 4, 8, 16) for dpw in (1, 4)]
    assert len(want) == 38 + 20
    assert sorted(n for n in every if n.startswith("bf::das_mimo_kernel<")) == sorted(want)     # (the names are matched as demangled)


def test_hardwired_quads_survive_between_the_two_statements_of_a_mic(chk, asm):
    """das_pair2_kernel reads a mic's quads into v96..v111 in its statement S1 and consumes them in S2; both name those registers
    as clobbers, so the compiler may use them in between -- where only the scalar table requests belong.  No instruction in any
    S1 -> S2 gap of the generated code may name one of those registers."""
    pairs, bad = chk.hardwired_gaps(asm)
    assert pairs >= 2 * 5          # five mic bodies of das_pair2_kernel (three in the trip loop, two after it), the rest das_long_kernel's
    assert not bad, bad[:5]


def test_convolution_and_split_kernels_use_no_scratch():
    """Every detector convolution kernel (LDS-DMA in float32 native / split and float16, register-staged, the stem's patch kernel), the split MVDR quadratic
    form and the tiled DFT compile without scratch memory: a spill in these loops is a silent 2-5x (hipcc's kernel-resource-usage remarks, gfx950).
    (The phase-steer power GEMM's 2- to 4-row-tile instantiations do spill a few registers, measured and accepted in DESIGN.md section 7: not asserted.)"""
    import re
    import subprocess
    import __graft_entry__ as ge
    CSRC = ge.CSRC
    seen = {}
    for name in ("conv_kernels.hip", "freq_kernels.hip"):
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + [f for f in ge.HIPCC_FLAGS if f != "-fPIC"] + [
            "--cuda-device-only", "-c", os.path.join(CSRC, name), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, timeout=900).stderr
        cur = None
        for line in err.splitlines():
            m = re.search(r"remark: +Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                continue
            m = re.search(r"remark: +ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and cur:
                seen[cur] = int(m.group(1))
    conv = {k: v for k, v in seen.items() if "conv_dma_kernel" in k or "conv_igemm_kernel" in k or "conv_patch_kernel" in k}
    assert len(conv) >= 40, sorted(seen)[:5]                   # float32 native + split, float16, three kernels, all tile shapes
    assert not {k: v for k, v in conv.items() if v}, {k: v for k, v in conv.items() if v}
    others = {k: v for k, v in seen.items() if "dft_tile_kernel" in k or "cholesky_inverse_reg_kernel" in k or re.search(r"cgemm_bins_kernelILi2ELi1ELb[01]E", k)}
    assert len(others) >= 4, [k for k in seen if "cgemm_bins" in k][:4]
    assert not {k: v for k, v in others.items() if v}, {k: v for k, v in others.items() if v}
