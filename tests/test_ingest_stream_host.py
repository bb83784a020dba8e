"""CPU: the host-side contract of bf_ingest_stream_device (every argument is checked before device bring-up, so the refusals run
without a GPU), bf_default_disabled_mics against what get_data zeroes, ingest.PacketIngest's host logic, and the gfx950 resources
of the two kernels of ingest_kernel.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import util
from support import entry, FAKE, refused

M, N = 256, 256         # the as-shipped sizes


_stream = entry("bf_ingest_stream_device", d_packets=FAKE, n_datagrams=4 * N, n_arrays=4, rows=8, columns=8, hop=N, frames=4, m_total=M,
                d_row_mask=None, protocol_ver=2, d_frames=FAKE, d_status=None)


@pytest.mark.parametrize("kw,match", [
    (dict(d_packets=None), "bf_ingest_stream_device: d_packets is null"),
    (dict(d_frames=None), "bf_ingest_stream_device: d_frames is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(frames=-2), "frames = -2 < 1"),
    (dict(hop=0), "hop = 0 < 1"),
    (dict(hop=-256), "hop = -256 < 1"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(columns=0), "columns = 0 < 1"),
    (dict(columns=-8), "columns = -8 < 1"),
    (dict(n_arrays=0), "n_arrays = 0 < 1"),
    (dict(n_arrays=-1), "n_arrays = -1 < 1"),
    (dict(n_arrays=5), r"n_arrays\*rows\*columns = 320 > N_MICROPHONES = 256"),
    (dict(rows=9, m_total=512), r"n_arrays\*rows\*columns = 288 > N_MICROPHONES = 256"),
    (dict(n_arrays=3, m_total=191), r"n_arrays\*rows\*columns = 192 > m_total = 191"),
    (dict(m_total=0), r"n_arrays\*rows\*columns = 256 > m_total = 0"),
    (dict(n_datagrams=4 * N - 1), r"\(frames - 1\) \* hop \+ N_SAMPLES = 1024 > n_datagrams = 1023"),
    (dict(hop=1, frames=7, n_datagrams=N + 5), r"\(frames - 1\) \* hop \+ N_SAMPLES = 262 > n_datagrams = 261"),
    (dict(hop=2 ** 30, frames=2 ** 20, n_datagrams=2 ** 40), r"\(frames - 1\) \* hop \+ N_SAMPLES = 1125898833101056 > n_datagrams = 1099511627776"),
    (dict(n_datagrams=0), r"N_SAMPLES = 1024 > n_datagrams = 0"),
    (dict(d_packets=FAKE + 2), "d_packets = 0x10002 is not 4-byte aligned"),
    (dict(d_packets=FAKE + 1), "d_packets = 0x10001 is not 4-byte aligned"),
    (dict(d_frames=FAKE + 6), "d_frames = 0x10006 is not 4-byte aligned"),
])
def test_ingest_stream_argument_errors(native, kw, match):
    util.configure("shipped")
    native.lib.bf_clear_error()
    refused(native, _stream(native, **kw), match)


def test_ingest_stream_checks_follow_the_configured_sizes(native):
    """N_MICROPHONES and N_SAMPLES of the checks are the run-time sizes (bf_configure), not the as-shipped ones."""
    util.configure("cfg2")                         # 64 microphones x 256 samples
    native.lib.bf_clear_error()
    refused(native, _stream(native, n_arrays=2, m_total=128), r"n_arrays\*rows\*columns = 128 > N_MICROPHONES = 64")
    util.configure("cfg5")                         # 256 x 1024
    refused(native, _stream(native, frames=1, n_datagrams=1023), r"\(frames - 1\) \* hop \+ N_SAMPLES = 1024 > n_datagrams = 1023")
    util.configure("shipped")


def test_ingest_stream_valid_arguments_without_gpu(native):
    """Arguments that pass every check reach device bring-up, 4-byte aligned pointers and the optional ones included."""
    if native.gpu_available():
        pytest.skip("without a GPU only: with one, valid arguments would enqueue")
    util.configure("shipped")
    native.lib.bf_clear_error()
    refused(native, _stream(native), "no usable HIP device")
    refused(native, _stream(native, d_packets=FAKE + 4, d_frames=FAKE + 12, d_row_mask=FAKE, d_status=FAKE, hop=1, frames=190, n_datagrams=N + 189),
             "no usable HIP device")
    refused(native, _stream(native, n_arrays=1, m_total=64, hop=N + 37, frames=2, n_datagrams=2 * N + 37), "no usable HIP device")


def test_default_disabled_mics_are_what_get_data_zeroes(native):
    """bf_default_disabled_mics: 122 strictly increasing rows, equal to the rows get_data zeroes in a published frame of ones
    (PC/src/api.c:830-859)."""
    util.configure("shipped")
    lib = native.lib
    n = lib.bf_default_disabled_mics(None)
    assert n == 122
    rows = np.full(n + 2, -7, dtype=np.int32)
    assert lib.bf_default_disabled_mics(native.iptr(rows)) == n
    assert rows[n] == -7 and rows[n + 1] == -7               # nothing written past the count
    rows = rows[:n]
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < M
    ones = np.ones((M, N), dtype=np.float32)
    lib.bf_publish_frame(native.fptr(ones)); native.check()
    got = np.full((M, N), np.nan, dtype=np.float32)
    lib.get_data(native.fptr(got)); native.check()
    zero_rows = np.flatnonzero((got == 0.0).all(axis=1))
    assert np.array_equal(zero_rows, rows)
    assert np.array_equal(got[np.setdiff1d(np.arange(M), rows)], ones[: M - n])
    lib.stop_receiving()


# ------------------------------------------------------------------ ingest.PacketIngest, host logic

def test_packet_ingest_frame_count(native):
    import ingest
    util.configure("shipped")
    pi = ingest.PacketIngest(4)
    assert (pi.hop, pi.m_total, pi.stride, pi.rows, pi.columns, pi.protocol_ver) == (N, M, 8 + 4 * M, 8, 8, 2)
    assert [pi.n_frames(t) for t in (0, 255, 256, 257, 511, 512, 190 * 256)] == [0, 0, 1, 1, 1, 2, 190]
    half = ingest.PacketIngest(4, hop=N // 2)
    assert [half.n_frames(t) for t in (255, 256, 383, 384, 512)] == [0, 1, 1, 2, 3]
    one = ingest.PacketIngest(1, hop=1, m_total=64)
    assert [one.n_frames(t) for t in (255, 256, 257, 445)] == [0, 1, 2, 190]
    gap = ingest.PacketIngest(3, hop=N + 37)
    assert [gap.n_frames(t) for t in (256, 548, 549, 6 * 293 + 256)] == [1, 1, 2, 7]
    for F in (1, 2, 7, 190):                       # n_frames is the largest F the library accepts
        for p in (half, one, gap):
            T = (F - 1) * p.hop + N
            assert p.n_frames(T) == F and p.n_frames(T - 1) == F - 1
    util.configure("cfg5")
    assert ingest.PacketIngest(4).n_frames(4 * 1024 + 1023) == 4
    util.configure("shipped")


def test_packet_ingest_mask_construction(native):
    import ingest
    util.configure("shipped")
    assert ingest.PacketIngest(4).mask is None
    dead = ingest.default_disabled_mics()
    assert dead.dtype == np.int32 and dead.size == 122
    ref = ingest.PacketIngest(4, dead_mics="reference")
    assert ref.mask.dtype == np.uint8 and ref.mask.shape == (M,) and np.array_equal(np.flatnonzero(ref.mask), dead)
    small = ingest.PacketIngest(1, dead_mics="reference", m_total=100)              # rows outside the frame are dropped, as get_data's loop does
    assert small.mask.shape == (100,) and np.array_equal(np.flatnonzero(small.mask), dead[dead < 100])
    some = ingest.PacketIngest(3, dead_mics=(5, 191, 5, 200, 255))
    assert np.array_equal(np.flatnonzero(some.mask), [5, 191, 200, 255])
    assert np.array_equal(np.flatnonzero(ingest.PacketIngest(2, dead_mics=iter(range(128)), m_total=128).mask), np.arange(128))
    assert not ingest.PacketIngest(2, dead_mics=[]).mask.any()
    with pytest.raises(ValueError, match="dead_mics must be"):
        ingest.PacketIngest(4, dead_mics="all")
    with pytest.raises(ValueError, match="names row -1"):
        ingest.PacketIngest(4, dead_mics=[3, -1])


def test_packet_ingest_constructor_and_shape_validation(native):
    import torch
    import ingest
    util.configure("shipped")
    with pytest.raises(ValueError, match="n_arrays = 5: 320 rows must fit N_MICROPHONES = 256"):
        ingest.PacketIngest(5)
    with pytest.raises(ValueError, match="n_arrays = 0"):
        ingest.PacketIngest(0)
    with pytest.raises(ValueError, match="192 rows must fit N_MICROPHONES = 256 and m_total = 128"):
        ingest.PacketIngest(3, m_total=128)
    with pytest.raises(ValueError, match="hop = 0 < 1"):
        ingest.PacketIngest(4, hop=0)
    pi = ingest.PacketIngest(4)
    S = pi.stride
    with pytest.raises(ValueError, match="uint8"):
        pi.frames(torch.zeros((N, S), dtype=torch.int8))
    with pytest.raises(ValueError, match="uint8"):
        pi.frames(np.zeros((N, S), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"must be \[T, 1032\]"):
        pi.frames(torch.zeros((N, S - 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        pi.frames(torch.zeros((1, N, S), dtype=torch.uint8))
    with pytest.raises(ValueError, match="whole datagrams of 1032 bytes, got 264191 bytes"):
        pi.frames(torch.zeros(N * S - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="255 datagrams do not fill one frame of N_SAMPLES = 256"):
        pi.frames(torch.zeros((N - 1, S), dtype=torch.uint8))
    util.configure("cfg2")
    with pytest.raises(ValueError, match="built for 256 microphones x 256 samples, but the configured sizes are now 64 x 256"):
        pi.frames(torch.zeros((N, S), dtype=torch.uint8))          # sizes changed under an existing object: refused, not mis-sized
    assert ingest.PacketIngest(1).stride == 8 + 4 * 64 and ingest.PacketIngest(1).m_total == 64
    with pytest.raises(ValueError, match="128 rows must fit N_MICROPHONES = 64"):
        ingest.PacketIngest(2)
    util.configure("shipped")


def test_packet_ingest_without_gpu(native):
    """Well-formed packets on a box without a GPU: listen.py's error, no CPU fallback."""
    if native.gpu_available():
        pytest.skip("without a GPU only")
    import torch
    import ingest
    import pipeline
    util.configure("shipped")
    pi = ingest.PacketIngest(4, dead_mics="reference")
    for pk in (torch.zeros((2 * N, pi.stride), dtype=torch.uint8), torch.zeros(N * pi.stride, dtype=torch.uint8)):
        with pytest.raises(native.BeamformerError, match="no usable HIP device"):
            pi.frames(pk)
    assert hasattr(pipeline.FusedPipeline, "step_packets")


# ------------------------------------------------------------------ gfx950 resources of ingest_kernel.hip

@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel name without its mangling: metadata fields} of ingest_kernel.hip compiled for gfx950 with the build's flags."""
    import __graft_entry__ as ge
    src = os.path.join(ge.CSRC, "ingest_kernel.hip")
    out = str(tmp_path_factory.mktemp("ingest_isa") / "ingest_kernel.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + ge.HIPCC_FLAGS + ["--cuda-device-only", "-S", src, "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        short = re.search(r"\d+(ingest\w*kernel)E", name.group(1)).group(1)
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        found[short] = dict(vgprs=g("vgpr_count"), sgprs=g("sgpr_count"), lds=g("group_segment_fixed_size"), scratch=g("private_segment_fixed_size"),
                            vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"), wg=g("max_flat_workgroup_size"))
    return found, text


def test_ingest_kernels_compile_for_gfx950_without_scratch(resources):
    found, text = resources
    assert sorted(found) == ["ingest_kernel", "ingest_stream_kernel"]
    s = found["ingest_stream_kernel"]
    print("ingest_stream_kernel:", s)
    assert s["scratch"] == 0 and s["vgpr_spill"] == 0 and s["sgpr_spill"] == 0
    assert s["wg"] == 256 and s["vgprs"] <= 64             # eight waves per SIMD stay possible
    assert s["lds"] <= 20 * 1024                           # at least eight workgroups per CU
    # the one-frame kernel is untouched: its resource line is the one the build before this kernel was added reported
    assert found["ingest_kernel"] == dict(vgprs=8, sgprs=25, lds=16640, scratch=0, vgpr_spill=0, sgpr_spill=0, wg=256)


def test_ingest_stream_kernel_access_widths(resources):
    """The stream kernel's ISA holds the wide forms the design rests on: 8-byte datagram reads and 16-byte frame stores."""
    _, text = resources
    m = re.search(r"^(_ZN\S*ingest_stream_kernel\S*):[^\n]*\n(.*?)\n\.Lfunc_end", text, flags=re.S | re.M)
    assert m
    body = m.group(2)
    assert "global_load_dwordx2" in body and "global_store_dwordx4" in body
    assert not re.search(r"\bscratch_", body)
