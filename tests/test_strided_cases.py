"""GPU (-m gpu): every row of tests/strided_cases.py -- each instantiation and tiling class of das_mimo_kernel<.., true>, das_select_kernel and
das_miso_kernel<.., true> (csrc/das_strided.hip; true = HIST, the continuous-stream mode) -- through bf_das_stream_device, bf_das_select_device, bf_das_select_stream_device and
bf_miso_stream_device.  Each row asserts

  1. what ran: bf_last_strided_plan after the launch names the row's kernel, algorithm, NC, DPW, chunk count and tile size, and
     equals the plan the planner export gave for the row's sizes;
  2. every output equal IN BITS to the committed C checker: the extended-window restatement for the stream rows, select_np.powers
     for the window-local ones; status words equal; rejected entries the quiet NaN 0x7fc00000 (a NaN for any NaN on hostile rows only);
  3. canary blocks in front of and behind every output and status buffer untouched, and the gap of every row;
  4. a select-stream row's values equal, byte for byte, what bf_das_stream_device writes at the same directions of the same stream.

Tables, streams and expectations come from strided_cases (shared with the CPU file, which holds them finite and positive); the select
calls go through test_das_select._call, the tables through test_miso_device.Tables.  The map and beam calls have launchers of their own
here: test_stream's keep a sentinel behind the output only, and these rows want one in front as well.  The last test prints how many
instantiations ran and, when every row ran, asserts that they are all 90."""
import ctypes as C

import numpy as np
import pytest

import strided_cases as sc
import util
from support import nat
from test_das_select import CANARY, CANARY_BITS, _call
from test_miso_device import MIC_GAIN, Tables

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
RAN = {}            # row name -> the instantiation bf_last_strided_plan reported


def _rows(kernel):
    return pytest.mark.parametrize("row", [r for r in sc.ROWS if r.kernel == kernel], ids=lambda r: r.name)


def _load(nat, row):
    """The planner's answer for the row (before anything is launched), then the row's sizes and table in the product."""
    from interface import config
    want_plan = sc.export(nat.lib, row)
    config.configure(N_MICROPHONES=row.M_total, N_SAMPLES=row.N, MAX_RES_X=row.D, MAX_RES_Y=1, N_TAPS=row.T)
    mics, delays, taps, tab = sc.tables(row)
    loaded = Tables(nat, None, row.algo, delays, taps, row.n, row.T)
    assert loaded.entries == tab.entries and np.array_equal(loaded.whole, tab.whole)
    if row.algo in sc.PLAIN:
        assert nat.lib.bf_stream_history(util.ALGOS[row.algo]) == sc.history(row)
    return want_plan, mics


def _ran(nat, row, want_plan):
    """bf_last_strided_plan names the row's instantiation and the export's plan: asserted on what was dispatched, not predicted."""
    out = (C.c_longlong * 12)(*([-7] * 12))
    assert nat.lib.bf_last_strided_plan(out) == 0, nat.lib.bf_last_error()
    got = dict(zip(sc.PLAN_KEYS, list(out)[:10]))
    assert sc.KERNELS[out[10]] == row.kernel and out[11] == util.ALGOS[row.algo], list(out)
    assert got["nc"] == row.NC and (got["n_chunks"] > 1) == (row.chunks == "several"), got
    if row.kernel != "beam":
        assert got["dpw"] == row.DPW and sc.tile_class(got, row.count, row.F) == row.tile, got
    assert got == want_plan, (got, want_plan)
    RAN[row.name] = (row.kernel, row.algo, got["nc"], None if row.kernel == "beam" else got["dpw"])


def _canaried(words):
    torch = util.torch_gpu()
    return torch.full((CANARY + words + CANARY,), CANARY_BITS, dtype=torch.int32, device="cuda")


def _payload(buf, rows, stride, used):
    """The [rows, used] payload of a canaried buffer as uint32, after checking both canary blocks and every row's gap."""
    host = buf.cpu().numpy()
    assert (host[:CANARY] == CANARY_BITS).all() and (host[CANARY + rows * stride:] == CANARY_BITS).all()
    body = host[CANARY:CANARY + rows * stride].reshape(rows, stride)
    assert (body[:, used:] == CANARY_BITS).all()
    return np.ascontiguousarray(body[:, :used]).view(np.uint32)


def _dev(a):
    return None if a is None else util.torch_gpu().from_numpy(np.ascontiguousarray(a)).cuda()


def _map_call(nat, row, mics, frames, hop, prev, gap=3):
    """bf_das_stream_device on directions [d0, d0 + count) into rows of count + gap floats -> float32 [F, count]."""
    torch = util.torch_gpu()
    F, stride = frames.shape[0], row.count + gap
    d_sig, d_prev = _dev(frames), _dev(prev)
    buf = _canaried(F * stride)
    rc = nat.lib.bf_das_stream_device(util.ALGOS[row.algo], d_sig.data_ptr(), row.M_total, buf.data_ptr() + 4 * CANARY, stride, F, hop,
                                      None if d_prev is None else d_prev.data_ptr(), nat.iptr(mics), row.n, row.d0, row.d0 + row.count,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert nat.lib.bf_last_das_variant() == 9
    return _payload(buf, F, stride, row.count).view(np.float32)


def _beam_call(nat, row, mics, frames, hop, prev, offsets, gain, gap=5):
    """bf_miso_stream_device with out_stride = N + gap -> (float32 [F, B, N], status int32 [F, B])."""
    torch = util.torch_gpu()
    F, B, stride = frames.shape[0], offsets.shape[1], row.N + gap
    d_sig, d_prev, d_off = _dev(frames), _dev(prev), _dev(np.ascontiguousarray(offsets, dtype=np.int32))
    buf, st = _canaried(F * B * stride), _canaried(F * B)
    before = nat.lib.bf_last_das_variant()
    rc = nat.lib.bf_miso_stream_device(util.ALGOS[row.algo], d_sig.data_ptr(), row.M_total, F, hop, None if d_prev is None else d_prev.data_ptr(), nat.iptr(mics),
                                       row.n, d_off.data_ptr(), B, float(gain), buf.data_ptr() + 4 * CANARY, stride, st.data_ptr() + 4 * CANARY,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert nat.lib.bf_last_das_variant() == before
    return _payload(buf, F * B, stride, row.N).view(np.float32).reshape(F, B, row.N), _payload(st, 1, F * B, F * B).view(np.int32).reshape(F, B)


def _equal(got, want, row):
    hostile = "hostile" in row.tags
    assert got.shape == want.shape
    assert hostile or not np.isnan(want).any() or (want.view(np.uint32)[np.isnan(want)] == NAN_BITS).all()
    assert util.bits_differ(got, want, nan_is_nan=hostile) == ""


# ------------------------------------------------------------------ das_mimo_kernel<.., true>

@_rows("map")
def test_stream_map_row(nat, oracle_lib, row):
    want_plan, mics = _load(nat, row)
    hop = sc.hop_of(row)
    for with_prev in ((True, False) if row.tile == "small" else (True,)):        # d_prev given; NULL (silence before the stream) on the small rows
        st, full = sc.stream_map(oracle_lib, row, with_prev)
        got = _map_call(nat, row, mics, st.frames(), hop, st.prev())
        _ran(nat, row, want_plan)
        _equal(got, np.ascontiguousarray(full[:, row.d0:row.d0 + row.count]), row)
        if "hostile" in row.tags:
            # the row discriminates: NaN, finite and (pad; lerp's difference of two infinities is a NaN) infinite powers all occur
            assert np.isnan(got).any() and np.isfinite(got).any() and (np.isinf(got).any() or row.algo == "lerp")


# ------------------------------------------------------------------ das_select_kernel<.., false>

@_rows("select")
def test_select_row(nat, oracle_lib, row):
    want_plan, mics = _load(nat, row)
    offs, _ = sc.listed(row)
    frames = sc.window_frames(row)
    want, want_st = sc.want_listed(oracle_lib, row)
    got, status = _call(nat, row.algo, frames, mics, offs, gap=3)
    _ran(nat, row, want_plan)
    assert np.array_equal(status, want_st) and (got.view(np.uint32)[want_st != 0] == NAN_BITS).all()
    _equal(got, want, row)
    if row.tile == "small":                                                      # a shared list, no status array: the same values
        shared, none = _call(nat, row.algo, frames, mics, offs[0], status=False)
        want0, _ = sc.select_np.powers(oracle_lib, sc.tables(row)[3], frames, mics, np.broadcast_to(offs[0], offs.shape), row.N)
        assert none is None
        _equal(shared, want0, row)


# ------------------------------------------------------------------ das_select_kernel<.., true>

@_rows("select_hist")
def test_select_stream_row(nat, oracle_lib, row):
    want_plan, mics = _load(nat, row)
    hop = sc.hop_of(row)
    offs, dirs = sc.listed(row)
    st, _ = sc.stream_map(oracle_lib, row)
    want, want_st = sc.want_listed(oracle_lib, row)
    frames, prev = st.frames(), st.prev()
    got, status = _call(nat, row.algo, frames, mics, offs, gap=2, stream=(hop, prev))
    _ran(nat, row, want_plan)
    assert np.array_equal(status, want_st) and (got.view(np.uint32)[want_st != 0] == NAN_BITS).all()
    _equal(got, want, row)
    # the map call on the same sizes, table and stream (the row's twin in the table): byte for byte at the listed directions
    assert "twin" in row.tags
    img = _map_call(nat, row._replace(kernel="map", count=row.D, d0=0), mics, frames, hop, prev)
    ok = want_st == 0
    assert got[ok].tobytes() == np.take_along_axis(img, dirs, axis=1)[ok].tobytes()
    if row.tile == "small":                                                      # silence before the stream, a shared list, no status array
        st0, full0 = sc.stream_map(oracle_lib, row, False)
        shared, none = _call(nat, row.algo, st0.frames(), mics, offs[0], status=False, stream=(hop, None))
        want0 = np.ascontiguousarray(full0[:, dirs[0]])
        want0.view(np.uint32)[:, want_st[0] != 0] = NAN_BITS
        assert none is None
        _equal(shared, want0, row)


# ------------------------------------------------------------------ das_miso_kernel<.., true>

@_rows("beam")
def test_stream_beam_row(nat, oracle_lib, row):
    """1, 16 and 17 beams (one wave, a full group, a group and one), hop N, N / 2 and H, d_prev given and NULL; mic_gain on the 17."""
    want_plan, mics = _load(nat, row)
    for hop in sc.hops(row):
        assert sc.history(row) <= hop <= row.N
        for with_prev in (True, False):
            st = sc.make_stream(row, hop, with_prev, mics)
            frames, prev = st.frames(), st.prev()
            for B in (1, 16, 17):
                offs = sc.beam_offsets(row, B)
                gain = MIC_GAIN if B == 17 else 0.0
                want, want_st = sc.stream_beams(oracle_lib, row, st, offs)
                if gain:
                    ok = want_st == 0
                    with np.errstate(invalid="ignore", over="ignore"):
                        want[ok] = (want[ok] / np.float32(row.n)) * np.float32(gain)
                    assert want.dtype == np.float32
                got, status = _beam_call(nat, row, mics, frames, hop, prev, offs, gain)
                _ran(nat, row, want_plan)
                assert np.array_equal(status, want_st) and want_st.sum() == (row.F if B >= 16 else 0)
                assert (got.view(np.uint32)[want_st != 0] == NAN_BITS).all()
                _equal(got, want, row)


# ------------------------------------------------------------------ the union

def test_every_instantiation_ran(capsys):
    ran = set(RAN.values())
    with capsys.disabled():
        print("\n[strided cases] %d rows ran %d of the 90 instantiations of das_mimo_kernel<.., true>, das_select_kernel and das_miso_kernel<.., true>" % (len(RAN), len(ran)))
    assert ran <= sc.all_instantiations()
    if len(RAN) == len(sc.ROWS):                                                 # (a run of a few rows, -k, has nothing to claim)
        assert sorted(map(str, sc.all_instantiations() - ran)) == []
