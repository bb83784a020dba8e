"""GPU (-m gpu): bf_remove_sources_device and BeamListener.maps / remove / separate, bit for bit against tests/separate_np.py.

The kernel has four forms per algorithm -- 16-byte or 4-byte accesses of the frames, beams staged in LDS or read through L2 -- and
every one must give the restatement's bits: the edge cases run the 16-byte staged form, the long rows all four (a pointer 4 bytes
off a 16-byte boundary; 2 beams of 1024 samples fit the 32 KiB staging budget, 9 do not)."""
import numpy as np
import pytest

import separate_np as snp
import util
from support import nat
from test_miso_device import Tables, _run as miso_run, _rows as miso_rows
from test_remove_sources_host import MICS, exact_case

pytestmark = pytest.mark.gpu

SENTINEL = 16
SENTINEL_BITS = 0x7fc0beef      # a NaN with a payload nobody computes
ALGO_ID = {"pad": snp.PAD, "lerp": snp.LERP}


def _flat(torch, count, shift_floats):
    """A sentinel-filled device buffer of `count` floats + tail, starting `shift_floats` floats past a 16-byte boundary."""
    buf = torch.full((count + SENTINEL + shift_floats,), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    assert buf.data_ptr() % 16 == 0
    return buf[shift_floats:]


def _remove(nat, algo, x, mics, offs, beams, gain, inplace=False, shift=0, status=True):
    """bf_remove_sources_device on device copies -> (residual [F, M, N] as numpy, status numpy or None).  Checks the sentinel tail."""
    torch = util.torch_gpu()
    F, M, N = x.shape
    B, stride = beams.shape[1], beams.shape[2]
    src = _flat(torch, x.size, shift)
    src[:x.size] = torch.from_numpy(np.ascontiguousarray(x).ravel()).cuda()
    dst = src if inplace else _flat(torch, x.size, shift)
    d_off = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int32)).cuda()
    d_beams = torch.from_numpy(np.ascontiguousarray(beams, dtype=np.float32)).cuda()
    st = torch.full((F, B), -7, dtype=torch.int32, device="cuda") if status else None
    mics = np.ascontiguousarray(mics, dtype=np.int32)
    rc = nat.lib.bf_remove_sources_device(util.ALGOS[algo], src.data_ptr(), M, F, nat.iptr(mics), mics.size, d_off.data_ptr(), B, d_beams.data_ptr(), stride,
                                          float(gain), dst.data_ptr(), st.data_ptr() if status else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[x.size:].view(np.int32) == SENTINEL_BITS).all(), "the floats behind d_residual were written"
    if not inplace:
        assert src.cpu().numpy()[:x.size].tobytes() == np.ascontiguousarray(x).tobytes(), "d_signals was written"
    return host[:x.size].reshape(F, M, N).copy(), (st.cpu().numpy() if status else None)


def _same(got, want):
    assert got.dtype == want.dtype == np.float32
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.int32) != want.view(np.int32))[:8]


def _tables(nat, oracle_lib, algo, delays, N, n):
    """Load `delays` [D, n] for `algo` into the library -> (Tables, whole, h) of the restatement."""
    D = delays.shape[0]
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, 8), algo, delays, np.zeros((D, n, 8), np.float32), n, 8)
    whole, h = snp.pad_table(tab.whole, N) if algo == "pad" else snp.lerp_table(tab.d32, N)
    return tab, whole, h


# ------------------------------------------------------------------ 1. edges

def _edge_case():
    rng = np.random.default_rng(2024)
    M_total, N, D, F, B = 6, 32, 5, 3, 3
    n = MICS.size
    delays = rng.uniform(0, 12, (D, n))
    # 0, a whole number (h = 1), N - 1 and N - 2 (lerp windows of length 0 and 1), an entry >= N
    delays[0, 0], delays[0, 1], delays[1, 0], delays[1, 1], delays[2, 2], delays[3, 3] = 0.0, 7.0, N - 1 + 0.25, N - 2 + 0.5, N + 3.75, float(N)
    x = (rng.standard_normal((F, M_total, N)) * 0.25).astype(np.float32)
    beams = rng.standard_normal((F, B, N + 5)).astype(np.float32)
    offs = np.array([[0, n, 2 * n], [4 * n, -1, 3 * n], [D * n - n + 1, 2 * n, 0]], dtype=np.int32)
    beams[1, 1], beams[2, 0] = np.nan, np.nan                   # the rows of the rejected offsets: never read
    return M_total, N, D, delays, x, beams, offs


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("gain", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_edges(nat, oracle_lib, algo, gain, inplace):
    from interface import config
    M_total, N, D, delays, x, beams, offs = _edge_case()
    config.configure(N_MICROPHONES=M_total, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=8)
    _, whole, h = _tables(nat, oracle_lib, algo, delays, N, MICS.size)
    got, st = _remove(nat, algo, x, MICS, offs, beams, gain, inplace=inplace)
    want, want_st = snp.remove(ALGO_ID[algo], x, MICS, whole, h, offs, beams, gain)
    _same(got, want)
    assert st.tolist() == want_st.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0]]
    assert np.isfinite(got).all()
    _same(got[:, [2, 5]], x[:, [2, 5]])
    if gain == 0.0:
        _same(got, x)
    else:
        assert (got[:, MICS].view(np.int32) != x[:, MICS].view(np.int32)).any()


def test_null_status_and_unloaded_table(nat, oracle_lib):
    from interface import config
    M_total, N, D, delays, x, beams, offs = _edge_case()
    config.configure(N_MICROPHONES=M_total, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=8)
    _, whole, h = _tables(nat, oracle_lib, "lerp", delays, N, MICS.size)
    got, st = _remove(nat, "lerp", x, MICS, offs, beams, 1.0, status=False)
    assert st is None
    _same(got, snp.remove(snp.LERP, x, MICS, whole, h, offs, beams, 1.0)[0])
    torch = util.torch_gpu()
    nat.lib.unload_coefficients_pad()
    nat.lib.bf_clear_error()
    d = torch.zeros((M_total * N,), dtype=torch.float32, device="cuda")
    o = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    rc = nat.lib.bf_remove_sources_device(util.ALGOS["pad"], d.data_ptr(), M_total, 1, nat.iptr(MICS), MICS.size, o.data_ptr(), 1, d.data_ptr(), N, 1.0,
                                          d.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    with pytest.raises(nat.BeamformerError, match="bf_remove_sources_device: load_coefficients_pad has not been called"):
        nat.check()


# ------------------------------------------------------------------ 2. real tables, beams made by bf_miso_device, the Python front end

@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_cfg1_tables_and_listener(nat, oracle_lib, algo):
    torch = util.torch_gpu()
    import listen
    import synth
    c = util.configure("cfg1")
    M, N, D = c["M"], c["N"], c["X"] * c["Y"]
    mics = np.arange(M, dtype=np.int32)
    table = util.table_for(algo, "cfg1")
    if algo == "pad":
        nat.lib.load_coefficients_pad(nat.iptr(table), table.size)
        whole, h = snp.pad_table(table, N)
    else:
        nat.lib.load_coefficients_lerp(nat.fptr(table), table.size)
        whole, h = snp.lerp_table(table, N)
    nat.check()
    F, B = 5, 2
    frames = synth.frame_batch(M, N, F, seed0=300)
    rng = np.random.default_rng(3)
    offs = (rng.integers(0, D, (F, B)) * M).astype(np.int32)
    out, st = miso_run(nat, algo, frames, mics, offs)
    beams = miso_rows(out, F, B, N).copy()
    assert (st.cpu().numpy() == 0).all() and np.isfinite(beams).all()
    want, _ = snp.remove(ALGO_ID[algo], frames, mics, whole, h, offs, beams, 0.75)
    got, st = _remove(nat, algo, frames, mics, offs, beams, 0.75)
    _same(got, want)
    assert (st == 0).all() and (got != frames).any()
    # the front end: out of place, then in place
    bl = listen.BeamListener(algo, mics=mics)
    d_frames = torch.from_numpy(frames).cuda()
    d_beams, _ = bl.listen(d_frames, offs)
    res, st = bl.remove(d_frames, offs, d_beams, gain=0.75)
    torch.cuda.synchronize()
    assert res.shape == (F, M, N) and res.dtype == torch.float32 and st.shape == (F, B) and st.dtype == torch.int32
    _same(res.cpu().numpy(), want)
    _same(d_frames.cpu().numpy(), frames)
    res2, _ = bl.remove(d_frames, offs, d_beams, gain=0.75, out=d_frames)
    torch.cuda.synchronize()
    assert res2 is d_frames
    _same(d_frames.cpu().numpy(), want)


# ------------------------------------------------------------------ 3. long rows: every form of the kernel

@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "4_bytes_off"])
@pytest.mark.parametrize("B", [2, 9], ids=["staged", "through_l2"])
@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_long_rows(nat, oracle_lib, algo, B, shift):
    from interface import config
    M_total, N, D, F = 8, 1024, 3, 2
    mics = np.array([7, 1, 2, 5, 0, 3], dtype=np.int32)
    config.configure(N_MICROPHONES=M_total, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=8)
    rng = np.random.default_rng(1024)
    delays = rng.uniform(0, 300, (D, mics.size))
    delays[1, 2] = 300.0
    _, whole, h = _tables(nat, oracle_lib, algo, delays, N, mics.size)
    x = (rng.standard_normal((F, M_total, N)) * 0.25).astype(np.float32)
    beams = rng.standard_normal((F, B, N)).astype(np.float32)
    offs = (rng.integers(0, D, (F, B)) * mics.size).astype(np.int32)
    offs[1, B - 1] = -1
    beams[1, B - 1] = np.nan
    want, want_st = snp.remove(ALGO_ID[algo], x, mics, whole, h, offs, beams, 1.0)
    for inplace in (False, True):
        got, st = _remove(nat, algo, x, mics, offs, beams, 1.0, inplace=inplace, shift=shift)
        _same(got, want)
        assert (st == want_st).all()
    _same(want[:, [4, 6]], x[:, [4, 6]])


# ------------------------------------------------------------------ 4. the adjoint of the library's own beam kernel

@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_adjoint_of_the_beam_kernel(nat, oracle_lib, algo):
    from interface import config
    M_total, N = 6, 32
    config.configure(N_MICROPHONES=M_total, N_SAMPLES=N, MAX_RES_X=1, MAX_RES_Y=1, N_TAPS=8)
    n = MICS.size
    for seed in (0, 1, 2):
        x, o, _, _, d32 = exact_case(ALGO_ID[algo], seed)
        _tables(nat, oracle_lib, algo, d32.astype(np.float64)[None, :], N, n)
        zero = np.zeros((1, 1), dtype=np.int32)
        out, st = miso_run(nat, algo, x[None], MICS, zero)
        fwd = miso_rows(out, 1, 1, N)[0, 0]
        # frames of zeros, gain = -n: c = -1 exactly and the residual is the adjoint of o
        adj, _ = _remove(nat, algo, np.zeros_like(x)[None], MICS, zero, o[None, None], -float(n))
        lhs = np.sum(fwd.astype(np.float64) * o.astype(np.float64))
        rhs = np.sum(x.astype(np.float64) * adj[0].astype(np.float64))
        assert lhs == rhs and lhs != 0.0, (lhs, rhs)
        assert (adj[0][[2, 5]] == 0).all()


# ------------------------------------------------------------------ 5. the most beams one call takes

@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_64_beams_in_order(nat, oracle_lib, algo):
    from interface import config
    M_total, N, D, F, B = 6, 32, 5, 2, 64
    config.configure(N_MICROPHONES=M_total, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=8)
    rng = np.random.default_rng(64)
    delays = rng.uniform(0, 20, (D, MICS.size))
    _, whole, h = _tables(nat, oracle_lib, algo, delays, N, MICS.size)
    x = (rng.standard_normal((F, M_total, N)) * 0.25).astype(np.float32)
    # beams of very different sizes: a float32 sum of these depends on its order
    beams = (rng.standard_normal((F, B, N)) * 10.0 ** rng.integers(-3, 4, (F, B, 1))).astype(np.float32)
    offs = (rng.integers(0, D, (F, B)) * MICS.size).astype(np.int32)
    want, _ = snp.remove(ALGO_ID[algo], x, MICS, whole, h, offs, beams, 1.0)
    backwards, _ = snp.remove(ALGO_ID[algo], x, MICS, whole, h, offs[:, ::-1], beams[:, ::-1], 1.0)
    assert want.tobytes() != backwards.tobytes()
    got, st = _remove(nat, algo, x, MICS, offs, beams, 1.0)
    _same(got, want)
    assert (st == 0).all()


# ------------------------------------------------------------------ 6. maps -> sources -> listen -> remove as one captured graph

def test_graph_of_one_iteration(nat, oracle_lib):
    torch = util.torch_gpu()
    import listen
    import synth
    c = util.configure("cfg1")
    M, N, X, Y = c["M"], c["N"], c["X"], c["Y"]
    table = util.table_for("lerp", "cfg1")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    bl = listen.BeamListener("lerp", mics=np.arange(M, dtype=np.int32))
    F = 3
    batches = [synth.frame_batch(M, N, F, seed0=s) for s in (500, 600, 700)]
    x = torch.from_numpy(batches[0]).cuda()
    res = torch.empty_like(x)
    kept = {}

    def step():
        power = bl.maps(x)
        offs, vals, _ = bl.sources(power, 1, max(X, Y), 0.0, 0.0)
        beam, _ = bl.listen(x, offs)
        _, st = bl.remove(x, offs, beam, 1.0, out=res)
        kept.update(offs=offs, vals=vals, beam=beam, st=st)

    def snapshot():
        torch.cuda.synchronize()
        return [res.cpu().numpy().copy()] + [kept[k].cpu().numpy().copy() for k in ("offs", "vals", "beam", "st")]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up: digest built, row map uploaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    captured = dict(kept)
    replays = []
    for batch in batches[1:]:
        x.copy_(torch.from_numpy(batch).cuda())
        g.replay()
        kept.update(captured)
        replays.append(snapshot())
    for batch, got in zip(batches[1:], replays):
        x.copy_(torch.from_numpy(batch).cuda())
        step()
        want = snapshot()
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        assert (want[4] == 0).all() and (want[0] != batch).any()
    assert replays[0][0].tobytes() != replays[1][0].tobytes()


# ------------------------------------------------------------------ 7. end to end: the weak source under the strong one's response

def test_separate_finds_the_weak_source(nat, oracle_lib):
    torch = util.torch_gpu()
    import listen
    from interface import config
    s = snp.SCENE
    rows, cols, M, N = s["rows"], s["cols"], s["M"], s["N"]
    frames, table, (w_offs, w_vals, w_beams, w_res), plain = snp.scene_reference(oracle_lib)
    config.configure(N_MICROPHONES=M, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=rows, MAX_RES_Y=cols, N_TAPS=8)
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    bl = listen.BeamListener("lerp", mics=np.arange(M, dtype=np.int32))
    d_frames = torch.from_numpy(frames.copy()).cuda()
    offs, vals, beams, res = bl.separate(d_frames, 2, gain=1.0)
    d_plain = bl.maps(d_frames)
    p_offs, _, _ = bl.sources(d_plain, 2, 3, floor_rel=0.0)
    torch.cuda.synchronize()
    assert offs.shape == (2, 2) and offs.dtype == torch.int32 and vals.shape == (2, 2) and beams.shape == (2, 2, N) and res.shape == (2, M, N)
    _same(d_frames.cpu().numpy(), frames)                                   # the input is left alone
    offs, p_offs = offs.cpu().numpy(), p_offs.cpu().numpy()
    assert (offs == w_offs).all(), (offs, w_offs)
    _same(vals.cpu().numpy(), w_vals)
    _same(beams.cpu().numpy(), w_beams)
    _same(res.cpu().numpy(), w_res)
    _same(d_plain.cpu().numpy(), plain)
    for f, (a_dir, b_dir) in enumerate(((s["A"], s["B"]), (s["B"], s["A"]))):
        da, db = snp.chebyshev(offs[f, 0], M, cols, a_dir), snp.chebyshev(offs[f, 1], M, cols, b_dir)
        near = [snp.chebyshev(o, M, cols, b_dir) for o in p_offs[f] if o >= 0]
        print("frame %d: first component %s from A, second %s from B; plain peaks %s from B" % (f, da, db, near))
        assert da is not None and da <= 1
        assert db is not None and db <= 2
        assert all(d > 2 for d in near)
