"""GPU (-m gpu): bf_das_select_device / bf_das_select_stream_device, BeamListener.powers and zoom.CoarseToFine, bit for bit against
tests/select_np.py (the committed C checker on the listed table rows; the extended-window restatement of tests/test_stream.py for the
stream call) and against the map calls themselves.

Every output sits between canary blocks; d_status is compared wherever it is given.  Shapes are the smallest that reach a branch of
das_select_kernel: the plan of every case that is there for a tiling branch is read back from bf_plan_das_select (256 compute units,
the MI355X's) and asserted, so a change of the planner cannot silently empty a case."""
import ctypes as C

import numpy as np
import pytest

import select_np
import util
from support import nat
from test_miso_device import Tables
from test_stream import Case, Stream

pytestmark = pytest.mark.gpu

ALGOS = ["pad", "lerp", "hybrid", "fir_vec"]
CANARY = 64
CANARY_BITS = 0x7FA5A5A5            # a NaN no kernel writes
NAN_BITS = select_np.NAN_BITS


class Setup:
    """Sizes, microphone list and table of one case, loaded into the product."""

    def __init__(self, nat, algo, M_total, n, N, D, pmax, T=8, seed=0):
        from interface import config
        config.configure(N_MICROPHONES=M_total, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=T)
        rng = np.random.default_rng([seed, M_total, n, N, D])
        self.M_total, self.n, self.N, self.D, self.T, self.algo = M_total, n, N, D, T, algo
        self.mics = (np.arange(M_total) if n == M_total else rng.choice(M_total, n, replace=False)).astype(np.int32)
        delays = rng.uniform(0, pmax, size=(D, n))
        taps = rng.uniform(-0.5, 0.5, size=(D, n, T)).astype(np.float32)
        self.tab = Tables(nat, None, algo, delays, taps, n, T)
        self.max_whole = int(min(self.tab.whole.max(), N)) if algo != "fir_vec" else 0
        self.rng = rng

    def frames(self, F):
        return (self.rng.standard_normal((F, self.M_total, self.N)) * 0.25).astype(np.float32)

    def plan(self, nat, F, count, stream=False):
        out = (C.c_longlong * 10)()
        assert nat.lib.bf_plan_das_select(util.ALGOS[self.algo], self.n, F, count, self.max_whole, int(stream), 256, out) == 0
        return dict(zip(("nc", "lead", "row_stride", "mic_chunk", "n_chunks", "waves", "dpw", "tile_dirs", "n_tiles", "lds"), out))


def _call(nat, algo, frames, mics, offsets, gap=0, status=True, stream=None):
    """One select call on device copies: offsets [B] (shared list) or [F, B]; stream = (hop, prev or None) for the stream call.
    -> (power [F, B] host, status [F, B] host or None), after checking the canaries and the untouched gap of every row."""
    torch = util.torch_gpu()
    F, M, N = frames.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    B = offsets.shape[-1]
    stride = B + gap
    d_sig = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    d_off = torch.from_numpy(offsets).cuda()
    buf = torch.full((CANARY + F * stride + CANARY,), CANARY_BITS, dtype=torch.int32, device="cuda")
    st = torch.full((CANARY + F * B + CANARY,), -7, dtype=torch.int32, device="cuda")
    p_ptr, s_ptr = buf.data_ptr() + 4 * CANARY, (st.data_ptr() + 4 * CANARY) if status else None
    s = torch.cuda.current_stream().cuda_stream
    if stream is None:
        rc = nat.lib.bf_das_select_device(util.ALGOS[algo], d_sig.data_ptr(), M, F, nat.iptr(mics), mics.size, d_off.data_ptr(), B, int(offsets.ndim == 2),
                                          p_ptr, stride, s_ptr, s)
    else:
        hop, prev = stream
        d_prev = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev)).cuda()
        rc = nat.lib.bf_das_select_stream_device(util.ALGOS[algo], d_sig.data_ptr(), M, F, hop, None if d_prev is None else d_prev.data_ptr(), nat.iptr(mics),
                                                 mics.size, d_off.data_ptr(), B, int(offsets.ndim == 2), p_ptr, stride, s_ptr, s)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    host, sth = buf.cpu().numpy(), st.cpu().numpy()
    assert (host[:CANARY] == CANARY_BITS).all() and (host[CANARY + F * stride:] == CANARY_BITS).all()
    rows = host[CANARY:CANARY + F * stride].reshape(F, stride)
    assert (rows[:, B:] == CANARY_BITS).all()                              # floats [count, power_stride) of every row untouched
    assert (sth[:CANARY] == -7).all() and (sth[CANARY + F * B:] == -7).all()
    if not status:
        assert (sth == -7).all()
    return np.ascontiguousarray(rows[:, :B]).view(np.float32), sth[CANARY:CANARY + F * B].reshape(F, B) if status else None


def _check(nat, oracle_lib, su, frames, offsets, hostile=False, **kw):
    got, st = _call(nat, su.algo, frames, su.mics, offsets, **kw)
    F = frames.shape[0]
    per_frame = np.broadcast_to(np.asarray(offsets), (F, np.shape(offsets)[-1]))
    want, want_st = select_np.powers(oracle_lib, su.tab, frames, su.mics, per_frame, su.N)
    if st is not None:
        assert np.array_equal(st, want_st)
    assert np.array_equal(got.view(np.uint32)[want_st != 0], np.full(int((want_st != 0).sum()), NAN_BITS, dtype=np.uint32))
    assert np.isfinite(want[want_st == 0]).all() or hostile
    assert util.bits_differ(got, want, nan_is_nan=hostile) == ""
    return got


# ------------------------------------------------------------------ 1. the window-local call: sizes, list shapes, tilings

@pytest.mark.parametrize("algo", ALGOS)
def test_one_entry_one_frame_one_column_per_lane(nat, oracle_lib, algo):
    """N_SAMPLES = 64, 16 microphones (a power of two: the reciprocal multiply), a shared list of one entry, one frame; no status."""
    su = Setup(nat, algo, 16, 16, 64, 12, 12.0)
    _check(nat, oracle_lib, su, su.frames(1), [su.tab.offset(7)], status=False)


@pytest.mark.parametrize("count", [16, 17], ids=["full_group", "group_plus_one"])
@pytest.mark.parametrize("algo", ALGOS)
def test_wave_groups(nat, oracle_lib, algo, count):
    """N_SAMPLES = 256, n = 64, a grid of 12 directions, 3 frames with lists that differ: exactly one wave group (16 entries, one per
    wave) and one group plus one entry."""
    su = Setup(nat, algo, 64, 64, 256, 12, 47.0)
    p = su.plan(nat, 3, count)
    assert p["waves"] * p["dpw"] == 16 and p["n_chunks"] == 1
    dirs = np.array([[(5 * b + 3 * f) % 12 for b in range(count)] for f in range(3)])
    _check(nat, oracle_lib, su, su.frames(3), su.tab.offset(dirs))


@pytest.mark.parametrize("N", [100, 102, 99], ids=["N100", "N102_fused_tail", "N99_odd"])
@pytest.mark.parametrize("algo", ALGOS)
def test_rejected_entries_gather_and_row_gap(nat, oracle_lib, algo, N):
    """n = 5 rows gathered out of 7 (true division), N not a multiple of 64 / of 4 / odd, 3 frames, unsorted per-frame lists with
    repeats and rejected entries between good ones (-1, one past the table, for fir_vec an offset off a multiple of N_TAPS, and an
    offset that is no row start: accepted, as bf_miso_device accepts it), power_stride = count + 3."""
    su = Setup(nat, algo, 7, 5, N, 12, 30.0)
    t = su.tab
    last = t.offset(11)
    row = [t.offset(4), -1, t.offset(0), last + 1, last, t.offset(4), -2 ** 31, t.offset(9), 2 ** 31 - 1, t.offset(2) + t.per * 3, t.offset(11)]
    if algo == "fir_vec":
        row += [su.T + 3, t.offset(1)]
    offs = np.array([np.roll(row, f) for f in range(3)], dtype=np.int64)
    got = _check(nat, oracle_lib, su, su.frames(3), offs, gap=3)
    assert np.isnan(got).sum() == 3 * (5 if algo == "fir_vec" else 4)


@pytest.mark.parametrize("algo", ALGOS)
def test_three_workgroups_per_frame_last_partial_shared_list(nat, oracle_lib, algo):
    """301 entries shared by 3 frames: tiles of 4 entries, 76 workgroups per frame, the last with one entry; d_status NULL."""
    su = Setup(nat, algo, 7, 5, 102, 12, 30.0)
    p = su.plan(nat, 3, 301)
    assert p["n_tiles"] >= 3 and 301 % p["tile_dirs"] != 0 and p["tile_dirs"] > 1
    dirs = su.rng.integers(0, 12, 301)
    _check(nat, oracle_lib, su, su.frames(3), su.tab.offset(dirs), status=False)


@pytest.mark.parametrize("algo", ALGOS)
def test_several_groups_per_tile(nat, oracle_lib, algo):
    """2200 entries x 16 frames: tiles of two wave groups, so a wave walks groups whose entries it requested a group ahead; rejected
    entries among them."""
    su = Setup(nat, algo, 7, 5, 64, 12, 20.0)
    p = su.plan(nat, 16, 2200)
    assert p["tile_dirs"] >= 2 * p["waves"] * p["dpw"] and 2200 % p["tile_dirs"] != 0
    offs = su.tab.offset(su.rng.integers(0, 12, (16, 2200)))
    offs[:, ::37] = -1
    _check(nat, oracle_lib, su, su.frames(16), offs)


@pytest.mark.parametrize("count,F", [(8, 2), (2100, 8)], ids=["8_entries", "whole_groups"])
@pytest.mark.parametrize("algo", ALGOS)
def test_several_microphone_chunks(nat, oracle_lib, algo, count, F):
    """N_SAMPLES = 1024 and 40 microphones: the frame does not fit LDS beside the power scratch, bf_plan_das and the select plan both
    stage it in chunks, and a wave carries 4 (hybrid: 2) entries across them.  8 listed directions leave one entry per wave; 2100
    x 8 frames fill whole groups, so every wave carries its full set."""
    su = Setup(nat, algo, 40, 40, 1024, 12, 100.0)
    das = (C.c_longlong * 10)()
    assert nat.lib.bf_plan_das(util.ALGOS[algo], 40, F, 0, 12, su.max_whole, 256, das) == 0 and das[4] > 1
    p = su.plan(nat, F, count)
    assert p["n_chunks"] > 1 and p["dpw"] == (2 if algo == "hybrid" else 4)
    if count > 8:
        assert p["tile_dirs"] == p["waves"] * p["dpw"]
    offs = su.tab.offset(su.rng.integers(0, 12, (F, count)))
    offs[:, 5::11] = -1
    _check(nat, oracle_lib, su, su.frames(F), offs)


@pytest.mark.parametrize("algo", ALGOS)
def test_hostile_samples(nat, oracle_lib, algo):
    """Frames of NaN, Inf, subnormals and signed zeros: the same bits as the checker, a NaN for a NaN whatever its payload."""
    su = Setup(nat, algo, 7, 5, 100, 12, 30.0)
    frames = su.frames(3)
    frames[0, :, ::7] = np.float32(1e-41)
    frames[0, 2, 5:9] = [0.0, -0.0, np.float32(-1e-44), 0.0]
    frames[1, su.mics[1], 17] = np.nan
    frames[1, su.mics[3], 60] = np.inf
    frames[2, su.mics[0], 3] = -np.inf
    frames[2, su.mics[4]] = -0.0
    offs = su.tab.offset(np.array([[b % 12 for b in range(14)]] * 3))
    offs[:, 6] = -1
    _check(nat, oracle_lib, su, frames, offs, hostile=True)


def test_unloaded_table_is_an_error(nat):
    torch = util.torch_gpu()
    Setup(nat, "pad", 7, 5, 64, 12, 20.0)
    nat.lib.unload_coefficients_lerp()
    nat.lib.bf_clear_error()
    z = torch.zeros(7 * 64, dtype=torch.float32, device="cuda")
    o = torch.zeros(4, dtype=torch.int32, device="cuda")
    p = torch.zeros(4, dtype=torch.float32, device="cuda")
    rc = nat.lib.bf_das_select_device(util.ALGOS["lerp"], z.data_ptr(), 7, 1, nat.iptr(np.arange(5, dtype=np.int32)), 5, o.data_ptr(), 4, 0, p.data_ptr(),
                                      4, None, None)
    assert rc == -1
    with pytest.raises(nat.BeamformerError, match="bf_das_select_device: load_coefficients_lerp has not been called"):
        nat.check()


# ------------------------------------------------------------------ 2. equal to bf_das_device, whichever family it chose

# bf_last_das_variant per grid: at cfg1's 121 directions pad and lerp take the 8-wave one-frame sweep (family 2: grids under 256 directions),
# hybrid its two-frame kernel; on the 41 x 23 grid all three take their two-frame kernels (5, 8, 7).
FAMILY = {"cfg1": {"pad": 2, "lerp": 2, "hybrid": 7}, "g41x23": {"pad": 5, "lerp": 8, "hybrid": 7}}


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("algo", ["pad", "lerp", "hybrid"])
@pytest.mark.parametrize("grid", ["cfg1", "g41x23"])
def test_equals_the_map_kernels_image(nat, grid, algo, F):
    """cfg1 and the 41 x 23 grid (64 x 256) with 2 and 3 frames, where bf_das_device takes the families above: powers at every
    direction in a shuffled order, another one per frame, is its image byte for byte.  The select call leaves bf_last_das_variant alone."""
    torch = util.torch_gpu()
    import directions_np
    import listen
    from interface import config
    if grid == "cfg1":
        c = util.configure("cfg1")
        table = util.table_for(algo, "cfg1")
    else:
        c = dict(M=64, N=256, X=41, Y=23)
        config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=256, MAX_RES_X=41, MAX_RES_Y=23, N_TAPS=8)
        delays = directions_np.calculate_delays(41, 23, arrays=1)
        table = directions_np.whole_samples(delays) if algo == "pad" else np.float32(delays)
    if algo == "pad":
        t = np.ascontiguousarray(table, dtype=np.int32).ravel()
        nat.lib.load_coefficients_pad(nat.iptr(t), t.size)
    else:
        t = np.ascontiguousarray(table, dtype=np.float32).ravel()
        getattr(nat.lib, "load_coefficients_lerp" if algo == "lerp" else "load_coefficients_convolve_hybrid")(nat.fptr(t), t.size)
    nat.check()
    D = c["X"] * c["Y"]
    rng = np.random.default_rng([5, F, len(algo)])
    frames = torch.from_numpy((rng.standard_normal((F, c["M"], c["N"])) * 0.25).astype(np.float32)).cuda()
    bl = listen.BeamListener(algo, mics=np.arange(c["M"]))
    image = bl.maps(frames)
    variant = nat.lib.bf_last_das_variant()
    assert variant == FAMILY[grid][algo]
    order = np.stack([rng.permutation(D) for _ in range(F)])
    power, status = bl.powers(frames, torch.from_numpy((order * bl.offset_per_dir).astype(np.int32)).cuda())
    torch.cuda.synchronize()
    assert nat.lib.bf_last_das_variant() == variant
    assert not status.cpu().numpy().any()
    img = image.cpu().numpy()
    assert power.cpu().numpy().tobytes() == np.take_along_axis(img, order, axis=1).tobytes()
    shared, _ = bl.powers(frames, (order[0] * bl.offset_per_dir).tolist())           # a host sequence: one list for every frame
    assert shared.cpu().numpy().tobytes() == img[:, order[0]].tobytes()


# ------------------------------------------------------------------ 3. the stream call

@pytest.mark.parametrize("with_prev", [True, False], ids=["prev", "no_prev"])
@pytest.mark.parametrize("hop_kind", ["N", "half"])
@pytest.mark.parametrize("N", [64, 100])
@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_stream_call(nat, oracle_lib, algo, N, hop_kind, with_prev):
    """3 frames, 9 of 16 microphones, hop N and N / 2, with and without a previous frame: equal to the extended-window restatement
    and to what bf_das_stream_device writes at the same directions; rejected entries NaN."""
    torch = util.torch_gpu()
    M_total, D, F = 16, 12, 3
    rng = np.random.default_rng([9, N, len(algo)])
    mics = rng.choice(M_total, 9, replace=False).astype(np.int32)
    case = Case(nat, oracle_lib, algo, sizes=(M_total, N, D, 8), delays=rng.uniform(0, N // 2 - 2, size=(D, 9)), mics=mics)
    hop = N if hop_kind == "N" else N // 2
    assert case.H <= hop
    st = Stream([4, N, hop, len(algo)], M_total, N, hop, F, with_prev=with_prev)
    frames = st.frames()
    dirs = np.array([[(7 * b + f) % D for b in range(19)] for f in range(F)])
    offs = case.offset(dirs)
    offs[:, 4], offs[:, 11] = -1, case.offset(D - 1) + 1
    got, status = _call(nat, algo, frames, mics, offs, gap=2, stream=(hop, st.prev()))
    want_st = select_np.verdicts(algo, offs, 9, 8, D * 9)
    assert np.array_equal(status, want_st) and want_st.sum() == 2 * F
    d_sig = torch.from_numpy(frames).cuda()
    d_prev = None if st.prev() is None else torch.from_numpy(st.prev()).cuda()
    img = torch.empty((F, D), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_stream_device(util.ALGOS[algo], d_sig.data_ptr(), M_total, img.data_ptr(), D, F, hop, None if d_prev is None else d_prev.data_ptr(),
                                        nat.iptr(mics), 9, 0, D, torch.cuda.current_stream().cuda_stream) == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    img = img.cpu().numpy()
    powers = {}
    for f in range(F):
        for b in range(19):
            if want_st[f, b]:
                assert got[f, b].view(np.uint32) == NAN_BITS
                continue
            d = int(dirs[f, b])
            if (f, d) not in powers:
                powers[(f, d)] = np.float32(case.want_power(st, f, d))
            assert got[f, b].tobytes() == powers[(f, d)].tobytes(), (f, b, got[f, b], powers[(f, d)])
            assert got[f, b].tobytes() == img[f, d].tobytes()
    shared, _ = _call(nat, algo, frames, mics, offs[0], status=False, stream=(hop, st.prev()))      # per_frame == 0
    for f in range(F):
        ok = want_st[0] == 0
        assert shared[f, ok].tobytes() == img[f, dirs[0, ok]].tobytes()


# ------------------------------------------------------------------ 4. CoarseToFine

def _zoom_setup(nat, name, algo="lerp"):
    import directions_np
    from interface import config
    z = select_np.ZOOM[name]
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=z["N"], MAX_RES_X=z["X"], MAX_RES_Y=z["Y"], N_TAPS=8)
    delays = directions_np.calculate_delays(z["X"], z["Y"], arrays=1)
    d32 = np.ascontiguousarray(np.float32(delays)).ravel()
    nat.lib.load_coefficients_lerp(nat.fptr(d32), d32.size)
    nat.check()
    return z, delays, select_np.zoom_frames(name, delays)


def _want_locate(z, full):
    return select_np.locate(full, z["X"], z["Y"], z["step"], z["radius"], z["k"], z["radius_c"], z["floor_rel"], 0.0, 64)


def _same_locate(got, want):
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (g, w)


@pytest.mark.parametrize("name", ["g41x23", "g101"])
def test_locate_equals_the_restatement(nat, oracle_lib, name):
    """The 41 x 23 grid (3 frames, one of them silent: fewer than k peaks) and the issue's 101 x 101 scene, lattice step 4, window
    radius 4: offsets, values and counts of the restatement on the C checker's full map."""
    torch = util.torch_gpu()
    import listen
    import zoom
    z, delays, frames = _zoom_setup(nat, name)
    mics = np.arange(64, dtype=np.int32)
    orc = oracle_lib.Oracle(z["N"], z["X"], z["Y"], 8)
    full = np.stack([orc.mimo_lerp(f, np.float32(delays), mics).ravel() for f in frames])
    bl = listen.BeamListener("lerp", mics=mics)
    ctf = zoom.CoarseToFine(bl, z["step"], radius=z["radius"], shape=(z["X"], z["Y"]))
    xs, ys, lat = select_np.lattice(z["X"], z["Y"], z["step"])
    assert ctf.coarse_shape == (xs.size, ys.size) and ctf.lattice.cpu().numpy().tolist() == (lat * 64).tolist()
    d_frames = torch.from_numpy(frames).cuda()
    assert ctf.scan(d_frames).cpu().numpy().tobytes() == full[:, lat].tobytes()
    _same_locate(ctf.locate(d_frames, z["k"], z["radius_c"], z["floor_rel"]), _want_locate(z, full))


def test_locate_on_a_stream(nat, oracle_lib):
    """The 41 x 23 scene's frames as back-to-back windows of one stream (hop = N, silence before it) through a StreamBeamformer."""
    torch = util.torch_gpu()
    import stream
    import zoom
    name = "g41x23"
    z = select_np.ZOOM[name]
    import directions_np
    delays = directions_np.calculate_delays(z["X"], z["Y"], arrays=1)
    frames = select_np.zoom_frames(name, delays)
    F, M, N, D = frames.shape[0], 64, z["N"], z["X"] * z["Y"]
    case = Case(nat, oracle_lib, "lerp", sizes=(M, N, D, 8), delays=delays.reshape(D, M))
    st = Stream(0, M, N, N, F, with_prev=False)
    st.S = np.ascontiguousarray(np.concatenate(list(frames), axis=1))
    st.Sz = np.concatenate([np.zeros((M, st.P), np.float32), st.S], axis=1)
    assert np.array_equal(st.frames(), frames)
    full = np.array([[case.want_power(st, f, d) for d in range(D)] for f in range(F)], dtype=np.float32)
    sb = stream.StreamBeamformer("lerp", mics=np.arange(M))
    ctf = zoom.CoarseToFine(sb, z["step"], radius=z["radius"], shape=(z["X"], z["Y"]))
    d_frames = torch.from_numpy(frames).cuda()
    assert sb.maps(d_frames).cpu().numpy().tobytes() == full.tobytes()
    _same_locate(ctf.locate(d_frames, z["k"], z["radius_c"], z["floor_rel"]), _want_locate(z, full))
    assert sb._prev is None                                                 # powers / locate leave the carried state alone


def test_locate_in_a_graph(nat):
    """locate captured after one warm-up call; the frames overwritten in place; the replay equals the eager call on the new frames."""
    torch = util.torch_gpu()
    import listen
    import zoom
    z, delays, frames = _zoom_setup(nat, "g41x23")
    bl = listen.BeamListener("lerp", mics=np.arange(64))
    ctf = zoom.CoarseToFine(bl, z["step"], radius=z["radius"], shape=(z["X"], z["Y"]))
    static = torch.from_numpy(frames).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctf.locate(static, z["k"], z["radius_c"], z["floor_rel"])           # warm-up: the adaptive array's upload, the peak search's buffers
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ctf.locate(static, z["k"], z["radius_c"], z["floor_rel"])
    fresh = torch.from_numpy(np.ascontiguousarray(frames[[1, 2, 0]] * np.float32(0.5))).cuda()
    static.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    eager = ctf.locate(fresh, z["k"], z["radius_c"], z["floor_rel"])
    torch.cuda.synchronize()
    for g, e in zip(out, eager):
        assert g.cpu().numpy().tobytes() == e.cpu().numpy().tobytes()
    assert out[2].cpu().numpy()[:, 0].tolist() == [1, 1, 2]
