"""GPU (-m gpu): bf_miso_device / bf_peak_offsets_device, the batched steered beams, bit for bit against the oracle.

bf_miso_device runs das_miso_kernel<ALGO, NC> with one workgroup per (frame, group of up to 16 beams), one wave per beam, the
frame's microphone chunks staged once per workgroup.  Every beam keeps the reference's mic order and operation order, so each
[frame, beam] row must equal the oracle's miso_* of that frame at that offset BIT FOR BIT, at every NC class and with chunked
staging (test_miso_parity.MISO_CASES)."""
import numpy as np
import pytest

import util
from support import nat
from test_miso_parity import MISO_CASES, _configure, case_id, case_tables

pytestmark = pytest.mark.gpu

DEVICE_ALGOS = ["pad", "lerp", "hybrid", "fir_vec"]
SENTINEL = 16
MIC_GAIN = 128.0        # PC/src/config.json:62


class Tables:
    """One algorithm's table for a case, loaded into the product, and the oracle call that goes with it."""

    def __init__(self, nat, orc, algo, delays, taps, n, T):
        self.algo, self.orc, self.n, self.T = algo, orc, n, T
        self.d32 = np.ascontiguousarray(np.float32(delays)).ravel()
        self.whole = np.floor(self.d32).astype(np.int32)
        self.h = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        if algo == "pad":
            nat.lib.load_coefficients_pad(nat.iptr(self.whole), self.whole.size)
        elif algo == "lerp":
            nat.lib.load_coefficients_lerp(nat.fptr(self.d32), self.d32.size)
        elif algo == "hybrid":
            nat.lib.load_coefficients_convolve_hybrid(nat.fptr(self.d32), self.d32.size)
        else:
            nat.lib.load_coefficients_convolve(nat.fptr(self.h), self.h.size)
        nat.check()
        self.per = T if algo == "fir_vec" else 1
        self.entries = self.h.size if algo == "fir_vec" else self.d32.size

    def offset(self, d):
        return d * self.n * self.per

    def want(self, sig, mics, off):
        if self.algo == "pad":
            return self.orc.miso_pad(sig, self.whole, mics, off)
        if self.algo == "lerp":
            return self.orc.miso_lerp(sig, self.d32, mics, off)
        if self.algo == "hybrid":
            return self.orc.miso_hybrid(sig, self.d32, mics, off)
        return self.orc.miso_convolve_vectorized(sig, self.h, mics, off)


def _frames(case, F):
    """F different seeded frames [F, M_total, N]; frame 0 is the case's own signal block."""
    M_total, n, N = case[:3]
    sig = case_tables(case)[0]
    rng = np.random.default_rng([7] + list(case[:5]))
    rest = [(rng.standard_normal((M_total, N)) * 0.25).astype(np.float32) for _ in range(F - 1)]
    return np.ascontiguousarray(np.stack([sig] + rest))


def _run(nat, algo, frames, mics, offsets, gain=0.0, out_stride=None, status=True, out=None):
    """bf_miso_device on device copies of frames [F, M, N] and offsets [F, B] -> (out tensor, status tensor or None)."""
    torch = util.torch_gpu()
    F, M, N = frames.shape
    B = offsets.shape[1]
    out_stride = out_stride or N
    d_sig = torch.from_numpy(frames).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)).cuda()
    if out is None:
        out = torch.full((F * B * out_stride + SENTINEL,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((F, B), -7, dtype=torch.int32, device="cuda") if status else None
    rc = nat.lib.bf_miso_device(util.ALGOS[algo], d_sig.data_ptr(), M, F, nat.iptr(mics), mics.size, d_off.data_ptr(), B, float(gain),
                                out.data_ptr(), out_stride, st.data_ptr() if status else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    return out, st


def _rows(out, F, B, N, out_stride=None):
    out_stride = out_stride or N
    return out.cpu().numpy()[:F * B * out_stride].reshape(F, B, out_stride)[:, :, :N]


def _same(got, want):
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got.view(np.int32) != want.view(np.int32))[:8]


def _beams(D, F):
    """5 beams per frame: the first and last direction, a repeated direction and directions that change from frame to frame."""
    return np.array([[0, D - 1, f % D, f % D, (D - 1 - f) % D] for f in range(F)], dtype=np.int64)


# ------------------------------------------------------------------ 1. every algorithm, every MISO case

@pytest.mark.parametrize("case", MISO_CASES, ids=case_id)
@pytest.mark.parametrize("algo", DEVICE_ALGOS)
def test_batched_beams_match_oracle(nat, oracle_lib, algo, case):
    M_total, n, N, T, D = case[:5]
    _, mics, delays, taps, _ = case_tables(case)
    _configure(case)
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, T), algo, delays, taps, n, T)
    F = 3
    frames = _frames(case, F)
    dirs = _beams(D, F)
    offs = tab.offset(dirs)
    out, st = _run(nat, algo, frames, mics, offs)
    got = _rows(out, F, 5, N)
    assert (st.cpu().numpy() == 0).all()
    for f in range(F):
        for b in range(5):
            want = tab.want(frames[f], mics, int(offs[f, b]))
            assert np.isfinite(want).all()
            _same(got[f, b], want)
    assert np.isnan(out.cpu().numpy()[F * 5 * N:]).all()


# ------------------------------------------------------------------ 2. several beam groups per frame, the last one partial

@pytest.mark.parametrize("algo", ["pad", "hybrid"])
def test_beam_groups(nat, oracle_lib, algo):
    case = MISO_CASES[5]                          # N = 256 (NC 4), pad / lerp stage three chunks
    M_total, n, N, T, D = case[:5]
    assert N > 128
    _, mics, delays, taps, _ = case_tables(case)
    _configure(case)
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, T), algo, delays, taps, n, T)
    F, B = 2, 37                                   # groups of 16, 16 and 5 beams
    frames = _frames(case, F)
    dirs = np.array([[(3 * b + f) % D for b in range(B)] for f in range(F)])
    offs = tab.offset(dirs)
    out, st = _run(nat, algo, frames, mics, offs)
    got = _rows(out, F, B, N)
    assert (st.cpu().numpy() == 0).all()
    wants = {(f, d): tab.want(frames[f], mics, tab.offset(d)) for f in range(F) for d in range(D)}
    for f in range(F):
        for b in range(B):
            _same(got[f, b], wants[(f, int(dirs[f, b]))])


# ------------------------------------------------------------------ 3. output layout: the gaps of a wider row stay untouched

def test_out_stride_gaps_untouched(nat, oracle_lib):
    case = MISO_CASES[2]
    M_total, n, N, T, D = case[:5]
    _, mics, delays, taps, _ = case_tables(case)
    _configure(case)
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, T), "lerp", delays, taps, n, T)
    F, B, stride = 3, 5, N + 7
    frames = _frames(case, F)
    offs = tab.offset(_beams(D, F))
    out, _ = _run(nat, "lerp", frames, mics, offs, out_stride=stride, status=False)
    host = out.cpu().numpy()
    nan_bits = np.full(1, np.nan, dtype=np.float32).view(np.int32)[0]
    rows = host[:F * B * stride].reshape(F, B, stride)
    assert (rows[:, :, N:].view(np.int32) == nan_bits).all()
    assert (host[F * B * stride:].view(np.int32) == nan_bits).all()
    for f in range(F):
        for b in range(B):
            _same(rows[f, b, :N], tab.want(frames[f], mics, int(offs[f, b])))


# ------------------------------------------------------------------ 4. mic_gain: (beam / n) * gain, two float32 roundings

@pytest.mark.parametrize("case_index", [1, 2], ids=["n16", "n9"])
def test_mic_gain(nat, oracle_lib, case_index):
    case = MISO_CASES[case_index]
    M_total, n, N, T, D = case[:5]
    assert (n & (n - 1) == 0) == (case_index == 1)
    _, mics, delays, taps, _ = case_tables(case)
    _configure(case)
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, T), "pad", delays, taps, n, T)
    F = 3
    frames = _frames(case, F)
    offs = tab.offset(_beams(D, F))
    out, _ = _run(nat, "pad", frames, mics, offs, gain=MIC_GAIN)
    got = _rows(out, F, 5, N)
    for f in range(F):
        for b in range(5):
            raw = tab.want(frames[f], mics, int(offs[f, b]))
            want = (raw / np.float32(n)) * np.float32(MIC_GAIN)
            assert want.dtype == np.float32
            _same(got[f, b], want)


# ------------------------------------------------------------------ 5. rejected offsets, mixed with valid beams in one call

@pytest.mark.parametrize("algo", DEVICE_ALGOS)
def test_invalid_offsets_are_nan_with_status(nat, oracle_lib, algo):
    case = MISO_CASES[4]
    M_total, n, N, T, D = case[:5]
    _, mics, delays, taps, _ = case_tables(case)
    _configure(case)
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, T), algo, delays, taps, n, T)
    last = tab.offset(D - 1)
    row = [tab.offset(0), -1, last + 1, last]
    want_status = [0, 1, 1, 0]
    if algo == "fir_vec":
        row += [T + 3]
        want_status += [2]
    F = 2
    frames = _frames(case, F)
    offs = np.array([row] * F, dtype=np.int64)
    out, st = _run(nat, algo, frames, mics, offs)
    got = _rows(out, F, len(row), N)
    assert (st.cpu().numpy() == np.array([want_status] * F)).all(), st
    for f in range(F):
        for b, s in enumerate(want_status):
            if s:
                assert np.isnan(got[f, b]).all()
            else:
                _same(got[f, b], tab.want(frames[f], mics, int(offs[f, b])))


def test_unloaded_table_is_an_error(nat):
    torch = util.torch_gpu()
    case = MISO_CASES[0]
    _configure(case)
    N = case[2]
    mics = np.arange(4, dtype=np.int32)
    nat.lib.unload_coefficients_convolve_hybrid()
    x = torch.zeros((1, 8, N), dtype=torch.float32, device="cuda")
    offs = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    out = torch.zeros((N,), dtype=torch.float32, device="cuda")
    rc = nat.lib.bf_miso_device(util.ALGOS["hybrid"], x.data_ptr(), 8, 1, nat.iptr(mics), 4, offs.data_ptr(), 1, 0.0, out.data_ptr(), N, None,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    with pytest.raises(nat.BeamformerError, match="load_coefficients_convolve_hybrid has not been called"):
        nat.check()


# ------------------------------------------------------------------ 6. the loudest direction

def _peaks(nat, power, stride, n_dirs, per):
    torch = util.torch_gpu()
    F = power.shape[0]
    d_p = torch.from_numpy(np.ascontiguousarray(power, dtype=np.float32)).cuda()
    d_o = torch.full((F, 1), -5, dtype=torch.int32, device="cuda")
    assert nat.lib.bf_peak_offsets_device(d_p.data_ptr(), F, stride, n_dirs, per, d_o.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


def test_peak_offsets_follow_argmax(nat):
    rng = np.random.default_rng(44)
    F, D, stride, per = 9, 1000, 1003, 64
    p = rng.uniform(0, 1, (F, stride)).astype(np.float32)
    p[:, D:] = 10.0                                    # past n_dirs: never looked at
    p[0, [17, 400, 999]] = 2.0                         # tie of three maxima: the first wins
    p[1, [3, 700]] = np.nan                            # the first NaN wins over everything
    p[1, 5] = 5.0
    p[2, 999] = 3.0                                    # the last direction
    p[3, :D] = -np.inf                                 # all equal: index 0
    p[4, 0] = 4.0
    p[5, [300, 301]] = 1.5; p[5, 302] = np.nan         # a NaN after the maximum still wins
    p[6, :D] = 0.0; p[6, 10] = -0.0                    # zeros of both signs are equal
    p[7, 1:D] = np.float32(0.25); p[7, 0] = np.nan     # NaN at index 0
    got = _peaks(nat, p, stride, D, per)
    want = np.array([np.argmax(p[f, :D]) for f in range(F)], dtype=np.int64) * per
    assert got.shape == (F, 1) and (got[:, 0] == want).all(), (got[:, 0], want)
    # one workgroup lane's worth of directions and fewer
    for n_dirs in (1, 3, 64, 257):
        got = _peaks(nat, p, stride, n_dirs, 1)
        assert (got[:, 0] == np.array([np.argmax(p[f, :n_dirs]) for f in range(F)])).all()


def test_peak_of_plane_wave_map(nat):
    torch = util.torch_gpu()
    c = util.configure("cfg2")
    M, N, D = c["M"], c["N"], c["X"] * c["Y"]
    mics = np.arange(M, dtype=np.int32)
    table = util.table_for("lerp", "cfg2")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    sig = util.inputs("cfg2")["s3"]
    d_sig = torch.from_numpy(np.ascontiguousarray(sig[None])).cuda()
    d_img = torch.empty((1, D), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert nat.lib.bf_das_device(util.ALGOS["lerp"], d_sig.data_ptr(), M, d_img.data_ptr(), D, 1, nat.iptr(mics), M, 0, D, s) == 0
    got = _peaks(nat, d_img.cpu().numpy(), D, D, M)
    img = d_img.cpu().numpy()[0]
    assert got[0, 0] == int(np.argmax(img)) * M and img[got[0, 0] // M] == img.max()


# ------------------------------------------------------------------ 7. maps -> peak -> beams as one captured graph

def test_graph_maps_peak_beams(nat, oracle_lib):
    torch = util.torch_gpu()
    import synth
    c = util.configure("cfg2")
    M, N, X, Y, T = c["M"], c["N"], c["X"], c["Y"], c["T"]
    D = X * Y
    mics = np.arange(M, dtype=np.int32)
    table = util.table_for("lerp", "cfg2")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    F = 3
    first = synth.frame_batch(M, N, F)
    rng = np.random.default_rng(71)
    second = np.ascontiguousarray(util.inputs("cfg2")["s3"][None].repeat(F, 0) + (rng.standard_normal((F, M, N)) * 0.05).astype(np.float32))
    x = torch.from_numpy(first).cuda()
    img = torch.empty((F, D), dtype=torch.float32, device="cuda")
    offs = torch.empty((F, 1), dtype=torch.int32, device="cuda")
    out = torch.empty((F, 1, N), dtype=torch.float32, device="cuda")
    st = torch.empty((F, 1), dtype=torch.int32, device="cuda")

    def step():
        s = torch.cuda.current_stream().cuda_stream
        assert nat.lib.bf_das_device(util.ALGOS["lerp"], x.data_ptr(), M, img.data_ptr(), D, F, nat.iptr(mics), M, 0, D, s) == 0
        assert nat.lib.bf_peak_offsets_device(img.data_ptr(), F, D, D, M, offs.data_ptr(), s) == 0
        assert nat.lib.bf_miso_device(util.ALGOS["lerp"], x.data_ptr(), M, F, nat.iptr(mics), M, offs.data_ptr(), 1, 0.0, out.data_ptr(), N,
                                      st.data_ptr(), s) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up: digest built, adaptive array uploaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    x.copy_(torch.from_numpy(second).cuda())
    g.replay()
    torch.cuda.synchronize()
    got_out, got_offs, got_st = out.cpu().numpy().copy(), offs.cpu().numpy().copy(), st.cpu().numpy().copy()
    step()                                              # eager on the same windows
    torch.cuda.synchronize()
    assert (out.cpu().numpy().tobytes() == got_out.tobytes()) and (offs.cpu().numpy() == got_offs).all()
    assert (got_st == 0).all()
    orc = oracle_lib.Oracle(N, X, Y, T)
    for f in range(F):
        peak = int(np.argmax(orc.mimo_lerp(second[f], table, mics).ravel()))
        assert got_offs[f, 0] == peak * M
        _same(got_out[f, 0], orc.miso_lerp(second[f], table, mics, peak * M))


# ------------------------------------------------------------------ 8. real sizes

@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_cfg2_tables(nat, oracle_lib, algo):
    import synth
    c = util.configure("cfg2")
    M, N, X, Y, T = c["M"], c["N"], c["X"], c["Y"], c["T"]
    D = X * Y
    mics = np.arange(M, dtype=np.int32)
    table = util.table_for(algo, "cfg2")
    if algo == "pad":
        nat.lib.load_coefficients_pad(nat.iptr(table), table.size)
    else:
        nat.lib.load_coefficients_lerp(nat.fptr(table), table.size)
    nat.check()
    F, B = 16, 8
    frames = synth.frame_batch(M, N, F)
    rng = np.random.default_rng(88)
    dirs = rng.integers(0, D, (F, B))
    dirs[:, 0], dirs[:, 1] = 0, D - 1
    offs = dirs * M
    out, st = _run(nat, algo, frames, mics, offs)
    got = _rows(out, F, B, N)
    assert (st.cpu().numpy() == 0).all()
    orc = oracle_lib.Oracle(N, X, Y, T)
    for f in range(F):
        for b in range(B):
            want = orc.miso_pad(frames[f], table, mics, int(offs[f, b])) if algo == "pad" else orc.miso_lerp(frames[f], table, mics, int(offs[f, b]))
            _same(got[f, b], want)


@pytest.mark.parametrize("algo", ["lerp", "hybrid"])
def test_long_blocks_five_directions(nat, oracle_lib, algo):
    from interface import config
    M, N, D, T = 256, 1024, 5, 8
    config.configure(N_MICROPHONES=M, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=T)
    rng = np.random.default_rng(256)
    mics = np.arange(M, dtype=np.int32)
    delays = rng.uniform(0, 100, (D, M))
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, T), algo, delays, np.zeros((D, M, T), np.float32), M, T)
    F = 2
    frames = (rng.standard_normal((F, M, N)) * 0.25).astype(np.float32)
    dirs = np.array([[0, 4, 2, 2], [3, 1, 4, 0]])
    offs = tab.offset(dirs)
    out, st = _run(nat, algo, frames, mics, offs)
    got = _rows(out, F, 4, N)
    assert (st.cpu().numpy() == 0).all()
    for f in range(F):
        for b in range(4):
            _same(got[f, b], tab.want(frames[f], mics, int(offs[f, b])))


# ------------------------------------------------------------------ 9. the Python front-end

def test_beam_listener(nat, oracle_lib):
    torch = util.torch_gpu()
    import listen
    case = MISO_CASES[2]
    M_total, n, N, T, D = case[:5]
    _, mics, delays, taps, _ = case_tables(case)
    _configure(case)
    tab = Tables(nat, oracle_lib.Oracle(N, D, 1, T), "fir_vec", delays, taps, n, T)
    F = 3
    frames = _frames(case, F)
    bl = listen.BeamListener("fir_vec", mics=mics)
    assert bl.offset_per_dir == n * T
    offs = [tab.offset(d) for d in (0, D - 1, 1)]
    d_frames = torch.from_numpy(frames).cuda()
    out, st = bl.listen(d_frames, offs)
    torch.cuda.synchronize()
    assert out.shape == (F, 3, N) and out.dtype == torch.float32 and out.is_cuda
    assert st.shape == (F, 3) and st.dtype == torch.int32 and (st.cpu().numpy() == 0).all()
    ref, _ = _run(nat, "fir_vec", frames, mics, np.array([offs] * F))
    assert out.cpu().numpy().tobytes() == _rows(ref, F, 3, N).tobytes()
    _same(out.cpu().numpy()[2, 1], tab.want(frames[2], mics, tab.offset(D - 1)))
    # per-frame offsets, gain, and the loudest direction of a made-up map
    per_frame = np.array([[tab.offset(f % D)] for f in range(F)], dtype=np.int32)
    g, _ = bl.listen(d_frames, torch.from_numpy(per_frame).cuda(), mic_gain=MIC_GAIN)
    raw = tab.want(frames[1], mics, tab.offset(1))
    _same(g.cpu().numpy()[1, 0], (raw / np.float32(n)) * np.float32(MIC_GAIN))
    power = torch.zeros((F, D), dtype=torch.float32, device="cuda")
    power[0, 2] = 1.0; power[1, D - 1] = 3.0; power[2, 0] = 2.0
    loud = bl.loudest(power)
    assert loud.shape == (F, 1) and loud.dtype == torch.int32
    assert loud.cpu().numpy()[:, 0].tolist() == [tab.offset(2), tab.offset(D - 1), tab.offset(0)]
