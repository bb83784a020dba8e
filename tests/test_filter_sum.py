"""GPU (-m gpu): bf_filter_sum_device and filtersum.FilterSumListener, bit for bit against the NumPy restatement of the definition
(tests/filtersum_np.py: band_np's fmaf chain per (beam, microphone), then a float32 add over the microphones in order).

Data: floats whose magnitudes spread over 2^-12 .. 2^12 in taps and samples, so a chain or a microphone sum taken in any other
order, or a product rounded before the add, shows in the bits.  Every call writes into the middle of a buffer of canary floats,
which must survive -- the gaps between the rows of a strided output included."""
import numpy as np
import pytest

import band_np
import filtersum_np as fsn
import util
from util import CANARY, CANARY_VALUE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat(native):
    assert native.gpu_available(), "these tests need the MI355X"
    yield native
    native.lib.bf_filter_sum_waves(0)
    util.configure("cfg1")


def _beams(nat, x, mics, taps, hop, prev=None, off_in=0, off_out=0, gap=0, expect_rc=0):
    """bf_filter_sum_device on device copies -> float32 [F, B, N]; the canaries around the output and in its rows' gaps are checked."""
    torch = util.torch_gpu()
    F, m_total, N = x.shape
    B, n, T = taps.shape
    stride = N + gap
    total = F * B * stride
    keep_x, d_x = util.place(x, off_in)
    keep_g, d_g = util.place(taps, off_in)
    keep_p, d_p = (None, None) if prev is None else util.place(prev, off_in)
    buf = torch.full((CANARY + 4 + total + CANARY,), CANARY_VALUE, dtype=torch.float32, device="cuda")
    out = buf[CANARY + off_out:CANARY + off_out + total]
    assert out.data_ptr() % 16 == 4 * off_out and d_x.data_ptr() % 16 == 4 * off_in
    mics = np.ascontiguousarray(mics, dtype=np.int32)
    rc = nat.lib.bf_filter_sum_device(d_x.data_ptr(), m_total, F, hop, None if d_p is None else d_p.data_ptr(), nat.iptr(mics), n, d_g.data_ptr(), T, B,
                                      out.data_ptr(), stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo, hi = CANARY + off_out, CANARY + off_out + total
    if expect_rc != 0:
        assert rc == expect_rc and nat.lib.bf_last_error()
        nat.lib.bf_clear_error()
        assert (host == np.float32(CANARY_VALUE)).all()             # nothing was enqueued
        return None
    assert rc == 0, nat.lib.bf_last_error()
    assert (host[:lo] == np.float32(CANARY_VALUE)).all() and (host[hi:] == np.float32(CANARY_VALUE)).all()
    rows = host[lo:hi].reshape(F, B, stride)
    assert (rows[:, :, N:] == np.float32(CANARY_VALUE)).all()       # floats past N_SAMPLES in a row are left untouched
    return rows[:, :, :N].copy()


def _mics(rng, n, m_total):
    """n rows of m_total, not the identity and not sorted; rows repeat only when there are more microphones than rows."""
    return (rng.permutation(m_total)[:n] if n <= m_total else rng.integers(0, m_total, size=n)).astype(np.int32)


# ------------------------------------------------------------------ the definition, every shape the kernel treats differently

#        N    T   hop   n  m_total B  F  prev   off_in off_out gap
CASES = [
    (64, 1, 0, 1, 3, 1, 1, False, 0, 0, 0),          # T = 1, one microphone, one beam: no history, no sum
    (64, 1, 32, 3, 5, 3, 5, True, 0, 0, 4),
    (64, 2, 1, 3, 5, 3, 5, True, 0, 0, 0),           # hop = T - 1 = 1
    (64, 2, 64, 5, 9, 16, 1, False, 0, 0, 0),        # 16 beams
    (64, 5, 32, 70, 72, 3, 5, True, 0, 0, 5),        # T % 4 = 1; 70 microphones: more than one pass of the waves, and not a multiple of them
    (64, 5, 4, 3, 5, 1, 5, False, 0, 0, 0),          # hop = T - 1; silence before frame 0, real history for frames 1 ..
    (64, 64, 64, 3, 5, 1, 5, True, 0, 0, 0),         # T = N: a history of N - 1 samples with hop = N
    (64, 64, 63, 5, 9, 3, 1, False, 0, 0, 3),        # hop = T - 1 = N - 1
    (64, 64, 0, 3, 5, 16, 5, True, 0, 0, 0),         # hop = 0: independent windows, d_prev given and ignored
    (256, 65, 128, 70, 72, 3, 5, True, 0, 0, 0),
    (256, 65, 256, 3, 5, 1, 1, True, 0, 0, 8),
    (256, 65, 0, 5, 9, 16, 5, False, 0, 0, 0),
    (256, 129, 128, 3, 5, 1, 5, True, 0, 0, 0),      # hop = T - 1 = 128
    (256, 129, 256, 70, 72, 16, 1, False, 0, 0, 0),
    (256, 65, 128, 3, 5, 3, 5, True, 1, 0, 0),       # input 4 bytes off a 16-byte boundary
    (256, 65, 128, 3, 5, 3, 5, True, 0, 1, 4),       # output 4 bytes off
    (256, 66, 128, 1, 3, 1, 5, True, 1, 1, 1),       # both, T % 4 = 2, an output stride that is no multiple of 4
    (100, 5, 50, 3, 5, 3, 5, True, 0, 0, 0),         # N = 100: 25 lanes own a quad, the other 39 idle
    (100, 65, 100, 70, 64, 1, 1, False, 0, 0, 0),    # more microphones than rows: rows are listed twice
    (100, 5, 0, 1, 3, 16, 5, False, 1, 1, 0),
    (102, 5, 51, 3, 5, 3, 5, True, 0, 0, 2),         # N % 4 != 0: the last lane's quad is cut, rows are only 8-byte aligned
    (99, 65, 99, 70, 72, 1, 2, True, 0, 0, 0),       # odd N: rows are only 4-byte aligned, 16-byte accesses are impossible
    (99, 2, 49, 5, 9, 16, 5, False, 0, 0, 1),
    (300, 65, 150, 5, 9, 3, 2, True, 0, 0, 0),       # two chunks of outputs, the second cut; its history is the row itself
    (1024, 129, 512, 3, 5, 2, 2, True, 0, 0, 0),     # the longest row the library takes: four chunks
]


@pytest.mark.parametrize("N,T,hop,n,m_total,B,F,with_prev,off_in,off_out,gap", CASES)
def test_matches_the_definition(nat, N, T, hop, n, m_total, B, F, with_prev, off_in, off_out, gap):
    util.configure_small(N)
    rng = np.random.default_rng([N, T, hop, n, B, F])
    x, prev = util.stream_windows(rng, m_total, N, hop, F)
    if not with_prev:
        prev = None
    mics = _mics(rng, n, m_total)
    g = util.wild(rng, (B, n, T))
    got = _beams(nat, x, mics, g, hop, prev, off_in, off_out, gap)
    util.same_bits(got, fsn.filter_sum(x, mics, g, hop, prev))


def test_result_does_not_depend_on_the_waves_or_on_the_beams_launched_together(nat):
    """Pinned to 1, 2, 4, 8 and 16 waves a workgroup deals its microphones differently each time; a beam launched alone, among 3 and
    among 16 sits in another workgroup of another grid.  All give the bits of the restatement."""
    util.configure_small(256)
    rng = np.random.default_rng(31)
    n, m_total, T, hop, F = 70, 72, 33, 128, 2
    x, prev = util.stream_windows(rng, m_total, 256, hop, F)
    mics = _mics(rng, n, m_total)
    g = util.wild(rng, (16, n, T))
    want = fsn.filter_sum(x, mics, g, hop, prev)
    try:
        for waves in (1, 2, 4, 8, 16):
            nat.lib.bf_filter_sum_waves(waves)
            util.same_bits(_beams(nat, x, mics, g[9:10], hop, prev), want[:, 9:10])
            util.same_bits(_beams(nat, x, mics, g[7:10], hop, prev), want[:, 7:10])
            util.same_bits(_beams(nat, x, mics, g, hop, prev), want)
    finally:
        assert nat.lib.bf_filter_sum_waves(0) == 16


@pytest.mark.parametrize("N,T,hop,off", [(64, 5, 16, 0), (256, 65, 64, 0), (100, 9, 50, 0), (99, 9, 50, 0), (256, 65, 64, 1)])
def test_overlap_and_split_batch_identities(nat, N, T, hop, off):
    util.configure_small(N)
    rng = np.random.default_rng([N, T, hop, 98])
    F, F1, n, m_total, B = 5, 2, 5, 7, 3
    x, prev = util.stream_windows(rng, m_total, N, hop, F)
    mics = _mics(rng, n, m_total)
    g = util.wild(rng, (B, n, T))
    whole = _beams(nat, x, mics, g, hop, prev, off, off)
    for f in range(1, F):                                            # overlapping windows agree where both exist
        util.same_bits(whole[f, :, :N - hop], whole[f - 1, :, hop:])
    a = _beams(nat, x[:F1], mics, g, hop, prev, off, off)
    b = _beams(nat, x[F1:], mics, g, hop, x[F1 - 1], off, off)       # the carried window
    util.same_bits(np.concatenate([a, b], axis=0), whole)


# ------------------------------------------------------------------ delta taps are the delay-and-sum beams of a loaded pad table

def test_delta_taps_equal_the_pad_beams(nat):
    torch = util.torch_gpu()
    c = util.configure("cfg1")
    M, N, D = c["M"], c["N"], c["X"] * c["Y"]
    table = np.ascontiguousarray(util.table_for("pad", "cfg1"), dtype=np.int32).reshape(D, M)
    nat.lib.load_coefficients_pad(nat.iptr(table), table.size); nat.check()
    max_whole = int(table.max())
    assert 0 < max_whole < 64
    rng = np.random.default_rng(17)
    hop, F = 128, 3
    x, prev = util.stream_windows(rng, M, N, hop, F)
    x[0, 5, :4] = [-0.0, 0.0, -1e-45, 1e-45]
    mics = rng.permutation(M).astype(np.int32)                       # entry m of a table row belongs to frame row mics[m]
    dirs = np.array([0, D // 2 + 3, D - 1], dtype=np.int32)
    d_x, d_prev = torch.from_numpy(x).cuda(), torch.from_numpy(prev).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(np.tile(dirs * M, (F, 1)))).cuda()                 # int32 [F, 3]: every frame's offsets
    want = torch.empty((F, 3, N), dtype=torch.float32, device="cuda")
    status = torch.empty((F, 3), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert nat.lib.bf_miso_device(util.ALGOS["pad"], d_x.data_ptr(), M, F, nat.iptr(mics), M, d_off.data_ptr(), 3, 0.0, want.data_ptr(), N, status.data_ptr(),
                                  s) == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    for T in (max_whole + 1, max_whole + 6):                         # the shortest filter that holds every delay, and one with taps to skip
        util.same_bits(_beams(nat, x, mics, fsn.delta_taps(table[dirs], T), 0), want.cpu().numpy())
    # with a hop: the continuous-stream beams, every sample of them
    assert nat.lib.bf_miso_stream_device(util.ALGOS["pad"], d_x.data_ptr(), M, F, hop, d_prev.data_ptr(), nat.iptr(mics), M, d_off.data_ptr(), 3, 0.0,
                                         want.data_ptr(), N, status.data_ptr(), s) == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    for T in (max_whole + 1, hop + 1):
        util.same_bits(_beams(nat, x, mics, fsn.delta_taps(table[dirs], T), hop, prev), want.cpu().numpy())


# ------------------------------------------------------------------ refusals that are worth a device: nothing may be enqueued

def test_refused_calls_enqueue_nothing_and_touching_ranges_are_fine(nat):
    torch = util.torch_gpu()
    util.configure_small(64)
    rng = np.random.default_rng(5)
    m_total, n, B, T, hop, F = 5, 3, 2, 9, 32, 2
    x, prev = util.stream_windows(rng, m_total, 64, hop, F)
    mics = np.array([4, 0, 2], dtype=np.int32)
    g = util.wild(rng, (B, n, T))
    for bad_hop in (7, 65, -1):
        assert _beams(nat, x, mics, g, bad_hop, prev, expect_rc=-1) is None
    assert _beams(nat, x, mics, util.wild(rng, (17, n, T)), hop, prev, expect_rc=-1) is None
    assert _beams(nat, x, np.array([4, 5, 2]), g, hop, prev, expect_rc=-1) is None
    assert _beams(nat, x, mics, g, hop, prev, gap=-1, expect_rc=-1) is None
    # one allocation: [prev | frames | taps | out], every range touching the next; then overlapping, which is refused and leaves the buffer as it was
    n_prev, n_in, n_taps, n_out = prev.size, x.size, g.size, F * B * 64
    buf = torch.full((n_prev + n_in + n_taps + n_out + CANARY,), CANARY_VALUE, dtype=torch.float32, device="cuda")
    buf[:n_prev].copy_(torch.from_numpy(prev.ravel()))
    buf[n_prev:n_prev + n_in].copy_(torch.from_numpy(x.ravel()))
    buf[n_prev + n_in:n_prev + n_in + n_taps].copy_(torch.from_numpy(g.ravel()))
    s = torch.cuda.current_stream().cuda_stream
    p = buf.data_ptr()
    at_out = n_prev + n_in + n_taps
    call = lambda out_at: nat.lib.bf_filter_sum_device(p + 4 * n_prev, m_total, F, hop, p, nat.iptr(mics), n, p + 4 * (n_prev + n_in), T, B, p + 4 * out_at, 64, s)
    assert call(at_out) == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    util.same_bits(host[at_out:at_out + n_out].reshape(F, B, 64), fsn.filter_sum(x, mics, g, hop, prev))
    assert (host[at_out + n_out:] == np.float32(CANARY_VALUE)).all()
    for out_at in (at_out - 1, n_prev + n_in, n_prev + n_in - 1, n_prev, n_prev - 1, 0):
        assert call(out_at) == -1 and b"overlaps" in nat.lib.bf_last_error()
        nat.lib.bf_clear_error()
    torch.cuda.synchronize()
    assert np.array_equal(util.bits(buf.cpu().numpy()), util.bits(host))


# ------------------------------------------------------------------ one captured graph: filter-and-sum -> band filter on its beams

def test_graph_beams_then_band_filter(nat):
    torch = util.torch_gpu()
    import band
    import synth
    c = util.configure("cfg1")
    M, N = c["M"], c["N"]
    mics = np.arange(M, dtype=np.int32)[::-1].copy()
    rng = np.random.default_rng(73)
    F, B, T, hop = 3, 3, 33, 128
    g = util.wild(rng, (B, M, T))
    h = band.design([(3000.0, 8000.0)], n_taps=65)
    first = synth.frame_batch(M, N, F)
    second = np.ascontiguousarray(util.inputs("cfg1")["s3"][None].repeat(F, 0) + (rng.standard_normal((F, M, N)) * 0.05).astype(np.float32))
    x = torch.from_numpy(first).cuda()
    d_g, d_h = torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()
    beams = torch.empty((F, B, N), dtype=torch.float32, device="cuda")
    y = torch.empty((F, B, N), dtype=torch.float32, device="cuda")

    def step():
        s = torch.cuda.current_stream().cuda_stream
        assert nat.lib.bf_filter_sum_device(x.data_ptr(), M, F, hop, None, nat.iptr(mics), M, d_g.data_ptr(), T, B, beams.data_ptr(), N, s) == 0
        assert nat.lib.bf_band_filter_device(beams.data_ptr(), F * B, 1, 0, None, d_h.data_ptr(), 65, 1, y.data_ptr(), s) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up: the adaptive array is uploaded here, not in the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    x.copy_(torch.from_numpy(second).cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy().copy() for t in (beams, y)]
    step()                                              # eager on the same windows
    torch.cuda.synchronize()
    for a, t in zip(got, (beams, y)):
        assert a.tobytes() == t.cpu().numpy().tobytes()
    want = fsn.filter_sum(second, mics, g, hop, None)
    util.same_bits(got[0], want)
    util.same_bits(got[1], band_np.band_filter(want.reshape(1, F * B, N), h)[0, 0].reshape(F, B, N))


# ------------------------------------------------------------------ filtersum.FilterSumListener on the two-talker scene

def test_listener_nulls_the_second_talker(nat):
    """The scene of tests/test_filter_sum_host.py as float32 frames cut from the stream (hop 128): cross_null's two beams are the
    restatement bit for bit, and the interferer alone through the device beam aimed at the look source comes out at least 20 dB
    below what the same designer's delay-and-sum beam (no nulls) lets through."""
    torch = util.torch_gpu()
    import filtersum
    from interface import config
    from lib import directions
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=256, MAX_RES_X=fsn.GRID[0], MAX_RES_Y=fsn.GRID[1], N_TAPS=8)
    M, N, hop, F, T = 64, 256, 128, 14, 65
    tau = directions.calculate_delays().reshape(-1, M)
    look, null = fsn.flat(fsn.LOOK), fsn.flat(fsn.INTERFERER)
    rng = np.random.default_rng(0)
    L = hop * (F + 1) + N
    x_look = fsn.at_microphones(fsn.band_noise(rng, L), tau[look], L)
    x_int = fsn.at_microphones(fsn.band_noise(rng, L), tau[null], L)
    cut = lambda s: (np.ascontiguousarray(np.stack([s[:, (f + 1) * hop:(f + 1) * hop + N] for f in range(F)]), dtype=np.float32),
                     np.ascontiguousarray(s[:, :N], dtype=np.float32))
    both, both_prev = cut(x_look + x_int)
    alone, alone_prev = cut(x_int)

    offsets = np.array([look * M, -1, null * M, 7], dtype=np.int32)           # what sources() writes, with an empty slot and a stray entry
    fl = filtersum.FilterSumListener.cross_null(tau, offsets, M, hop=hop, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    assert fl.dirs == [look, null] and fl.B == 2 and fl.taps.shape == (2, M, T) and fl.delay == 32.0 and fl.kept.all()
    want_taps, _ = filtersum.design_lcmv(tau, [look, null], [[null], [look]], n_taps=T, band=fsn.BAND, fs=fsn.FS)
    util.same_bits(fl.taps, want_taps)
    mics = fl.mics
    assert np.array_equal(mics, np.arange(M))

    d_both = torch.from_numpy(both).cuda()
    cold = fl.listen(d_both).cpu().numpy()
    util.same_bits(cold, fsn.filter_sum(both, mics, fl.taps, hop, None))
    fl.advance(torch.from_numpy(both_prev[None]).cuda())
    whole = fl.listen(d_both).cpu().numpy()
    util.same_bits(whole, fsn.filter_sum(both, mics, fl.taps, hop, both_prev))
    a = fl.listen(d_both[:5]).cpu().numpy()
    carried = fl._prev.data_ptr()
    fl.advance(d_both[:5])
    assert fl._prev.data_ptr() == carried               # copied in place: a captured graph's pointer stays valid
    b = fl.listen(d_both[5:])
    util.same_bits(np.concatenate([a, b.cpu().numpy()], axis=0), whole)
    audio = fl.audio(torch.from_numpy(whole).cuda()).cpu().numpy()
    assert audio.shape == (2, F * hop)
    util.same_bits(audio, whole[:, :, N - hop:].transpose(1, 0, 2).reshape(2, F * hop))
    fl.reset()
    util.same_bits(fl.listen(d_both).cpu().numpy(), cold)

    # the interferer alone: through the null-steered beam, and through the same designer's beam without nulls
    das_taps, _ = filtersum.design_lcmv(tau, [look], None, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    das = filtersum.FilterSumListener(das_taps, hop=hop)
    d_alone, d_alone_prev = torch.from_numpy(alone).cuda(), torch.from_numpy(alone_prev[None]).cuda()
    fl.advance(d_alone_prev)
    das.advance(d_alone_prev)
    power = lambda y: float(np.mean(y.astype(np.float64) ** 2))
    leak_lcmv = fsn.db(power(fl.audio(fl.listen(d_alone)).cpu().numpy()[0]))
    leak_das = fsn.db(power(das.audio(das.listen(d_alone)).cpu().numpy()[0]))
    print("interferer through the device beams: delay-and-sum %.1f dB, null-steered %.1f dB (%.1f dB better)" % (leak_das, leak_lcmv, leak_das - leak_lcmv))
    assert leak_das - leak_lcmv >= 20.0

    with pytest.raises(ValueError):
        filtersum.FilterSumListener(das_taps, hop=32)                # 64 samples of history do not fit a hop of 32
    with pytest.raises(ValueError):
        filtersum.FilterSumListener(das_taps[:, :5])                 # taps for 5 microphones, 64 listed
    with pytest.raises(ValueError):
        filtersum.FilterSumListener.cross_null(tau, np.array([-1, -1]), M)
    with pytest.raises(ValueError):
        filtersum.FilterSumListener(das_taps).audio(torch.zeros((1, 1, N), device="cuda"))
