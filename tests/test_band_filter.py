"""GPU (-m gpu): bf_band_filter_device and band.BandFilter, bit for bit against the NumPy restatement of the definition
(tests/band_np.py: a Python loop over the taps in order, every step one single-rounding fmaf).

Data: floats whose magnitudes spread over 2^-12 .. 2^12 in taps and samples, so a chain summed in any other order, or a product
rounded before the add, shows in the bits.  Every call writes into the middle of a buffer of canary floats, which must survive."""
import numpy as np
import pytest

import band_np
import util
from support import nat_restoring as nat
from util import CANARY, CANARY_VALUE

pytestmark = pytest.mark.gpu


def _filter(nat, x, taps, hop, prev=None, off_in=0, off_out=0, expect_rc=0):
    """bf_band_filter_device on device copies -> float32 [K, F, R, N]; the canaries around the output are checked."""
    torch = util.torch_gpu()
    F, R, N = x.shape
    K, T = taps.shape
    total = K * F * R * N
    keep_x, d_x = util.place(x, off_in)
    keep_h, d_h = util.place(taps, 0)
    keep_p, d_p = (None, None) if prev is None else util.place(prev, off_in)
    buf = torch.full((CANARY + 4 + total + CANARY,), CANARY_VALUE, dtype=torch.float32, device="cuda")
    out = buf[CANARY + off_out:CANARY + off_out + total]
    assert out.data_ptr() % 16 == 4 * off_out and d_x.data_ptr() % 16 == 4 * off_in
    rc = nat.lib.bf_band_filter_device(d_x.data_ptr(), R, F, hop, None if d_p is None else d_p.data_ptr(), d_h.data_ptr(), T, K, out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
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
    return host[lo:hi].reshape(K, F, R, N).copy()


# ------------------------------------------------------------------ the definition, every shape the kernel treats differently

#        N    T   hop  rows frames K  prev   off_in off_out
CASES = [
    (64, 1, 0, 1, 1, 1, False, 0, 0),        # T = 1: no history at all
    (64, 1, 16, 3, 5, 3, True, 0, 0),
    (64, 2, 1, 3, 5, 3, True, 0, 0),         # hop = T - 1 = 1
    (64, 2, 64, 1, 1, 16, False, 0, 0),
    (64, 5, 32, 70, 5, 16, True, 0, 0),      # T % 4 = 1; 70 rows: 17 full workgroups and one of two rows
    (64, 5, 4, 3, 5, 1, False, 0, 0),        # hop = T - 1; silence before frame 0, real history for frames 1 ..
    (64, 64, 64, 3, 5, 1, True, 0, 0),       # T = N: a history of N - 1 samples with hop = N
    (64, 64, 64, 1, 1, 3, False, 0, 0),
    (64, 64, 0, 3, 5, 3, True, 0, 0),        # hop = 0: independent windows, d_prev given and ignored
    (256, 65, 128, 70, 5, 3, True, 0, 0),
    (256, 65, 256, 3, 1, 1, True, 0, 0),
    (256, 65, 0, 3, 5, 16, False, 0, 0),
    (256, 129, 128, 3, 5, 1, True, 0, 0),    # hop = T - 1 = 128
    (256, 129, 256, 70, 1, 16, False, 0, 0),
    (256, 65, 128, 3, 5, 3, True, 1, 0),     # input 4 bytes off a 16-byte boundary
    (256, 65, 128, 3, 5, 3, True, 0, 1),     # output 4 bytes off
    (256, 66, 128, 1, 5, 1, True, 1, 1),     # both, T % 4 = 2
    (100, 9, 50, 3, 5, 3, True, 0, 0),       # N = 100: 25 lanes own a quad, the other 39 idle
    (100, 9, 100, 70, 1, 1, False, 0, 0),
    (100, 7, 0, 1, 5, 16, False, 1, 1),      # T % 4 = 3
    (102, 9, 51, 3, 5, 3, True, 0, 0),       # N % 4 != 0 (100 is a multiple of 4): the last lane's quad is cut, rows are only 8-byte aligned
    (99, 9, 99, 70, 2, 1, True, 0, 0),       # odd N: rows are only 4-byte aligned, 16-byte accesses are impossible
    (99, 10, 9, 3, 5, 16, False, 0, 0),
]


@pytest.mark.parametrize("N,T,hop,R,F,K,with_prev,off_in,off_out", CASES)
def test_matches_the_definition(nat, N, T, hop, R, F, K, with_prev, off_in, off_out):
    util.configure_small(N)
    rng = np.random.default_rng([N, T, hop, R, F, K])
    x, prev = util.stream_windows(rng, R, N, hop, F)
    if not with_prev:
        prev = None
    h = util.wild(rng, (K, T))
    got = _filter(nat, x, h, hop, prev, off_in, off_out)
    util.same_bits(got, band_np.band_filter(x, h, hop, prev))


@pytest.mark.parametrize("N,T,hop,off", [(64, 5, 16, 0), (256, 65, 64, 0), (100, 9, 50, 0), (99, 9, 50, 0), (256, 65, 64, 1)])
def test_overlap_and_split_batch_identities(nat, N, T, hop, off):
    util.configure_small(N)
    rng = np.random.default_rng([N, T, hop, 99])
    F, F1, R, K = 5, 2, 3, 3
    x, prev = util.stream_windows(rng, R, N, hop, F)
    h = util.wild(rng, (K, T))
    whole = _filter(nat, x, h, hop, prev, off, off)
    for f in range(1, F):                                            # overlapping windows agree where both exist
        util.same_bits(whole[:, f, :, :N - hop], whole[:, f - 1, :, hop:])
    a = _filter(nat, x[:F1], h, hop, prev, off, off)
    b = _filter(nat, x[F1:], h, hop, x[F1 - 1], off, off)            # the carried window
    util.same_bits(np.concatenate([a, b], axis=1), whole)


# ------------------------------------------------------------------ refusals that are worth a device: nothing may be enqueued

def test_refused_calls_enqueue_nothing_and_touching_ranges_are_fine(nat):
    torch = util.torch_gpu()
    util.configure_small(64)
    rng = np.random.default_rng(5)
    x, prev = util.stream_windows(rng, 3, 64, 32, 2)
    h = util.wild(rng, (2, 9))
    for kw in (dict(hop=7), dict(hop=65), dict(hop=-1)):
        assert _filter(nat, x, h, kw["hop"], prev, expect_rc=-1) is None
    assert _filter(nat, x, util.wild(rng, (17, 9)), 32, prev, expect_rc=-1) is None
    # one allocation: [prev | frames | out], every range touching the next; then in place, which is refused and leaves the buffer as it was
    n_in, n_prev, n_out = x.size, prev.size, 2 * x.size
    buf = torch.full((n_prev + n_in + n_out + CANARY,), CANARY_VALUE, dtype=torch.float32, device="cuda")
    buf[:n_prev].copy_(torch.from_numpy(prev.ravel()))
    buf[n_prev:n_prev + n_in].copy_(torch.from_numpy(x.ravel()))
    d_h = torch.from_numpy(h).cuda()
    s = torch.cuda.current_stream().cuda_stream
    p = buf.data_ptr()
    call = lambda out_at: nat.lib.bf_band_filter_device(p + 4 * n_prev, 3, 2, 32, p, d_h.data_ptr(), 9, 2, p + 4 * out_at, s)
    assert call(n_prev + n_in) == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    util.same_bits(host[n_prev + n_in:n_prev + n_in + n_out].reshape(2, 2, 3, 64), band_np.band_filter(x, h, 32, prev))
    assert (host[n_prev + n_in + n_out:] == np.float32(CANARY_VALUE)).all()
    for out_at in (n_prev, n_prev + n_in - 1, n_prev - 1, 0):
        assert call(out_at) == -1 and b"overlaps" in nat.lib.bf_last_error()
        nat.lib.bf_clear_error()
    torch.cuda.synchronize()
    assert np.array_equal(util.bits(buf.cpu().numpy()), util.bits(host))


# ------------------------------------------------------------------ one captured graph: filter -> bf_das_device -> bf_peaks_device

def test_graph_filter_maps_peaks(nat):
    torch = util.torch_gpu()
    import band
    import synth
    c = util.configure("cfg1")
    M, N, X, Y = c["M"], c["N"], c["X"], c["Y"]
    D = X * Y
    mics = np.arange(M, dtype=np.int32)
    table = util.table_for("lerp", "cfg1")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    F, k = 3, 2
    h = band.design([(3000.0, 8000.0)], n_taps=65)
    first = synth.frame_batch(M, N, F)
    rng = np.random.default_rng(72)
    second = np.ascontiguousarray(util.inputs("cfg1")["s3"][None].repeat(F, 0) + (rng.standard_normal((F, M, N)) * 0.05).astype(np.float32))
    x = torch.from_numpy(first).cuda()
    d_h = torch.from_numpy(h).cuda()
    y = torch.empty((F, M, N), dtype=torch.float32, device="cuda")
    img = torch.empty((F, D), dtype=torch.float32, device="cuda")
    offs = torch.empty((F, k), dtype=torch.int32, device="cuda")
    vals = torch.empty((F, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty((F, 3), dtype=torch.int32, device="cuda")

    def step():
        s = torch.cuda.current_stream().cuda_stream
        assert nat.lib.bf_band_filter_device(x.data_ptr(), M, F, 128, None, d_h.data_ptr(), 65, 1, y.data_ptr(), s) == 0
        assert nat.lib.bf_das_device(util.ALGOS["lerp"], y.data_ptr(), M, img.data_ptr(), D, F, nat.iptr(mics), M, 0, D, s) == 0
        assert nat.lib.bf_peaks_device(img.data_ptr(), F, D, X, Y, 2, k, 0.25, 0.0, M, offs.data_ptr(), vals.data_ptr(), cnt.data_ptr(), s) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up for the map's digest and adaptive array; the filter needs none
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    x.copy_(torch.from_numpy(second).cuda())
    g.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy().copy() for t in (y, img, offs, vals, cnt)]
    step()                                              # eager on the same windows
    torch.cuda.synchronize()
    for a, t in zip(got, (y, img, offs, vals, cnt)):
        assert a.tobytes() == t.cpu().numpy().tobytes()
    util.same_bits(got[0], band_np.band_filter(second, h, 128, None)[0])
    assert (got[4][:, 0] >= 1).all()


# ------------------------------------------------------------------ band.BandFilter

def test_band_filter_class(nat):
    torch = util.torch_gpu()
    import band
    from listen import BeamListener
    c = util.configure("cfg1")
    M, N, D = c["M"], c["N"], c["X"] * c["Y"]
    table = util.table_for("lerp", "cfg1")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    rng = np.random.default_rng(11)
    hop, F = 128, 4
    x, prev = util.stream_windows(rng, M, N, hop, F)
    bf = band.BandFilter([(3000.0, 8000.0), (0.0, 2000.0), (6000.0, 1e9)], n_taps=65, hop=hop)
    assert bf.taps.shape == (3, 65) and bf.taps.dtype == np.float32
    d_x = torch.from_numpy(x).cuda()
    # a batch in two halves with advance() == the batch in one call behind the same carried window
    bf.advance(torch.from_numpy(prev[None]).cuda())
    whole = bf.frames(d_x).cpu().numpy()
    util.same_bits(whole, band_np.band_filter(x, bf.taps, hop, prev))
    a = bf.frames(d_x[:2]).cpu().numpy()
    carried = bf._prev.data_ptr()
    bf.advance(d_x[:2])
    assert bf._prev.data_ptr() == carried               # copied in place: a captured graph's pointer stays valid
    b = bf.frames(d_x[2:]).cpu().numpy()
    util.same_bits(np.concatenate([a, b], axis=1), whole)
    bf.reset()
    util.same_bits(bf.frames(d_x).cpu().numpy(), band_np.band_filter(x, bf.taps, hop, None))
    # maps: one bl.maps call on the [K * F, R, N] view of the filtered frames; a band's maps on their own may take another of the
    # map kernels (the planner looks at the frame count), which agree to the project's map tolerance, not in the bits
    bl = BeamListener("lerp", mics=np.arange(M, dtype=np.int32))
    maps = bf.maps(bl, d_x)
    assert tuple(maps.shape) == (3, F, D)
    y = bf.frames(d_x)
    assert maps.cpu().numpy().tobytes() == bl.maps(y.view(3 * F, M, N)).cpu().numpy().tobytes()
    for k in range(3):
        assert util.max_rel(maps[k].cpu().numpy(), bl.maps(y[k]).cpu().numpy()) < util.REL_TOL
    # taps= instead of a design; independent windows
    ready = band.BandFilter(taps=bf.taps[:1])
    assert ready.hop == 0 and ready.K == 1
    util.same_bits(ready.frames(d_x).cpu().numpy(), band_np.band_filter(x, bf.taps[:1], 0, None))
    with pytest.raises(ValueError):
        band.BandFilter([(3000.0, 8000.0)], n_taps=65, hop=32)      # 64 samples of history do not fit a hop of 32
    with pytest.raises(ValueError):
        band.BandFilter()


def test_filter_commutes_with_the_beam_exactly(nat):
    """Linearity end to end, in exact arithmetic: integer samples in [-8, 8], taps +-1, +-2, +-4 -- every product and partial sum is
    an integer far below 2^24, so float32 makes no rounding and the two orders must give the same bits.  Pad beams, independent
    windows (hop = 0).  The restriction taken here: the REAL cfg1 pad table (non-zero delays), compared from sample
    T - 1 + max_whole on -- the samples at which every microphone's delayed, filtered window is fully inside the window."""
    torch = util.torch_gpu()
    import band
    from listen import BeamListener
    c = util.configure("cfg1")
    M, N, D = c["M"], c["N"], c["X"] * c["Y"]
    table = np.ascontiguousarray(util.table_for("pad", "cfg1"), dtype=np.int32).ravel()
    nat.lib.load_coefficients_pad(nat.iptr(table), table.size); nat.check()
    max_whole = int(table.max())
    rng = np.random.default_rng(21)
    F, T = 3, 5
    x = rng.integers(-8, 9, size=(F, M, N)).astype(np.float32)
    h = (rng.choice([-1.0, 1.0], size=(2, T)) * np.exp2(rng.integers(0, 3, size=(2, T)))).astype(np.float32)
    bf = band.BandFilter(taps=h)
    bl = BeamListener("pad", mics=np.arange(M, dtype=np.int32))
    offsets = np.array([0, (D // 2) * M, (D - 1) * M], dtype=np.int32)
    d_x = torch.from_numpy(x).cuda()
    raw, st = bl.listen(d_x, offsets)
    assert (st.cpu().numpy() == 0).all()
    after = bf.beams(raw).cpu().numpy()                                 # [K, F, B, N]
    y = bf.frames(d_x)
    start = T - 1 + max_whole
    assert 0 < start < N // 2
    for k in range(2):
        before, st = bl.listen(y[k], offsets)
        util.same_bits(before.cpu().numpy()[:, :, start:], after[k][:, :, start:])
    assert np.abs(after).max() > 100 and np.array_equal(after, np.round(after))
    util.same_bits(after, band_np.band_filter(raw.cpu().numpy().reshape(1, F * 3, N), h)[:, 0].reshape(2, F, 3, N))
