"""GPU (-m gpu): bf_whiten_device and whiten.Whitener against the NumPy restatement of the definition (tests/whiten_np.py) within its
derived tolerance, the definition's promises on the bytes, one captured graph, and the claim the feature rests on: under a hum 20 dB
above it, the whitened map's loudest source is the broadband source and the plain band-pass map's is not.

Data: white-noise rows whose scales spread over 2^-6 .. 2^5 plus a tone at bin 3 of the row's own scale (the one-bin bands sit there: a
band of one noise bin can be arbitrarily quiet, and then no float32 transform resolves its sign).  Every call writes into the middle of
a buffer of canary floats, which must survive."""
import numpy as np
import pytest

import util
import whiten_np as wn
from support import nat_restoring as nat
from util import CANARY, CANARY_VALUE

pytestmark = pytest.mark.gpu

TONE_BIN = 3


def _whiten(nat, x, window, bins, beta, gain, floor_rel=1e-3, floor_abs=0.0, off_in=0, off_out=0, off_win=0):
    """bf_whiten_device on device copies of x float32 [F, R, N] -> float32 [K, F, R, N]; the canaries around the output are checked."""
    torch = util.torch_gpu()
    F, R, N = x.shape
    bins = np.ascontiguousarray(bins, dtype=np.int32).reshape(-1, 2)
    K = bins.shape[0]
    beta, gain = np.ascontiguousarray(beta, dtype=np.float32), np.ascontiguousarray(gain, dtype=np.float32)
    assert beta.shape == gain.shape == (K,)
    total = K * F * R * N
    keep_x, d_x = util.place(x, off_in)
    keep_w, d_w = (None, None) if window is None else util.place(window, off_win)
    buf = torch.full((CANARY + 4 + total + CANARY,), CANARY_VALUE, dtype=torch.float32, device="cuda")
    out = buf[CANARY + off_out:CANARY + off_out + total]
    assert out.data_ptr() % 16 == 4 * off_out and d_x.data_ptr() % 16 == 4 * off_in
    rc = nat.lib.bf_whiten_device(d_x.data_ptr(), R, F, None if d_w is None else d_w.data_ptr(), nat.iptr(bins), nat.fptr(beta), nat.fptr(gain), K,
                                  floor_rel, floor_abs, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, nat.lib.bf_last_error()
    host = buf.cpu().numpy()
    lo, hi = CANARY + off_out, CANARY + off_out + total
    assert (host[:lo] == np.float32(CANARY_VALUE)).all() and (host[hi:] == np.float32(CANARY_VALUE)).all()
    return host[lo:hi].reshape(K, F, R, N).copy()


def rows_with_tone(rng, shape):
    """wn.noise_rows plus a tone at TONE_BIN of each row's own scale and a random phase."""
    N = shape[-1]
    scale = np.exp2(rng.integers(-6, 6, size=shape[:-1] + (1,)).astype(np.float64))
    phase = rng.uniform(0, 2 * np.pi, size=shape[:-1] + (1,))
    t = np.arange(N, dtype=np.float64)
    return ((rng.standard_normal(shape) + np.cos(2 * np.pi * TONE_BIN * t / N + phase)) * scale).astype(np.float32)


def sixteen(N, widest):
    """16 bands of at most `widest` bins: some touch bin 0, some bin N / 2, some are the one bin of the tone; beta cycles 0, 0.5, 1."""
    top = N // 2 + 1
    bands = []
    for i in range(16):
        beta = (0.0, 0.5, 1.0)[i % 3]
        if i % 4 == 0:
            bands.append((0, min(widest, top) - i, beta))
        elif i % 4 == 1:
            bands.append((max(top - widest, 0) + i, top + 5, beta))             # (past the end: clipped)
        elif i % 4 == 2:
            bands.append((TONE_BIN, TONE_BIN + 1, beta))
        else:
            bands.append((1 + i % 7, min(1 + i % 7 + widest, top - 1), beta))
    return bands


# ------------------------------------------------------------------ the definition, every shape the kernel treats differently

#        N     R   F  bands (lo, hi, beta)                                        floor_rel floor_abs window off_in off_out off_win
CASES = [
    (32, 1, 1, [(0, 17, 1.0)], 1e-3, 0.0, "hann", 0, 0, 0),                                    # smallest: one wave, half a pass per lane
    (32, 3, 2, sixteen(32, 17), 5e-2, 0.0, None, 0, 0, 0),                                     # K = 16, no window
    (256, 64, 3, [(1, 129, 1.0)], 1e-3, 0.25, "hann", 1, 0, 0),                                # floor_abs > 0; input one float off
    (512, 70, 5, [(0, 257, 1.0), (128, 257, 0.5), (TONE_BIN, TONE_BIN + 1, 1.0)], 1e-3, 0.0, "hann", 0, 0, 0),    # largest one-wave; 350 workgroups
    (512, 1, 1, sixteen(512, 257), 5e-2, 0.0, "hann", 0, 1, 1),                                # output and window one float off
    (1024, 3, 2, sixteen(1024, 513), 1e-3, 0.0, "hann", 1, 1, 0),                              # four waves, K = 16, both pointers off
    (1024, 70, 5, [(1, 513, 1.0)], 5e-2, 0.0, None, 0, 0, 0),                                  # four waves, 350 workgroups, no window
    (1024, 1, 1, [(0, 513, 0.0)], 1e-3, 0.0, None, 0, 0, 0),                                   # beta = 0, rect, full band: the identity
    (1024, 3, 2, sixteen(1024, 513), 5e-2, 0.5, "hann", 0, 0, 0),                              # K = 16 under an absolute floor
    (64, 70, 40, [(0, 33, 1.0), (TONE_BIN, TONE_BIN + 1, 0.5)], 1e-3, 0.0, "hann", 0, 0, 0),   # 2800 items on a grid of 2048: 752 one-wave workgroups walk to a second item
    (1024, 70, 30, [(1, 513, 1.0)], 5e-2, 0.0, "hann", 0, 0, 0),                               # 2100 items: 52 four-wave workgroups walk
    # (N = 2048 and 4096, which the entry point and the kernel take, cannot be reached: bf_configure refuses N_SAMPLES > 1024)
]

@pytest.mark.parametrize("N,R,F,bands,floor_rel,floor_abs,window,off_in,off_out,off_win", CASES)
def test_matches_the_definition(nat, N, R, F, bands, floor_rel, floor_abs, window, off_in, off_out, off_win):
    """Within the derived tolerance of whiten_np (largest error / tolerance measured on the MI355X over these cases: see DESIGN.md 2);
    a case counts only if the tolerance is at most 0.05 of every row's RMS output, which the restatement alone decides."""
    import features
    util.configure_small(N)
    rng = np.random.default_rng([N, R, F, len(bands)])
    x = rows_with_tone(rng, (F, R, N))
    w = features.hann(N) if window == "hann" else None
    bins = [(lo, hi) for lo, hi, _ in bands]
    beta = [b for _, _, b in bands]
    gain = [N / np.sqrt(max(min(hi, N // 2 + 1) - lo, 1)) for lo, hi, _ in bands]
    want, tol = wn.whiten(x, w, bins, beta, gain, floor_rel, floor_abs, with_tol=True)
    condition = float((tol.max(axis=-1) / wn.row_rms(want)).max())
    assert np.isfinite(tol).all() and condition <= 0.05, condition
    got = _whiten(nat, x, w, bins, beta, gain, floor_rel, floor_abs, off_in, off_out, off_win)
    ratio = float((np.abs(got - want) / tol).max())
    print("N = %d, %d x %d rows, K = %d: largest error / tolerance %.4f (tolerance / row RMS at most %.4f)" % (N, F, R, len(bands), ratio, condition))
    assert np.isfinite(got).all() and ratio <= 1.0, ratio
    if bands == [(0, 513, 0.0)]:                   # the identity to roundoff: out == gain * x
        assert np.abs(got[0] - gain[0] * x.astype(np.float64)).max() <= tol.max()


# ------------------------------------------------------------------ the promises, on the bytes

def _setup(N, seed):
    import features
    util.configure_small(N)
    rng = np.random.default_rng([N, seed])
    return rng, features.hann(N)


BANDS3 = ([(1, 40), (0, 17), (5, 6)], [1.0, 0.5, 0.0], [3.0, 1.0, -2.0])


@pytest.mark.parametrize("N", [64, 1024])
def test_a_band_of_a_k_band_call_equals_the_single_band_call(nat, N):
    rng, w = _setup(N, 1)
    x = rows_with_tone(rng, (2, 3, N))
    bins, beta, gain = BANDS3
    whole = _whiten(nat, x, w, bins, beta, gain)
    for b in range(3):
        util.same_bits(_whiten(nat, x, w, bins[b:b + 1], beta[b:b + 1], gain[b:b + 1])[0], whole[b])
    swapped = _whiten(nat, x, w, bins[::-1], beta[::-1], gain[::-1])
    util.same_bits(swapped[::-1], whole)


@pytest.mark.parametrize("N", [64, 512, 1024])
def test_a_row_equals_itself_alone_elsewhere_and_at_another_alignment(nat, N):
    rng, w = _setup(N, 2)
    F, R = 5, 70
    x = rows_with_tone(rng, (F, R, N))
    bins, beta, gain = BANDS3
    whole = _whiten(nat, x, w, bins, beta, gain)
    row = x[3, 41]
    alone = _whiten(nat, row[None, None], w, bins, beta, gain, off_in=1, off_out=1, off_win=1)            # one row, every pointer off
    util.same_bits(alone[:, 0, 0], whole[:, 3, 41])
    y = rows_with_tone(rng, (2, 7, N))
    y[1, 6] = row                                                                                        # another index, frame and batch size
    util.same_bits(_whiten(nat, y, w, bins, beta, gain, off_in=1)[:, 1, 6], whole[:, 3, 41])
    util.same_bits(_whiten(nat, x[:2, :9], w, bins, beta, gain, off_out=1), whole[:, :2, :9])


GRID = 2048             # workgroups of a launch (kWhitenMaxGrid in whiten.hip): item i >= GRID is the second item of workgroup i - GRID


@pytest.mark.parametrize("N,F,R", [(64, 40, 70), (1024, 30, 70)])
def test_a_row_a_workgroup_takes_as_its_second_item_equals_itself_alone(nat, N, F, R):
    """More items than the grid has workgroups: the rows past GRID are second items, computed behind another row in the same LDS with the
    twiddles of the first trip.  They equal themselves alone and as a first item, and so do the first items in front of them."""
    rng, w = _setup(N, 6)
    assert F * R > GRID
    x = rows_with_tone(rng, (F, R, N))
    bins, beta, gain = BANDS3
    whole = _whiten(nat, x, w, bins, beta, gain).reshape(3, F * R, N)
    flat = x.reshape(F * R, N)
    tail = _whiten(nat, flat[None, GRID:], w, bins, beta, gain, off_in=1)[:, 0]      # the second items as the first items of a smaller call
    util.same_bits(tail, whole[:, GRID:])
    for i in (GRID, F * R - 1, F * R - 1 - GRID):                                   # a second item, the last one, and the first item in front of it
        util.same_bits(_whiten(nat, flat[None, None, i], w, bins, beta, gain, off_out=1)[:, 0, 0], whole[:, i])
    nan = x.copy()
    nan.reshape(F * R, N)[5, 3] = np.nan                                            # a NaN first item leaves the second item of its workgroup alone
    after = _whiten(nat, nan, w, bins, beta, gain).reshape(3, F * R, N)
    util.same_bits(after[:, 5 + GRID], whole[:, 5 + GRID])
    assert np.isnan(after[:, 5]).all()


@pytest.mark.parametrize("N", [32, 1024])
@pytest.mark.parametrize("floor_abs", [0.0, 0.5])
def test_zero_rows_give_zeros_and_leave_their_neighbours_alone(nat, N, floor_abs):
    rng, w = _setup(N, 3)
    x = rows_with_tone(rng, (2, 5, N))
    bins, beta, gain = [(0, N // 2 + 1), (1, 9), (0, 17)], [1.0, 0.5, 0.0], [1.0, 2.0, 3.0]
    before = _whiten(nat, x, w, bins, beta, gain, floor_abs=floor_abs)
    z = x.copy()
    z[0, 2] = 0.0
    z[1, 4] = 0.0
    after = _whiten(nat, z, w, bins, beta, gain, floor_abs=floor_abs)
    assert not after[:, 0, 2].any() and not after[:, 1, 4].any()
    keep = np.ones((2, 5), bool)
    keep[0, 2] = keep[1, 4] = False
    util.same_bits(after[:, keep], before[:, keep])
    assert not _whiten(nat, np.zeros((1, 1, N), np.float32), None, bins, beta, gain, floor_abs=floor_abs).any()


@pytest.mark.parametrize("N", [64, 1024])
def test_a_power_of_two_gain_leaves_phat_unchanged_and_scales_the_band_pass_exactly(nat, N):
    rng, w = _setup(N, 4)
    x = rows_with_tone(rng, (2, 6, N))
    e = np.array([-9, -3, -1, 1, 4, 11], dtype=np.float64)[None, :, None]
    scaled = (x * np.exp2(e)).astype(np.float32)
    assert np.array_equal(scaled.astype(np.float64), x * np.exp2(e))
    bins, beta, gain = [(1, N // 2), (0, N // 2 + 1), (1, N // 2)], [1.0, 1.0, 0.0], [N / 8.0, 1.0, 1.0]
    for fr in (1e-3, 5e-2):
        a = _whiten(nat, x, w, bins, beta, gain, floor_rel=fr)
        b = _whiten(nat, scaled, w, bins, beta, gain, floor_rel=fr)
        util.same_bits(b[:2], a[:2])
        util.same_bits(b[2], (a[2] * np.exp2(e)).astype(np.float32))
        assert np.array_equal(b[2].astype(np.float64), a[2] * np.exp2(e))


@pytest.mark.parametrize("N", [64, 1024])
def test_a_nan_row_and_an_inf_row_leave_every_other_row_as_it_was(nat, N):
    rng, w = _setup(N, 5)
    x = rows_with_tone(rng, (3, 4, N))
    bins, beta, gain = BANDS3
    before = _whiten(nat, x, w, bins, beta, gain)
    bad = x.copy()
    bad[1, 2, 7] = np.nan
    bad[2, 0, N - 1] = np.inf
    bad[0, 3, 0] = -np.inf
    after = _whiten(nat, bad, w, bins, beta, gain)
    keep = np.ones((3, 4), bool)
    keep[1, 2] = keep[2, 0] = keep[0, 3] = False
    util.same_bits(after[:, keep], before[:, keep])
    assert not np.isfinite(after[:, ~keep]).all()


# ------------------------------------------------------------------ Whitener, one captured graph, and the claim on the device

def _listener(nat, X, Y, N):
    """BeamListener on the 8 x 8 array over an X x Y grid of N-sample windows, lerp tables of the scene's delays."""
    import directions_np as D
    from interface import config
    from listen import BeamListener
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=8)
    delays = np.ascontiguousarray(D.calculate_delays(X, Y, arrays=1), dtype=np.float32)
    nat.lib.load_coefficients_lerp(nat.fptr(delays), delays.size); nat.check()
    return BeamListener("lerp", mics=np.arange(64, dtype=np.int32))


def _hum_batch(seeds):
    import directions_np as D
    delays = D.calculate_delays(wn.HUM["X"], wn.HUM["Y"], arrays=1)
    return np.stack([wn.hum_frame(s, delays, **wn.HUM) for s in seeds])


def test_graph_replay_of_whitener_maps_equals_eager(nat):
    torch = util.torch_gpu()
    import whiten
    X, Y, N = wn.HUM["X"], wn.HUM["Y"], wn.HUM["n"]
    bl = _listener(nat, X, Y, N)
    wh = whiten.Whitener([(1000.0, 12000.0), (1000.0, 12000.0, 0.0)], fs=wn.HUM["fs"])
    first, second = _hum_batch([10, 11]), _hum_batch([12, 13])
    x = torch.from_numpy(first).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bl.maps(torch.cat([x, x]))                      # eager warm-up for the map's digest and adaptive array; the whitener needs none:
                                                        # its first call is the captured one (the window went to the device in __init__)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        maps = wh.maps(bl, x)
    x.copy_(torch.from_numpy(second).cuda())
    g.replay()
    torch.cuda.synchronize()
    got = maps.cpu().numpy().copy()
    assert tuple(got.shape) == (2, 2, X * Y)
    eager = wh.maps(bl, x).cpu().numpy()
    assert got.tobytes() == eager.tobytes()
    y = wh.frames(x)
    assert eager.tobytes() == bl.maps(y.view(4, 64, N)).cpu().numpy().tobytes()      # ONE bl.maps call on the [K * F, R, N] view
    want = wn.whiten(second, wh.window, wh.bins, wh.beta, wh.gain, wh.floor_rel, wh.floor_abs)
    assert np.abs(y.cpu().numpy() - want).max() < 1e-3 * wn.row_rms(want).max()


def test_the_whitened_map_finds_the_source_under_the_hum(nat):
    """The hum scene (wn.HUM, seeds 0 .. 3) through Whitener.maps and bl.sources on the device: the whitened band's loudest source is the
    source's cell, the beta = 0 band's is not, and listening on the RAW frames at the whitened map's offset works."""
    torch = util.torch_gpu()
    import whiten
    X, Y, N, fs = wn.HUM["X"], wn.HUM["Y"], wn.HUM["n"], wn.HUM["fs"]
    lo, hi = wn.HUM["bins"]
    bl = _listener(nat, X, Y, N)
    f_lo, f_hi = lo * fs / N, (hi - 1) * fs / N
    wh = whiten.Whitener([(f_lo, f_hi + 1.0), (f_lo, f_hi + 1.0, 0.0)], fs=fs)
    assert wh.bins.tolist() == [[lo, hi], [lo, hi]]
    x = torch.from_numpy(_hum_batch([0, 1, 2, 3])).cuda()
    maps = wh.maps(bl, x)                               # [2, 4, D]
    src_cell = wn.HUM["src"][0] * Y + wn.HUM["src"][1]
    for b, name in ((0, "whitened"), (1, "band-pass")):
        offs, vals, cnt = bl.sources(maps[b], k=1, radius=2)
        cells = (offs.cpu().numpy()[:, 0] // 64).tolist()
        n3 = [wn.within_3db(m) for m in maps[b].cpu().numpy()]
        print("%s: loudest cells %s (source %d), cells within 3 dB %s" % (name, [divmod(c, Y) for c in cells], src_cell, n3))
        if b == 0:
            assert cells == [src_cell] * 4, cells
            out, st = bl.listen(x, offs[:, :1])
            assert (st.cpu().numpy() == 0).all() and np.isfinite(out.cpu().numpy()).all()
        else:
            assert src_cell not in cells, cells
