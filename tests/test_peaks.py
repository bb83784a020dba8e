"""GPU (-m gpu): bf_peaks_device, the K loudest separated sources of every map, EQUAL to the NumPy restatement (tests/peaks_np.py).

The feature is comparisons and one float32 multiplication, so offsets, values and counts are compared for equality -- on both
internal forms (one workgroup per frame up to 13632 directions; row pass / column pass / merge over tiles of 1024 entries above,
here 361 x 361), which must not differ in any output."""
import numpy as np
import pytest

import peaks_np
import util
from support import nat

pytestmark = pytest.mark.gpu

SENTINEL_I, SENTINEL_F, TAIL = -77, -123.5, 16
SHAPES = [(11, 11), (57, 32), (101, 101), (361, 361), (1, 300), (300, 1)]
RADII = [0, 1, 4, 12, 400]                     # 400 >= max(rows, cols) of every shape


def _call(nat, d_power, F, stride, rows, cols, radius, k, floor_rel, floor_abs, per, values=True, counts=True):
    """bf_peaks_device into sentinel-filled buffers with a tail -> (offsets, values or None, counts or None) as host arrays; the tails
    are checked here."""
    torch = util.torch_gpu()
    d_o = torch.full((F * k + TAIL,), SENTINEL_I, dtype=torch.int32, device="cuda")
    d_v = torch.full((F * k + TAIL,), SENTINEL_F, dtype=torch.float32, device="cuda") if values else None
    d_c = torch.full((F * 3 + TAIL,), SENTINEL_I, dtype=torch.int32, device="cuda") if counts else None
    rc = nat.lib.bf_peaks_device(d_power.data_ptr(), F, stride, rows, cols, radius, k, floor_rel, floor_abs, per, d_o.data_ptr(),
                                 d_v.data_ptr() if values else None, d_c.data_ptr() if counts else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    o = d_o.cpu().numpy()
    assert (o[F * k:] == SENTINEL_I).all()
    out = [o[:F * k].reshape(F, k)]
    for d, n, s in ((d_v, k, np.float32(SENTINEL_F)), (d_c, 3, SENTINEL_I)):
        if d is None:
            out.append(None)
            continue
        h = d.cpu().numpy()
        assert (h[F * n:] == s).all()
        out.append(h[:F * n].reshape(F, n))
    return out


def _same(got, want, what):
    for name, g, w in zip(("offsets", "values", "counts"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert bad.size == 0, (what, name, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _populations(rng, rows, cols):
    """One frame per kind of map the issue lists (the 190-frame batch has its own test)."""
    D = rows * cols
    uniform = rng.uniform(0, 1, D).astype(np.float32)
    quant = (rng.integers(0, 4, D) * 0.25).astype(np.float32)            # four levels: ties and plateaus, across every tile edge of the tiled form
    constant = np.full(D, 0.375, dtype=np.float32)
    all_nan = np.full(D, np.nan, dtype=np.float32)
    signed = rng.standard_normal(D).astype(np.float32)                   # negative powers do not occur, the order does not care
    signed[rng.uniform(0, 1, D) < 0.05] = -0.0
    frames = [uniform, quant, constant, all_nan, signed]
    for base in (uniform, quant):
        m = base.copy()
        u = rng.uniform(0, 1, D)
        m[u < 0.10] = np.nan
        m[(u >= 0.10) & (u < 0.125)] = np.inf
        m[(u >= 0.125) & (u < 0.15)] = -np.inf
        frames.append(m)
    # smooth lobes: what a power map looks like (few candidates at a large radius, one per pixel of a lobe at radius 0)
    x, y = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    lobes = sum(a * np.exp(-((x - cx * rows) ** 2 + (y - cy * cols) ** 2) / (2.0 * (0.06 * max(rows, cols) + 1) ** 2))
                for a, cx, cy in ((1.0, 0.3, 0.6), (0.7, 0.75, 0.2), (0.4, 0.1, 0.1)))
    frames.append(lobes.astype(np.float32).ravel())
    return np.stack(frames)


class CachedCandidates:
    """peaks_np.candidates, once per (map, radius): the parameter sweeps below reuse the masks."""

    def __init__(self):
        self.memo = {}

    def __call__(self, img, radius):
        key = (img.shape, radius, util.sha(img))
        if key not in self.memo:
            self.memo[key] = peaks_np.candidates(img, radius)
        return self.memo[key]


# ------------------------------------------------------------------ 1. parity with the restatement

@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_parity_with_restatement(nat, shape, radius):
    torch = util.torch_gpu()
    rows, cols = shape
    D = rows * cols
    rng = np.random.default_rng([rows, cols, radius])
    maps = _populations(rng, rows, cols)
    F = maps.shape[0]
    n, T = 64, 8
    cand = CachedCandidates()
    above = float(np.nanmax(np.where(np.isfinite(maps), maps, np.nan)) * 2 + 1)
    sweeps = [  # k, floor_rel, floor_abs, stride - D, offset_per_dir
        (1, 0.0, 0.0, 0, n),
        (4, 0.25, 0.0, 13, n * T),
        (64, 0.0, -1e30, 0, n),
        (64, 1.0, 0.0, 5, n),
        (4, 0.0, above, 0, n),
        (4, 0.5, 0.26, 0, 1),
    ]
    for k, floor_rel, floor_abs, pad, per in sweeps:
        stride = D + pad
        power = np.empty((F, stride), dtype=np.float32)
        power[:, :D] = maps
        power[:, D:] = np.array([3e38, np.nan, np.inf] * 5, dtype=np.float32)[:pad]      # poison past the map: never read
        d_p = torch.from_numpy(power).cuda()
        got = _call(nat, d_p, F, stride, rows, cols, radius, k, floor_rel, floor_abs, per)
        want = peaks_np.peaks(power, rows, cols, radius, k, floor_rel, floor_abs, per, cand_fn=cand)
        _same(got, want, (shape, radius, k, floor_rel, floor_abs, pad, per))
    # what the definition promises, on the device results of the last sweep and of the first
    offs, vals, cnt = _call(nat, torch.from_numpy(maps).cuda(), F, D, rows, cols, radius, 64, 0.0, -1e30, 1)
    assert cnt[3].tolist() == [0, 0, D] and (offs[3] == -1).all() and (vals[3] == 0).all()          # all-NaN
    assert offs[2, 0] == 0                                                                           # constant: index 0 comes first
    if radius >= max(rows, cols):
        assert (cnt[[0, 1, 2, 4, 5, 6, 7], 1] == 1).all()                                            # one candidate per frame with a finite entry
    for f in range(F):
        filled = offs[f, :cnt[f, 0]]
        pts = np.stack([filled // cols, filled % cols], axis=1)
        if len(pts) > 1:
            d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)
            d[np.arange(len(pts)), np.arange(len(pts))] = 1 << 30
            assert d.min() > radius


def test_radius_zero_is_a_plain_top_k(nat):
    torch = util.torch_gpu()
    rows, cols, k = 101, 101, 64
    D = rows * cols
    rng = np.random.default_rng(3)
    maps = rng.uniform(0, 1, (3, D)).astype(np.float32)
    maps[1] = np.round(maps[1] * 8) / 8                                                             # heavy ties
    offs, vals, cnt = _call(nat, torch.from_numpy(maps).cuda(), 3, D, rows, cols, 0, k, 0.0, 0.0, 1)
    for f in range(3):
        order = np.argsort(-maps[f], kind="stable")[:k]
        assert offs[f].tolist() == order.tolist() and (vals[f] == maps[f][order]).all() and cnt[f].tolist() == [k, D, 0]


# ------------------------------------------------------------------ 2. one poisoned frame of a 190-frame batch

@pytest.mark.parametrize("shape,radius", [((57, 32), 4), ((101, 101), 4)], ids=["shipped", "cfg2"])
def test_one_poisoned_frame_of_a_batch(nat, shape, radius):
    torch = util.torch_gpu()
    rows, cols = shape
    D, F, bad = rows * cols, 190, 97
    rng = np.random.default_rng([F, rows, cols])
    clean = rng.uniform(0, 1, (F, D)).astype(np.float32)
    clean[::7] = np.round(clean[::7] * 4) / 4
    dirty = clean.copy()
    u = rng.uniform(0, 1, D)
    dirty[bad, u < 0.2] = np.nan
    dirty[bad, (u >= 0.2) & (u < 0.25)] = np.inf
    dirty[bad, (u >= 0.25) & (u < 0.3)] = -np.inf
    a = _call(nat, torch.from_numpy(clean).cuda(), F, D, rows, cols, radius, 4, 0.25, 0.0, 64)
    b = _call(nat, torch.from_numpy(dirty).cuda(), F, D, rows, cols, radius, 4, 0.25, 0.0, 64)
    _same(b, peaks_np.peaks(dirty, rows, cols, radius, 4, 0.25, 0.0, 64), "dirty")
    keep = np.arange(F) != bad
    for x, y in zip(a, b):
        assert x[keep].tobytes() == y[keep].tobytes()
    assert b[2][bad, 2] == int((~np.isfinite(dirty[bad])).sum()) and (a[2][:, 2] == 0).all()


# ------------------------------------------------------------------ 3. output hygiene

@pytest.mark.parametrize("shape", [(57, 32), (361, 361)], ids=["one_workgroup", "tiled"])
def test_null_outputs_and_repeatability(nat, shape):
    torch = util.torch_gpu()
    rows, cols = shape
    D, F = rows * cols, 5
    rng = np.random.default_rng(17)
    maps = (rng.integers(0, 16, (F, D)) / 16).astype(np.float32)
    d_p = torch.from_numpy(maps).cuda()
    full = _call(nat, d_p, F, D, rows, cols, 4, 8, 0.25, 0.0, 3)
    again = _call(nat, d_p, F, D, rows, cols, 4, 8, 0.25, 0.0, 3)
    for x, y in zip(full, again):
        assert x.tobytes() == y.tobytes()
    for values, counts in ((False, True), (True, False), (False, False)):
        part = _call(nat, d_p, F, D, rows, cols, 4, 8, 0.25, 0.0, 3, values=values, counts=counts)
        for x, y in zip(full, part):
            assert y is None or x.tobytes() == y.tobytes()


@pytest.mark.parametrize("shape", [(11, 11), (57, 32), (101, 101), (361, 361), (1, 300)], ids=lambda s: "%dx%d" % s)
def test_one_source_whole_grid_is_the_argmax_call(nat, shape):
    torch = util.torch_gpu()
    rows, cols = shape
    D, F, per = rows * cols, 6, 64
    rng = np.random.default_rng([9, rows, cols])
    maps = rng.uniform(0, 1, (F, D)).astype(np.float32)
    maps[1] = np.round(maps[1] * 4) / 4
    maps[2] = 0.5
    maps[3, D - 1] = 2.0
    d_p = torch.from_numpy(maps).cuda()
    d_a = torch.full((F, 1), -5, dtype=torch.int32, device="cuda")
    assert nat.lib.bf_peak_offsets_device(d_p.data_ptr(), F, D, D, per, d_a.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    offs, vals, cnt = _call(nat, d_p, F, D, rows, cols, max(rows, cols), 1, 0.0, 0.0, per)
    assert (offs == d_a.cpu().numpy()).all()
    assert (vals[:, 0] == maps.max(axis=1)).all() and (cnt == np.array([[1, 1, 0]] * F)).all()


@pytest.mark.parametrize("shape", [(101, 101), (361, 361)], ids=["one_workgroup", "tiled"])
def test_runs_in_a_captured_graph(nat, shape):
    torch = util.torch_gpu()
    rows, cols = shape
    D, F, k, radius, per = rows * cols, 4, 4, 4, 64
    rng = np.random.default_rng(23)
    first, second = (rng.uniform(0, 1, (F, D)).astype(np.float32) for _ in range(2))
    d_p = torch.from_numpy(first).cuda()
    d_o = torch.full((F, k), SENTINEL_I, dtype=torch.int32, device="cuda")
    d_v = torch.full((F, k), SENTINEL_F, dtype=torch.float32, device="cuda")
    d_c = torch.full((F, 3), SENTINEL_I, dtype=torch.int32, device="cuda")

    def step():
        assert nat.lib.bf_peaks_device(d_p.data_ptr(), F, D, rows, cols, radius, k, 0.25, 0.0, per, d_o.data_ptr(), d_v.data_ptr(), d_c.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up: the tiled form's buffer is allocated here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    d_p.copy_(torch.from_numpy(second).cuda())
    d_o.fill_(SENTINEL_I); d_v.fill_(SENTINEL_F); d_c.fill_(SENTINEL_I)
    g.replay()
    torch.cuda.synchronize()
    got = (d_o.cpu().numpy(), d_v.cpu().numpy(), d_c.cpu().numpy())
    _same(got, peaks_np.peaks(second, rows, cols, radius, k, 0.25, 0.0, per), "graph replay")


def test_sources_front_end(nat):
    torch = util.torch_gpu()
    import listen
    from interface import config
    util.configure("cfg1")
    bl = listen.BeamListener("fir_vec", mics=np.arange(5))
    rows, cols = config.MAX_RES_X, config.MAX_RES_Y
    rng = np.random.default_rng(31)
    maps = rng.uniform(0, 1, (3, rows * cols + 4)).astype(np.float32)
    d_p = torch.from_numpy(maps).cuda()
    offs, vals, cnt = bl.sources(d_p, k=3, radius=2)
    torch.cuda.synchronize()
    assert offs.shape == (3, 3) and offs.dtype == torch.int32 and vals.dtype == torch.float32 and cnt.shape == (3, 3) and offs.is_cuda
    want = peaks_np.peaks(maps, rows, cols, 2, 3, 0.5, 0.0, 5 * config.N_TAPS)
    _same((offs.cpu().numpy(), vals.cpu().numpy(), cnt.cpu().numpy()), want, "sources")
    # another grid than the configured one, and a column slice of a wider tensor
    offs, vals, cnt = bl.sources(d_p[:, :60], k=2, radius=1, floor_rel=0.0, floor_abs=0.1, shape=(6, 10))
    want = peaks_np.peaks(maps[:, :60], 6, 10, 1, 2, 0.0, 0.1, 5 * config.N_TAPS)
    _same((offs.cpu().numpy(), vals.cpu().numpy(), cnt.cpu().numpy()), want, "sources, shape")
    with pytest.raises(ValueError):
        bl.sources(d_p[:, :50], k=2, radius=1, shape=(6, 10))
    with pytest.raises(nat.BeamformerError, match="k = 65 > 64"):
        bl.sources(d_p, k=65, radius=1)


# ------------------------------------------------------------------ 4. end to end at the as-shipped size: two talkers, two beams

def two_source_frame():
    """256 mics x 256 samples: a plane wave from direction (19, 21) plus 0.7 x one from (42, 8)."""
    import synth
    c = util.CONFIGS["shipped"]
    d = util.oracle_delays("shipped")
    return np.ascontiguousarray(synth.s3_plane_wave(d[19, 21], c["N"], seed=1) + np.float32(0.7) * synth.s3_plane_wave(d[42, 8], c["N"], seed=2), dtype=np.float32)


def test_two_sources_end_to_end(nat, oracle_lib):
    torch = util.torch_gpu()
    import listen
    c = util.configure("shipped")
    M, N, X, Y, T = c["M"], c["N"], c["X"], c["Y"], c["T"]
    D = X * Y
    mics = np.arange(M, dtype=np.int32)
    table = util.table_for("lerp", "shipped")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    sig = two_source_frame()
    assert sig.shape == (M, N)
    d_sig = torch.from_numpy(sig[None]).cuda()
    d_img = torch.empty((1, D), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert nat.lib.bf_das_device(util.ALGOS["lerp"], d_sig.data_ptr(), M, d_img.data_ptr(), D, 1, nat.iptr(mics), M, 0, D, s) == 0
    bl = listen.BeamListener("lerp", mics=mics)
    offs, vals, cnt = bl.sources(d_img, k=4, radius=4, floor_rel=0.25)
    out, st = bl.listen(d_sig, offs)
    torch.cuda.synchronize()
    offs, vals, cnt, st, out = (t.cpu().numpy() for t in (offs, vals, cnt, st, out))
    img = d_img.cpu().numpy()[0]
    print("two-source map: sources", (offs[0] // M).tolist(), "powers", vals[0].tolist(), "counts", cnt[0].tolist())
    d1, d2 = 19 * Y + 21, 42 * Y + 8
    assert offs[0].tolist() == [d1 * M, d2 * M, -1, -1]
    assert cnt[0].tolist() == [2, 2, 0]
    assert vals[0, 0] == img[d1] and vals[0, 1] == img[d2] and (vals[0, 2:] == 0).all()
    assert st[0].tolist() == [0, 0, 1, 1]
    # the device map is the oracle's map bit for bit, so the restatement on the oracle's map gives the same answer
    orc = oracle_lib.Oracle(N, X, Y, T)
    want_img = orc.mimo_lerp(sig, table, mics).ravel()
    assert img.tobytes() == want_img.tobytes()
    want = peaks_np.peaks(want_img[None], X, Y, 4, 4, 0.25, 0.0, M)
    _same((offs, vals, cnt), want, "oracle map")
    # the two beams are bf_miso_device's at d * n; the empty slots are NaN rows
    d_direct = torch.tensor([[d1 * M, d2 * M]], dtype=torch.int32, device="cuda")
    d_out = torch.empty((1, 2, N), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_miso_device(util.ALGOS["lerp"], d_sig.data_ptr(), M, 1, nat.iptr(mics), M, d_direct.data_ptr(), 2, 0.0, d_out.data_ptr(), N, None, s) == 0
    torch.cuda.synchronize()
    assert out[0, :2].tobytes() == d_out.cpu().numpy()[0].tobytes()
    assert np.isfinite(out[0, :2]).all() and np.isnan(out[0, 2:]).all()
    for b, d in enumerate((d1, d2)):
        assert out[0, b].tobytes() == orc.miso_lerp(sig, table, mics, d * M).tobytes()
