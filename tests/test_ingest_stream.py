"""GPU (-m gpu): bf_ingest_stream_device / ingest.PacketIngest, a datagram stream -> a batch of frames in one launch, BIT FOR BIT
against the oracle chain: every frame is `oracle_ingest` (the checker pinned to the reference's real receiver, tests/test_ingest.py)
on that frame's slice of the stream, with the masked rows and the rows past n_arrays * 64 zeroed in NumPy.  No tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import util
from support import nat

pytestmark = pytest.mark.gpu

PROBES = [2 ** 31 - 1, -2 ** 31, 16777217, -16777217, 33554433, 1, -1, 0]      # int -> float roundings (test_ingest.datagrams)
VER = 2
CANARY = 0x5A5AA5A5
GUARD = 1024                                                                    # 4-byte elements: 4 KiB on either side


@pytest.fixture(autouse=True)
def shipped_sizes_afterwards():
    yield
    util.configure("shipped")


def sizes(M, N):
    from interface import config
    config.configure(N_MICROPHONES=M, N_SAMPLES=N, ACTIVE_TILES=M // 64)


def datagrams(T, M, n_arrays, seed, counter0=1000):
    """T seeded datagrams [T, 8 + 4 * M] as test_ingest.datagrams makes them; the rounding probes sit in every 61st datagram (so every
    frame of every hop sees some) at a column that moves, the header carries n_arrays, version 2 and a counter that steps by one."""
    rng = np.random.default_rng([seed, T, M])
    stream = rng.integers(-2 ** 23, 2 ** 23, size=(T, M), dtype=np.int32)
    for i, t in enumerate(range(0, T, 61)):
        c = (11 * i) % (M - 7)
        stream[t, c:c + 8] = PROBES
    stream[T - 1, M - 8:] = PROBES
    pk = np.zeros((T, 8 + 4 * M), dtype=np.uint8)
    pk[:, 8:] = stream.view(np.uint8).reshape(T, 4 * M)
    pk[:, 0], pk[:, 1] = 0xBC, 0xBE                                             # frequency: not looked at
    pk[:, 2], pk[:, 3] = n_arrays, VER
    set_counters(pk, (np.arange(T, dtype=np.int64) + counter0).astype(np.uint32))
    return pk


def set_counters(pk, counters):
    pk[:, 4:8] = np.ascontiguousarray(counters, dtype="<u4").view(np.uint8).reshape(-1, 4)


def reference_rows(nat, m_total):
    n = nat.lib.bf_default_disabled_mics(None)
    rows = np.zeros(n, dtype=np.int32)
    nat.lib.bf_default_disabled_mics(nat.iptr(rows))
    return rows[rows < m_total]


def mask_of(nat, kind, m_total):
    """None | "reference" | "single" | "every" -> uint8 [m_total] or None."""
    if kind is None:
        return None
    mask = np.zeros(m_total, dtype=np.uint8)
    if kind == "reference":
        mask[reference_rows(nat, m_total)] = 1
    elif kind == "single":
        mask[min(37, m_total - 1)] = 1
    else:
        mask[:] = 1
    return mask


def oracle_frames(oracle_lib, pk, M, N, n_arrays, hop, F, m_total, mask):
    """The expected batch: oracle_ingest per frame slice, then the zeroing the issue states, in NumPy."""
    lib = C.CDLL(os.path.join(util.ROOT, "oracle", "libdas_oracle.so"))
    want = np.zeros((F, m_total, N), dtype=np.float32)
    k = n_arrays * 64
    for f in range(F):
        piece = np.ascontiguousarray(pk[f * hop:f * hop + N])
        assert piece.shape[0] == N
        out = np.zeros(M * N, dtype=np.float32)
        lib.oracle_ingest(piece.ctypes.data_as(C.c_void_p), N, M, n_arrays, 8, 8, out.ctypes.data_as(C.POINTER(C.c_float)))
        want[f, :k] = out.reshape(M, N)[:k]
    want[:, k:] = 0.0
    if mask is not None:
        want[:, mask.astype(bool)] = 0.0
    return want


def numpy_status(pk, N, n_arrays, hop, F, ver=VER):
    st = np.zeros((F, 4), dtype=np.int64)
    for f in range(F):
        h = pk[f * hop:f * hop + N]
        c = np.ascontiguousarray(h[:, 4:8]).view("<u4").ravel()
        st[f] = [(h[:, 3] != ver).sum(), (h[:, 2] != n_arrays).sum(), ((c[1:] - c[:-1]).astype(np.uint32) != 1).sum(), c[:1].view(np.int32)[0]]
    return st.astype(np.int32)


def run(nat, d_pk, T, n_arrays, hop, F, m_total, d_mask, d_frames, d_status, ver=VER):
    torch = util.torch_gpu()
    rc = nat.lib.bf_ingest_stream_device(d_pk.data_ptr(), T, n_arrays, 8, 8, hop, F, m_total, None if d_mask is None else d_mask.data_ptr(), ver,
                                         d_frames.data_ptr(), None if d_status is None else d_status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()


def _same(got, want):
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.int32) != want.view(np.int32))[:8]


# ------------------------------------------------------------------ 1. frame parity
#         M    N     n_arrays F    hop        m_total mask         byte offsets of d_packets / d_frames inside their allocations
CASES = [
    (256, 256,  4, 190, "N",     256, "reference", 0, 0),          # the bench batch at the as-shipped size; the past-the-datagram element
    (256, 256,  3, 7,   "N/2",   192, None,        0, 0),
    (256, 256,  1, 2,   "1",     256, "single",    0, 0),
    (256, 256,  4, 1,   "N",     256, "every",     0, 0),
    (256, 256,  3, 2,   "N+37",  256, "reference", 0, 0),
    (256, 256,  4, 7,   "N/2",   300, "single",    4, 4),          # pointers only 4-byte aligned: the narrow forms of both sides
    (64,  256,  1, 190, "N",     64,  None,        0, 0),          # the bench batch at the config 2 size
    (64,  256,  1, 190, "1",     64,  "reference", 0, 0),
    (64,  256,  1, 7,   "N+37",  100, "single",    0, 8),
    (256, 1024, 4, 7,   "N/2",   256, None,        0, 0),          # config 5
    (256, 1024, 4, 2,   "N+37",  300, "reference", 0, 0),
    (128, 100,  1, 7,   "N",     64,  None,        0, 0),
    (128, 100,  2, 2,   "N/2",   130, "reference", 0, 0),
    (128, 100,  2, 190, "1",     128, "every",     0, 0),
    (128, 100,  1, 1,   "N",     128, "single",    4, 12),
    (256, 516,  4, 7,   "N+37",  256, "reference", 0, 0),
    (256, 516,  4, 2,   "1",     256, None,        0, 0),
    (256, 516,  4, 1,   "N/2",   257, "single",    8, 4),
]


def hop_of(text, N):
    return {"N": N, "N/2": N // 2, "1": 1, "N+37": N + 37}[text]


def test_cases_cover_what_the_issue_lists():
    assert {c[:3] for c in CASES} >= {(256, 256, 1), (256, 256, 3), (256, 256, 4), (64, 256, 1), (256, 1024, 4), (128, 100, 1), (128, 100, 2), (256, 516, 4)}
    assert {c[3] for c in CASES} == {1, 2, 7, 190} and {c[4] for c in CASES} == {"N", "N/2", "1", "N+37"}
    assert {c[6] for c in CASES} == {None, "reference", "single", "every"}
    assert any(c[5] == c[2] * 64 for c in CASES) and any(c[5] > c[2] * 64 for c in CASES)
    assert (256, 256, 190) in {(c[0], c[1], c[3]) for c in CASES} and (64, 256, 190) in {(c[0], c[1], c[3]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-a%d-F%d-hop%s-m%d-%s-o%d.%d" % c)
def test_frames_match_oracle(nat, oracle_lib, case):
    torch = util.torch_gpu()
    M, N, n_arrays, F, hop_text, m_total, mask_kind, off_in, off_out = case
    sizes(M, N)
    hop = hop_of(hop_text, N)
    T = (F - 1) * hop + N + 3                                                   # three datagrams more than the frames need
    pk = datagrams(T, M, n_arrays, seed=F + hop)
    mask = mask_of(nat, mask_kind, m_total)
    whole_in = torch.zeros(pk.size + 16, dtype=torch.uint8, device="cuda")
    d_pk = whole_in[off_in:off_in + pk.size]
    d_pk.copy_(torch.from_numpy(pk.ravel()))
    whole_out = torch.full((F * m_total * N + 4,), float("nan"), dtype=torch.float32, device="cuda")
    d_frames = whole_out[off_out // 4:off_out // 4 + F * m_total * N]
    d_status = torch.full((F, 4), -7, dtype=torch.int32, device="cuda")
    d_mask = None if mask is None else torch.from_numpy(mask).cuda()
    run(nat, d_pk, T, n_arrays, hop, F, m_total, d_mask, d_frames, d_status)
    got = d_frames.cpu().numpy().reshape(F, m_total, N)
    want = oracle_frames(oracle_lib, pk, M, N, n_arrays, hop, F, m_total, mask)
    assert not np.isnan(got).any()                                              # every element is written
    _same(got, want)
    if mask_kind is None:       # the comparison is not one of zeros with zeros: at most one row (the past-the-datagram one) and the probes' zeros are 0
        assert np.count_nonzero(got[:, :n_arrays * 64]) > 0.99 * F * (n_arrays * 64 - 1) * N
    assert np.array_equal(d_status.cpu().numpy(), numpy_status(pk, N, n_arrays, hop, F))
    edge = whole_out.cpu().numpy()
    assert np.isnan(edge[:off_out // 4]).all() and np.isnan(edge[off_out // 4 + F * m_total * N:]).all()


def test_past_the_datagram_element_is_zero_in_a_stream(nat, oracle_lib):
    """All four arrays present: row 248 (last array, last row, x = 0) reads stream[256], which in a stream is the next datagram's header.
    It comes out as 0 whatever that header holds, and the rows around it are data."""
    torch = util.torch_gpu()
    M = N = 256
    sizes(M, N)
    F, T = 2, 2 * N
    pk = datagrams(T, M, 4, seed=3, counter0=0x7F7F7F7F)
    pk[:, 0], pk[:, 1] = 0xFF, 0x7F                                             # a header word that would be a large sample
    d_frames = torch.full((F, M, N), float("nan"), dtype=torch.float32, device="cuda")
    run(nat, torch.from_numpy(pk).cuda(), T, 4, N, F, M, None, d_frames, None)
    got = d_frames.cpu().numpy()
    assert (got[:, 248] == 0.0).all() and np.count_nonzero(got[:, 247]) > 0 and np.count_nonzero(got[:, 249]) > 0
    _same(got, oracle_frames(oracle_lib, pk, M, N, 4, N, F, M, None))


# ------------------------------------------------------------------ 2. the header report

@pytest.mark.parametrize("hop_text", ["N", "N/2", "N+37", "1"])
def test_status_counts(nat, hop_text):
    torch = util.torch_gpu()
    M, N, n_arrays = 256, 256, 3
    sizes(M, N)
    hop = hop_of(hop_text, N)
    F = 7
    T = (F - 1) * hop + N
    pk = datagrams(T, M, n_arrays, seed=9)
    counters = (np.arange(T, dtype=np.int64) + 2 ** 31 - 300).astype(np.uint32)  # steps through the int32 wrap at datagram 300: not a jump
    for t, jump in ((5, 2), (301, -3), (700, 2 ** 31)):
        if t < T:
            counters[t:] += np.uint32(jump % 2 ** 32)
    if 300 < T:
        counters[300:] += np.uint32(6)                                          # a jump across the wrap itself: 2^31 - 1 -> -2^31 + 6
    for f in range(1, F):                                                       # jumps lying exactly on frame boundaries of the hop = N framing
        if f * N < T and f in (2, 3):
            counters[f * N:] += np.uint32(40)
    set_counters(pk, counters)
    for t in (0, 17, N - 1, N, T - 1, T // 2):
        pk[t, 3] = 1                                                            # wrong version
    for t in (1, N // 2, N + 1, T - 2):
        pk[t, 2] = n_arrays + 1                                                 # wrong n_arrays
    pk[T // 3, 2], pk[T // 3, 3] = 0xFF, 0x82                                   # both, with the sign bit set
    want = numpy_status(pk, N, n_arrays, hop, F)
    d_frames = torch.empty((F, M, N), dtype=torch.float32, device="cuda")
    d_status = torch.full((F, 4), 12345, dtype=torch.int32, device="cuda")      # not cleared by the caller
    d_pk = torch.from_numpy(pk).cuda()
    run(nat, d_pk, T, n_arrays, hop, F, M, None, d_frames, d_status)
    got = d_status.cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    if hop_text == "N":
        assert want[:, 0].sum() == 7 and want[:, 1].sum() == 5 and want[:, 2].sum() == 4    # the boundary jumps (2N, 3N) are in no frame's count
    if hop_text == "N/2":
        assert want[:, 2].sum() > 4                                             # overlapping windows see the same jumps inside a frame
    run(nat, d_pk, T, n_arrays, hop, F, M, None, d_frames, d_status)           # a second call over the first one's results: same report
    assert np.array_equal(d_status.cpu().numpy(), want)
    ok = datagrams(T, M, n_arrays, seed=9)
    run(nat, torch.from_numpy(ok).cuda(), T, n_arrays, hop, F, M, None, d_frames, d_status)
    clean = d_status.cpu().numpy()
    assert (clean[:, :3] == 0).all() and clean[:, 3].tolist() == [1000 + f * hop for f in range(F)]
    run(nat, torch.from_numpy(ok).cuda(), T, n_arrays + 1, hop, F, M, None, d_frames, d_status, ver=3)   # expectations that nothing meets
    assert (d_status.cpu().numpy()[:, :3] == [N, N, 0]).all()


# ------------------------------------------------------------------ 3. guard bands

@pytest.mark.parametrize("shape", [(256, 256, 4, 190, 256, 256), (256, 1024, 4, 7, 512, 256), (128, 100, 2, 7, 50, 130), (256, 516, 4, 2, 1, 257),
                                   (64, 256, 1, 190, 1, 64)], ids=lambda s: "%dx%d-a%d-F%d-hop%d-m%d" % s)
def test_stream_kernel_stays_inside_its_buffers(nat, shape):
    """d_frames and d_status each between two 4 KiB canary blocks inside one allocation, at the largest and the oddest shapes: the
    canaries are intact and the results equal a run on plain buffers."""
    torch = util.torch_gpu()
    M, N, n_arrays, F, hop, m_total = shape
    sizes(M, N)
    T = (F - 1) * hop + N
    pk = datagrams(T, M, n_arrays, seed=5)
    whole_pk = torch.full((pk.size // 4 + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")     # the stream too: what lies past it is never data
    d_pk = whole_pk[GUARD:GUARD + pk.size // 4].view(torch.uint8)
    d_pk.copy_(torch.from_numpy(pk.ravel()))
    d_mask = torch.from_numpy(mask_of(nat, "reference", m_total)).cuda()
    results = []
    for use_guards in (True, False):
        n_f, n_s = F * m_total * N, F * 4
        if use_guards:
            whole_f = torch.full((n_f + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")
            whole_s = torch.full((n_s + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")
            d_frames, d_status = whole_f[GUARD:GUARD + n_f].view(torch.float32), whole_s[GUARD:GUARD + n_s]
        else:
            d_frames = torch.zeros(n_f, dtype=torch.float32, device="cuda")
            d_status = torch.zeros(n_s, dtype=torch.int32, device="cuda")
        run(nat, d_pk, T, n_arrays, hop, F, m_total, d_mask, d_frames, d_status)
        if use_guards:
            for name, whole in (("frames", whole_f), ("status", whole_s), ("packets", whole_pk)):
                assert bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all()), name
        results.append((d_frames.clone(), d_status.clone()))
    assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32)) and torch.equal(results[0][1], results[1][1])
    assert int(torch.count_nonzero(results[0][0])) > 0


# ------------------------------------------------------------------ 4. equality with the one-frame entry point

@pytest.mark.parametrize("M,N,n_arrays,F", [(256, 256, 4, 7), (64, 256, 1, 7), (256, 1024, 4, 2), (128, 100, 2, 3)])
def test_equals_per_frame_ingest(nat, M, N, n_arrays, F):
    torch = util.torch_gpu()
    sizes(M, N)
    m_total = n_arrays * 64
    T = F * N
    pk = datagrams(T, M, n_arrays, seed=21)
    d_pk = torch.from_numpy(pk).cuda()
    batched = torch.full((F, m_total, N), float("nan"), dtype=torch.float32, device="cuda")
    run(nat, d_pk, T, n_arrays, N, F, m_total, None, batched, None)
    looped = torch.full((F, m_total, N), float("nan"), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for f in range(F):
        assert nat.lib.bf_ingest_device(d_pk[f * N:].data_ptr(), n_arrays, 8, 8, looped[f].data_ptr(), s) == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    _same(batched.cpu().numpy(), looped.cpu().numpy())


# ------------------------------------------------------------------ 5. datagrams -> frames -> maps -> loudest beam, all on the device

def _cfg2_lerp(nat):
    c = util.configure("cfg2")
    table = util.table_for("lerp", "cfg2")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    return c, table


def test_chain_packets_to_beams(nat, oracle_lib):
    torch = util.torch_gpu()
    import ingest
    import listen
    c, table = _cfg2_lerp(nat)
    M, N, X, Y, T_ = c["M"], c["N"], c["X"], c["Y"], c["T"]
    D, F, hop = X * Y, 3, N // 2
    mics = np.arange(M, dtype=np.int32)
    n_dgram = (F - 1) * hop + N + 50                                            # 50 datagrams that fill no frame
    pk = datagrams(n_dgram, M, 1, seed=33)
    pi = ingest.PacketIngest(1, hop=hop, dead_mics=[3, 40])
    assert pi.n_frames(n_dgram) == F
    d_frames, status = pi.frames(torch.from_numpy(pk).cuda())
    assert d_frames.shape == (F, M, N) and d_frames.dtype == torch.float32 and status.shape == (F, 4) and status.dtype == torch.int32
    flat, _ = pi.frames(torch.from_numpy(pk.ravel()).cuda())                    # the flat form of the same bytes
    img = torch.empty((F, D), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_device(util.ALGOS["lerp"], d_frames.data_ptr(), M, img.data_ptr(), D, F, nat.iptr(mics), M, 0, D,
                                 torch.cuda.current_stream().cuda_stream) == 0, nat.lib.bf_last_error()
    bl = listen.BeamListener("lerp", mics=mics)
    offs = bl.loudest(img)
    out, st = bl.listen(d_frames, offs)
    torch.cuda.synchronize()
    mask = np.zeros(M, dtype=np.uint8); mask[[3, 40]] = 1
    want = oracle_frames(oracle_lib, pk, M, N, 1, hop, F, M, mask)
    _same(d_frames.cpu().numpy(), want)
    _same(flat.cpu().numpy(), want)
    assert np.array_equal(status.cpu().numpy(), numpy_status(pk, N, 1, hop, F))
    orc = oracle_lib.Oracle(N, X, Y, T_)
    assert (st.cpu().numpy() == 0).all()
    for f in range(F):
        power = orc.mimo_lerp(want[f], table, mics).ravel()
        _same(img.cpu().numpy()[f], power)
        peak = int(np.argmax(power))
        assert int(offs.cpu().numpy()[f, 0]) == peak * M
        _same(out.cpu().numpy()[f, 0], orc.miso_lerp(want[f], table, mics, peak * M))


def test_fused_pipeline_step_packets(nat, oracle_lib):
    torch = util.torch_gpu()
    import ingest
    import visual
    from pipeline import FusedPipeline
    c = util.configure("cfg2")
    M, N, B = c["M"], c["N"], 4
    pipe = FusedPipeline("lerp", 640)
    pipe.load_tables(util.oracle_delays("cfg2"), np.arange(M))
    pk = datagrams(B * N, M, 1, seed=44)
    pk[N + 3, 3] = 9
    cam = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (B, 640, 640, 3), dtype=np.uint8)).cuda()
    pi = ingest.PacketIngest(1, dead_mics="reference")
    got = pipe.step_packets(torch.from_numpy(pk).cuda(), cam, pi)
    assert len(got) == 5
    mask = mask_of(nat, "reference", M)
    windows = oracle_frames(oracle_lib, pk, M, N, 1, N, B, M, mask)
    pipe.stream_state = visual.HeatmapStream(640, 640, "cuda")                  # the temporal blend starts over
    want = pipe.step(torch.from_numpy(windows).cuda(), cam)
    torch.cuda.synchronize()
    for g, w in zip(got[:4], want):
        assert g.shape == w.shape and torch.equal(g, w)
    assert got[0].cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()    # the maps, bit for bit
    assert np.array_equal(got[4].cpu().numpy(), numpy_status(pk, N, 1, N, B)) and got[4].cpu().numpy()[1, 0] == 1


# ------------------------------------------------------------------ 6. ingest + delay-and-sum as one captured graph

def test_graph_ingest_then_maps(nat, oracle_lib):
    torch = util.torch_gpu()
    c, table = _cfg2_lerp(nat)
    M, N, X, Y, T_ = c["M"], c["N"], c["X"], c["Y"], c["T"]
    D, F, hop = X * Y, 3, N // 2
    mics = np.arange(M, dtype=np.int32)
    n_dgram = (F - 1) * hop + N
    first, second = datagrams(n_dgram, M, 1, seed=51), datagrams(n_dgram, M, 1, seed=52, counter0=77)
    d_pk = torch.from_numpy(first).cuda()
    d_mask = torch.from_numpy(mask_of(nat, "single", M)).cuda()
    d_frames = torch.empty((F, M, N), dtype=torch.float32, device="cuda")
    d_status = torch.empty((F, 4), dtype=torch.int32, device="cuda")
    img = torch.empty((F, D), dtype=torch.float32, device="cuda")

    def step():                                         # a linear chain: one kernel after the other on one stream
        s = torch.cuda.current_stream().cuda_stream
        assert nat.lib.bf_ingest_stream_device(d_pk.data_ptr(), n_dgram, 1, 8, 8, hop, F, M, d_mask.data_ptr(), VER, d_frames.data_ptr(),
                                               d_status.data_ptr(), s) == 0
        assert nat.lib.bf_das_device(util.ALGOS["lerp"], d_frames.data_ptr(), M, img.data_ptr(), D, F, nat.iptr(mics), M, 0, D, s) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # eager warm-up: delay-and-sum builds its digest and uploads the adaptive array
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    d_pk.copy_(torch.from_numpy(second).cuda())
    g.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy().copy() for t in (d_frames, d_status, img)]
    step()                                              # eager on the same datagrams
    torch.cuda.synchronize()
    for a, b in zip(got, (d_frames, d_status, img)):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    want = oracle_frames(oracle_lib, second, M, N, 1, hop, F, M, mask_of(nat, "single", M))
    _same(got[0], want)
    assert got[1][:, 3].tolist() == [77 + f * hop for f in range(F)]
    orc = oracle_lib.Oracle(N, X, Y, T_)
    _same(got[2][F - 1], orc.mimo_lerp(want[F - 1], table, mics).ravel())
