"""GPU (-m gpu): bf_resample_device and audio_out.AudioOut, byte for byte against the NumPy restatement of the definition
(tests/resample_np.py: the taps in order, every step one single-rounding fmaf; Python ints for the state; np.rint for the PCM).

Data: floats whose magnitudes spread over 2^-12 .. 2^12 in taps and samples, so a chain summed in any other order, or a product
rounded before the add, shows in the bits.  Rows are in_stride = n + 3 floats apart with NaN between them, out_stride = cap + 5;
every output sits between canaries, which must survive, as must the floats of a row past cap."""
import numpy as np
import pytest

import resample_np as R
import util
from support import nat_restoring as nat

pytestmark = pytest.mark.gpu

CANARY = 64                 # elements in front of and behind every device output
CANARY_F = -1234.5
CANARY_I = 0x5A5A
N = 64


def _windows(rng, rows, n, hop, F, make=util.wild):
    """A stream cut into F windows of n every `hop` samples (0: back to back), and the window before the first."""
    step = hop if hop > 0 else n
    S = make(rng, (rows, step * F + n))
    frames = np.ascontiguousarray(np.stack([S[:, (f + 1) * step:(f + 1) * step + n] for f in range(F)]))
    return frames, np.ascontiguousarray(S[:, :n])


def _strided(x, stride):
    """[.., n] -> [.., stride] with NaN behind every row: a kernel that read past n would show it."""
    out = np.full(x.shape[:-1] + (stride,), np.nan, dtype=np.float32)
    out[..., :x.shape[-1]] = x
    return out


def _convert(nat, x, h, L, M, state=(0, 0), hop=0, prev=None, gain=1.0, off=0, want_out=True, want_pcm=True, clip0=None, with_clip=True, expect_rc=0):
    """bf_resample_device on device copies -> what the restatement returns, plus the meter `clip`.  The canaries are checked."""
    torch = util.torch_gpu()
    F, rows, n = x.shape
    T = h.shape[1]
    stride = n + 3
    S = F * (hop or n)
    cap = R.capacity(S, L, M)
    assert nat.lib.bf_resample_capacity(S, L, M) == cap
    out_stride = cap + 5
    d_x = util.place_words(_strided(x, stride), off)
    d_p = None if prev is None else util.place_words(_strided(prev, stride), off)
    d_h = util.place_words(h, off)
    d_state = util.place_words(np.array([state[0], state[1], 77, -5], dtype=np.int32), off)        # the reserved words are written 0
    d_count = util.place_words(np.array([-9, -9], dtype=np.int32), off)
    clip0 = np.zeros(rows, np.int32) if clip0 is None else np.asarray(clip0, dtype=np.int32)
    d_clip = util.place_words(clip0, off)
    fbuf = torch.full((CANARY + 4 + rows * out_stride + CANARY,), CANARY_F, dtype=torch.float32, device="cuda")
    ibuf = torch.full((CANARY + 4 + cap * rows + CANARY,), CANARY_I, dtype=torch.int16, device="cuda")
    f_lo, i_lo = CANARY + off, CANARY + 2 * off
    d_out, d_pcm = fbuf[f_lo:f_lo + rows * out_stride], ibuf[i_lo:i_lo + cap * rows]
    assert d_out.data_ptr() % 16 == 4 * off and d_pcm.data_ptr() % 16 == 4 * off
    rc = nat.lib.bf_resample_device(d_x.data_ptr(), rows, F, n, stride, hop, None if d_p is None else d_p.data_ptr(), d_h.data_ptr(), L, M, T, d_state.data_ptr(),
                                    gain, d_out.data_ptr() if want_out else None, out_stride if want_out else 0, d_pcm.data_ptr() if want_pcm else None,
                                    d_clip.data_ptr() if with_clip else None, d_count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fhost, ihost = fbuf.cpu().numpy(), ibuf.cpu().numpy()
    st, cnt, clip = d_state.cpu().numpy(), d_count.cpu().numpy(), d_clip.cpu().numpy()
    if expect_rc != 0:
        assert rc == expect_rc and nat.lib.bf_last_error()
        nat.lib.bf_clear_error()
        assert (fhost == np.float32(CANARY_F)).all() and (ihost == CANARY_I).all() and st.tolist() == [state[0], state[1], 77, -5]      # nothing was enqueued
        assert cnt.tolist() == [-9, -9] and np.array_equal(clip, clip0)
        return None
    assert rc == 0, nat.lib.bf_last_error()
    assert (fhost[:f_lo] == np.float32(CANARY_F)).all() and (fhost[f_lo + rows * out_stride:] == np.float32(CANARY_F)).all()
    assert (ihost[:i_lo] == CANARY_I).all() and (ihost[i_lo + cap * rows:] == CANARY_I).all()
    y = fhost[f_lo:f_lo + rows * out_stride].reshape(rows, out_stride)
    pcm = ihost[i_lo:i_lo + cap * rows].reshape(cap, rows)
    if want_out:
        assert (y[:, cap:] == np.float32(CANARY_F)).all()                # past cap a row is left untouched
    else:
        assert (y == np.float32(CANARY_F)).all()
    if not want_pcm:
        assert (pcm == CANARY_I).all()
    return dict(y=y[:, :cap].copy(), pcm=pcm.copy(), clip=clip, count=int(cnt[0]), status=int(cnt[1]), state=(int(st[0]), int(st[1])), words=st.tolist(), cap=cap)


def _check(got, want, clip0=None, nan_is_nan=False, want_out=True, want_pcm=True):
    assert (got["count"], got["status"], got["state"], got["cap"]) == (want["count"], want["status"], want["state"], want["cap"])
    if want["status"] == 0:
        assert got["words"][2:] == [0, 0]
    if want_out:
        assert util.bits_differ(got["y"], want["y"], nan_is_nan=nan_is_nan) == ""
    if want_pcm:
        assert got["pcm"].tobytes() == want["pcm"].tobytes(), np.argwhere(got["pcm"] != want["pcm"])[:8]
    base = np.zeros_like(got["clip"]) if clip0 is None else np.asarray(clip0)
    assert np.array_equal(got["clip"], base + (want["clipped"] if want_pcm else 0))


# ------------------------------------------------------------------ the definition: every ratio on every hop, rows and frames dealt round

RATIOS = [(1, 1, 1), (2, 3, 4), (3, 2, 5), (7, 5, 8), (5, 1, 3), (1, 4, 8), (160, 441, 16), (4000, 4069, 32)]
HOPS = [0, 16, 33, 64]
# (the call refuses a history longer than a window's share of the stream: 32 taps on a hop of 16)
CASES = [(L, M, T, hop, (1, 3, 5)[(i + j) % 3], (1, 3, 5)[(i + 2 * j) % 3]) for i, (L, M, T) in enumerate(RATIOS) for j, hop in enumerate(HOPS)
         if T - 1 <= (hop or N)]
# 70 rows; the steepest decimation, whose reach shortens a workgroup's run to 32 outputs (80 windows: three runs a row); 190 / 3
CASES += [(4000, 4069, 32, 64, 70, 5), (1, 64, 65, 0, 2, 80), (3, 190, 7, 33, 5, 5)]


def test_the_cases_cover_the_shapes():
    for L, M, T in RATIOS:
        mine = [c for c in CASES if c[:3] == (L, M, T)]
        assert {c[3] for c in mine} == {h for h in HOPS if T - 1 <= (h or N)}
        assert len({c[4] for c in mine}) >= 2 and len({c[5] for c in mine}) >= 2
    assert {c[4] for c in CASES} >= {1, 3, 5} and {c[5] for c in CASES} >= {1, 3, 5}


@pytest.mark.parametrize("L,M,T,hop,rows,frames", CASES)
def test_matches_the_definition(nat, L, M, T, hop, rows, frames):
    rng = np.random.default_rng([L, M, T, hop, rows, frames])
    x, prev = _windows(rng, rows, N, hop, frames)
    h = util.wild(rng, (L, T))
    state = (int(rng.integers(0, 3)), int(rng.integers(0, L)))
    if (L + hop) % 2:
        prev = None                                                      # silence before the stream
    gain = float(np.float32(2.0 ** -8 * 1.37))
    clip0 = rng.integers(0, 1000, size=rows).astype(np.int32)
    got = _convert(nat, x, h, L, M, state, hop, prev, gain, clip0=clip0)
    _check(got, R.resample(x, h, L, M, state, hop, prev, gain), clip0)


@pytest.mark.parametrize("L,M,T,hop", [(4000, 4069, 32, 33), (3, 2, 5, 16), (7, 5, 8, 0)])
def test_every_pointer_one_float_off(nat, L, M, T, hop):
    """... a 16-byte boundary: the table's rows are then read with dword loads although T % 4 == 0, and the bits are the same."""
    rng = np.random.default_rng([L, M, T, hop, 1])
    x, prev = _windows(rng, 3, N, hop, 3)
    h = util.wild(rng, (L, T))
    state = (1, L // 3)
    got = _convert(nat, x, h, L, M, state, hop, prev, 0.001, off=1)
    want = R.resample(x, h, L, M, state, hop, prev, 0.001)
    _check(got, want)
    aligned = _convert(nat, x, h, L, M, state, hop, prev, 0.001, off=0)
    assert aligned["y"].tobytes() == got["y"].tobytes() and aligned["pcm"].tobytes() == got["pcm"].tobytes()


def _subnormal(rng, shape):
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-12, 13, size=shape)) * 1e-41).astype(np.float32)


def _hostile(rng, shape):
    x = util.wild(rng, shape)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=max(8, flat.size // 16), replace=False)
    flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3e38, -3e38, 1e-45], dtype=np.float32), size=idx.size)
    return x


@pytest.mark.parametrize("kind", ["subnormal_samples", "subnormal_taps", "hostile"])
@pytest.mark.parametrize("L,M,T,hop", [(7, 5, 8, 16), (3, 2, 5, 33)])
def test_input_kinds(nat, kind, L, M, T, hop):
    rng = np.random.default_rng([L, M, T, hop, len(kind)])
    x, prev = _windows(rng, 3, N, hop, 3, make=_subnormal if kind == "subnormal_samples" else _hostile if kind == "hostile" else util.wild)
    h = _subnormal(rng, (L, T)) if kind == "subnormal_taps" else util.wild(rng, (L, T))
    gain = 1.0 if kind != "hostile" else 0.01
    if kind == "subnormal_taps":
        x, prev = (x / np.float32(4096.0)).astype(np.float32), (prev / np.float32(4096.0)).astype(np.float32)
    if kind == "subnormal_samples":
        h = (h / np.float32(4096.0)).astype(np.float32)                  # keep the sums subnormal
    got = _convert(nat, x, h, L, M, (0, 1), hop, prev, gain)
    want = R.resample(x, h, L, M, (0, 1), hop, prev, gain)
    if kind == "hostile":
        assert np.isnan(want["y"]).any() and np.isinf(want["y"]).any() and want["clipped"].sum() > 0
    else:
        tiny = np.abs(want["y"][:, :want["count"]])
        assert ((tiny > 0) & (tiny < np.float32(1.1754944e-38))).mean() > 0.5      # the results are subnormal, and kept
    _check(got, want, nan_is_nan=(kind == "hostile"))       # (a NaN's payload is the machine's; that it is a NaN, and its PCM, is the definition's)


# ------------------------------------------------------------------ split calls and the sparse stream on the device

@pytest.mark.parametrize("L,M,T,hop", [(2, 3, 4, 16), (3, 2, 5, 0), (7, 5, 8, 33), (4000, 4069, 32, 64)])
def test_split_calls_equal_one_call(nat, L, M, T, hop):
    rng = np.random.default_rng([L, M, T, hop, 2])
    F, F1, rows = 5, 2, 3
    x, prev = _windows(rng, rows, N, hop, F)
    h = util.wild(rng, (L, T))
    state = (1, L // 2)
    whole = _convert(nat, x, h, L, M, state, hop, prev, 0.01)
    a = _convert(nat, x[:F1], h, L, M, state, hop, prev, 0.01)
    b = _convert(nat, x[F1:], h, L, M, a["state"], hop, x[F1 - 1], 0.01, clip0=a["clip"])      # the carried state, window and meter
    _check(whole, R.resample(x, h, L, M, state, hop, prev, 0.01))
    assert a["count"] + b["count"] == whole["count"] and b["state"] == whole["state"] and np.array_equal(b["clip"], whole["clip"])
    assert np.concatenate([a["y"][:, :a["count"]], b["y"][:, :b["count"]]], axis=1).tobytes() == whole["y"][:, :whole["count"]].tobytes()
    assert np.concatenate([a["pcm"][:a["count"]], b["pcm"][:b["count"]]], axis=0).tobytes() == whole["pcm"][:whole["count"]].tobytes()


def test_sparse_outputs(nat):
    """down = 200: one output every 50 samples (up = 4; the call refuses down > 64 * up, so 200 / 1 is the restatement's alone, in
    tests/test_resample_host.py) from windows that add 16 samples each: calls that emit nothing still move the state."""
    rng = np.random.default_rng(200)
    h = util.wild(rng, (4, 8))
    state, prev, seen = (0, 0), None, []
    for call in range(4):
        x = util.wild(rng, (1, 2, N))
        got = _convert(nat, x, h, 4, 200, state, 16, prev, 1.0)
        _check(got, R.resample(x, h, 4, 200, state, 16, prev, 1.0))
        assert got["cap"] == 1
        seen.append((got["count"], got["state"][0]))
        state, prev = got["state"], x[0]
    assert seen == [(1, 34), (0, 18), (0, 2), (1, 36)]


@pytest.mark.parametrize("state", [(0, 3), (-1, 0), (5, -2), (-7, 9)])
def test_corrupt_state(nat, state):
    rng = np.random.default_rng(9)
    x, prev = _windows(rng, 3, N, 16, 3)
    h = util.wild(rng, (3, 5))
    clip0 = np.array([4, 0, 9], np.int32)
    got = _convert(nat, x, h, 3, 2, state, 16, prev, 1e6, clip0=clip0)       # a gain that would clip, were anything converted
    assert (got["count"], got["status"]) == (0, 1) and got["words"] == [state[0], state[1], 77, -5]
    assert not got["y"].any() and not got["pcm"].any() and np.array_equal(got["clip"], clip0)
    want = R.resample(x, h, 3, 2, state, 16, prev, 1e6)
    assert want["status"] == 1 and want["cap"] == got["cap"]


# ------------------------------------------------------------------ PCM

PCM_IN = np.array([0.0, 32768.0, -32768.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32767.5, 32766.5, 32767.0, -32768.5, -32769.0, 0.49999, 16384.0], dtype=np.float32) / np.float32(32768.0)
PCM_OUT = [0, 32767, -32768, 0, 2, 2, 0, -2, -2, 32767, 32766, 32767, -32768, -32768, 0, 16384]
PCM_CLIPPED = [0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0]


def test_pcm_rounding_clipping_and_the_meter(nat):
    one = np.ones((1, 1), np.float32)
    x = np.zeros((1, 2, N), np.float32)
    x[0, 0, :16] = PCM_IN
    x[0, 1, :4] = [np.nan, np.inf, -np.inf, 1.0]
    assert PCM_IN[1] == 1.0 and PCM_IN[2] == -1.0 and float(PCM_IN[9]) * 32768 == 32767.5       # the ties are exact in float32
    got = _convert(nat, x, one, 1, 1)
    assert got["pcm"][:16, 0].tolist() == PCM_OUT and got["pcm"][:4, 1].tolist() == [0, 32767, -32768, 32767]
    assert got["clip"].tolist() == [sum(PCM_CLIPPED), 4]
    want = R.resample(x, one, 1, 1)
    _check(got, want, nan_is_nan=True)
    again = _convert(nat, x, one, 1, 1, clip0=got["clip"])             # the meter adds up over calls
    assert again["clip"].tolist() == [2 * sum(PCM_CLIPPED), 8]
    half = _convert(nat, x, one, 1, 1, gain=0.5)                         # the gain comes before the conversion: 1.0 no longer clips
    _check(half, R.resample(x, one, 1, 1, gain=0.5), nan_is_nan=True)
    assert half["pcm"][1, 0] == 16384 and half["clip"].tolist() == [0, 3]


def test_either_output_alone(nat):
    rng = np.random.default_rng(12)
    x, prev = _windows(rng, 3, N, 33, 3)
    h = util.wild(rng, (7, 8))
    want = R.resample(x, h, 7, 5, (2, 3), 33, prev, 0.01)
    assert want["clipped"].sum() > 0
    _check(_convert(nat, x, h, 7, 5, (2, 3), 33, prev, 0.01, want_pcm=False), want, want_pcm=False)      # the meter counts PCM samples: untouched
    _check(_convert(nat, x, h, 7, 5, (2, 3), 33, prev, 0.01, want_out=False), want, want_out=False)
    got = _convert(nat, x, h, 7, 5, (2, 3), 33, prev, 0.01, with_clip=False, clip0=[5, 6, 7])             # no meter
    assert got["clip"].tolist() == [5, 6, 7]
    assert got["pcm"].tobytes() == want["pcm"].tobytes() and util.bits_differ(got["y"], want["y"]) == ""
    assert _convert(nat, x, h, 7, 5, (2, 3), 33, prev, 0.01, want_out=False, want_pcm=False, expect_rc=-1) is None
    assert _convert(nat, x, h, 7, 5, (2, 3), 65, prev, 0.01, expect_rc=-1) is None
    assert _convert(nat, x, h, 7, 5, (2, 3), 33, prev, float("inf"), expect_rc=-1) is None


# ------------------------------------------------------------------ audio_out.AudioOut: a captured push, and the chain end to end


def test_graph_replay_advances_the_state(nat):
    torch = util.torch_gpu()
    import audio_out
    util.configure_small(N)
    rng = np.random.default_rng(48)
    hop, F, B = 33, 2, 3
    step = hop * F
    S = (rng.standard_normal((B, step * 4 + N)) * 0.3).astype(np.float32)
    S[0, 68:76] = 1.5                                                    # a plateau that clips
    batches = [np.ascontiguousarray(np.stack([S[:, c * step + (f + 1) * hop:c * step + (f + 1) * hop + N] for f in range(F)])) for c in range(4)]
    audio_out.AudioOut(48000, rows=B, hop=hop).push(torch.from_numpy(batches[0]).cuda())       # (another object: a first launch loads the kernels)
    torch.cuda.synchronize()
    ao = audio_out.AudioOut(48000, rows=B, hop=hop)
    assert (ao.up, ao.down, ao.T) == (4000, 4069, 32) and ao.delay == (4000 * 32 - 1) / 8000.0
    x = torch.from_numpy(batches[0]).cuda()
    carried = ao._prev.data_ptr()
    got = []
    audio, pcm, count = ao.push(x)                                       # call 1, eager
    torch.cuda.synchronize()
    got.append((audio.cpu().numpy(), pcm.cpu().numpy(), count.cpu().numpy().copy(), ao.last_count))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        audio, pcm, count = ao.push(x)                                   # captured, not run
    assert ao._prev.data_ptr() == carried
    for c in (1, 2, 3):                                                  # calls 2 .. 4: the input overwritten, the graph replayed
        x.copy_(torch.from_numpy(batches[c]).cuda())
        g.replay()
        torch.cuda.synchronize()
        got.append((audio.cpu().numpy(), pcm.cpu().numpy(), count.cpu().numpy().copy(), None))
    state, prev, clipped = (0, 0), None, np.zeros(B, np.int64)
    for c in range(4):
        want = R.resample(batches[c], ao.taps, ao.up, ao.down, state, hop, prev, 1.0)
        y, q, cnt, mirror = got[c]
        assert cnt.tolist() == [want["count"], 0] and y.shape == (B, want["cap"]) and q.shape == (want["cap"], B)
        assert mirror is None or mirror == want["count"]
        assert util.bits_differ(y, want["y"]) == "" and q.tobytes() == want["pcm"].tobytes()
        state, prev, clipped = want["state"], batches[c][-1], clipped + want["clipped"]
    assert ao.state.cpu().numpy().tolist() == [state[0], state[1], 0, 0]
    assert np.array_equal(ao.clip.cpu().numpy(), clipped) and clipped.sum() >= 1
    assert np.array_equal(util.bits(ao._prev.cpu().numpy()), util.bits(batches[3][-1]))
    ao.reset()
    assert not ao.state.cpu().numpy().any() and not ao.clip.cpu().numpy().any() and not ao._prev.cpu().numpy().any() and ao._prev.data_ptr() == carried
    audio, pcm, count = ao.push(x)                                       # a new stream: silence before it
    want = R.resample(batches[3], ao.taps, ao.up, ao.down, (0, 0), hop, None, 1.0)
    assert util.bits_differ(audio.cpu().numpy(), want["y"]) == "" and ao.last_count == want["count"]


def test_push_flat_and_float_only(nat):
    torch = util.torch_gpu()
    import audio_out
    rng = np.random.default_rng(44)
    ao = audio_out.AudioOut(44100, taps=16, pcm=False, gain=0.5)
    assert (ao.up, ao.down) == (3675, 4069)
    state, prev = (0, 0), None
    for c in range(3):
        x = (rng.standard_normal((2, 200)) * 0.3).astype(np.float32)
        audio, pcm, count = ao.push_flat(torch.from_numpy(x).cuda())
        want = R.resample(x[None], ao.taps, ao.up, ao.down, state, 0, prev, 0.5)
        assert pcm is None and count.cpu().numpy().tolist() == [want["count"], 0] and ao.last_count == want["count"]
        assert util.bits_differ(audio.cpu().numpy(), want["y"]) == ""
        state, prev = want["state"], x
    assert not ao.clip.cpu().numpy().any()
    with pytest.raises(ValueError):
        ao.push_flat(torch.zeros((2, 100), device="cuda"))              # a stream keeps its layout
    with pytest.raises(ValueError):
        audio_out.AudioOut(48000, hop=16).push(torch.zeros((1, 2, 64), device="cuda"))      # 31 samples of history, 16 per window


def test_stream_beams_to_a_sound_card(nat):
    """StreamBeamformer.listen -> AudioOut.push on a 1 kHz plane wave, two batches: the converted beams are the restatement applied to
    the joined beams sb.audio(out), byte for byte."""
    torch = util.torch_gpu()
    import audio_out
    import stream
    c = util.configure("cfg1")
    Mics, n, D = c["M"], c["N"], c["X"] * c["Y"]
    table = util.table_for("lerp", "cfg1")
    nat.lib.load_coefficients_lerp(nat.fptr(table), table.size); nat.check()
    delays = util.oracle_delays("cfg1").reshape(D, Mics)
    hop, F = n // 2, 4
    src = D // 2
    t = np.arange(hop * F + n, dtype=np.float64)[None, :] + delays[src][:, None]          # microphone m leads by its delay
    S = (0.5 * np.sin(2 * np.pi * 1000.0 * t / 48828.0)).astype(np.float32)
    frames = np.ascontiguousarray(np.stack([S[:, f * hop:f * hop + n] for f in range(F)]))
    offsets = np.array([src * Mics, 0, (D - 1) * Mics], dtype=np.int32)
    sb = stream.StreamBeamformer("lerp", hop=hop, mics=np.arange(Mics, dtype=np.int32))
    ao = audio_out.AudioOut(48000, hop=hop, gain=1.0 / Mics)
    d_frames = torch.from_numpy(frames).cuda()
    state, prev = (0, 0), None
    for f0, f1 in ((0, 1), (1, F)):
        out, st = sb.listen(d_frames[f0:f1], offsets)
        audio, pcm, count = ao.push(out)
        sb.advance(d_frames[f0:f1])
        joined = sb.audio(out).cpu().numpy()                              # [B, (f1 - f0) * hop]
        want = R.resample(joined[None], ao.taps, ao.up, ao.down, state, 0, prev, ao.gain)
        assert (st.cpu().numpy() == 0).all() and count.cpu().numpy().tolist() == [want["count"], 0] and ao.last_count == want["count"]
        assert util.bits_differ(audio.cpu().numpy(), want["y"]) == "" and pcm.cpu().numpy().tobytes() == want["pcm"].tobytes()
        state = want["state"]
        prev = joined if joined.shape[1] >= ao.T - 1 else None
        assert prev is not None
    assert not ao.clip.cpu().numpy().any()
    k = ao.last_count
    assert np.abs(audio.cpu().numpy()[0, :k]).max() > 0.3 and np.abs(pcm.cpu().numpy()[:k, 0]).max() > 10000      # the steered beam is the loud one
