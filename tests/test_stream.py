"""GPU (-m gpu): the continuous-stream mode of the device path -- bf_miso_stream_device, bf_das_stream_device, StreamBeamformer --
bit for bit against the committed C checker run on an EXTENDED window.

The oracle.  The tests keep their own continuous stream array S [M_total, L]; frame f of a call is S[:, s_f : s_f + N] with
s_f = s_0 + f * hop.  For frame f the checker gets ext = S[:, s_f - P : s_f + N] (P >= H history samples in front of the window;
zeros where the stream has not begun) and runs as Oracle(N + P, ..).miso_pad / miso_lerp; the result's [P:] is the expectation.
For t' >= P >= H every microphone contributes, in the same microphone order and with the reference's own roundings, which is the
definition in include/beamformer_hip.h.  Maps: float32(sum_t (o / n)^2 in t order) / N with `o` from the same oracle, summed by
np.add.accumulate in float32.  Every comparison is on the raw bits.

Also here, because they need a table loaded on a device: the `H > hop` refusal and the refusal of a table whose entries the
loader had to clamp to N_SAMPLES."""
import ctypes as C

import numpy as np
import pytest

import util
from support import nat
from test_miso_device import MIC_GAIN, SENTINEL, Tables

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the stream, its windows and the extended-window oracle

class Stream:
    """A seeded stream S [M_total, L] (rows in `dead` zeroed, as the ingest's row mask leaves them) cut into windows of N every `hop`
    samples from `start` on; `start` >= hop keeps a previous frame in front of the first window (with_prev), start = 0 does not."""

    def __init__(self, seed, M_total, N, hop, F, with_prev, dead=()):
        self.N, self.hop, self.F = N, hop, F
        self.start = hop if with_prev else 0
        L = self.start + (F - 1) * hop + N
        rng = np.random.default_rng(seed)
        self.S = (rng.standard_normal((M_total, L)) * 0.25).astype(np.float32)
        self.S[list(dead)] = 0.0
        self.P = hop                                      # history the oracle sees: H <= hop
        self.Sz = np.concatenate([np.zeros((M_total, self.P), np.float32), self.S], axis=1)

    def frames(self, f0=0, f1=None):
        f1 = self.F if f1 is None else f1
        return np.ascontiguousarray(np.stack([self.S[:, self.start + f * self.hop:self.start + f * self.hop + self.N] for f in range(f0, f1)]))

    def prev(self):
        """The frame that started `hop` samples before frame 0 (None: the stream begins with frame 0)."""
        return np.ascontiguousarray(self.S[:, :self.N]) if self.start else None

    def ext(self, f):
        s = self.start + f * self.hop                     # Sz is S behind P zeros: S[s - P : s + N]
        return np.ascontiguousarray(self.Sz[:, s:s + self.P + self.N])


class Case:
    """Sizes + table of one configuration, loaded into the product; `want(stream, f, offset)` is the extended-window oracle."""

    def __init__(self, nat, oracle_lib, algo, name=None, sizes=None, delays=None, mics=None):
        from interface import config
        if name is not None:
            c = util.configure(name)
            self.M_total, self.N, self.D, T = c["M"], c["N"], c["X"] * c["Y"], c["T"]
            delays = util.oracle_delays(name).reshape(self.D, self.M_total)
        else:
            self.M_total, self.N, self.D, T = sizes
            config.configure(N_MICROPHONES=self.M_total, N_SAMPLES=self.N, MAX_RES_X=self.D, MAX_RES_Y=1, N_TAPS=T)
        self.mics = np.arange(self.M_total, dtype=np.int32) if mics is None else np.ascontiguousarray(mics, dtype=np.int32)
        if mics is not None and name is not None:
            delays = delays[:, self.mics]                 # the table of a microphone subset: [D, n]
        self.n, self.T, self.algo, self.nat, self.oracle_lib = self.mics.size, T, algo, nat, oracle_lib
        self.tab = Tables(nat, None, algo, delays, np.zeros(1, np.float32), self.n, T)
        self.max_whole = int(self.tab.whole.max())
        self.H = self.max_whole + (1 if algo == "lerp" else 0)
        self._orc = {}

    def offset(self, d):
        return self.tab.offset(d)

    def want(self, st, f, off):
        P = st.P
        assert P >= self.H
        if P not in self._orc:
            self._orc[P] = self.oracle_lib.Oracle(self.N + P, self.D, 1, self.T)
        self.tab.orc = self._orc[P]
        out = self.tab.want(st.ext(f), self.mics, int(off))
        assert out.shape == (self.N + P,) and np.isfinite(out).all()
        return out[P:]

    def want_power(self, st, f, d):
        o = self.want(st, f, self.offset(d))
        q = o / np.float32(self.n)
        sq = q * q
        assert sq.dtype == np.float32
        return np.add.accumulate(sq, dtype=np.float32)[-1] / np.float32(self.N)


def _dev(a):
    torch = util.torch_gpu()
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _beams(nat, case, frames, hop, prev, offsets, gain=0.0, status=True, expect_rc=0):
    """bf_miso_stream_device -> (out [F, B, N] host array, the 16-float tail behind it, status host array or None)."""
    torch = util.torch_gpu()
    F, M, N = frames.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    B = offsets.shape[1]
    d_sig, d_prev, d_off = _dev(frames), _dev(prev), _dev(offsets)
    out = torch.full((F * B * N + SENTINEL,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((F, B), -7, dtype=torch.int32, device="cuda") if status else None
    rc = nat.lib.bf_miso_stream_device(util.ALGOS[case.algo], d_sig.data_ptr(), M, F, hop, _ptr(d_prev), nat.iptr(case.mics), case.n, d_off.data_ptr(), B,
                                       float(gain), out.data_ptr(), N, _ptr(st), torch.cuda.current_stream().cuda_stream)
    if expect_rc != 0:
        assert rc == expect_rc
        return None, None, None
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    return host[:F * B * N].reshape(F, B, N), host[F * B * N:], None if st is None else st.cpu().numpy()


def _maps(nat, case, frames, hop, prev, d0, d1, pad=3):
    """bf_das_stream_device on directions [d0, d1) with image_stride = d1 - d0 + pad -> (maps [F, d1 - d0], the untouched rest)."""
    torch = util.torch_gpu()
    F, M, N = frames.shape
    stride = d1 - d0 + pad
    d_sig, d_prev = _dev(frames), _dev(prev)
    img = torch.full((F, stride), float("nan"), dtype=torch.float32, device="cuda")
    rc = nat.lib.bf_das_stream_device(util.ALGOS[case.algo], d_sig.data_ptr(), M, img.data_ptr(), stride, F, hop, _ptr(d_prev), nat.iptr(case.mics), case.n,
                                      d0, d1, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert nat.lib.bf_last_das_variant() == 9
    host = img.cpu().numpy()
    return host[:, :d1 - d0], host[:, d1 - d0:]


def _dead_rows(nat):
    n = nat.lib.bf_default_disabled_mics(None)
    out = np.zeros(n, dtype=np.int32)
    nat.lib.bf_default_disabled_mics(nat.iptr(out))
    return out.tolist()


def _hop(kind, N, H):
    return {"N": N, "half": N // 2, "H": max(H, 1)}[kind]


def _check_history(nat, case):
    """bf_stream_history against the resident table (bf_get_pad_table / bf_get_lerp_tables)."""
    n = case.tab.whole.size
    whole = np.full(n, -1, dtype=np.int32)
    if case.algo == "pad":
        assert nat.lib.bf_get_pad_table(nat.iptr(whole), n) == 0
    else:
        h = np.zeros(n, dtype=np.float32)
        assert nat.lib.bf_get_lerp_tables(nat.iptr(whole), nat.fptr(h), n) == 0
    assert int(whole.max()) == case.max_whole
    assert nat.lib.bf_stream_history(util.ALGOS[case.algo]) == case.H
    assert nat.lib.bf_stream_history(util.ALGOS["hybrid"]) == -1


# ------------------------------------------------------------------ 1. beams equal the oracle

@pytest.mark.parametrize("hop_kind", ["N", "half", "H"])
@pytest.mark.parametrize("algo", ["pad", "lerp"])
@pytest.mark.parametrize("name", ["cfg1", "shipped"])
def test_beams_match_extended_window_oracle(nat, oracle_lib, name, algo, hop_kind):
    """cfg1-sized (one staging chunk) and shipped-sized (several chunks, 256 microphones with get_data's dead rows zeroed, delays up to
    47); 6 frames; hop N, N / 2 and H.  The shipped cases ask for 19 beams (groups of 16 and 3) and, for hop N / 2, mic_gain 128; the
    stream begins with frame 0 (d_prev NULL) for hop N and has a previous frame otherwise."""
    case = Case(nat, oracle_lib, algo, name=name)
    _check_history(nat, case)
    N, D, F = case.N, case.D, 6
    hop = _hop(hop_kind, N, case.H)
    shipped = name == "shipped"
    st = Stream([11, N, hop, len(algo)], case.M_total, N, hop, F, with_prev=hop_kind != "N", dead=_dead_rows(nat) if shipped else ())
    B = 19 if shipped else 5
    rng = np.random.default_rng([5, hop, B])
    dirs = rng.integers(0, D, (F, B))
    dirs[:, 0], dirs[:, 1] = 0, D - 1
    dirs[:, 2] = int(np.argmax(case.tab.whole.reshape(D, case.n).max(axis=1)))       # the direction that holds the largest delay
    offs = case.offset(dirs)
    gain = MIC_GAIN if (shipped and hop_kind == "half") else 0.0
    got, tail, status = _beams(nat, case, st.frames(), hop, st.prev(), offs, gain=gain)
    assert (status == 0).all() and np.isnan(tail).all()
    for f in range(F):
        for b in range(B):
            want = case.want(st, f, offs[f, b])
            if gain:
                want = (want / np.float32(case.n)) * np.float32(gain)
                assert want.dtype == np.float32
            util.same_bits(got[f, b], want)


@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_long_windows(nat, oracle_lib, algo):
    """N = 1024 (NC 16), 256 microphones, random delays up to 100: the rows are staged in many chunks, the history refilled with each."""
    M, N, D, T = 256, 1024, 5, 8
    rng = np.random.default_rng(1024)
    case = Case(nat, oracle_lib, algo, sizes=(M, N, D, T), delays=rng.uniform(0, 100, (D, M)))
    _check_history(nat, case)
    F, hop = 6, N // 2
    st = Stream([3, N, len(algo)], M, N, hop, F, with_prev=True)
    dirs = np.array([[0, 4, f % D, (f + 2) % D] for f in range(F)])
    offs = case.offset(dirs)
    got, tail, status = _beams(nat, case, st.frames(), hop, st.prev(), offs)
    assert (status == 0).all() and np.isnan(tail).all()
    for f in range(F):
        for b in range(dirs.shape[1]):
            util.same_bits(got[f, b], case.want(st, f, offs[f, b]))


# ------------------------------------------------------------------ 2. maps equal the k-ordered power of the oracle's beams

@pytest.mark.parametrize("with_prev", [False, True], ids=["from_silence", "with_prev"])
@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_maps_cfg1_grid(nat, oracle_lib, algo, with_prev):
    case = Case(nat, oracle_lib, algo, name="cfg1")
    N, D, F, hop = case.N, case.D, 4, case.N // 2
    st = Stream([21, len(algo), int(with_prev)], case.M_total, N, hop, F, with_prev=with_prev)
    got, rest = _maps(nat, case, st.frames(), hop, st.prev(), 0, D)
    assert np.isnan(rest).all()
    want = np.array([[case.want_power(st, f, d) for d in range(D)] for f in range(F)], dtype=np.float32)
    assert np.isfinite(want).all() and (want > 0).all()
    util.same_bits(got, want)


@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_maps_direction_shard_chunked(nat, oracle_lib, algo):
    """The shipped size stages its 256 rows in several chunks (four directions per wave carried across them); a shard of the grid,
    written at the shard's origin."""
    case = Case(nat, oracle_lib, algo, name="shipped")
    N, F, hop = case.N, 4, case.N // 2
    d0, d1 = 1000, 1100
    st = Stream([22, len(algo)], case.M_total, N, hop, F, with_prev=True, dead=_dead_rows(nat))
    got, rest = _maps(nat, case, st.frames(), hop, st.prev(), d0, d1)
    assert np.isnan(rest).all()
    want = np.array([[case.want_power(st, f, d) for d in range(d0, d1)] for f in range(F)], dtype=np.float32)
    util.same_bits(got, want)


@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_maps_n_not_a_power_of_two(nat, oracle_lib, algo):
    """48 of cfg1's 64 rows, permuted: out / n is a true division."""
    mics = np.random.default_rng(48).permutation(64)[:48]
    case = Case(nat, oracle_lib, algo, name="cfg1", mics=mics)
    assert case.n == 48
    N, D, F, hop = case.N, case.D, 4, case.N
    st = Stream([23, len(algo)], case.M_total, N, hop, F, with_prev=True)
    got, _ = _maps(nat, case, st.frames(), hop, st.prev(), 0, D)
    want = np.array([[case.want_power(st, f, d) for d in range(D)] for f in range(F)], dtype=np.float32)
    util.same_bits(got, want)
    # and a shard of it
    got, _ = _maps(nat, case, st.frames(), hop, st.prev(), 17, 60)
    util.same_bits(got, want[:, 17:60])


# ------------------------------------------------------------------ 3. batch-split invariance (StreamBeamformer)

@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_batch_split_invariance(nat, oracle_lib, algo):
    torch = util.torch_gpu()
    import stream
    case = Case(nat, oracle_lib, algo, name="cfg1")
    N, D, F, hop = case.N, case.D, 7, case.N // 2
    st = Stream([31, len(algo)], case.M_total, N, hop, F, with_prev=False)
    d_frames = _dev(st.frames())
    offs = [case.offset(d) for d in (0, D - 1, D // 2)]

    def run(splits):
        sb = stream.StreamBeamformer(algo, hop=hop, mics=case.mics)
        assert sb.history == case.H
        beams, maps, f0 = [], [], 0
        for k in splits:
            batch = d_frames[f0:f0 + k]
            state = None if sb._prev is None else sb._prev.clone()
            out, status = sb.listen(batch, offs)
            img = sb.maps(batch)
            assert (status.cpu().numpy() == 0).all()
            assert (state is None and sb._prev is None) or torch.equal(state, sb._prev)      # listen / maps leave the carried state alone
            sb.advance(batch)
            assert torch.equal(sb._prev, batch[-1])
            beams.append(out.cpu().numpy()); maps.append(img.cpu().numpy())
            f0 += k
        assert f0 == F
        return np.concatenate(beams), np.concatenate(maps)

    whole_b, whole_m = run([F])
    assert whole_b.shape == (F, 3, N) and whole_m.shape == (F, D)
    for splits in ([1] * F, [3, 1, 2, 1], [1, 4, 2]):
        b, m = run(splits)
        util.same_bits(b, whole_b)
        util.same_bits(m, whole_m)
    # the split results are the oracle's, not merely each other's
    util.same_bits(whole_b[4, 1], case.want(st, 4, offs[1]))
    util.same_bits(whole_m[5, 7], np.float32(case.want_power(st, 5, 7)))
    # reset(): the next batch starts from silence again
    sb = stream.StreamBeamformer(algo, hop=hop, mics=case.mics)
    sb.advance(d_frames[:2])
    sb.reset()
    out, _ = sb.listen(d_frames[:1], offs)
    util.same_bits(out.cpu().numpy()[0], whole_b[0])


# ------------------------------------------------------------------ 4. anchor to the pinned path

@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_anchor_to_bf_miso_device(nat, oracle_lib, algo):
    """From sample H on, a stream beam IS bf_miso_device's beam of the same window; for pad from silence, frame 0 is it entirely."""
    torch = util.torch_gpu()
    case = Case(nat, oracle_lib, algo, name="shipped")
    N, D, F, hop, H = case.N, case.D, 6, case.N // 2, case.H
    assert 0 < H < hop
    st = Stream([41, len(algo)], case.M_total, N, hop, F, with_prev=False)
    frames = st.frames()
    dirs = np.array([[0, D - 1, (37 * f) % D, (D // 2 + f) % D] for f in range(F)])
    offs = np.ascontiguousarray(case.offset(dirs), dtype=np.int32)
    got, _, _ = _beams(nat, case, frames, hop, None, offs)
    d_sig, d_off = _dev(frames), _dev(offs)
    plain = torch.full((F, 4, N), float("nan"), dtype=torch.float32, device="cuda")
    before = nat.lib.bf_last_das_variant()
    rc = nat.lib.bf_miso_device(util.ALGOS[algo], d_sig.data_ptr(), case.M_total, F, nat.iptr(case.mics), case.n, d_off.data_ptr(), 4, 0.0, plain.data_ptr(),
                                N, None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, nat.lib.bf_last_error()
    torch.cuda.synchronize()
    assert nat.lib.bf_last_das_variant() == before
    plain = plain.cpu().numpy()
    util.same_bits(got[:, :, H:], plain[:, :, H:])
    assert not np.array_equal(util.bits(got[1:, :, :H]), util.bits(plain[1:, :, :H]))       # the head of a later window differs: that is the feature
    if algo == "pad":
        util.same_bits(got[0], plain[0])


def test_beam_call_leaves_last_variant_alone(nat, oracle_lib):
    case = Case(nat, oracle_lib, "pad", name="cfg1")
    st = Stream([42], case.M_total, case.N, case.N, 2, with_prev=False)
    _maps(nat, case, st.frames(), case.N, None, 0, 5)
    assert nat.lib.bf_last_das_variant() == 9
    torch = util.torch_gpu()
    d_sig = _dev(st.frames())
    img = torch.empty((2, case.D), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_device(util.ALGOS["pad"], d_sig.data_ptr(), case.M_total, img.data_ptr(), case.D, 2, nat.iptr(case.mics), case.n, 0, case.D,
                                 torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    other = nat.lib.bf_last_das_variant()
    assert other != 9
    _beams(nat, case, st.frames(), case.N, None, np.zeros((2, 1), dtype=np.int32))
    assert nat.lib.bf_last_das_variant() == other


# ------------------------------------------------------------------ 5. rejected offsets, refusals that need a loaded table

@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_invalid_offsets_are_nan_with_status(nat, oracle_lib, algo):
    case = Case(nat, oracle_lib, algo, name="cfg1")
    N, D, F, hop = case.N, case.D, 2, case.N // 2
    st = Stream([51, len(algo)], case.M_total, N, hop, F, with_prev=True)
    last = case.offset(D - 1)
    row = [case.offset(0), -1, last + 1, last, 2 ** 31 - 1]
    want_status = [0, 1, 1, 0, 1]
    offs = np.array([row] * F, dtype=np.int64)
    got, tail, status = _beams(nat, case, st.frames(), hop, st.prev(), offs)
    assert (status == np.array([want_status] * F)).all(), status
    assert np.isnan(tail).all()
    for f in range(F):
        for b, s in enumerate(want_status):
            if s:
                assert np.isnan(got[f, b]).all()
            else:
                util.same_bits(got[f, b], case.want(st, f, offs[f, b]))
    # without a status array the beams are the same
    again, _, none = _beams(nat, case, st.frames(), hop, st.prev(), offs, status=False)
    assert none is None
    util.same_bits(again, got)


@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_history_longer_than_hop_is_refused(nat, oracle_lib, algo):
    torch = util.torch_gpu()
    case = Case(nat, oracle_lib, algo, name="shipped")
    H = case.H
    assert H > 1
    st = Stream([52], case.M_total, case.N, case.N, 1, with_prev=False)
    nat.lib.bf_clear_error()
    _beams(nat, case, st.frames(), H - 1, None, np.zeros((1, 1), dtype=np.int32), expect_rc=-1)
    with pytest.raises(nat.BeamformerError, match=r"bf_miso_stream_device: the loaded table needs H = %d samples of history but hop = %d" % (H, H - 1)):
        nat.check()
    d_sig = _dev(st.frames())
    img = torch.empty((1, case.D), dtype=torch.float32, device="cuda")
    rc = nat.lib.bf_das_stream_device(util.ALGOS[algo], d_sig.data_ptr(), case.M_total, img.data_ptr(), case.D, 1, H - 1, None, nat.iptr(case.mics), case.n,
                                      0, case.D, torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    with pytest.raises(nat.BeamformerError, match=r"bf_das_stream_device: the loaded table needs H = %d samples of history but hop = %d" % (H, H - 1)):
        nat.check()


def test_clamped_and_unloaded_tables_are_refused(nat, oracle_lib):
    from interface import config
    M, N, D = 8, 64, 3
    config.configure(N_MICROPHONES=M, N_SAMPLES=N, MAX_RES_X=D, MAX_RES_Y=1, N_TAPS=8)
    whole = np.full(D * M, 5, dtype=np.int32)
    whole[7] = N + 9                                        # the loader clamps it to N: the stream cannot reach that far back
    nat.lib.load_coefficients_pad(nat.iptr(whole), whole.size); nat.check()
    assert nat.lib.bf_stream_history(util.ALGOS["pad"]) == N
    mics = np.arange(M, dtype=np.int32)
    x = _dev(np.zeros((1, M, N), dtype=np.float32))
    offs = _dev(np.zeros((1, 1), dtype=np.int32))
    out = _dev(np.zeros((1, 1, N), dtype=np.float32))
    s = util.torch_gpu().cuda.current_stream().cuda_stream
    rc = nat.lib.bf_miso_stream_device(util.ALGOS["pad"], x.data_ptr(), M, 1, N, None, nat.iptr(mics), M, offs.data_ptr(), 1, 0.0, out.data_ptr(), N, None, s)
    assert rc == -1
    with pytest.raises(nat.BeamformerError, match="1 entries of the loaded table lie beyond N_SAMPLES = 64"):
        nat.check()
    nat.lib.unload_coefficients_pad()
    assert nat.lib.bf_stream_history(util.ALGOS["pad"]) == -1
    rc = nat.lib.bf_miso_stream_device(util.ALGOS["pad"], x.data_ptr(), M, 1, N, None, nat.iptr(mics), M, offs.data_ptr(), 1, 0.0, out.data_ptr(), N, None, s)
    assert rc == -1
    with pytest.raises(nat.BeamformerError, match="bf_miso_stream_device: load_coefficients_pad has not been called"):
        nat.check()


# ------------------------------------------------------------------ 6. audio(): two consecutive batches are the beam of the stream

@pytest.mark.parametrize("hop_kind", ["N", "half"])
@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_audio_of_two_batches_is_the_beam_of_the_stream(nat, oracle_lib, algo, hop_kind):
    import stream
    case = Case(nat, oracle_lib, algo, name="cfg1")
    N, D, F = case.N, case.D, 7
    hop = _hop(hop_kind, N, case.H)
    st = Stream([61, len(algo), hop], case.M_total, N, hop, F, with_prev=False)
    d_frames = _dev(st.frames())
    dirs = [0, D - 1, int(np.argmax(case.tab.whole.reshape(D, case.n).max(axis=1)))]
    offs = [case.offset(d) for d in dirs]
    sb = stream.StreamBeamformer(algo, hop=hop, mics=case.mics)
    parts = []
    for f0, f1 in ((0, 4), (4, F)):
        out, _ = sb.listen(d_frames[f0:f1], offs)
        parts.append(sb.audio(out).cpu().numpy())
        sb.advance(d_frames[f0:f1])
    audio = np.concatenate(parts, axis=1)
    L = st.S.shape[1]
    assert L == (F - 1) * hop + N and audio.shape == (3, F * hop) and F * hop == L - (N - hop)
    # the whole stream as ONE extended window: P zeros of silence, then all L samples
    P = 64
    assert P >= case.H
    orc = oracle_lib.Oracle(L + P, D, 1, case.T)
    ext = np.ascontiguousarray(np.concatenate([np.zeros((case.M_total, P), np.float32), st.S], axis=1))
    case.tab.orc = orc
    for b, off in enumerate(offs):
        want = case.tab.want(ext, case.mics, int(off))[P:]
        util.same_bits(audio[b], want[N - hop:])
