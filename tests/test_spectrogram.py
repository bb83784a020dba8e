"""GPU (-m gpu): bf_spectrogram_device and features.BeamFeatures against the NumPy restatement of the definition
(tests/spectrogram_np.py: u in float32 as defined, the rest in float64) within the derived bound, and the definition's bit-exact
promises on the bytes: the cut of the stream into calls, the row count, the frame index, the pointer alignment, a NaN's reach.

Data: floats whose magnitudes spread over 2^-12 .. 2^12 from one stretch of the stream to the next.  Rows are in_stride = len + 3
floats apart with NaN between them, and NaN stands where d_len says no sample is; d_out has out_frames = cap + 2; d_out, d_hist,
d_state and d_count sit between canaries, which must survive, as must the frames of a row past cap."""
import numpy as np
import pytest

import spectrogram_np as S
import util
from support import nat_restoring as nat

pytestmark = pytest.mark.gpu

CANARY = 64                 # elements in front of and behind every device output
CANARY_F = -1234.5
CANARY_I = 0x5A5A5A
FLOOR3, FLOOR6, FLOOR10 = (float(np.float32(v)) for v in (1e-3, 1e-6, 1e-10))       # floors as the float32 the call receives
RATIOS = {}                 # kind of output -> the largest |error| / bound seen (printed by the last test)


def _wild(rng, rows, n, stretch):
    """[rows, n]: normal samples whose magnitude changes by a power of two in 2^-12 .. 2^12 every `stretch` samples."""
    e = rng.integers(-12, 13, size=(rows, n // max(stretch, 1) + 1))
    return (rng.standard_normal((rows, n)) * np.exp2(np.repeat(e, max(stretch, 1), axis=1)[:, :n])).astype(np.float32)


def _between_canaries(a, off, value):
    """(buffer, lo): a device buffer of canaries with `a` at [lo, lo + a.size), off words past a 16-byte boundary."""
    torch = util.torch_gpu()
    a = np.ascontiguousarray(a).ravel()
    buf = torch.full((CANARY + 4 + a.size + CANARY,), value, dtype=torch.from_numpy(a).dtype, device="cuda")
    lo = CANARY + off
    buf[lo:lo + a.size].copy_(torch.from_numpy(a))
    assert buf[lo:].data_ptr() % 16 == 4 * off
    return buf, lo


def _inner(buf, lo, size, value):
    """The host copy of buf[lo : lo + size], after checking the canaries around it."""
    host = buf.cpu().numpy()
    assert (host[:lo] == host.dtype.type(value)).all() and (host[lo + size:] == host.dtype.type(value)).all(), "a canary was overwritten"
    return host[lo:lo + size].copy()


def _run(nat, x, hist, s0, window, n_fft, hop, bank=None, support=None, scale=0.0, floor=1e-10, d_len=None, off=0, expect_rc=0):
    """bf_spectrogram_device on device copies -> dict(out, count, status, s0, words, hist, cap).  The canaries are checked."""
    torch = util.torch_gpu()
    rows, length = x.shape
    n_win = window.shape[0]
    H = n_win - 1
    n_bands = n_fft // 2 + 1 if bank is None else bank.shape[0]
    cap = S.capacity(length, hop)
    assert nat.lib.bf_spectrogram_capacity(length, hop) == cap
    out_frames = cap + 2
    stride = length + 3
    L = length if d_len is None else min(max(d_len, 0), length)
    xs = np.full((rows, stride), np.nan, dtype=np.float32)
    xs[:, :L] = x[:, :L]                                                 # NaN behind every row, and where no sample is
    d_x = util.place_words(xs, off)
    d_w = util.place_words(window, off)
    d_b = None if bank is None else util.place_words(bank, off)
    d_s = None if support is None else util.place_words(support.astype(np.int32), off)
    d_l = None if d_len is None else util.place_words(np.array([d_len], dtype=np.int32), off)
    words0 = np.array([s0, 77, -5, 9], dtype=np.int32)                   # the reserved words are written 0
    obuf, o_lo = _between_canaries(np.full(rows * out_frames * n_bands, CANARY_F, np.float32), off, CANARY_F)
    hbuf, h_lo = _between_canaries(hist.astype(np.float32), off, CANARY_F)
    sbuf, s_lo = _between_canaries(words0, off, CANARY_I)
    cbuf, c_lo = _between_canaries(np.array([-9, -9], dtype=np.int32), off, CANARY_I)
    ptr = lambda t, lo=0: t[lo:].data_ptr()
    rc = nat.lib.bf_spectrogram_device(ptr(d_x), rows, stride, length, None if d_l is None else ptr(d_l), ptr(hbuf, h_lo), ptr(sbuf, s_lo), ptr(d_w), n_win,
                                       n_fft, hop, None if d_b is None else ptr(d_b), None if d_s is None else ptr(d_s), n_bands, scale, floor,
                                       ptr(obuf, o_lo), out_frames, ptr(cbuf, c_lo), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = _inner(obuf, o_lo, rows * out_frames * n_bands, CANARY_F).reshape(rows, out_frames, n_bands)
    new_hist = _inner(hbuf, h_lo, rows * H, CANARY_F).reshape(rows, H)
    words = _inner(sbuf, s_lo, 4, CANARY_I)
    cnt = _inner(cbuf, c_lo, 2, CANARY_I)
    if expect_rc != 0:
        assert rc == expect_rc and nat.lib.bf_last_error()
        nat.lib.bf_clear_error()
        assert (out == np.float32(CANARY_F)).all() and words.tolist() == words0.tolist() and cnt.tolist() == [-9, -9]      # nothing was enqueued
        return None
    assert rc == 0, nat.lib.bf_last_error()
    assert (out[:, cap:] == np.float32(CANARY_F)).all(), "a frame past cap was written"
    return dict(out=out[:, :cap].copy(), count=int(cnt[0]), status=int(cnt[1]), s0=int(words[0]), words=words.tolist(), hist=new_hist, cap=cap)


def _check(got, want, scale=None, floor=None):
    assert (got["count"], got["status"], got["s0"], got["cap"]) == (want["count"], want["status"], want["s0"], want["cap"])
    if want["status"] == 0:
        assert got["words"][1:] == [0, 0, 0]
    assert got["hist"].tobytes() == want["hist"].astype(np.float32).tobytes()
    assert not got["out"][:, want["count"]:].any() and not np.signbit(got["out"][:, want["count"]:]).any()       # +0.0f behind the last frame
    assert S.inside(got["out"], want) == ""
    ratio = S.worst_ratio(got["out"], want)
    if scale is not None:                                                # (the log outputs apart, and apart again where a band sits on the floor)
        on_floor = want["out"] == scale * np.log10(floor) if scale else np.zeros(want["out"].shape, bool)
        for name, where in (("log outputs on the floor", on_floor), ("log outputs" if scale else "linear outputs", ~on_floor)):
            RATIOS[name] = max(RATIOS.get(name, 0.0), S.worst_ratio(got["out"], want, where))
    return ratio


# ------------------------------------------------------------------ banks

def _bank(kind, n_fft, rng):
    """(bank, support) of a kind.  Where a support is given the weights outside it are NaN: they are not read."""
    import features
    n_bins = n_fft // 2 + 1
    if kind == "none":
        return None, None
    if kind == "full":                                                   # no support: whole rows, weights of either sign
        return rng.standard_normal((5, n_bins)).astype(np.float32), None
    if kind == "mel":                                                    # more triangles than the low bins can hold: some are empty
        bank, support = features.design_mel(16000, n_fft, {32: 21, 64: 41, 512: 80, 1024: 64, 4096: 128}[n_fft])
        if n_fft <= 64:
            assert (support[:, 0] == support[:, 1]).any()
    else:                                                                # "bands": rectangles, one of them emptied by hand
        bank, support = features.design_bands(16000, n_fft, [0.0, 300.0, 1001.0, 1002.0, 3000.0, 8000.1])     # (no bin lies in [1001, 1002) Hz)
        assert support[2, 0] == support[2, 1] and bank.sum() == n_bins
    bank = bank.copy()
    k = np.arange(n_bins)[None, :]
    bank[~((k >= support[:, :1]) & (k < support[:, 1:]))] = np.nan
    return bank, support


def _stream(rng, rows, n, n_win):
    return _wild(rng, rows, n, max(n_win // 2, 1))


# (n_fft, n_win, hop, rows, len, s0, bank, scale, d_len)
CASES = [
    (32, 25, 10, 3, 64, 0, "bands", 1.0, None),          # the start of a stream
    (32, 32, 1, 1, 40, -31, "none", 0.0, None),          # hop 1, the history read to its first sample
    (32, 31, 31, 65, 100, -5, "mel", 10.0, None),        # hop = n_win, 65 rows, empty triangles
    (32, 25, 28, 3, 90, 2, "full", 0.0, None),           # hop = n_win + 3: s0 positive, samples skipped
    (32, 25, 10, 3, 0, -7, "bands", 1.0, None),          # len 0: the second launch alone
    (32, 25, 10, 3, 1, -24, "mel", 1.0, None),           # len 1 = s0 + n_win: one frame, of history and one sample
    (32, 25, 10, 3, 1, -23, "mel", 1.0, None),           # len 1: no frame, the history moves by one
    (32, 25, 10, 3, 23, -24, "none", 10.0, None),        # len = n_win - 2: the history shifts inside itself
    (32, 25, 10, 3, 65, 0, "full", 1.0, None),           # the last frame ends on the last sample
    (32, 25, 10, 3, 64, 0, "bands", 0.0, None),          # ... and one sample short of that
    (32, 25, 10, 3, 90, 200, "none", 1.0, None),         # s0 beyond the call: no frame, s0 comes closer
    (64, 64, 67, 3, 200, -10, "none", 1.0, 150),         # d_len below len
    (64, 63, 1, 1, 70, 0, "mel", 1.0, 1000),             # d_len above len: clamped
    (64, 63, 63, 3, 130, -62, "bands", 0.0, -4),         # d_len below 0: clamped
    (64, 40, 16, 3, 100, -3, "mel", 10.0, 0),            # d_len 0
    (512, 400, 160, 3, 1000, -399, "mel", 1.0, None),    # the speech shape, 80 mel bands
    (512, 512, 515, 1, 1100, 0, "none", 10.0, None),
    (512, 511, 511, 3, 1100, -300, "bands", 0.0, 1022),
    (512, 400, 160, 3, 398, -100, "full", 1.0, None),    # len = n_win - 2 on the speech shape
    (1024, 1024, 300, 3, 2000, -100, "mel", 1.0, None),  # the first four-wave size
    (1024, 1023, 1026, 1, 2100, 0, "none", 0.0, None),
    (1024, 1024, 1, 1, 5, -1023, "bands", 10.0, None),   # hop 1 on four waves: five frames a sample apart
    (4096, 4096, 1000, 2, 6000, -4095, "bands", 10.0, None),
    (4096, 4095, 4098, 1, 8300, 0, "none", 1.0, None),
    (4096, 4096, 4096, 3, 4094, -2000, "mel", 0.0, None),  # len = n_win - 2 with 4095 samples of history: sixteen a lane
]


def _case(n_fft, n_win, hop, rows, length, s0, bank_kind, scale, d_len):
    rng = np.random.default_rng([n_fft, n_win, hop, rows, length, abs(s0), int(scale)])
    x = _stream(rng, rows, length, n_win)
    hist = _stream(rng, rows, n_win - 1, n_win)
    window = (rng.standard_normal(n_win) * 0.5 + 1.0).astype(np.float32) if n_win % 2 else None
    if window is None:
        import features
        window = features.hann(n_win)
    bank, support = _bank(bank_kind, n_fft, rng)
    return x, hist, window, bank, support


def test_the_cases_cover_the_shapes():
    assert {c[0] for c in CASES} == {32, 64, 512, 1024, 4096}
    for n_fft in (32, 64, 512, 1024, 4096):
        mine = [c for c in CASES if c[0] == n_fft]
        assert {n_fft, n_fft - 1} <= {c[1] for c in mine}                             # n_win = n_fft and n_fft - 1
        assert "none" in {c[6] for c in mine} and len({c[6] for c in mine}) >= 3 and {c[7] for c in mine} == {0.0, 1.0, 10.0}
        assert any(c[2] == c[1] + 3 for c in mine) and any(c[2] in (1, c[1]) for c in mine)
    assert (32, 25) in {c[:2] for c in CASES}
    assert {c[3] for c in CASES} >= {1, 3, 65} and {c[7] for c in CASES} == {0.0, 1.0, 10.0}
    assert {c[4] for c in CASES} >= {0, 1} and any(c[4] == c[1] - 2 for c in CASES) and any(c[4] == c[5] + c[1] for c in CASES)
    assert any(c[8] is not None and 0 < c[8] < c[4] for c in CASES) and any(c[8] is not None and c[8] > c[4] for c in CASES)
    assert any(c[2] == 1 for c in CASES) and any(c[2] == c[1] for c in CASES) and any(c[5] > 0 for c in CASES)
    assert any(c[5] + (S.advance(c[5], c[4], c[1], c[2])[0] - 1) * c[2] + c[1] == c[4] for c in CASES if c[8] is None)   # a last frame on the last sample


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_matches_the_definition(nat, case):
    n_fft, n_win, hop, rows, length, s0, bank_kind, scale, d_len = case
    x, hist, window, bank, support = _case(*case)
    floor = FLOOR3 if scale else 0.0
    got = _run(nat, x, hist, s0, window, n_fft, hop, bank, support, scale, floor, d_len)
    want = S.spectrogram(x, hist, s0, window, n_fft, hop, bank, support, scale, floor, L=d_len)
    ratio = _check(got, want, scale, floor)
    print("%s: count %d of cap %d, error / bound <= %.4f" % (case, got["count"], got["cap"], ratio))
    if bank_kind in ("mel", "bands") and scale and got["count"]:                     # an empty band is the floor
        empty = np.flatnonzero(support[:, 0] == support[:, 1])
        assert (empty.size or n_fft > 64) and np.unique(got["out"][:, :got["count"], empty]).size == min(empty.size, 1)


# ------------------------------------------------------------------ the bit-exact promises

STREAMS = [(32, 25, 10, "bands", 1.0), (32, 25, 28, "none", 0.0), (64, 64, 1, "full", 10.0), (512, 400, 160, "mel", 1.0), (1024, 1024, 300, "none", 1.0),
           (4096, 4095, 1500, "bands", 0.0)]


def _pushed(nat, x, cuts, window, n_fft, hop, bank, support, scale, off=0, pad_to=None):
    """The stream x pushed in the pieces `cuts` marks -> (frames [rows, total, n_bands], counts, final s0, final hist).  pad_to: every
    call is given that many slots and a d_len (the pieces then differ only in the device-side count)."""
    rows, n_win = x.shape[0], window.shape[0]
    hist, s0, parts, counts = np.zeros((rows, n_win - 1), np.float32), 0, [], []
    for a, b in zip([0] + cuts, cuts + [x.shape[1]]):
        piece, d_len = x[:, a:b], None
        if pad_to is not None:
            piece, d_len = np.concatenate([piece, np.zeros((rows, pad_to - (b - a)), np.float32)], axis=1), b - a
        got = _run(nat, piece, hist, s0, window, n_fft, hop, bank, support, scale, FLOOR6, d_len, off)
        assert got["status"] == 0
        parts.append(got["out"][:, :got["count"]])
        counts.append(got["count"])
        hist, s0 = got["hist"], got["s0"]
    return np.concatenate(parts, axis=1), counts, s0, hist


@pytest.mark.parametrize("n_fft,n_win,hop,bank_kind,scale", STREAMS)
def test_the_cut_of_the_stream_does_not_show(nat, n_fft, n_win, hop, bank_kind, scale):
    """One push, two and seven ragged ones (a piece of 0, of 1 and of n_win - 2 samples among them), and seven pushes whose length is a
    device value: the same bytes, the same frames, the same final state."""
    import features
    rng = np.random.default_rng([n_fft, n_win, hop, 7])
    total = 5 * max(hop, n_win) + n_win + 3
    x = _stream(rng, 3, total, n_win)
    window = features.hann(n_win)
    bank, support = _bank(bank_kind, n_fft, rng)
    one, counts1, s1, h1 = _pushed(nat, x, [], window, n_fft, hop, bank, support, scale)
    want = S.spectrogram(x, np.zeros((3, n_win - 1), np.float32), 0, window, n_fft, hop, bank, support, scale, FLOOR6)
    assert counts1 == [want["count"]] and want["count"] >= 5 and S.inside(one, dict(lo=want["lo"][:, :want["count"]], hi=want["hi"][:, :want["count"]])) == ""
    seven = [1, 1, n_win - 1, total // 3, total // 2 + 5, total - 7]                 # pieces of 1, 0, n_win - 2, ... samples
    assert seven == sorted(seven)
    for cuts, pad_to in (([total // 2 - 3], None), (seven, None), (seven, total)):
        many, counts, s0, hist = _pushed(nat, x, list(cuts), window, n_fft, hop, bank, support, scale, pad_to=pad_to)
        assert sum(counts) == counts1[0] and s0 == s1, (counts, counts1)
        assert many.tobytes() == one.tobytes(), np.argwhere(many.view(np.uint32) != one.view(np.uint32))[:4]
        assert hist.tobytes() == h1.tobytes()


@pytest.mark.parametrize("n_fft,n_win,hop,bank_kind,scale", STREAMS[:4])
def test_a_row_alone_and_among_64_others(nat, n_fft, n_win, hop, bank_kind, scale):
    """... and at another place in memory: every pointer one float off a 16-byte boundary."""
    import features
    rng = np.random.default_rng([n_fft, n_win, hop, 65])
    total = 3 * max(hop, n_win) + n_win
    x = _stream(rng, 65, total, n_win)
    hist = _stream(rng, 65, n_win - 1, n_win)
    window = features.hann(n_win)
    bank, support = _bank(bank_kind, n_fft, rng)
    s0 = -(n_win // 2)
    crowd = _run(nat, x, hist, s0, window, n_fft, hop, bank, support, scale, FLOOR6)
    for r, off in ((0, 0), (37, 1), (64, 3)):
        alone = _run(nat, x[r:r + 1], hist[r:r + 1], s0, window, n_fft, hop, bank, support, scale, FLOOR6, off=off)
        assert alone["count"] == crowd["count"] >= 3 and alone["s0"] == crowd["s0"]
        assert alone["out"][0].tobytes() == crowd["out"][r].tobytes() and alone["hist"][0].tobytes() == crowd["hist"][r].tobytes()
    shifted = _run(nat, x, hist, s0, window, n_fft, hop, bank, support, scale, FLOOR6, off=1)
    assert shifted["out"].tobytes() == crowd["out"].tobytes() and shifted["hist"].tobytes() == crowd["hist"].tobytes()


@pytest.mark.parametrize("n_fft,n_win,hop,bank_kind,scale", [STREAMS[0], STREAMS[3], STREAMS[4]])
def test_a_nan_reaches_only_the_frames_that_hold_it(nat, n_fft, n_win, hop, bank_kind, scale):
    import features
    rng = np.random.default_rng([n_fft, n_win, hop, 99])
    total = 6 * hop + n_win
    x = _stream(rng, 3, total, n_win)
    hist = np.zeros((3, n_win - 1), np.float32)
    window = features.hann(n_win) + np.float32(0.01)                                 # (no zero weight: a NaN under it would still be a NaN)
    bank, support = _bank(bank_kind, n_fft, rng)
    clean = _run(nat, x, hist, 0, window, n_fft, hop, bank, support, scale, FLOOR6)
    at = 3 * hop + n_win // 2
    bad = x.copy()
    bad[1, at] = np.nan
    got = _run(nat, bad, hist, 0, window, n_fft, hop, bank, support, scale, FLOOR6)
    assert got["count"] == clean["count"] == 7
    holds = np.array([j * hop <= at < j * hop + n_win for j in range(7)])
    assert holds.any() and not holds.all()
    assert got["out"][[0, 2]].tobytes() == clean["out"][[0, 2]].tobytes()             # the other rows
    assert got["out"][1, :7][~holds].tobytes() == clean["out"][1, :7][~holds].tobytes()
    live = np.ones(got["out"].shape[2], bool) if support is None else support[:, 0] < support[:, 1]
    assert np.isnan(got["out"][1, :7][holds][:, live]).all()                         # every band that reads a bin
    assert np.array_equal(got["hist"][[0, 2]], clean["hist"][[0, 2]])


def test_a_corrupt_state_is_reported_and_nothing_moves(nat):
    import features
    rng = np.random.default_rng(13)
    n_fft, n_win, hop = 32, 25, 10
    x, hist = _stream(rng, 3, 64, n_win), _stream(rng, 3, n_win - 1, n_win)
    for s0 in (-25, -1000, -(1 << 31)):
        got = _run(nat, x, hist, s0, features.hann(n_win), n_fft, hop, None, None, 1.0, FLOOR6)
        assert (got["count"], got["status"], got["cap"]) == (0, 1, 7) and got["words"] == [s0, 77, -5, 9]
        assert got["hist"].tobytes() == hist.tobytes() and not got["out"].any()
        _check(got, S.spectrogram(x, hist, s0, features.hann(n_win), n_fft, hop, None, None, 1.0, FLOOR6))
    assert _run(nat, x, hist, 0, features.hann(n_win), n_fft, hop, None, None, float("nan"), FLOOR6, expect_rc=-1) is None


# ------------------------------------------------------------------ features.BeamFeatures: a captured chain, and a tone end to end


def test_graph_replay_of_audio_out_and_features(nat):
    """AudioOut.push then BeamFeatures.push on its device count, captured as the objects' first call and replayed three times over fresh
    beams, against three eager pushes on a second pair: bytes and counts.  The counts differ from push to push (4000 / 4069)."""
    torch = util.torch_gpu()
    import audio_out
    import features
    N, hop, F, B = 64, 33, 2, 3
    util.configure_small(N)
    rng = np.random.default_rng(58)
    step = hop * F
    stream = (rng.standard_normal((B, step * 4 + N)) * 0.3).astype(np.float32)
    batches = [np.ascontiguousarray(np.stack([stream[:, c * step + (f + 1) * hop:c * step + (f + 1) * hop + N] for f in range(F)])) for c in range(4)]
    bank, support = features.design_bands(48000, 32, [0.0, 2000.0, 5000.0, 9000.0, 24000.1])
    make = lambda: (audio_out.AudioOut(48000, rows=B, hop=hop, pcm=False), features.BeamFeatures(48000, B, n_fft=32, n_win=25, hop=10, bank=bank, support=support))
    ao, bf = make()
    bf.push_from(ao, torch.from_numpy(batches[3]).cuda())                 # (a third pair: a first launch loads the kernels)
    torch.cuda.synchronize()
    eager = []
    ao, bf = make()
    hist, s0 = np.zeros((B, 24), np.float32), 0
    for c in range(3):
        audio, _, n_audio = ao.push(torch.from_numpy(batches[c]).cuda())
        feat, count = bf.push(audio, length=ao.last_count, d_len=n_audio)
        torch.cuda.synchronize()
        eager.append((feat.cpu().numpy(), count.cpu().numpy().copy()))
        want = S.spectrogram(audio.cpu().numpy(), hist, s0, features.hann(25), 32, 10, bank, support, 1.0, FLOOR10, L=int(n_audio[0]))
        assert eager[-1][1].tolist() == [want["count"], 0] and bf.last_count == want["count"] and S.inside(eager[-1][0], want) == ""
        hist, s0 = want["hist"], want["s0"]
    eager_state, eager_hist = bf.state.cpu().numpy(), bf.hist.cpu().numpy()
    ao, bf = make()
    x = torch.from_numpy(batches[0]).cuda()
    carried = (bf.hist.data_ptr(), bf.state.data_ptr(), bf.count.data_ptr())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        feat, count = bf.push_from(ao, x)                                 # captured, not run: the objects' first call
    assert carried == (bf.hist.data_ptr(), bf.state.data_ptr(), bf.count.data_ptr())
    for c in range(3):
        x.copy_(torch.from_numpy(batches[c]).cuda())
        g.replay()
        torch.cuda.synchronize()
        assert count.cpu().numpy().tolist() == eager[c][1].tolist()
        assert feat.cpu().numpy().tobytes() == eager[c][0].tobytes()
    assert np.array_equal(bf.state.cpu().numpy(), eager_state) and bf.hist.cpu().numpy().tobytes() == eager_hist.tobytes()
    bf.reset()
    assert not bf.state.cpu().numpy().any() and not bf.hist.cpu().numpy().any() and bf.last_count == 0 and carried[0] == bf.hist.data_ptr()


def test_a_tone_peaks_in_its_mel_band(nat):
    """1 kHz at 48828 Hz through AudioOut(16000) and BeamFeatures' defaults with 80 mel bands -- the shape speech models take -- in two
    pushes: every complete frame peaks in the band whose triangle holds 1 kHz (bin 32 of 512 at 16 kHz)."""
    torch = util.torch_gpu()
    import audio_out
    import features
    import pipeline
    N, hop, F = 256, 128, 40
    util.configure_small(N)
    t = np.arange(hop * (F + 1), dtype=np.float64)
    tone = (0.5 * np.sin(2 * np.pi * 1000.0 * t / 48828.0)).astype(np.float32)
    frames = np.ascontiguousarray(np.stack([tone[f * hop:f * hop + N] for f in range(F)]))[:, None, :]          # [F, 1, N]
    ao = audio_out.AudioOut(16000, rows=1, hop=hop, pcm=False)
    bank, support = features.design_mel(16000, 512, 80)
    bf = features.BeamFeatures(16000, 1, bank=bank, support=support)
    assert (bf.n_fft, bf.n_win, bf.hop, bf.n_bands, bf.scale) == (512, 400, 160, 80, 1.0)
    band = int(np.argmax(bank[:, 32]))
    assert support[band, 0] <= 32 < support[band, 1]
    d_frames = torch.from_numpy(frames).cuda()
    seen = 0
    for f0, f1 in ((0, 11), (11, F)):
        feat, count = pipeline.FusedPipeline.features(None, d_frames[f0:f1], ao, bf)
        n = int(count.cpu().numpy()[0])
        assert n == bf.last_count and count.cpu().numpy()[1] == 0 and feat.shape[0] == 1 and feat.shape[2] == 80 and n <= feat.shape[1]
        got = feat.cpu().numpy()[0, :n]
        assert (np.argmax(got, axis=1) == band).all(), np.argmax(got, axis=1)
        far = np.abs(np.arange(80) - band) >= 2
        print("frames %d..%d: the bands two or more from the peak lie %.1f .. %.1f dB below it" % (seen, seen + n, 10 * (got[:, band, None] - got[:, far]).min(),
                                                                                              10 * (got[:, band, None] - got[:, far]).max()))
        seen += n
    assert seen >= 7


def test_print_the_ratios():
    for name in sorted(RATIOS):
        print("largest error / bound, %s: %.4f" % (name, RATIOS[name]))
    if RATIOS:
        print("largest error / bound overall: %.4f" % max(RATIOS.values()))
