"""Spectral frames of beam audio: what an audio model reads.

A classifier, a keyword spotter or a drone / no-drone network reads windowed STFT power through a filterbank on a log scale, and a user
watching a beam wants its spectrum or band levels.  `BeamFeatures` computes them on the device from a continuous float32 stream
(bf_spectrogram_device, include/beamformer_hip.h has the definition): the samples a frame still needs and the start of the next frame
live in device memory, so a captured graph keeps framing correctly when it is replayed, and the sample count of a push may itself be a
device value -- AudioOut's count -- so nothing waits for the host.

    ao = AudioOut(16000, rows=B, hop=sb.hop, pcm=False)
    bank, support = design_mel(16000, 512, 80)
    bf = BeamFeatures(16000, B, bank=bank, support=support)         # n_fft 512, n_win 400, hop 160: the shape speech models take
    out, st = sb.listen(d_frames, offsets)                           # [F, B, N_SAMPLES]
    feat, count = bf.push_from(ao, out)                              # float32 [B, cap, 80] log-mel, int32 [2] = (count, status)
    n = bf.last_count                                                # host mirror: feat[:, :n] are this push's frames, no sync
"""
import numpy as np

from lib._native import _entry, _torch, call

MAX_BANDS = 4096


def hann(n_win):
    """The periodic Hann window 0.5 - 0.5 cos(2 pi t / n_win), t < n_win, designed in float64 and stored as float32."""
    n_win = int(n_win)
    if n_win < 1:
        raise ValueError("n_win must be >= 1, got %d" % n_win)
    t = np.arange(n_win, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * t / n_win)).astype(np.float32)


# The mel scales.  HTK (S. Young et al., The HTK Book, 3.4, eq. 5.13): mel = 2595 log10(1 + f / 700).  Slaney (M. Slaney, Auditory Toolbox,
# Interval Research TR 1998-010, mfcc.m): linear, 200 / 3 Hz per mel, below 1000 Hz; above it 27 mels per factor 6.4 (log-spaced).
_F_SP = 200.0 / 3.0
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f, htk=False):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m, htk=False):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (np.maximum(m, _MIN_LOG_MEL) - _MIN_LOG_MEL)), _F_SP * m)


def _supports(bank):
    """[lo, hi) of every row's non-zero weights (0, 0 for an all-zero row)."""
    support = np.zeros((bank.shape[0], 2), dtype=np.int32)
    for b, row in enumerate(bank):
        nz = np.flatnonzero(row)
        if nz.size:
            support[b] = (nz[0], nz[-1] + 1)
    return support


def _check_fft(sr, n_fft):
    n_fft = int(n_fft)
    if n_fft < 32 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError("n_fft must be a power of two in [32, 4096], got %d" % n_fft)
    if not float(sr) > 0.0:
        raise ValueError("sr must be > 0, got %r" % (sr,))
    return float(sr), n_fft


def design_mel(sr, n_fft, n_mels, f_lo=0.0, f_hi=None, htk=False, norm="slaney"):
    """Triangular mel filters -> (bank float32 [n_mels, n_fft / 2 + 1], support int32 [n_mels, 2]).  n_mels + 2 points equally spaced on
    the mel scale between f_lo and f_hi (default sr / 2) are the edges f_0 .. f_{n_mels + 1}; band b is the triangle that rises from
    f_b to 1 at f_{b+1} and falls to 0 at f_{b+2}, sampled at the bin frequencies k sr / n_fft:
        w_b[k] = max(0, min((f - f_b) / (f_{b+1} - f_b), (f_{b+2} - f) / (f_{b+2} - f_{b+1})))
    norm "slaney": times 2 / (f_{b+2} - f_b), unit area per band (Slaney's mfcc.m); None: unit peak (HTK's filters).  Designed in
    float64, rounded once.  support[b] = [lo, hi) spans the band's non-zero weights; a triangle that holds no bin is lo == hi."""
    sr, n_fft = _check_fft(sr, n_fft)
    n_mels = int(n_mels)
    f_hi = sr / 2.0 if f_hi is None else float(f_hi)
    f_lo = float(f_lo)
    if n_mels < 1 or n_mels > MAX_BANDS:
        raise ValueError("n_mels must be in [1, %d], got %d" % (MAX_BANDS, n_mels))
    if not 0.0 <= f_lo < f_hi <= sr / 2.0:
        raise ValueError("0 <= f_lo < f_hi <= sr / 2 must hold, got %g, %g at sr = %g" % (f_lo, f_hi, sr))
    if norm not in ("slaney", None):
        raise ValueError("norm must be 'slaney' or None, got %r" % (norm,))
    edges = mel_to_hz(np.linspace(hz_to_mel(f_lo, htk), hz_to_mel(f_hi, htk), n_mels + 2), htk)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
    width = np.diff(edges)
    lower = (f[None, :] - edges[:-2, None]) / width[:-1, None]
    upper = (edges[2:, None] - f[None, :]) / width[1:, None]
    bank = np.maximum(0.0, np.minimum(lower, upper))
    if norm == "slaney":
        bank *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    return bank, _supports(bank)


def design_bands(sr, n_fft, edges):
    """Rectangular bands between consecutive edges (Hz, ascending; third-octave edges, say): band b sums the bins with
    edges[b] <= k sr / n_fft < edges[b + 1], weight 1 -> (bank float32 [len(edges) - 1, n_fft / 2 + 1], support int32 [.., 2])."""
    sr, n_fft = _check_fft(sr, n_fft)
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2 or edges.size - 1 > MAX_BANDS or not (np.diff(edges) > 0).all():
        raise ValueError("edges must be 2 .. %d ascending frequencies" % (MAX_BANDS + 1))
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
    band = np.searchsorted(edges, f, side="right") - 1           # the band of every bin; -1 and len(edges) - 1 are outside
    bank = np.zeros((edges.size - 1, f.size), dtype=np.float32)
    inside = (band >= 0) & (band < edges.size - 1)
    bank[band[inside], np.flatnonzero(inside)] = 1.0
    return bank, _supports(bank)


def advance_frames(s0, L, n_win, hop):
    """The definition's integer arithmetic in Python ints: the next frame's start s0 before a call on L samples -> (count, s0')."""
    count = (L - n_win - s0) // hop + 1 if s0 + n_win <= L else 0
    return count, s0 + count * hop - L


class BeamFeatures:
    """Spectral frames of `rows` streams at `sr` Hz: frames of n_win samples every `hop`, under `window` (default hann(n_win)),
    transformed at n_fft points, |.|^2, through `bank` / `support` (design_mel, design_bands; bank None: the power spectrum, n_fft / 2 + 1
    bands), then `scale` * log10(max(., floor)) (scale 1: log-mel, 10: dB, 0: linear).  `max_len`: the longest push (None: any), refused
    beyond.
    Device state, allocated once and updated in place so that a captured graph's addresses stay valid: `state` int32 [4] (the start
    of the next frame), `hist` float32 [rows, n_win - 1] (the samples before the next push), `count` int32 [2] (the last push's frame
    count and status).  `last_count` is the host's mirror of count[0], advanced by push with the same integer arithmetic; under graph
    replay only `count` on the device is authoritative."""

    def __init__(self, sr, rows, n_fft=512, n_win=400, hop=160, bank=None, support=None, scale=1.0, floor=1e-10, max_len=None, window=None, device="cuda"):
        torch = _torch()
        self.sr, self.n_fft = _check_fft(sr, n_fft)
        self.rows, self.n_win, self.hop = int(rows), int(n_win), int(hop)
        if self.rows < 1 or not 1 <= self.n_win <= self.n_fft or self.hop < 1:
            raise ValueError("rows >= 1, 1 <= n_win <= n_fft and hop >= 1 must hold, got %d, %d, %d" % (self.rows, self.n_win, self.hop))
        n_bins = self.n_fft // 2 + 1
        w = hann(self.n_win) if window is None else np.ascontiguousarray(window, dtype=np.float32)
        if w.shape != (self.n_win,):
            raise ValueError("window must have n_win = %d values, got %s" % (self.n_win, w.shape))
        if bank is None:
            if support is not None:
                raise ValueError("a support needs a bank")
            self.n_bands, self.d_bank, self.d_support = n_bins, None, None
        else:
            bank = np.ascontiguousarray(bank, dtype=np.float32)
            if bank.ndim != 2 or bank.shape[1] != n_bins or not 1 <= bank.shape[0] <= MAX_BANDS:
                raise ValueError("bank must be [1 .. %d, n_fft / 2 + 1 = %d], got %s" % (MAX_BANDS, n_bins, bank.shape))
            self.n_bands = bank.shape[0]
            self.d_bank = torch.from_numpy(bank).to(device)
            self.d_support = None
            if support is not None:
                support = np.ascontiguousarray(support, dtype=np.int32)
                if support.shape != (self.n_bands, 2):
                    raise ValueError("support must be [%d, 2], got %s" % (self.n_bands, support.shape))
                self.d_support = torch.from_numpy(support).to(device)
        self.scale, self.floor, self.device = float(scale), float(floor), device
        if not np.isfinite(self.scale) or (self.scale != 0.0 and not (np.isfinite(self.floor) and self.floor > 0.0)):
            raise ValueError("scale must be finite and, unless it is 0, floor finite and > 0, got %g, %g" % (self.scale, self.floor))
        self.max_len = None if max_len is None else int(max_len)
        self.d_window = torch.from_numpy(w).to(device)
        self.state = torch.zeros(4, dtype=torch.int32, device=device)
        self.count = torch.zeros(2, dtype=torch.int32, device=device)
        self.hist = torch.zeros((self.rows, self.n_win - 1), dtype=torch.float32, device=device)
        self._s0 = 0                     # the host mirror of state[0]
        self.last_count = 0

    def capacity(self, length):
        """The frame slots a push of `length` samples fills."""
        return _entry("bf_spectrogram_capacity")(int(length), self.hop)

    def push(self, d_audio, length=None, d_len=None):
        """d_audio float32 cuda [rows, len], the next samples of every row's stream -> (feat float32 [rows, cap, n_bands], count int32
        [2]): feat[:, :count[0]] are the frames this push completed, the rest of the cap = capacity(len) slots are zero.  `d_len`
        (int32 cuda, element 0): only that many of the len samples are there -- a device value, AudioOut's count; `length` is the
        host's copy of it for `last_count` (neither: len; d_len alone: it is read back, which waits for the stream).  Enqueue only."""
        torch = _torch()
        if d_audio.dim() != 2 or d_audio.dtype != torch.float32 or not d_audio.is_cuda or d_audio.shape[0] != self.rows:
            raise ValueError("d_audio must be a float32 cuda tensor [%d, len], got %s %s" % (self.rows, d_audio.dtype, tuple(d_audio.shape)))
        n = d_audio.shape[1]
        if self.max_len is not None and n > self.max_len:
            raise ValueError("a push of %d samples, max_len = %d" % (n, self.max_len))
        if d_audio.stride(1) != 1 or d_audio.stride(0) < n:      # (rows a fixed number of floats apart are taken as they are)
            d_audio = d_audio.contiguous()
        stride = max(d_audio.stride(0), n)
        if d_len is not None and (d_len.dtype != torch.int32 or not d_len.is_cuda or d_len.numel() < 1):
            raise ValueError("d_len must be an int32 cuda tensor")
        cap = self.capacity(n)
        feat = torch.empty((self.rows, cap, self.n_bands), dtype=torch.float32, device=self.device)
        call("bf_spectrogram_device", d_audio.data_ptr(), self.rows, stride, n, None if d_len is None else d_len.data_ptr(), self.hist.data_ptr(),
             self.state.data_ptr(), self.d_window.data_ptr(), self.n_win, self.n_fft, self.hop, None if self.d_bank is None else self.d_bank.data_ptr(),
             None if self.d_support is None else self.d_support.data_ptr(), self.n_bands, self.scale, self.floor, feat.data_ptr(), cap, self.count.data_ptr())
        if length is None:
            length = n if d_len is None else int(d_len[0].item())
        L = min(max(int(length), 0), n)
        self.last_count, self._s0 = advance_frames(self._s0, L, self.n_win, self.hop)
        return feat, self.count

    def push_from(self, ao, out):
        """ao.push(out) (an audio_out.AudioOut on listen's beams), then the frames of what it emitted: its float output, its device
        count as d_len and its host mirror as length -> (feat, count).  Nothing waits for the host."""
        audio, _, count = ao.push(out)
        return self.push(audio, length=ao.last_count, d_len=count)

    def reset(self):
        """A new stream: state and history are zeroed in place, so a captured push stays valid and starts the new stream on replay."""
        self.state.zero_()
        self.count.zero_()
        self.hist.zero_()
        self._s0, self.last_count = 0, 0
