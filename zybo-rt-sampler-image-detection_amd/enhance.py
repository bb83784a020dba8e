"""Noise suppression of beam audio: the single-channel spectral post-filter behind the beamformer.

A beam carries the noise that arrives from its look direction and the sensors' own: spatial filtering does nothing about it (and on a
14 cm aperture nothing below a few kHz is attenuated spatially at all).  `Enhancer` is the textbook companion of a beamformer, a
short-time spectral gain on its output (bf_enhance_device, include/beamformer_hip.h has the definition): analysis frames, a gain per
(frame, bin) from a decision-directed Wiener rule over a recursively tracked noise spectrum -- or gains the caller supplies, a model's
mask say --, and overlap-add synthesis back into audio, continuous across windows and calls.  The history, the partial overlap sums, the
noise spectrum and the frame phase live in device memory, so a captured graph keeps enhancing correctly when it is replayed.

    en = Enhancer(rows=B, hop=sb.hop)                                # n_fft 256, hop_s 128: 5.2 ms frames at 48828 Hz
    ao = AudioOut(48000, rows=B, hop=None)
    out, st = sb.listen(d_frames, offsets)                           # [F, B, N_SAMPLES]
    clean, count = en.push(out)                                      # float32 [B, S]: the stream, enhanced, en.delay samples late
    audio, pcm, n = ao.push_flat(clean)                              # at the sound card's rate; or bf.push_from(ao, clean[None])
"""
import numpy as np

from lib._native import _entry, _torch, call

MAX_OVERLAP = 8


def _check_frames(n_fft, hop_s):
    n_fft, hop_s = int(n_fft), int(hop_s)
    if n_fft < 32 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError("n_fft must be a power of two in [32, 4096], got %d" % n_fft)
    if hop_s < 1 or n_fft % hop_s or n_fft // hop_s > MAX_OVERLAP:
        raise ValueError("hop_s must divide n_fft = %d into 1 .. %d frames a sample, got %d" % (n_fft, MAX_OVERLAP, hop_s))
    return n_fft, hop_s


def design_cola(n_fft, hop_s, kind="sqrt_hann"):
    """An analysis / synthesis window pair whose products overlap-add to 1 at hop_s -> (win_a float32 [n_fft], win_s float32 [n_fft],
    deviation).  kind "sqrt_hann": the root of the periodic Hann window on both sides; "hann": the periodic Hann window on both sides.
    win_s is win_a divided, in float64, by the overlap sum of win_a^2 at its position, so that sum_j win_a[t + j hop_s] win_s[t + j hop_s]
    = 1 for every t; `deviation` is the largest distance from 1 of that sum over the rounded float32 pair, computed in float64.
    hop_s == n_fft gives rectangular windows."""
    n_fft, hop_s = _check_frames(n_fft, hop_s)
    if kind not in ("sqrt_hann", "hann"):
        raise ValueError("kind must be 'sqrt_hann' or 'hann', got %r" % (kind,))
    if hop_s == n_fft:
        w = np.ones(n_fft, dtype=np.float64)
    else:
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)
        if kind == "sqrt_hann":
            w = np.sqrt(w)
    overlap = (w * w).reshape(-1, hop_s).sum(axis=0)                 # of position t % hop_s
    win_a = w.astype(np.float32)
    win_s = (w / np.tile(overlap, n_fft // hop_s)).astype(np.float32)
    total = (win_a.astype(np.float64) * win_s.astype(np.float64)).reshape(-1, hop_s).sum(axis=0)
    return win_a, win_s, float(np.max(np.abs(total - 1.0)))


def advance_frames(c, S, hop_s):
    """The definition's integer arithmetic: c samples since the last frame end before a call on S samples -> (count, c')."""
    return (c + S) // hop_s, (c + S) % hop_s


class FrameGrid:
    """The frame grid a stream stage walks (csrc/stream_grid.h states it): frames of n_fft samples every hop_s, on the last `hop` samples
    of every window (None: whole windows).  It holds the host's mirror of the stream's position on the grid -- `c`, the samples since the
    last frame end, and `last_count`, the frames the last call completed -- and the stage's workspace, which only grows."""

    def __init__(self, n_fft, hop_s, hop, device):
        self.n_fft, self.hop_s = _check_frames(n_fft, hop_s)
        self.n_bins, self.hop, self.device = self.n_fft // 2 + 1, 0 if hop is None else int(hop), device
        if self.hop < 0:
            raise ValueError("hop must be >= 1 (None: back-to-back windows), got %d" % self.hop)
        self.shape = (self.n_fft, self.hop_s, self.hop)
        self._work, self.c, self.last_count = None, 0, 0

    def capacity(self, samples):
        return (self.hop_s - 1 + int(samples)) // self.hop_s

    def samples(self, F, N):
        """The stream samples that F windows of N add."""
        if self.hop > N:
            raise ValueError("hop = %d > N = %d" % (self.hop, N))
        return F * (self.hop or N)

    def work(self, entry, lead, what, S):
        """The workspace of a call on S samples, `entry`(lead, S, n_fft, hop_s) floats; lead: the stage's rows or slots (`what`)."""
        words = _entry(entry)(lead, S, self.n_fft, self.hop_s)
        if words < 0:
            raise ValueError("no workspace for %d %s of %d samples" % (lead, what, S))
        if self._work is None or self._work.numel() < words:
            self._work = _torch().empty(words, dtype=_torch().float32, device=self.device)
        return self._work

    def advance(self, S):
        self.last_count, self.c = advance_frames(self.c, S, self.hop_s)

    def reset(self):
        self.c, self.last_count = 0, 0


class Enhancer:
    """Spectral noise suppression of `rows` streams of windows every `hop` samples (None: back-to-back windows, or flat blocks): frames
    of n_fft samples every hop_s under design_cola's pair (or `windows` = (win_a, win_s)), the decision-directed Wiener gain with
    smoothing `alpha` and floor `g_min` over a noise spectrum that takes the stream's first `n_init` frames as noise and then follows the
    power of every bin with a forgetting factor that slides from `a_noise` (P / noise <= g0) to 1, frozen, (P / noise >= g1).
    Device state, allocated once and updated in place so that a captured graph's addresses stay valid: `state` int32 [4], `hist`
    float32 [rows, n_fft - 1], `ola` float32 [rows, n_fft], `noise` and `prior` float32 [rows, n_fft / 2 + 1], `count` int32 [2] (the last
    push's frame count and status).  With rows=None they are allocated by the first push, which then must not be a captured one.
    `delay` = n_fft: the output is the stream that many samples late.  `last_count` is the host's mirror of count[0]."""

    def __init__(self, rows=None, hop=None, n_fft=256, hop_s=128, alpha=0.98, a_noise=0.9, g0=1.5, g1=5.0, g_min=0.1, n_init=8, windows=None,
                 device="cuda"):
        self.grid = FrameGrid(n_fft, hop_s, hop, device)
        self.n_fft, self.hop_s, self.n_bins, self.hop = self.grid.n_fft, self.grid.hop_s, self.grid.n_bins, self.grid.hop
        self.alpha, self.a_noise, self.g0, self.g1, self.g_min, self.n_init = float(alpha), float(a_noise), float(g0), float(g1), float(g_min), int(n_init)
        if not (0.0 <= self.alpha < 1.0 and 0.0 <= self.a_noise < 1.0 and 0.0 <= self.g0 < self.g1 < np.inf and 0.0 <= self.g_min <= 1.0 and self.n_init >= 1):
            raise ValueError("alpha and a_noise in [0, 1), 0 <= g0 < g1, g_min in [0, 1] and n_init >= 1 must hold")
        if windows is None:
            win_a, win_s, self.cola_deviation = design_cola(self.n_fft, self.hop_s)
        else:
            win_a, win_s = (np.ascontiguousarray(w, dtype=np.float32) for w in windows)
            if win_a.shape != (self.n_fft,) or win_s.shape != (self.n_fft,):
                raise ValueError("windows must be two arrays of n_fft = %d values" % self.n_fft)
            self.cola_deviation = None
        torch = _torch()
        self.device, self.delay = device, self.n_fft
        self.d_win_a, self.d_win_s = torch.from_numpy(win_a).to(device), torch.from_numpy(win_s).to(device)
        self.state = torch.zeros(4, dtype=torch.int32, device=device)
        self.count = torch.zeros(2, dtype=torch.int32, device=device)
        self.rows = None if rows is None else int(rows)
        self.hist = self.ola = self.noise = self.prior = None
        if self.rows is not None:
            self._allocate(self.rows)

    last_count = property(lambda self: self.grid.last_count)

    def _allocate(self, rows):
        torch = _torch()
        if rows < 1:
            raise ValueError("rows must be >= 1, got %d" % rows)
        self.rows = rows
        z = lambda n: torch.zeros((rows, n), dtype=torch.float32, device=self.device)
        self.hist, self.ola, self.noise, self.prior = z(self.n_fft - 1), z(self.n_fft), z(self.n_bins), z(self.n_bins)

    def capacity(self, samples):
        """The frame slots of a push of `samples` stream samples a row: the second dimension of `gains`."""
        return self.grid.capacity(samples)

    def push(self, out, gains=None, observe=False):
        """out float32 cuda [F, B, N] as listen() returns it (or [B, S], a flat block of every row's stream) -> (clean float32 [B, S],
        count int32 [2] = (frames completed, status)): the last `hop` samples of every window, S = F * hop in all, enhanced and
        delayed by n_fft.  `gains` float32 cuda [B, capacity(S), n_fft / 2 + 1]: the gain of every bin of the frames this push
        completes, instead of the Wiener rule; the noise tracker then stands still.  observe: also return (power, gain), float32
        [B, capacity(S), n_fft / 2 + 1], P and G of the completed frames and zeros behind them.  Enqueue only."""
        torch = _torch()
        if out.dim() == 2:
            if self.hop:
                raise ValueError("a flat block is a whole piece of the stream: this Enhancer has hop = %d" % self.hop)
            out = out.unsqueeze(0)
        if out.dim() != 3 or out.dtype != torch.float32 or not out.is_cuda or out.shape[0] < 1 or out.shape[1] < 1 or out.shape[2] < 1:
            raise ValueError("out must be a float32 cuda tensor [F, B, N] or [B, S], got %s %s" % (out.dtype, tuple(out.shape)))
        x = out.contiguous()
        F, B, N = x.shape
        if self.rows is None:
            self._allocate(B)
        if B != self.rows:
            raise ValueError("this Enhancer takes %d rows, out has %d" % (self.rows, B))
        S = self.grid.samples(F, N)
        cap = self.capacity(S)
        if gains is not None:
            if gains.dtype != torch.float32 or not gains.is_cuda or tuple(gains.shape) != (B, cap, self.n_bins):
                raise ValueError("gains must be a float32 cuda tensor %s, got %s %s" % ((B, cap, self.n_bins), gains.dtype, tuple(gains.shape)))
            gains = gains.contiguous()
        work = self.grid.work("bf_enhance_workspace", B, "rows", S)
        clean = torch.empty((B, S), dtype=torch.float32, device=self.device)
        power = torch.empty((B, cap, self.n_bins), dtype=torch.float32, device=self.device) if observe else None
        gain = torch.empty((B, cap, self.n_bins), dtype=torch.float32, device=self.device) if observe else None
        call("bf_enhance_device", x.data_ptr(), B, F, N, N, self.hop, self.hist.data_ptr(), self.ola.data_ptr(), self.noise.data_ptr(), self.prior.data_ptr(),
             self.state.data_ptr(), self.d_win_a.data_ptr(), self.d_win_s.data_ptr(), self.n_fft, self.hop_s, None if gains is None else gains.data_ptr(),
             self.alpha, self.a_noise, self.g0, self.g1, self.g_min, self.n_init, work.data_ptr(), clean.data_ptr(), S,
             None if power is None else power.data_ptr(), None if gain is None else gain.data_ptr(), self.count.data_ptr())
        self.grid.advance(S)
        return (clean, self.count, power, gain) if observe else (clean, self.count)

    def reset(self):
        """A new stream: all carried state is zeroed in place, so a captured push stays valid and starts the new stream on replay."""
        for t in (self.state, self.count, self.hist, self.ola, self.noise, self.prior):
            if t is not None:
                t.zero_()
        self.grid.reset()
