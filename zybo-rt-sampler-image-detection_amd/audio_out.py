"""The output stage: beams at a sound card's rate.

Every listening path -- BeamListener.listen, StreamBeamformer.listen / audio, BandFilter.beams, FilterSumListener.listen -- ends in
float32 rows on the device at the array's own rate, config.SAMPLE_RATE = 48828 Hz, the by-product of an FPGA clock divider that
no sound card, WAV player, codec or speech model takes.  `AudioOut` converts them by a rational factor up / down on the device
(bf_resample_device, include/beamformer_hip.h has the definition), continuous across windows and batches like every other stream
stage: the phase lives in device memory, so a captured graph keeps converting correctly when it is replayed.

    sb = StreamBeamformer("lerp", hop=128);  ao = AudioOut(48000, hop=sb.hop)
    out, st = sb.listen(d_frames, offsets)            # [F, B, N_SAMPLES]
    audio, pcm, count = ao.push(out)                  # float32 [B, cap], int16 [cap, B] interleaved, int32 [2] = (count, status)
    sb.advance(d_frames)                              # ao carries its own window
    n = ao.last_count                                 # host mirror: audio[:, :n] and pcm[:n] are this push's samples, no sync
"""
from fractions import Fraction

import numpy as np

from carried import CarriedFrame
from interface import config
from lib._native import _entry, _torch, call

MAX_PHASES = 16384
MAX_TAPS = 128


def rate_ratio(rate_out, rate_in=None):
    """(up, down) in lowest terms with rate_out / rate_in = up / down.  rate_in defaults to config.SAMPLE_RATE; either may be an int, a
    float (taken exactly) or a Fraction.  48828 -> 48000 Hz is 4000 / 4069, 48828 -> 44100 Hz is 3675 / 4069."""
    r_in = Fraction(config.SAMPLE_RATE if rate_in is None else rate_in)
    r_out = Fraction(rate_out)
    if r_in <= 0 or r_out <= 0:
        raise ValueError("rates must be > 0, got %s -> %s" % (r_in, r_out))
    q = r_out / r_in
    return q.numerator, q.denominator


def design_resampler(up, down, taps=32, att=80.0, rolloff=0.9):
    """The polyphase table of an up / down converter, float32 [up, taps]: h[p][t] = g[t * up + p] of a Kaiser-windowed sinc prototype g
    of length Q = up * taps at the upsampled rate, designed in float64 and rounded once:
        fc   = 0.5 * min(1, up / down) * rolloff        cycles per INPUT sample: below both Nyquist limits
        g[q] = 2 fc sinc(2 fc (q - (Q - 1) / 2) / up) * kaiser(Q, 0.1102 (att - 8.7))[q]
    Every phase has unit gain at DC (to the window's ripple); the delay is (Q - 1) / (2 up) input samples."""
    up, down, T = int(up), int(down), int(taps)
    if up < 1 or down < 1 or T < 1:
        raise ValueError("up, down and taps must be >= 1, got %d, %d, %d" % (up, down, T))
    if not 0.0 < rolloff <= 1.0:
        raise ValueError("rolloff must be in (0, 1], got %g" % rolloff)
    if att <= 8.7:
        raise ValueError("att must be > 8.7 dB (the Kaiser formula's range), got %g" % att)
    Q = up * T
    fc = 0.5 * min(1.0, up / down) * float(rolloff)
    q = np.arange(Q, dtype=np.float64) - (Q - 1) / 2.0
    g = 2.0 * fc * np.sinc(2.0 * fc * q / up) * np.kaiser(Q, 0.1102 * (float(att) - 8.7))
    return np.ascontiguousarray(g.reshape(T, up).T, dtype=np.float32)


def advance_state(o, phi, S, up, down):
    """The definition's integer arithmetic in Python ints: state (o, phi) before a call on S stream samples -> (count, o', phi')."""
    count = -((-((S - o) * up - phi)) // down) if o < S else 0
    A = phi + count * down
    return count, o + A // up - S, A % up


class AudioOut(CarriedFrame):
    """Rational rate conversion of beams, `rate_in` (default config.SAMPLE_RATE) -> `rate_out` Hz, by design_resampler(taps, att,
    rolloff).  `hop`: the owner's hop (None: the windows are back to back, every sample of every window is stream).  `rows`: beams
    per window (None: the first push decides, and allocates; give it where the first push is captured into a graph).  `pcm`: also
    produce int16.  `gain`: one float32 multiply on every sample, before the PCM conversion (MIC_GAIN / n for raw beams).
    Device state: `state` int32 [4] (the phase), `clip` int32 [rows] (PCM samples that left the range, a meter that adds up until
    reset), `count` int32 [2] (the last push's count and status), and the carried window: the last window pushed, silence before
    the first, updated in place (CarriedFrame's discipline) so that a captured graph's addresses stay valid.  `last_count` is the
    host's mirror of count[0], advanced by push with the same integer arithmetic -- slice with it without a sync; under graph
    replay only `count` on the device is authoritative.  `delay`: the filter's delay in input samples."""
    _ROWS = ("B", 1)

    def __init__(self, rate_out=48000, rows=None, hop=None, taps=32, att=80.0, rolloff=0.9, rate_in=None, pcm=True, gain=1.0, device="cuda"):
        torch = _torch()
        self.up, self.down = rate_ratio(rate_out, rate_in)
        if self.up > MAX_PHASES:
            raise ValueError("rate_out / rate_in = %d / %d: more than %d phases" % (self.up, self.down, MAX_PHASES))
        if self.down > 64 * self.up:
            raise ValueError("rate_out / rate_in = %d / %d: decimation by more than 64" % (self.up, self.down))
        self.taps = design_resampler(self.up, self.down, taps, att, rolloff)
        self.T = self.taps.shape[1]
        if self.T > MAX_TAPS or self.up * self.T > 1 << 20:
            raise ValueError("a table of %d x %d taps is too large (taps <= %d, up * taps <= %d)" % (self.up, self.T, MAX_TAPS, 1 << 20))
        self.hop = 0 if hop is None else int(hop)
        if self.hop < 0:
            raise ValueError("hop must be >= 1 (None: back-to-back windows), got %d" % self.hop)
        self.gain, self.want_pcm, self.device = float(gain), bool(pcm), device
        self.delay = (self.up * self.T - 1) / (2.0 * self.up)
        self.d_taps = torch.from_numpy(self.taps).to(device)
        self.state = torch.zeros(4, dtype=torch.int32, device=device)
        self.count = torch.zeros(2, dtype=torch.int32, device=device)
        self.rows = None if rows is None else int(rows)
        self.clip = None if rows is None else torch.zeros(self.rows, dtype=torch.int32, device=device)
        # with `rows` the carried window exists now, for windows of N_SAMPLES: the first push may then be a captured one (an
        # allocation inside a capture would zero the window again on every replay)
        self._prev = None if rows is None else torch.zeros((self.rows, config.N_SAMPLES), dtype=torch.float32, device=device)
        self._started = False
        self._host = (0, 0)              # (o, phi): the host mirror of `state`
        self.last_count = 0

    def _frames(self, out):
        torch = _torch()
        if out.dim() != 3 or out.dtype != torch.float32 or not out.is_cuda or out.shape[0] < 1 or out.shape[1] < 1:
            raise ValueError("out must be a float32 cuda tensor [F, B, N], got %s %s" % (out.dtype, tuple(out.shape)))
        F, B, N = out.shape
        if self.rows is not None and B != self.rows:
            raise ValueError("this AudioOut converts %d rows, out has %d" % (self.rows, B))
        if self._prev is not None and tuple(self._prev.shape) != (B, N) and not self._started:
            self._prev = None             # nothing pushed yet: the stream takes the layout of its first window
        if self._prev is not None and tuple(self._prev.shape) != (B, N):
            raise ValueError("the carried window is %s, out's windows are %s: a stream keeps its layout" % (tuple(self._prev.shape), (B, N)))
        if self.hop > N:
            raise ValueError("hop = %d > N = %d" % (self.hop, N))
        if self.T - 1 > (self.hop or N):
            raise ValueError("taps - 1 = %d samples of history but a window adds %d to the stream" % (self.T - 1, self.hop or N))
        return out.contiguous()

    def push(self, out):
        """out float32 cuda [F, B, N] as listen() returns it -> (audio float32 [B, cap], pcm int16 [cap, B] or None, count): the last
        `hop` samples of every window converted, behind the previous push's last window.  Enqueue only: the two launches, then the
        stream-ordered copy of out[-1] into the carried window.  audio[:, :count[0]] and pcm[:count[0]] are the samples, the rest of
        the cap slots are zero; `last_count` is count[0] on the host."""
        torch = _torch()
        x = self._frames(out)
        F, B, N = x.shape
        if self.rows is None:
            self.rows = B
            self.clip = torch.zeros(B, dtype=torch.int32, device=self.device)
        if self._prev is None:
            self._prev = torch.zeros((B, N), dtype=torch.float32, device=self.device)      # silence before the stream
        S = F * (self.hop or N)
        cap = _entry("bf_resample_capacity")(S, self.up, self.down)
        audio = torch.empty((B, cap), dtype=torch.float32, device=self.device)
        pcm = torch.empty((cap, B), dtype=torch.int16, device=self.device) if self.want_pcm else None
        call("bf_resample_device", x.data_ptr(), B, F, N, N, self.hop, self._prev.data_ptr(), self.d_taps.data_ptr(), self.up, self.down, self.T,
             self.state.data_ptr(), self.gain, audio.data_ptr(), cap, None if pcm is None else pcm.data_ptr(), self.clip.data_ptr(), self.count.data_ptr())
        self._started = True
        self._prev.copy_(x[-1])           # in place: the address a captured graph reads stays valid
        self.last_count, o, phi = advance_state(self._host[0], self._host[1], S, self.up, self.down)
        self._host = (o, phi)
        return audio, pcm, self.count

    def push_flat(self, x):
        """x float32 cuda [B, S], the next S samples of every row's stream (the same S every time) -> as push."""
        if x.dim() != 2:
            raise ValueError("x must be [B, S], got %s" % (tuple(x.shape),))
        if self.hop:
            raise ValueError("push_flat takes whole blocks of a stream: this AudioOut has hop = %d" % self.hop)
        return self.push(x.unsqueeze(0))

    def advance(self, d_frames):
        raise NotImplementedError("AudioOut.push carries its own window")

    def reset(self):
        """A new stream: the state and the clip meter are zeroed and the carried window is dropped for silence -- zeroed in place, so
        a captured push stays valid and starts the new stream when it is replayed."""
        self.state.zero_()
        self.count.zero_()
        if self.clip is not None:
            self.clip.zero_()
        if self._prev is not None:
            self._prev.zero_()
        self._host, self.last_count = (0, 0), 0
