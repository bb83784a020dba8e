"""Multichannel post-filter gains for beams: the Wiener gain read from the microphones' coherence behind the steering.

`Enhancer` on its own sees only the beam and has to guess the noise from the beam's history: it takes the first frames as noise and a
steady interferer for noise ever after.  The array carries what one channel lacks.  Behind the steering to the look direction the target
is coherent across the microphones and sensor or diffuse noise is not; the classical multichannel post-filter (Zelinski 1988; Simmer's
variant) reads the Wiener gain from that per frame and bin, with no noise history and no learning stretch.  `SpatialPostFilter` makes
those gains on the Enhancer's own frame grid, for the slots a tracker names, on the device (bf_postfilter_device, include/beamformer_hip.h
has the definition), and `push` hands them to `Enhancer.push(gains=...)`, which does the synthesis.

    sb = StreamBeamformer("lerp", hop=128)
    pf = SpatialPostFilter.for_listener(sb, slots=B)                  # tau from lib.directions, mics / hop / offset_per_dir from sb
    en = Enhancer(rows=B, hop=sb.hop)
    out, st = sb.listen(d_frames, offsets_row)                       # [F, B, N_SAMPLES]
    clean, count, status = pf.push(en, d_frames, out, offsets_row)   # float32 [B, S]: the beams behind the post-filter, en.delay late
"""
import numpy as np

from enhance import FrameGrid, design_cola
from lib import _native as nat
from lib._native import _torch, call

MAX_SLOTS = 8
MAX_MICS = 256
DEN_MODES = {"mics": 0, "beam": 1}


class SpatialPostFilter:
    """Post-filter gains of `slots` look directions over the microphone rows `mics` of frames every `hop` samples (None: back-to-back
    windows).  tau float64 [D, M]: delays in samples per (direction, microphone), as the designers of filtersum.py take it (microphone m
    LEADS by tau[d][m]); a slot's offset names direction offset / offset_per_dir.  Frames of n_fft samples every hop_s under `window`
    (default: design_cola's win_a, the Enhancer's); numerator and denominator smoothed with `beta` (0: none), gains floored at `g_min`.
    den "mics": Zelinski's denominator, the microphones' mean power -- suppresses most, over-suppresses at low SNR; "beam": Simmer's,
    the beam's power -- gentler on the target, and blind to a coherent interferer, which is in the beam.  `lag`: read the microphones
    that many samples late, for beams that are themselves late (a FilterSumListener's (T - 1) / 2).
    Device state, allocated once and updated in place so that a captured graph's addresses stay valid: `state` int32 [2 + slots], `hist`
    float32 [M, n_fft - 1 + lag], `num` and `den` float32 [slots, n_fft / 2 + 1], `steer` float32 [slots, M, n_fft / 2 + 1, 2] (the
    steering of the last call), `status` int32 [slots], `count` int32 [2].  `last_count` is the host's mirror of count[0]."""

    def __init__(self, tau, mics, slots, offset_per_dir, hop, m_total=None, n_fft=256, hop_s=128, beta=0.8, g_min=0.1, den="mics", lag=0, window=None,
                 device="cuda"):
        torch = _torch()
        self.grid = FrameGrid(n_fft, hop_s, hop, device)
        self.n_fft, self.hop_s, self.n_bins, self.hop = self.grid.n_fft, self.grid.hop_s, self.grid.n_bins, self.grid.hop
        self.mics = np.ascontiguousarray(np.asarray(mics).astype(np.int32).ravel())
        self.n = int(self.mics.size)
        if self.n < 2 or self.n > MAX_MICS:
            raise ValueError("2 .. %d microphones, got %d" % (MAX_MICS, self.n))
        if isinstance(tau, torch.Tensor):
            if tau.dtype != torch.float64 or tau.dim() != 2:
                raise ValueError("tau must be float64 [D, M], got %s %s" % (tau.dtype, tuple(tau.shape)))
            self.d_tau = tau.to(device).contiguous()
        else:
            t = np.ascontiguousarray(tau, dtype=np.float64)
            if t.ndim != 2:
                raise ValueError("tau must be [D, M], got shape %s" % (t.shape,))
            self.d_tau = torch.from_numpy(t).to(device)
        if self.d_tau.shape[1] != self.n or self.d_tau.shape[0] < 1:
            raise ValueError("tau is for %d microphones, mics lists %d" % (self.d_tau.shape[1], self.n))
        self.n_dirs = int(self.d_tau.shape[0])
        self.slots, self.offset_per_dir = int(slots), int(offset_per_dir)
        if self.slots < 1 or self.slots > MAX_SLOTS:
            raise ValueError("1 .. %d slots, got %d" % (MAX_SLOTS, self.slots))
        if self.offset_per_dir < 1:
            raise ValueError("offset_per_dir must be >= 1, got %d" % self.offset_per_dir)
        self.m_total = None if m_total is None else int(m_total)
        if self.m_total is not None and (self.mics.min() < 0 or self.mics.max() >= self.m_total):
            raise ValueError("mics names a row outside frames of m_total = %d rows" % self.m_total)
        self.beta, self.g_min, self.lag = float(beta), float(g_min), int(lag)
        if not (0.0 <= self.beta < 1.0 and 0.0 <= self.g_min <= 1.0):
            raise ValueError("beta in [0, 1) and g_min in [0, 1] must hold")
        if self.lag < 0 or self.lag > self.n_fft:
            raise ValueError("lag must be in [0, n_fft = %d], got %d" % (self.n_fft, self.lag))
        if den not in DEN_MODES:
            raise ValueError("den must be 'mics' or 'beam', got %r" % (den,))
        self.den = den
        win = design_cola(self.n_fft, self.hop_s)[0] if window is None else np.ascontiguousarray(window, dtype=np.float32)
        if win.shape != (self.n_fft,):
            raise ValueError("window must hold n_fft = %d values" % self.n_fft)
        self.device = device
        self.d_window = torch.from_numpy(win).to(device)
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)
        self.state, self.count, self.status = z(2 + self.slots, torch.int32), z(2, torch.int32), z(self.slots, torch.int32)
        self.hist = z((self.n, self.n_fft - 1 + self.lag))
        self.num, self.den_state = z((self.slots, self.n_bins)), z((self.slots, self.n_bins))
        self.steer = z((self.slots, self.n, self.n_bins, 2))

    last_count = property(lambda self: self.grid.last_count)

    @classmethod
    def for_listener(cls, listener, slots=None, tau=None, offset_per_dir=None, **kw):
        """A post-filter for the beams of a BeamListener, a StreamBeamformer or a FilterSumListener: its microphone rows, its hop (a
        BeamListener has none: back-to-back windows), lag = the (T - 1) / 2 of a FilterSumListener's beams (0 for delay-and-sum), and
        where not given: slots = the listener's beams, offset_per_dir the listener's, tau the tensor a FilterSumListener.for_slots
        holds or lib.directions.calculate_delays() over the listener's microphones."""
        if tau is None:
            tau = getattr(listener, "d_tau", None)
        if tau is None:
            import lib.directions
            tau = np.asarray(lib.directions.calculate_delays(), dtype=np.float64).reshape(-1, listener.n)
        lag = 0
        if hasattr(listener, "T"):       # a FilterSumListener: linear-phase beams, (T - 1) / 2 samples late
            if listener.T % 2 == 0:
                raise ValueError("beams of %d taps are (T - 1) / 2 = %.1f samples late: no whole lag lines the frames up" % (listener.T, listener.delay))
            lag = (listener.T - 1) // 2
        if slots is None:
            slots = getattr(listener, "B", None)
        if slots is None:
            raise ValueError("slots is needed: a %s has no fixed number of beams" % type(listener).__name__)
        if offset_per_dir is None:
            offset_per_dir = getattr(listener, "offset_per_dir", None)
        if offset_per_dir is None:
            raise ValueError("offset_per_dir is needed: this listener was not built for slots")
        kw.setdefault("lag", lag)
        kw.setdefault("device", listener.device)
        return cls(tau, listener.mics, slots, offset_per_dir, getattr(listener, "hop", None) or None, **kw)

    def capacity(self, samples):
        """The frame slots of a call on `samples` stream samples: the second dimension of the gains (the Enhancer's)."""
        return self.grid.capacity(samples)

    def gains(self, d_frames, offsets_row, observe=False):
        """d_frames float32 cuda [F, M_total, N]; offsets_row int32 [slots] (a cuda tensor: one row of what SourceTracker.update or
        BeamListener.sources wrote; or host values) -> (gains float32 [slots, capacity(S), n_fft / 2 + 1], count int32 [2] = (frames
        completed, status), status int32 [slots]: 0 a source, 1 none -- its gains are zeros).  The gains are Enhancer.push's `gains` for
        the same frames.  observe: also return (num, den), the raw numerator and denominator of every (slot, frame, bin).  Enqueue only."""
        torch = _torch()
        if d_frames.dim() != 3 or d_frames.dtype != torch.float32 or not d_frames.is_cuda or min(d_frames.shape) < 1:
            raise ValueError("d_frames must be a float32 cuda tensor [F, M_total, N], got %s %s" % (d_frames.dtype, tuple(d_frames.shape)))
        x = d_frames.contiguous()
        F, m_total, N = x.shape
        if self.m_total is not None and m_total != self.m_total:
            raise ValueError("this post-filter takes frames of %d rows, d_frames has %d" % (self.m_total, m_total))
        S = self.grid.samples(F, N)
        offs = offsets_row if isinstance(offsets_row, torch.Tensor) else torch.as_tensor(np.asarray(offsets_row, dtype=np.int32))
        offs = offs.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(offs.shape) != (self.slots,):
            raise ValueError("offsets_row must hold %d entries, got shape %s" % (self.slots, tuple(offs.shape)))
        cap = self.capacity(S)
        work = self.grid.work("bf_postfilter_workspace", self.slots, "slots", S)
        shape = (self.slots, cap, self.n_bins)
        g = torch.empty(shape, dtype=torch.float32, device=self.device)
        num = torch.empty(shape, dtype=torch.float32, device=self.device) if observe else None
        den = torch.empty(shape, dtype=torch.float32, device=self.device) if observe else None
        call("bf_postfilter_device", x.data_ptr(), m_total, F, N, self.hop, nat.iptr(self.mics), self.n, self.d_tau.data_ptr(), self.n_dirs, offs.data_ptr(),
             self.slots, self.offset_per_dir, self.hist.data_ptr(), self.num.data_ptr(), self.den_state.data_ptr(), self.state.data_ptr(),
             self.d_window.data_ptr(), self.n_fft, self.hop_s, self.lag, DEN_MODES[self.den], self.beta, self.g_min, work.data_ptr(),
             self.steer.data_ptr(), g.data_ptr(), None if num is None else num.data_ptr(), None if den is None else den.data_ptr(), self.status.data_ptr(),
             self.count.data_ptr())
        self.grid.advance(S)
        return (g, self.count, self.status, num, den) if observe else (g, self.count, self.status)

    def push(self, en, d_frames, out, offsets_row):
        """The gains of d_frames for the slots of offsets_row, applied by en (an enhance.Enhancer with rows = slots) to the beams `out`
        float32 [F, slots, N] that a listener made of the same frames -> (clean float32 [slots, S], en's count int32 [2], status int32
        [slots]).  The two must walk one frame grid: the same n_fft, hop_s and hop, and the same position in the stream."""
        if en.grid.shape != self.grid.shape:
            raise ValueError("the Enhancer's frames (n_fft %d, hop_s %d, hop %d) are not the post-filter's (%d, %d, %d)" % (en.grid.shape + self.grid.shape))
        if en.grid.c != self.grid.c:
            raise ValueError("the Enhancer is %d samples behind its last frame end, the post-filter %d: they were not pushed together" % (en.grid.c, self.grid.c))
        g, _, status = self.gains(d_frames, offsets_row)
        clean, count = en.push(out, gains=g)
        return clean, count, status

    def reset(self):
        """A new stream: all carried state is zeroed in place, so a captured call stays valid and starts the new stream on replay."""
        for t in (self.state, self.count, self.hist, self.num, self.den_state):
            t.zero_()
        self.grid.reset()
