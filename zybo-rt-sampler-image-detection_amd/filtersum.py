"""Filter-and-sum beams on the device path: null steering, and any fixed beamformer a caller brings along as taps.

Every other audio beam here is delay-and-sum, so a beam aimed at one talker still carries the other at sidelobe level -- and on a
14 cm aperture "sidelobe level" is a few dB.  Any fixed beamformer is a filter-and-sum: one FIR per (beam, microphone), then a sum
over the microphones (bf_filter_sum_device, include/beamformer_hip.h has the definition).  `design_lcmv` designs such filters on the
host in float64: unit response in the look direction, zero response in up to a few null directions, at every frequency bin of the
band (LCMV: linearly constrained minimum variance, for spatially white noise).  `FilterSumListener` runs them.

Recipe, two talkers:
    bl = BeamListener("lerp");  maps = bl.maps(d_frames);  offs, _, _ = bl.sources(maps, 2, radius)
    tau = lib.directions.calculate_delays().reshape(-1, bl.n)
    fs_ = FilterSumListener.cross_null(tau, offs[0].cpu().numpy(), bl.offset_per_dir, hop=hop)    # beam i: source i heard, the others nulled
    out = fs_.listen(d_frames);  fs_.advance(d_frames);  audio = fs_.audio(out)                    # delayed by fs_.delay samples

Limits of this step.  The design runs on the HOST: re-designing when a tracker moves a source is a host round trip.  Data-dependent
(MVDR) weights are not designed here; a caller who has them passes `taps=` to FilterSumListener.  A device-side designer and an
MVDR designer would reuse the kernel unchanged."""
import numpy as np

from interface import config
from lib import _native as nat
from listen import _entry, _fail, _torch

MAX_BEAMS = 16


def band_bins(n_taps, band, fs=None):
    """The bins k of the n_taps-point frequency grid, 0 <= k <= n_taps // 2, with k * fs / n_taps inside band = (f_lo, f_hi), inclusive."""
    fs = float(config.SAMPLE_RATE if fs is None else fs)
    T = int(n_taps)
    k = np.arange(T // 2 + 1)
    f = k * fs / T
    return k[(f >= float(band[0])) & (f <= float(band[1]))]


def design_lcmv(tau, look, nulls=None, n_taps=65, band=(3000.0, 8000.0), rho=0.95, fs=None):
    """Null-steering filter-and-sum taps by frequency sampling, designed in float64.

    tau   float64 [D, M]: delays in samples per (direction, active microphone) -- lib.directions.calculate_delays() reshaped.
          Microphone m LEADS by tau[d][m] (synth.s3_plane_wave), so the response of one beam's taps g [M, T] to a plane wave from
          d at w rad/sample is  H(w, d) = sum_m (sum_t g[m][t] e^{-jwt}) e^{+jw tau[d][m]}   (`response`).
    look  B flat direction indices, one beam each.
    nulls per beam a list of up to J direction indices (None: no nulls anywhere).
    ->    (taps float32 [B, M, T], kept bool [B, K, J]);  K = len(band_bins(n_taps, band, fs)), the in-band bins in ascending order.

    For every in-band bin k: w = 2 pi k / T, c_d[m] = e^{+jw tau[d][m]}, C = [c_look, kept nulls], target f = (e^{-jw(T-1)/2}, 0, ..),
    u = C (C^H C)^{-1} conj(f), gains G_k[m] = conj(u[m]): the minimum-norm gains with H(w, look) = e^{-jw(T-1)/2} and H(w, null) = 0.
    Bins outside the band are zero; the taps are the inverse real DFT of the G_k (which keeps the real part of a DC or Nyquist gain),
    rounded once to float32.  At a bin a null is DROPPED if |c^H c'| / M > rho against the look vector or a null already kept at
    that bin (tried in the order given): it cannot be told from them there, and forcing it would blow the white-noise gain up.
    `kept` reports the outcome; entries past a beam's own list are False.

    A beam's output is the look direction's signal delayed by (T - 1) / 2 samples and band-limited.  With no nulls the design is
    band-limited delay-and-sum with exact fractional delays."""
    fs = float(config.SAMPLE_RATE if fs is None else fs)
    tau = np.asarray(tau, dtype=np.float64)
    if tau.ndim != 2:
        raise ValueError("tau must be [D, M], got shape %s" % (tau.shape,))
    D, M = tau.shape
    T = int(n_taps)
    if T < 1:
        raise ValueError("n_taps must be >= 1, got %d" % T)
    look = [int(d) for d in np.asarray(look).ravel()]
    B = len(look)
    if B < 1:
        raise ValueError("look is empty")
    nulls = [[] for _ in look] if nulls is None else [[int(d) for d in np.asarray(row).ravel()] for row in nulls]
    if len(nulls) != B:
        raise ValueError("nulls must list the nulls of every beam: %d beams, %d lists" % (B, len(nulls)))
    for d in look + [d for row in nulls for d in row]:
        if d < 0 or d >= D:
            raise ValueError("direction %d is outside tau's %d directions" % (d, D))
    if not 0.0 < float(rho) <= 1.0:
        raise ValueError("rho must be in (0, 1], got %g" % rho)
    bins = band_bins(T, band, fs)
    if bins.size == 0:
        raise ValueError("no bin of the %d-point grid lies in the band (%g, %g) at fs = %g" % (T, band[0], band[1], fs))
    J = max([len(row) for row in nulls] + [0])
    kept = np.zeros((B, bins.size, J), dtype=bool)
    G = np.zeros((B, M, T // 2 + 1), dtype=np.complex128)
    for b in range(B):
        for i, k in enumerate(bins):
            w = 2.0 * np.pi * k / T
            cols = [np.exp(1j * w * tau[look[b]])]
            for j, d in enumerate(nulls[b]):
                c = np.exp(1j * w * tau[d])
                if all(abs(np.vdot(c, other)) / M <= rho for other in cols):
                    cols.append(c)
                    kept[b, i, j] = True
            C = np.stack(cols, axis=1)                                      # [M, 1 + kept nulls]
            f = np.zeros(C.shape[1], dtype=np.complex128)
            f[0] = np.exp(-1j * w * (T - 1) / 2.0)
            u = C @ np.linalg.solve(C.conj().T @ C, f.conj())
            G[b, :, k] = u.conj()
    taps = np.fft.irfft(G, n=T, axis=2)
    return np.ascontiguousarray(taps, dtype=np.float32), kept


def response(taps, tau_row, w):
    """H(w, d) of one beam in float64: taps [M, T], tau_row float64 [M] = tau[d], w rad/sample (a scalar or an array) -> complex, w's shape."""
    g = np.asarray(taps, dtype=np.float64)
    tau_row = np.asarray(tau_row, dtype=np.float64)
    if g.ndim != 2 or tau_row.shape != (g.shape[0],):
        raise ValueError("taps must be [M, T] and tau_row [M], got %s and %s" % (g.shape, tau_row.shape))
    w = np.asarray(w, dtype=np.float64)
    t = np.arange(g.shape[1], dtype=np.float64)
    flat = w.reshape(-1)
    per_mic = np.exp(-1j * flat[:, None] * t[None, :]) @ g.T                # [W, M]: sum_t g[m][t] e^{-jwt}
    h = np.sum(per_mic * np.exp(1j * flat[:, None] * tau_row[None, :]), axis=1)
    return h.reshape(w.shape) if w.ndim else complex(h[0])


class FilterSumListener:
    """B filter-and-sum beams over the microphone rows `mics` (default: lib.directions.active_microphones(), as BeamListener).
    `taps`: float32 [B, M, T], g[b][m][t] for microphone row mics[m] -- from `design_lcmv`, `cross_null`, or a caller's own design.
    `hop`: samples between the starts of consecutive frames, as given to the ingest (None: independent windows, every window starts
    from silence).  With a hop the carried state is one frame, the last one of the batch before: `advance` sets it, `reset` clears
    it, `listen` only reads it.  `.delay` is (T - 1) / 2, the delay of a design_lcmv beam in samples."""

    def __init__(self, taps, mics=None, hop=None, device="cuda"):
        g = np.ascontiguousarray(taps, dtype=np.float32)
        if g.ndim == 2:
            g = g[None]
        if g.ndim != 3 or g.shape[2] < 1:
            raise ValueError("taps must be [B, M, T], got shape %s" % (g.shape,))
        if mics is None:
            from lib.directions import active_microphones
            mics, _ = active_microphones()
        self.mics = np.ascontiguousarray(np.asarray(mics).astype(np.int32).ravel())
        self.n = int(self.mics.size)
        B, M, T = g.shape
        N = config.N_SAMPLES
        if B < 1 or B > MAX_BEAMS:
            raise ValueError("1 .. %d beams, got %d" % (MAX_BEAMS, B))
        if M != self.n:
            raise ValueError("taps are for %d microphones, mics lists %d" % (M, self.n))
        if T > N:
            raise ValueError("n_taps = %d > N_SAMPLES = %d" % (T, N))
        hop = 0 if hop is None else int(hop)
        if hop < 0 or hop > N:
            raise ValueError("hop must be in [0, N_SAMPLES = %d] (0 or None: independent windows), got %d" % (N, hop))
        if hop > 0 and T - 1 > hop:
            raise ValueError("n_taps - 1 = %d samples of history do not fit hop = %d" % (T - 1, hop))
        self.taps, self.B, self.T, self.hop, self.device = g, B, T, hop, device
        self.delay = (T - 1) / 2.0
        self.d_taps = _torch().from_numpy(g).to(device)
        self._prev = None
        self.dirs = self.kept = None                    # set by cross_null

    @classmethod
    def cross_null(cls, tau, offsets, offset_per_dir, mics=None, hop=None, device="cuda", **design):
        """One beam per valid source offset, every other valid source its null.  `offsets`: a HOST row of what BeamListener.sources /
        SourceTracker wrote; an entry is a source iff it is >= 0, a multiple of offset_per_dir and names one of tau's directions
        (the tracker's rule).  **design goes to design_lcmv (n_taps, band, rho, fs).  The listener's `.dirs` lists the beams'
        directions in the order of the valid offsets, `.kept` is design_lcmv's."""
        tau = np.asarray(tau, dtype=np.float64)
        step = int(offset_per_dir)
        if step < 1:
            raise ValueError("offset_per_dir must be >= 1, got %d" % step)
        dirs = [int(o) // step for o in np.asarray(offsets).ravel() if int(o) >= 0 and int(o) % step == 0 and int(o) // step < tau.shape[0]]
        if not dirs:
            raise ValueError("offsets holds no valid source")
        nulls = [[d for j, d in enumerate(dirs) if j != i] for i in range(len(dirs))]
        taps, kept = design_lcmv(tau, dirs, nulls, **design)
        self = cls(taps, mics=mics, hop=hop, device=device)
        self.dirs, self.kept = dirs, kept
        return self

    def _frames(self, d_frames):
        torch = _torch()
        if d_frames.dim() != 3 or d_frames.dtype != torch.float32 or not d_frames.is_cuda or d_frames.shape[2] != config.N_SAMPLES or d_frames.shape[0] < 1:
            raise ValueError("d_frames must be a float32 cuda tensor [F, M_total, %d], got %s %s" % (config.N_SAMPLES, d_frames.dtype, tuple(d_frames.shape)))
        frames = d_frames.contiguous()
        if self._prev is not None and self._prev.shape[0] != frames.shape[1]:
            raise ValueError("the carried frame has %d rows, d_frames %d: reset() before changing the frame layout" % (self._prev.shape[0], frames.shape[1]))
        return frames

    def listen(self, d_frames):
        """d_frames float32 cuda [F, M_total, N_SAMPLES] -> float32 [F, B, N_SAMPLES]; with a hop, frame f's history is frame f - 1,
        frame 0's the carried frame (silence without one).  Does not change the carried state."""
        torch = _torch()
        frames = self._frames(d_frames)
        F, m_total, N = frames.shape
        out = torch.empty((F, self.B, N), dtype=torch.float32, device=self.device)
        prev = self._prev if self.hop > 0 else None
        rc = _entry("bf_filter_sum_device")(frames.data_ptr(), m_total, F, self.hop, None if prev is None else prev.data_ptr(), nat.iptr(self.mics), self.n,
                                            self.d_taps.data_ptr(), self.T, self.B, out.data_ptr(), N, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _fail("bf_filter_sum_device")
        return out

    def advance(self, d_frames):
        """Done with this batch: keep a copy of its last frame as the history of the next batch's first frame."""
        frames = self._frames(d_frames)
        if self._prev is None:
            self._prev = frames[-1].clone()
        else:
            self._prev.copy_(frames[-1])      # in place: the address a captured graph reads stays valid

    def reset(self):
        """Forget the carried frame: the next batch starts a new stream (silence before it)."""
        self._prev = None

    def audio(self, out):
        """out [F, B, N_SAMPLES] from listen() -> [B, F * hop]: the last `hop` samples of every window joined, the gapless beams of the
        stream from sample N_SAMPLES - hop of the batch's first window on (StreamBeamformer.audio's convention)."""
        if self.hop < 1:
            raise ValueError("audio() joins the windows of a stream: this listener has no hop (independent windows)")
        if out.dim() != 3 or out.shape[2] != config.N_SAMPLES:
            raise ValueError("out must be [F, B, %d], got %s" % (config.N_SAMPLES, tuple(out.shape)))
        F, B, N = out.shape
        return out[:, :, N - self.hop:].permute(1, 0, 2).reshape(B, F * self.hop)
