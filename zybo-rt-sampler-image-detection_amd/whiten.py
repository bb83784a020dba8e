"""The phase transform (SRP-PHAT) on the time-domain device path: whitened frames, maps and peaks.

Every power map here weighs a frequency by how loud it is, and the frames are short rectangular windows of raw microphone samples: a
loud narrow-band interferer (a fan, a hum, a motor's harmonics) owns the map and a quieter broadband source is a bump on its skirt.
`BandFilter` cures that only when the caller knows which band to cut.  The phase transform gives every in-band DFT bin of every
microphone unit magnitude and keeps its phase, so each frequency votes once, by its inter-microphone delays.  The weighting is per
row and zero-phase, so it leaves every delay intact: a PHAT map is the existing map of whitened frames, and `bl.maps`, `bl.sources`,
`bl.powers`, `CoarseToFine`, `SourceTracker` and `SensorFusion.focus` work on it unchanged.  It also makes the map independent of
each microphone's gain.  `Whitener` is that weighting (bf_whiten_device, include/beamformer_hip.h has the definition): K bands, each
with its own exponent beta in [0, 1] (0: a plain band-pass, 1: PHAT), in one launch.

    wh = Whitener([(1000, 12000)])                       # Hann window, beta = 1, floor_rel = 1e-3
    maps = wh.maps(bl, d_frames)                         # [K, F, D]
    offs, vals, cnt = bl.sources(maps[0], k=2)
    out, st = bl.listen(d_frames, offs[:, 0])            # the RAW frames at the offsets the whitened map gave

Listening.  Whitened frames are for maps, peaks and listed directions.  Whitened audio is noise-like (every bin is as loud as every
other), so `listen` takes the raw frames at the offsets the whitened map gave.

Streams.  The windows are whitened independently: each is windowed and weighted by its own spectrum, so whitened overlapping windows
are NOT the windows of one stream -- there is no `hop` and no carried state here.  With a `StreamBeamformer`, use a `BeamListener`'s
map of the whitened windows for localisation and the stream itself for audio.

The analysis window is not optional: with a rectangular window the leakage of strong low tones carries their near-zero phase
differences into every bin and the whitened map peaks at the grid centre.  That is why `window` is an argument and Hann the default.
"""
import math

import numpy as np

from carried import check_frames
from features import hann
from interface import config
from lib._native import _torch, call, fptr, gpu_available, iptr

MAX_BANDS = 16
MIN_N, MAX_N = 32, 4096


def band_bins(f_lo, f_hi, n, fs):
    """[lo, hi) of the n-point bins inside [f_lo, f_hi] Hz: lo = ceil(f_lo n / fs), at least 1 unless f_lo < 0 (DC is dropped by
    default); hi = floor(f_hi n / fs) + 1, capped at n / 2 + 1."""
    lo = int(math.ceil(f_lo * n / fs))
    lo = max(lo, 0) if f_lo < 0 else max(lo, 1)
    hi = min(int(math.floor(f_hi * n / fs)) + 1, n // 2 + 1)
    return lo, hi


def two_sided_bins(lo, hi, n):
    """How many of the n two-sided DFT bins the half-spectrum band [lo, hi) covers: bins 0 and n / 2 count once, the others twice."""
    return 2 * (hi - lo) - (1 if lo <= 0 < hi else 0) - (1 if lo <= n // 2 < hi else 0)


class Whitener:
    """K whitened bands of the rows of device frame batches.  `bands`: list of (f_lo, f_hi) or (f_lo, f_hi, beta) in Hz (see
    `band_bins`); `beta`: the exponent of the bands that give none (1: PHAT, 0: a plain band-pass).  `window`: "hann" (periodic,
    features.hann), "rect", or a float32 [N_SAMPLES] array.  `floor_rel`, `floor_abs`: a bin quieter than max(floor_abs, floor_rel *
    the band's rms magnitude) is divided by that floor instead of its own magnitude, so bins that hold only noise are not raised to
    unit weight; floor_abs = 0 keeps the output independent of each row's gain.  `gain`: one number or one per band; None gives
    N_SAMPLES / sqrt(the band's two-sided bin count), which is unit-RMS rows at beta = 1, so map values compare from band to band."""

    def __init__(self, bands, beta=1.0, window="hann", floor_rel=1e-3, floor_abs=0.0, gain=None, fs=None, device="cuda"):
        N = config.N_SAMPLES
        if N < MIN_N or N > MAX_N or N & (N - 1):
            raise ValueError("N_SAMPLES = %d is not a power of two in [%d, %d]" % (N, MIN_N, MAX_N))
        fs = float(config.SAMPLE_RATE if fs is None else fs)
        if not fs > 0:
            raise ValueError("fs must be > 0, got %g" % fs)
        bands = [tuple(float(v) for v in b) for b in bands]
        K = len(bands)
        if K < 1 or K > MAX_BANDS:
            raise ValueError("1 .. %d bands, got %d" % (MAX_BANDS, K))
        bins, betas = np.empty((K, 2), np.int32), np.empty(K, np.float32)
        for k, b in enumerate(bands):
            if len(b) not in (2, 3):
                raise ValueError("band %d: want (f_lo, f_hi) or (f_lo, f_hi, beta), got %r" % (k, b))
            bk = float(beta) if len(b) == 2 else b[2]
            if not 0.0 <= bk <= 1.0:
                raise ValueError("band %d: beta must be in [0, 1], got %g" % (k, bk))
            if not (math.isfinite(b[0]) and math.isfinite(b[1])):
                raise ValueError("band %d: the edges must be finite, got (%g, %g)" % (k, b[0], b[1]))
            lo, hi = band_bins(b[0], b[1], N, fs)
            if lo >= hi:
                raise ValueError("band %d: (%g, %g) Hz holds no bin of %d points at fs = %g (bins [%d, %d))" % (k, b[0], b[1], N, fs, lo, hi))
            bins[k], betas[k] = (lo, hi), bk
        for name, v in (("floor_rel", floor_rel), ("floor_abs", floor_abs)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError("%s must be finite and >= 0, got %g" % (name, v))
        if gain is None:
            g = np.array([N / math.sqrt(two_sided_bins(lo, hi, N)) for lo, hi in bins], dtype=np.float32)
        else:
            g = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float32), (K,)))
            if not np.isfinite(g).all():
                raise ValueError("gain must be finite, got %s" % (g,))
        if isinstance(window, str):
            if window not in ("hann", "rect"):
                raise ValueError("window must be 'hann', 'rect' or a float32 [%d] array, got %r" % (N, window))
            w = hann(N) if window == "hann" else None
        else:
            w = np.ascontiguousarray(window, dtype=np.float32)
            if w.shape != (N,):
                raise ValueError("window must be 'hann', 'rect' or a float32 [%d] array, got shape %s" % (N, w.shape))
        self.bins, self.beta, self.gain, self.window, self.K = bins, betas, g, w, K
        self.floor_rel, self.floor_abs, self.fs, self.device = float(floor_rel), float(floor_abs), fs, device
        # as BandFilter's taps, the window goes to the device here, so that no call -- a captured one included -- copies anything
        # (without a device the object still answers for its bins and gains; frames() then refuses like every device call)
        self.d_window = None if w is None or not gpu_available() else _torch().from_numpy(w).to(device)

    def frames(self, d_frames):
        """d_frames float32 cuda [F, R, N_SAMPLES] -> [K, F, R, N_SAMPLES]: every row whitened in every band, each window on its own."""
        torch = _torch()
        x = check_frames(d_frames, "d_frames", "R", 1)
        F, R, N = x.shape
        out = torch.empty((self.K, F, R, N), dtype=torch.float32, device=self.device)
        call("bf_whiten_device", x.data_ptr(), R, F, None if self.window is None else self.d_window.data_ptr(), iptr(self.bins), fptr(self.beta),
             fptr(self.gain), self.K, self.floor_rel, self.floor_abs, out.data_ptr())
        return out

    def maps(self, bl, d_frames, dir_begin=0, dir_end=None):
        """Whitened power maps [K, F, dir_end - dir_begin] of a BeamListener `bl`: whiten, then ONE bl.maps call on the
        [K * F, R, N_SAMPLES] view of the whitened frames."""
        y = self.frames(d_frames)
        K, F, R, N = y.shape
        return bl.maps(y.view(K * F, R, N), dir_begin, dir_end).view(K, F, -1)
