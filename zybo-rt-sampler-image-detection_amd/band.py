"""Band selection on the time-domain device path: band-limited frames, maps and beams.

Everything time-domain here is broadband, as in the reference, whose band limits (`threshold_freq_lower` / `_upper`) exist on the
frequency-domain side only.  On a 14 cm aperture the low end of the spectrum has no directivity and the MEMS DC offsets sit on
every microphone, so a broadband map is nearly flat.  Delay-and-sum is linear: ONE filter applied to every microphone row leaves
all inter-microphone delays intact, so a band-limited map is the existing map of filtered frames, and band-limited audio is the
same filter on the beams -- [F, B, N] rows, far fewer than the microphones.  `BandFilter` is that filter (bf_band_filter_device,
include/beamformer_hip.h has the definition): K bands in one launch, continuous across windows -- the T - 1 samples a window's
first outputs need come from the window before it, not from silence.

Recipes.
    BeamListener, independent windows:        bf = BandFilter([(3000, 8000)]);  maps = bf.maps(bl, d_frames)           # [K, F, D]
    StreamBeamformer sb, one band (K = 1):    bf = BandFilter([(3000, 8000)], hop=sb.hop)
                                              y = bf.frames(d_frames)[0]          # filtered windows of the same stream
                                              maps = sb.maps(y); out, st = sb.listen(y, offsets)
                                              bf.advance(d_frames); sb.advance(y)                                     # both objects
      With n_taps - 1 <= hop the filtered overlapping windows agree bit for bit where both exist, so they are the windows of one
      stream, the filtered one, and sb's carried frame (the last FILTERED window) is the filtered history.  For K > 1 loop over
      the bands with one StreamBeamformer each.
    Audio:                                    out, st = bl.listen(d_frames, offsets);  y = bf.beams(out)               # [K, F, B, N]
"""
import numpy as np

from carried import CarriedFrame, check_frames
from interface import config
from lib._native import _torch, call

MAX_BANDS = 16
_WINDOWS = {"hamming": np.hamming, "hann": np.hanning, "blackman": np.blackman, "rect": np.ones}


def design(bands, n_taps=65, window="hamming", fs=None):
    """Windowed-sinc FIRs, float32 [K, n_taps]: band k passes (f_lo, f_hi) in Hz.  f_lo <= 0 gives a low-pass, f_hi >= fs / 2 a
    high-pass (odd n_taps only: an even-length symmetric filter is zero at fs / 2).  Designed in float64 -- the ideal band-pass
    response 2 f_hi/fs sinc(2 f_hi/fs m) - 2 f_lo/fs sinc(2 f_lo/fs m), m = n - (n_taps - 1) / 2, times the window, scaled to
    unit gain at the middle of the band (0 for a low-pass, fs / 2 for a high-pass) -- and rounded once to float32."""
    fs = float(config.SAMPLE_RATE if fs is None else fs)
    T = int(n_taps)
    if T < 1:
        raise ValueError("n_taps must be >= 1, got %d" % T)
    if window not in _WINDOWS:
        raise ValueError("window must be one of %s" % sorted(_WINDOWS))
    bands = [(float(lo), float(hi)) for lo, hi in bands]
    if not bands:
        raise ValueError("bands is empty")
    m = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    w = np.asarray(_WINDOWS[window](T), dtype=np.float64)
    out = np.empty((len(bands), T), dtype=np.float64)
    for k, (lo, hi) in enumerate(bands):
        lo, hi = max(lo, 0.0), min(hi, fs / 2.0)
        if not lo < hi:
            raise ValueError("band %d: want 0 <= f_lo < f_hi and f_lo < fs / 2, got (%g, %g) at fs = %g" % (k, bands[k][0], bands[k][1], fs))
        if hi >= fs / 2.0 and lo > 0.0 and T % 2 == 0:
            raise ValueError("band %d reaches fs / 2: a high-pass needs an odd n_taps, got %d" % (k, T))
        a, b = 2.0 * lo / fs, 2.0 * hi / fs
        h = (b * np.sinc(b * m) - a * np.sinc(a * m)) * w
        centre = 0.0 if lo <= 0.0 else (1.0 if hi >= fs / 2.0 else 0.5 * (a + b))       # in units of fs / 2
        gain = abs(np.sum(h * np.exp(-1j * np.pi * centre * m)))
        out[k] = h / gain
    return out.astype(np.float32)


class BandFilter(CarriedFrame):
    """K FIR band filters of n_taps taps on the rows of device frame batches.  `bands`: list of (f_lo, f_hi) in Hz (see `design`), or
    `taps=` a ready float32 [K, T] array instead of a design.  `hop`: samples between the starts of consecutive frames, as given to
    the ingest and to StreamBeamformer (None: independent windows, every window starts from silence -- BeamListener's convention).
    With a hop the carried state is one unfiltered frame, the last one of the batch before: `advance` sets it, `reset` clears it,
    the filtering calls only read it."""
    _ROWS = ("R", 1)

    def __init__(self, bands=None, n_taps=65, hop=None, window="hamming", fs=None, device="cuda", taps=None):
        if (bands is None) == (taps is None):
            raise ValueError("give either bands or taps")
        if taps is None:
            h = design(bands, n_taps, window, fs)
        else:
            h = np.ascontiguousarray(taps, dtype=np.float32)
            if h.ndim == 1:
                h = h[None, :]
            if h.ndim != 2 or h.shape[1] < 1:
                raise ValueError("taps must be [K, T], got shape %s" % (h.shape,))
        K, T = h.shape
        N = config.N_SAMPLES
        if K < 1 or K > MAX_BANDS:
            raise ValueError("1 .. %d bands, got %d" % (MAX_BANDS, K))
        if T > N:
            raise ValueError("n_taps = %d > N_SAMPLES = %d" % (T, N))
        hop = 0 if hop is None else int(hop)
        if hop < 0 or hop > N:
            raise ValueError("hop must be in [1, N_SAMPLES = %d] (None: independent windows), got %d" % (N, hop))
        if hop > 0 and T - 1 > hop:
            raise ValueError("n_taps - 1 = %d samples of history do not fit hop = %d" % (T - 1, hop))
        self.taps, self.K, self.T, self.hop, self.device = h, K, T, hop, device
        self.d_taps = _torch().from_numpy(h).to(device)

    def _run(self, x, frames, rows, hop, prev_ptr):
        torch = _torch()
        out = torch.empty((self.K, frames, rows, config.N_SAMPLES), dtype=torch.float32, device=self.device)
        call("bf_band_filter_device", x.data_ptr(), rows, frames, hop, prev_ptr, self.d_taps.data_ptr(), self.T, self.K, out.data_ptr())
        return out

    def frames(self, d_frames):
        """d_frames float32 cuda [F, R, N_SAMPLES] -> [K, F, R, N_SAMPLES]: every row filtered by every band; with a hop, frame f's
        history is frame f - 1, frame 0's the carried frame.  Does not change the carried state."""
        x = self._frames(d_frames)
        return self._run(x, x.shape[0], x.shape[1], self.hop, self._prev_ptr())

    def maps(self, bl, d_frames, dir_begin=0, dir_end=None):
        """Band-limited power maps [K, F, dir_end - dir_begin] of a BeamListener `bl`: filter, then ONE bl.maps call on the
        [K * F, R, N_SAMPLES] view of the filtered frames."""
        y = self.frames(d_frames)
        K, F, R, N = y.shape
        return bl.maps(y.view(K * F, R, N), dir_begin, dir_end).view(K, F, -1)

    def beams(self, out):
        """out float32 cuda [F, B, N_SAMPLES] from listen() -> [K, F, B, N_SAMPLES]: every beam filtered as one row, each window on
        its own (from silence): beams of independent windows have no common stream to continue."""
        x = check_frames(out, "out", *self._ROWS)
        F, B, N = x.shape
        return self._run(x, 1, F * B, 0, None).view(self.K, F, B, N)
