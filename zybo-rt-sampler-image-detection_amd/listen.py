"""Steered audio beams on the device path (the MISO side of the reference's live modes).

In the reference a playback child runs `miso_pad` at the steered table offset once per window and scales the block by
`/ n * MIC_GAIN` (PC/src/api.c:491-543); the offset comes from a mouse click (`stear_miso_beam`, main.pyx:517-528) or from a
detection box (`focus_beam`, sensorfusion/decider.py:70-88).  `BeamListener` is the batched, device-resident form: windows
already in HBM (bf_ingest_device output, FusedPipeline's batch) -> the beams of every frame at any number of offsets in one
enqueue (bf_miso_device), and `loudest` aims one beam per frame at the frame's loudest direction of a power map without a
host round trip (bf_peak_offsets_device); `sources` gives up to k beams per frame, one per separated source of the map
(bf_peaks_device).  All only enqueue on the current torch stream, so maps, peaks and beams can be captured as one graph.  Raw beams (mic_gain 0) are bit-identical to the reference's miso_* calls."""
import numpy as np

from interface import config
from lib import _native as nat

ALGOS = {"pad": nat.PAD, "lerp": nat.LERP, "hybrid": nat.HYBRID, "fir_naive": nat.FIR_NAIVE, "fir_vec": nat.FIR_VEC}


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise nat.BeamformerError("no usable HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch


def _entry(name):
    fn = getattr(nat.lib, name, None)
    if fn is None:
        raise nat.BeamformerError("%s is missing from %s (a build older than the batched beam path)" % (name, nat.LIB_PATH))
    return fn


def _fail(what):
    """A -1 return: raise with the library's message."""
    nat.check()
    raise nat.BeamformerError("%s failed" % what)


class BeamListener:
    """Beams of the table loaded for `algo` (load_coefficients_* / lib.beamformer's loaders), over the microphone rows `mics`
    (default: lib.directions.active_microphones(), as lib.beamformer uses)."""

    def __init__(self, algo="pad", mics=None, device="cuda"):
        if algo not in ALGOS:
            raise ValueError("algo must be one of %s" % sorted(ALGOS))
        self.algo, self.device = algo, device
        if mics is None:
            from lib.directions import active_microphones
            mics, _ = active_microphones()
        self.mics = np.ascontiguousarray(np.asarray(mics).astype(np.int32).ravel())
        self.n = int(self.mics.size)
        # the table offset of direction d: d * n, or d * n * N_TAPS floats for the vectorized FIR (miso_convolve_vectorized)
        self.offset_per_dir = self.n * (config.N_TAPS if algo == "fir_vec" else 1)

    def _offsets(self, offsets, frames):
        torch = _torch()
        o = offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets, dtype=np.int32))
        o = o.to(device=self.device, dtype=torch.int32)
        if o.dim() == 1:
            o = o.unsqueeze(0).expand(frames, -1)
        if o.dim() != 2 or o.shape[0] != frames or o.shape[1] < 1:
            raise ValueError("offsets must be [B] or [%d, B], got %s" % (frames, tuple(o.shape)))
        return o.contiguous()

    def listen(self, d_frames, offsets, mic_gain=0.0):
        """d_frames float32 cuda [F, M_total, N_SAMPLES]; offsets [B] (every frame) or [F, B] table offsets ->
        (out float32 [F, B, N_SAMPLES], status int32 [F, B]: 0 ok, 1 offset outside the table, 2 fir_vec offset not a multiple
        of N_TAPS -- rejected beams are NaN).  mic_gain 0: raw beams; otherwise (beam / n) * mic_gain."""
        torch = _torch()
        if d_frames.dim() != 3 or d_frames.dtype != torch.float32 or not d_frames.is_cuda or d_frames.shape[2] != config.N_SAMPLES:
            raise ValueError("d_frames must be a float32 cuda tensor [F, M_total, %d], got %s %s" % (config.N_SAMPLES, d_frames.dtype, tuple(d_frames.shape)))
        frames = d_frames.contiguous()
        F, m_total, N = frames.shape
        offs = self._offsets(offsets, F)
        B = offs.shape[1]
        out = torch.empty((F, B, N), dtype=torch.float32, device=self.device)
        status = torch.empty((F, B), dtype=torch.int32, device=self.device)
        rc = _entry("bf_miso_device")(ALGOS[self.algo], frames.data_ptr(), m_total, F, nat.iptr(self.mics), self.n, offs.data_ptr(), B,
                                      float(mic_gain), out.data_ptr(), N, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _fail("bf_miso_device")
        return out, status

    def loudest(self, d_power):
        """d_power float32 cuda [F, D] power maps -> int32 cuda [F, 1]: the table offset of each map's loudest direction
        (np.argmax: first maximum, a NaN counts as the maximum), ready for listen()."""
        torch = _torch()
        if d_power.dim() != 2 or d_power.dtype != torch.float32 or not d_power.is_cuda:
            raise ValueError("d_power must be a float32 cuda tensor [F, D], got %s %s" % (d_power.dtype, tuple(d_power.shape)))
        power = d_power if d_power.stride(1) == 1 else d_power.contiguous()
        F, D = power.shape
        offs = torch.empty((F, 1), dtype=torch.int32, device=self.device)
        rc = _entry("bf_peak_offsets_device")(power.data_ptr(), F, power.stride(0), D, self.offset_per_dir, offs.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _fail("bf_peak_offsets_device")
        return offs

    def sources(self, d_power, k, radius, floor_rel=0.5, floor_abs=0.0, shape=None):
        """d_power float32 cuda [F, >= rows*cols] power maps, shape = (rows, cols) of a map (default (config.MAX_RES_X, config.MAX_RES_Y))
        -> (offsets int32 [F, k], values float32 [F, k], counts int32 [F, 3]): the k loudest directions of every map that are the
        maximum of their (2*radius+1)^2 window and reach max(floor_abs, floor_rel * the map's maximum), loudest first, as table
        offsets ready for listen(); empty slots hold -1 (listen: status 1, a NaN beam) and value 0.  counts: slots filled, candidates
        kept before k cut the list, non-finite entries of the map (never sources).  bf_peaks_device in include/beamformer_hip.h."""
        torch = _torch()
        if d_power.dim() != 2 or d_power.dtype != torch.float32 or not d_power.is_cuda:
            raise ValueError("d_power must be a float32 cuda tensor [F, D], got %s %s" % (d_power.dtype, tuple(d_power.shape)))
        rows, cols = (config.MAX_RES_X, config.MAX_RES_Y) if shape is None else (int(shape[0]), int(shape[1]))
        if d_power.shape[1] < rows * cols:
            raise ValueError("d_power rows hold %d entries, a %d x %d map needs %d" % (d_power.shape[1], rows, cols, rows * cols))
        power = d_power if d_power.stride(1) == 1 else d_power.contiguous()
        F = power.shape[0]
        k = int(k)
        offs = torch.empty((F, max(k, 0)), dtype=torch.int32, device=self.device)
        vals = torch.empty((F, max(k, 0)), dtype=torch.float32, device=self.device)
        counts = torch.empty((F, 3), dtype=torch.int32, device=self.device)
        # a row narrower than rows*cols is refused by the library (image_stride < rows * cols); a wider one is never read past the map
        stride = power.stride(0) if F > 1 else power.shape[1]
        rc = _entry("bf_peaks_device")(power.data_ptr(), F, stride, rows, cols, int(radius), k, float(floor_rel), float(floor_abs),
                                       self.offset_per_dir, offs.data_ptr(), vals.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            _fail("bf_peaks_device")
        return offs, vals, counts
