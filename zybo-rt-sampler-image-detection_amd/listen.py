"""Steered audio beams on the device path (the MISO side of the reference's live modes).

In the reference a playback child runs `miso_pad` at the steered table offset once per window and scales the block by
`/ n * MIC_GAIN` (PC/src/api.c:491-543); the offset comes from a mouse click (`stear_miso_beam`, main.pyx:517-528) or from a
detection box (`focus_beam`, sensorfusion/decider.py:70-88).  `BeamListener` is the batched, device-resident form: windows
already in HBM (bf_ingest_device output, FusedPipeline's batch) -> the beams of every frame at any number of offsets in one
enqueue (bf_miso_device), and `loudest` aims one beam per frame at the frame's loudest direction of a power map without a
host round trip (bf_peak_offsets_device); `sources` gives up to k beams per frame, one per separated source of the map
(bf_peaks_device).  `maps` makes the power maps themselves (bf_das_device), `powers` only their values at listed offsets
(bf_das_select_device), `remove` takes beams back out of the frames
(bf_remove_sources_device) and `separate` runs the two in a loop -- map, loudest direction, beam, subtract -- so that a source
under a stronger one's sidelobes is found and heard: time-domain CLEAN.  All only enqueue on the current torch stream, so maps,
peaks, beams and residuals can be captured as one graph.  Raw beams (mic_gain 0) are bit-identical to the reference's miso_* calls."""
import numpy as np

from carried import check_frames
from interface import config
from lib import _native as nat
from lib._native import _torch, call

ALGOS = {"pad": nat.PAD, "lerp": nat.LERP, "hybrid": nat.HYBRID, "fir_naive": nat.FIR_NAIVE, "fir_vec": nat.FIR_VEC}


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

    def _offsets(self, offsets, frames, shared=False):
        """[B] or [F, B] offsets, host or device -> int32 cuda [F, B]; shared: a [B] list stays [B] (one list for every frame)."""
        torch = _torch()
        o = offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets, dtype=np.int32))
        o = o.to(device=self.device, dtype=torch.int32)
        if o.dim() == 1:
            if shared and o.shape[0] >= 1:
                return o.contiguous()
            o = o.unsqueeze(0).expand(frames, -1)
        if o.dim() != 2 or o.shape[0] != frames or o.shape[1] < 1:
            raise ValueError("offsets must be [B] or [%d, B], got %s" % (frames, tuple(o.shape)))
        return o.contiguous()

    def listen(self, d_frames, offsets, mic_gain=0.0):
        """d_frames float32 cuda [F, M_total, N_SAMPLES]; offsets [B] (every frame) or [F, B] table offsets ->
        (out float32 [F, B, N_SAMPLES], status int32 [F, B]: 0 ok, 1 offset outside the table, 2 fir_vec offset not a multiple
        of N_TAPS -- rejected beams are NaN).  mic_gain 0: raw beams; otherwise (beam / n) * mic_gain."""
        torch = _torch()
        frames = check_frames(d_frames, min_frames=0)
        F, m_total, N = frames.shape
        offs = self._offsets(offsets, F)
        B = offs.shape[1]
        out = torch.empty((F, B, N), dtype=torch.float32, device=self.device)
        status = torch.empty((F, B), dtype=torch.int32, device=self.device)
        call("bf_miso_device", ALGOS[self.algo], frames.data_ptr(), m_total, F, nat.iptr(self.mics), self.n, offs.data_ptr(), B, float(mic_gain),
             out.data_ptr(), N, status.data_ptr())
        return out, status

    def powers(self, d_frames, offsets):
        """d_frames float32 cuda [F, M_total, N_SAMPLES]; offsets [B] (one list for every frame) or [F, B] table offsets as listen()
        takes them -> (power float32 [F, B], status int32 [F, B]): the power map's value at every listed offset, bit for bit what
        maps() writes for that direction, without the rest of the map (bf_das_select_device).  Status as listen(); a rejected
        offset -- the -1 of an empty sources() slot -- gives NaN."""
        return self._powers(check_frames(d_frames), offsets, "bf_das_select_device")

    def _powers(self, frames, offsets, entry, *stream_args):
        torch = _torch()
        F, m_total, N = frames.shape
        offs = self._offsets(offsets, F, shared=True)
        B = offs.shape[-1]
        power = torch.empty((F, B), dtype=torch.float32, device=self.device)
        status = torch.empty((F, B), dtype=torch.int32, device=self.device)
        call(entry, ALGOS[self.algo], frames.data_ptr(), m_total, F, *stream_args, nat.iptr(self.mics), self.n, offs.data_ptr(), B, int(offs.dim() == 2),
             power.data_ptr(), B, status.data_ptr())
        return power, status

    def loudest(self, d_power):
        """d_power float32 cuda [F, D] power maps -> int32 cuda [F, 1]: the table offset of each map's loudest direction
        (np.argmax: first maximum, a NaN counts as the maximum), ready for listen()."""
        torch = _torch()
        if d_power.dim() != 2 or d_power.dtype != torch.float32 or not d_power.is_cuda:
            raise ValueError("d_power must be a float32 cuda tensor [F, D], got %s %s" % (d_power.dtype, tuple(d_power.shape)))
        power = d_power if d_power.stride(1) == 1 else d_power.contiguous()
        F, D = power.shape
        offs = torch.empty((F, 1), dtype=torch.int32, device=self.device)
        call("bf_peak_offsets_device", power.data_ptr(), F, power.stride(0), D, self.offset_per_dir, offs.data_ptr())
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
        call("bf_peaks_device", power.data_ptr(), F, stride, rows, cols, int(radius), k, float(floor_rel), float(floor_abs), self.offset_per_dir,
             offs.data_ptr(), vals.data_ptr(), counts.data_ptr())
        return offs, vals, counts

    def maps(self, d_frames, dir_begin=0, dir_end=None):
        """d_frames float32 cuda [F, M_total, N_SAMPLES] -> power maps float32 [F, dir_end - dir_begin] of the flat direction range
        (default: the whole grid) through bf_das_device."""
        torch = _torch()
        frames = check_frames(d_frames)
        F, m_total, N = frames.shape
        D = config.MAX_RES_X * config.MAX_RES_Y
        dir_end = D if dir_end is None else int(dir_end)
        dir_begin = int(dir_begin)
        if dir_begin < 0 or dir_end > D or dir_begin >= dir_end:
            raise ValueError("bad direction range [%d, %d) of %d" % (dir_begin, dir_end, D))
        img = torch.empty((F, dir_end - dir_begin), dtype=torch.float32, device=self.device)
        call("bf_das_device", ALGOS[self.algo], frames.data_ptr(), m_total, img.data_ptr(), img.shape[1], F, nat.iptr(self.mics), self.n, dir_begin, dir_end)
        return img

    def remove(self, d_frames, offsets, d_beams, gain=1.0, out=None):
        """d_frames float32 cuda [F, M_total, N_SAMPLES]; offsets [B] or [F, B] as listen() takes them; d_beams float32 cuda [F, B, >= N_SAMPLES],
        the raw beams listen() gave at those offsets -> (residual float32 [F, M_total, N_SAMPLES], status int32 [F, B]): the frames with
        gain / n times every accepted beam, projected back onto the microphones by the adjoint of the delay, subtracted
        (bf_remove_sources_device; pad and lerp).  Rejected offsets (status 1) subtract nothing.  out=d_frames runs in place."""
        torch = _torch()
        frames = check_frames(d_frames)
        if out is None:
            out = torch.empty_like(frames)
        else:
            if out.shape != d_frames.shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or not d_frames.is_contiguous():
                raise ValueError("out must be a contiguous float32 cuda tensor shaped like a contiguous d_frames, got %s %s" % (out.dtype, tuple(out.shape)))
            frames = d_frames
        F, m_total, N = frames.shape
        offs = self._offsets(offsets, F)
        B = offs.shape[1]
        if d_beams.dim() != 3 or d_beams.dtype != torch.float32 or not d_beams.is_cuda or d_beams.shape[:2] != (F, B) or d_beams.shape[2] < N:
            raise ValueError("d_beams must be a float32 cuda tensor [%d, %d, >= %d], got %s %s" % (F, B, N, d_beams.dtype, tuple(d_beams.shape)))
        beams = d_beams.contiguous()
        status = torch.empty((F, B), dtype=torch.int32, device=self.device)
        call("bf_remove_sources_device", ALGOS[self.algo], frames.data_ptr(), m_total, F, nat.iptr(self.mics), self.n, offs.data_ptr(), B, beams.data_ptr(),
             beams.shape[2], float(gain), out.data_ptr(), status.data_ptr())
        return out, status

    def separate(self, d_frames, k, gain=1.0, floor_rel=0.0, floor_abs=0.0):
        """d_frames float32 cuda [F, M_total, N_SAMPLES] -> (offsets int32 [F, k], values float32 [F, k], beams float32 [F, k, N_SAMPLES],
        residual float32 [F, M_total, N_SAMPLES]): k rounds of map -> loudest direction -> beam -> subtract on a copy of the frames.
        beams[:, i] is source i heard with sources 0 .. i-1 already taken out of the microphones, values[:, i] its power in the map of
        that residual.  A frame whose map falls below max(floor_abs, floor_rel * its maximum) -- or has no finite entry -- stops: its
        slot holds offset -1, value 0 and a NaN beam, and nothing more is subtracted from it.  No host synchronisation."""
        torch = _torch()
        frames = check_frames(d_frames)
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1, got %d" % k)
        residual = frames.clone()
        F, m_total, N = residual.shape
        offsets = torch.empty((F, k), dtype=torch.int32, device=self.device)
        values = torch.empty((F, k), dtype=torch.float32, device=self.device)
        beams = torch.empty((F, k, N), dtype=torch.float32, device=self.device)
        rows, cols = config.MAX_RES_X, config.MAX_RES_Y
        for i in range(k):
            power = self.maps(residual)
            offs, vals, _ = self.sources(power, 1, max(rows, cols), floor_rel, floor_abs)    # that radius leaves the one global maximum
            beam, _ = self.listen(residual, offs)
            self.remove(residual, offs, beam, gain, out=residual)
            offsets[:, i:i + 1], values[:, i:i + 1], beams[:, i:i + 1] = offs, vals, beam
        return offsets, values, beams, residual
