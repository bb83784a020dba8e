"""Identity over time for the sources of a map (the reference's open item "Tracking + Prediction", PC/TODO.md; its unused filter is
PC/src/kf.hpp).

`BeamListener.sources` orders every window's sources loudest first, so slot b of one window and slot b of the next need not be the
same talker.  `SourceTracker` turns those [F, k] offsets into [F, slots] offsets whose slot s follows ONE source: a gated greedy
nearest-neighbour association, a constant-velocity Kalman filter per slot, coasting through dropouts and confirmation after
min_hits windows (bf_track_sources_device in include/beamformer_hip.h holds the definition).  It runs as one HIP launch on the
current torch stream and carries its tracks in a device tensor from batch to batch, so maps -> sources -> tracker -> listen stays on
the device and can be captured as one graph:

    tr = SourceTracker(sb, slots=4)
    src, _, _ = sb.sources(sb.maps(d_frames), k=4, radius=4, floor_rel=0.25)
    offsets, ids, pos, match, counts = tr.update(src)
    out, status = sb.listen(d_frames, offsets); audio = sb.audio(out)   # audio[b] now follows ONE source"""
from interface import config
from lib import _native as nat
from lib._native import _entry, _torch, call


class SourceTracker:
    """Tracks for the offsets `listener.sources` writes (listener: a BeamListener or StreamBeamformer; it supplies offset_per_dir and
    the device).  slots: tracks held at once (<= 64); gate: the largest distance, in map pixels, at which a detection continues a
    track; max_miss: windows a track coasts without a detection before it ends; min_hits: detections before a track's offset is
    reported; q, r: process and measurement noise of the filter (kf.hpp's 0.1); shape: (rows, cols) of a map, default
    (config.MAX_RES_X, config.MAX_RES_Y) as in `sources`."""

    def __init__(self, listener, slots=4, gate=3.0, max_miss=5, min_hits=3, q=0.1, r=0.1, shape=None):
        torch = _torch()
        self.offset_per_dir, self.device = int(listener.offset_per_dir), listener.device
        self.slots, self.gate, self.max_miss, self.min_hits, self.q, self.r = int(slots), float(gate), int(max_miss), int(min_hits), float(q), float(r)
        self.rows, self.cols = (config.MAX_RES_X, config.MAX_RES_Y) if shape is None else (int(shape[0]), int(shape[1]))
        words = _entry("bf_track_state_words")(self.slots)
        if words < 0:
            raise ValueError("slots must be in [1, 64], got %d" % self.slots)
        # the tracks, in bf_track_sources_device's d_state layout (float fields by their bits): save and restore it to checkpoint
        self.state = torch.zeros((words,), dtype=torch.int32, device=self.device)

    def reset(self):
        """Forget every track and start ids at 1 again."""
        self.state.zero_()

    def update(self, src_offsets):
        """src_offsets int32 cuda [F, k], the offsets of `sources` -> (offsets int32 [F, slots] ready for listen(): -1 where the slot
        has no confirmed track; ids int32 [F, slots], 0 = free; pos float32 [F, slots, 4] = x, y, vx, vy in map pixels; match int32
        [F, slots], the column of src_offsets the slot took or -1; counts int32 [F, 4]: born, ended, dropped for want of a slot,
        entries ignored).  Frames are taken in order and continue where the previous call stopped."""
        torch = _torch()
        if src_offsets.dim() != 2 or src_offsets.dtype != torch.int32 or not src_offsets.is_cuda:
            raise ValueError("src_offsets must be an int32 cuda tensor [F, k], got %s %s" % (src_offsets.dtype, tuple(src_offsets.shape)))
        src = src_offsets.contiguous()
        F, k = src.shape
        S = self.slots
        offsets = torch.empty((F, S), dtype=torch.int32, device=self.device)
        ids = torch.empty((F, S), dtype=torch.int32, device=self.device)
        pos = torch.empty((F, S, 4), dtype=torch.float32, device=self.device)
        match = torch.empty((F, S), dtype=torch.int32, device=self.device)
        counts = torch.empty((F, 4), dtype=torch.int32, device=self.device)
        call("bf_track_sources_device", src.data_ptr(), F, k, self.rows, self.cols, self.offset_per_dir, S, self.gate, self.max_miss, self.min_hits, self.q,
             self.r, self.state.data_ptr(), offsets.data_ptr(), ids.data_ptr(), pos.data_ptr(), match.data_ptr(), counts.data_ptr())
        return offsets, ids, pos, match, counts
