"""Identity over time for the detector's boxes (the reference's image-detection/src/yolo_smooth_tracking.py:
`process_video_track_boxes_only`, :275-347, hands every frame's detections to SORT and passes on the tracked box with its id;
PC/sensorfusion/decider.py steers the listening beam at it).

`Detector.detect` orders a frame's rows by score, so row b of one frame and row b of the next need not be the same object, and a
one-frame false alarm takes a row.  `BoxTracker` turns those [F, max_boxes, 6] rows into [F, slots, 6] rows whose slot s follows ONE
object: SORT (Bewley et al. 2016) -- a constant-velocity Kalman filter per box, IoU association by the optimal assignment, max_age /
min_hits birth and death (bf_track_boxes_device in include/beamformer_hip.h holds the definition).  It runs as one HIP launch on
the current torch stream and carries its tracks in a device tensor from batch to batch, so detector -> box tracker -> focus -> listen
stays on the device and can be captured as one graph:

    bt = BoxTracker(slots=16)
    tracks, ids, match, live, counts = bt.update(boxes, n_boxes)        # boxes, n_boxes as Detector.detect returns them
    peak, *_ = sf.focus(d_maps, tracks)                                 # row s is ONE object over time; unreported slots give -1
    out, status = sb.listen(d_frames, peak[:, :4])"""
from lib._native import _entry, _torch, call


class BoxTracker:
    """slots: tracks held at once (<= 64); max_age: frames a track lives on without a detection; min_hits: consecutive updates before
    a track is reported (every track is reported while the stream is at most min_hits frames old); iou: the overlap a detection needs
    to continue a track -- SORT's defaults --; conf: the score a row needs to count as a detection (strictly above; the reference's
    0.1)."""

    def __init__(self, slots=16, max_age=1, min_hits=3, iou=0.3, conf=0.1, device="cuda"):
        torch = _torch()
        self.slots, self.max_age, self.min_hits, self.iou, self.conf = int(slots), int(max_age), int(min_hits), float(iou), float(conf)
        self.device = torch.device(device)
        words = _entry("bf_box_track_state_words")(self.slots)
        if words < 0:
            raise ValueError("slots must be in [1, 64], got %d" % self.slots)
        # the tracks, in bf_track_boxes_device's d_state layout (float fields by their bits): save and restore it to checkpoint
        self.state = torch.zeros((words,), dtype=torch.int32, device=self.device)

    def reset(self):
        """Forget every track; ids start at 1 and the frame count at 0 again."""
        self.state.zero_()

    def update(self, boxes, n_boxes=None):
        """boxes float32 cuda [F, max_boxes, 6] = x1, y1, x2, y2, score, cls (max_boxes <= 1024) and n_boxes int32 cuda [F] (or None:
        every row is a candidate) as `Detector.detect` returns them ->
        (tracks float32 [F, slots, 6]: a reported slot's tracked box with the score and class of the detection it took, zeros
         elsewhere -- `SensorFusion.focus` takes it as boxes with n_boxes None; ids int32 [F, slots], 0 = free; match int32
         [F, slots]: the row of boxes the slot took or was born from, -1 otherwise; live float32 [F, slots, 4]: the box of every
         live slot, coasting ones included; counts int32 [F, 4]: born, ended, dropped for want of a slot, rows ignored).
        Frames are taken in order and continue where the previous call stopped."""
        torch = _torch()
        if boxes.dim() != 3 or boxes.dtype != torch.float32 or not boxes.is_cuda or boxes.shape[0] < 1 or boxes.shape[1] < 1 or boxes.shape[2] != 6:
            raise ValueError("boxes must be a float32 cuda tensor [F, max_boxes, 6], got %s %s" % (boxes.dtype, tuple(boxes.shape)))
        F, B = boxes.shape[0], boxes.shape[1]
        if n_boxes is not None and (n_boxes.dim() != 1 or n_boxes.dtype != torch.int32 or not n_boxes.is_cuda or n_boxes.shape[0] != F):
            raise ValueError("n_boxes must be an int32 cuda tensor [%d], got %s %s" % (F, n_boxes.dtype, tuple(n_boxes.shape)))
        boxes = boxes.contiguous()
        n_boxes = None if n_boxes is None else n_boxes.contiguous()
        S = self.slots
        tracks = torch.empty((F, S, 6), dtype=torch.float32, device=self.device)
        ids = torch.empty((F, S), dtype=torch.int32, device=self.device)
        match = torch.empty((F, S), dtype=torch.int32, device=self.device)
        live = torch.empty((F, S, 4), dtype=torch.float32, device=self.device)
        counts = torch.empty((F, 4), dtype=torch.int32, device=self.device)
        call("bf_track_boxes_device", boxes.data_ptr(), None if n_boxes is None else n_boxes.data_ptr(), F, B, self.conf, S, self.iou, self.max_age,
             self.min_hits, self.state.data_ptr(), tracks.data_ptr(), ids.data_ptr(), match.data_ptr(), live.data_ptr(), counts.data_ptr())
        return tracks, ids, match, live, counts
