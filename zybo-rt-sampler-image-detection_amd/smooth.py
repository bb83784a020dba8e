"""Confidence hysteresis backed by image evidence (the reference's image-detection/src/yolo_smooth_tracking.py: `process_video`,
:87-143, with `track_with_correlation`, :59-69).

Detections above conf_high are trusted.  A frame that has none keeps a low-score candidate (conf_low < score <= conf_high) only if
a box of the previous frame can be re-found in the current camera image: the previous image's patch around the box is located in
the current image's search area by normalised cross-correlation (bf_match_boxes_device, the packed byte dot product on gfx950), and
the candidate is boosted to conf_high if it overlaps the moved box -- or, as the reference has it, if ANY previous box correlated
above `corr`, wherever the candidate lies; corr > 1 switches that arm off (bf_smooth_boxes_device in include/beamformer_hip.h holds
both definitions).  `BoxTracker` bridges a missed detection by a Kalman prediction that looks at no pixel; this looks at the pixels.
Everything is enqueued on the current torch stream and stays on the device, so it can be captured in one graph after one warm-up
call:

    sm = SmoothDetections(slots=16)
    out, boosted, counts, moved, score = sm.update(d_camera, boxes, n_boxes)   # boxes, n_boxes as Detector.detect returns them
    tracks, *_ = bt.update(out, None)                                           # a zero score is not a box to BoxTracker / SensorFusion"""
from lib._native import _entry, _torch, call


class SmoothDetections:
    """slots: previous boxes carried from frame to frame (<= 64); conf_low, conf_high, iou, corr: the reference's 0.3, 0.7, 0.5 and 0.8;
    t_pct, s_pct: the template and search scales in percent (the reference's 1.2 and 1.5)."""

    def __init__(self, slots=16, conf_low=0.3, conf_high=0.7, iou=0.5, corr=0.8, t_pct=120, s_pct=150, device="cuda"):
        torch = _torch()
        self.slots, self.t_pct, self.s_pct = int(slots), int(t_pct), int(s_pct)
        self.conf_low, self.conf_high, self.iou, self.corr = float(conf_low), float(conf_high), float(iou), float(corr)
        self.device = torch.device(device)
        words = _entry("bf_smooth_state_words")(self.slots)
        if words < 0:
            raise ValueError("slots must be in [1, 64], got %d" % self.slots)
        # bf_smooth_boxes_device's d_state: word 0 = the number of previous boxes, then their rows (float32 by their bits)
        self.state = torch.zeros((words,), dtype=torch.int32, device=self.device)
        self.prev_image = None          # the last image seen, uint8 [H, W, 3]; allocated at the first call
        self.prev_valid = False         # ... and valid once a frame has been seen

    def reset(self):
        """Start a new stream: no previous boxes, no previous image."""
        self.state.zero_()
        self.prev_valid = False

    @staticmethod
    def _images(torch, d_images):
        if d_images.dim() != 4 or d_images.dtype != torch.uint8 or not d_images.is_cuda or d_images.shape[0] < 1 or d_images.shape[3] != 3:
            raise ValueError("images must be a uint8 cuda tensor [F, H, W, 3], got %s %s" % (d_images.dtype, tuple(d_images.shape)))
        return d_images.contiguous()

    def match(self, d_images, d_prev, boxes, n_boxes=None):
        """The plain call: d_images uint8 cuda [F, H, W, 3], d_prev uint8 cuda [H, W, 3] or None, boxes float32 cuda [F, max_boxes, >= 4]
        (positions in the previous image), n_boxes int32 cuda [F] or None -> (moved float32 [F, max_boxes, 4], score float32
        [F, max_boxes], shift int32 [F, max_boxes, 2], status int32 [F, max_boxes]: 0 matched, 1 not a box, 2 off the image, 3 flat
        template, 4 no previous image)."""
        torch = _torch()
        d_images = self._images(torch, d_images)
        F, H, W = d_images.shape[:3]
        if d_prev is not None:
            if d_prev.dtype != torch.uint8 or not d_prev.is_cuda or tuple(d_prev.shape) != (H, W, 3):
                raise ValueError("d_prev must be a uint8 cuda tensor [%d, %d, 3], got %s %s" % (H, W, d_prev.dtype, tuple(d_prev.shape)))
            d_prev = d_prev.contiguous()
        if boxes.dim() != 3 or boxes.dtype != torch.float32 or not boxes.is_cuda or boxes.shape[0] != F or boxes.shape[1] < 1 or boxes.shape[2] < 4:
            raise ValueError("boxes must be a float32 cuda tensor [%d, max_boxes, >= 4], got %s %s" % (F, boxes.dtype, tuple(boxes.shape)))
        if n_boxes is not None and (n_boxes.dim() != 1 or n_boxes.dtype != torch.int32 or not n_boxes.is_cuda or n_boxes.shape[0] != F):
            raise ValueError("n_boxes must be an int32 cuda tensor [%d], got %s %s" % (F, n_boxes.dtype, tuple(n_boxes.shape)))
        boxes = boxes.contiguous()
        B = boxes.shape[1]
        moved = torch.empty((F, B, 4), dtype=torch.float32, device=self.device)
        score = torch.empty((F, B), dtype=torch.float32, device=self.device)
        shift = torch.empty((F, B, 2), dtype=torch.int32, device=self.device)
        status = torch.empty((F, B), dtype=torch.int32, device=self.device)
        call("bf_match_boxes_device", d_images.data_ptr(), None if d_prev is None else d_prev.data_ptr(), F, H, W, boxes.data_ptr(), boxes.shape[2],
             None if n_boxes is None else n_boxes.contiguous().data_ptr(), B, self.t_pct, self.s_pct, moved.data_ptr(), score.data_ptr(), shift.data_ptr(),
             status.data_ptr())
        return moved, score, shift, status

    def update(self, d_camera, boxes, n_boxes=None):
        """d_camera uint8 cuda [F, H, W, 3], boxes float32 cuda [F, max_boxes, 6] and n_boxes int32 cuda [F] (or None) as
        `Detector.detect` returns them ->
        (out float32 [F, max_boxes, 6]: the rows with the hysteresis applied to their scores -- a kept row keeps its score or is
         raised to conf_high, every other row's score is 0 --; boosted int32 [F, max_boxes]; counts int32 [F, 4]: valid rows,
         candidates, boosted rows, kept rows dropped for want of a slot; moved float32 [F, slots, 4] and score float32 [F, slots]: where
         and how well the previous frame's kept boxes were re-found in frame f).
        Frames are taken in order and continue where the previous call stopped: per frame one match launch on the state's rows, then
        one smooth launch; the batch's last image is kept for the next call."""
        torch = _torch()
        d_camera = self._images(torch, d_camera)
        F, H, W = d_camera.shape[:3]
        if boxes.dim() != 3 or boxes.dtype != torch.float32 or not boxes.is_cuda or boxes.shape[0] != F or boxes.shape[1] < 1 or boxes.shape[2] != 6:
            raise ValueError("boxes must be a float32 cuda tensor [%d, max_boxes, 6], got %s %s" % (F, boxes.dtype, tuple(boxes.shape)))
        if n_boxes is not None and (n_boxes.dim() != 1 or n_boxes.dtype != torch.int32 or not n_boxes.is_cuda or n_boxes.shape[0] != F):
            raise ValueError("n_boxes must be an int32 cuda tensor [%d], got %s %s" % (F, n_boxes.dtype, tuple(n_boxes.shape)))
        if self.prev_image is None or tuple(self.prev_image.shape) != (H, W, 3):
            self.prev_image = torch.zeros((H, W, 3), dtype=torch.uint8, device=self.device)
            self.prev_valid = False
        boxes = boxes.contiguous()
        n_boxes = None if n_boxes is None else n_boxes.contiguous()
        B, S = boxes.shape[1], self.slots
        out = torch.empty((F, B, 6), dtype=torch.float32, device=self.device)
        boosted = torch.empty((F, B), dtype=torch.int32, device=self.device)
        counts = torch.empty((F, 4), dtype=torch.int32, device=self.device)
        moved = torch.empty((F, S, 4), dtype=torch.float32, device=self.device)
        score = torch.empty((F, S), dtype=torch.float32, device=self.device)
        status = torch.empty((F, S), dtype=torch.int32, device=self.device)
        state = self.state.data_ptr()
        for f in range(F):
            prev = d_camera[f - 1].data_ptr() if f > 0 else (self.prev_image.data_ptr() if self.prev_valid else None)
            call("bf_match_boxes_device", d_camera[f].data_ptr(), prev, 1, H, W, state + 16, 4, state, S, self.t_pct, self.s_pct, moved[f].data_ptr(),
                 score[f].data_ptr(), None, status[f].data_ptr())
            call("bf_smooth_boxes_device", boxes[f].data_ptr(), None if n_boxes is None else n_boxes[f:].data_ptr(), B, self.conf_low, self.conf_high, self.iou,
                 self.corr, S, moved[f].data_ptr(), score[f].data_ptr(), status[f].data_ptr(), state, out[f].data_ptr(), boosted[f].data_ptr(),
                 counts[f].data_ptr())
        self.prev_image.copy_(d_camera[F - 1])
        self.prev_valid = True
        return out, boosted, counts, moved, score
