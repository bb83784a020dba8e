"""Detector boxes meet the acoustic map (the reference's PC/sensorfusion/decider.py: `focus_beam`, :70-88, steers the listening beam
at a detection box).

`FusedPipeline.step` returns power maps and boxes side by side; `SensorFusion.focus` relates them on the device.  For every box:
the part of the map it covers -- the nearest-cell inverse of the display path, colourise's flip and the overlay's half-pixel
upscale --, the loudest direction in it as a table offset `listen` takes, and the direction under its midpoint; for every source of
`sources` or `SourceTracker.update`: the best-scored box it lies in (bf_fuse_boxes_device in include/beamformer_hip.h holds the
definition).  It only enqueues on the current torch stream, so maps -> detector -> focus -> listen stays on the device and can be
captured as one graph:

    sf = SensorFusion(sb, image_size=(640, 640), conf=0.5)
    peak, power, center, rects, src_box, counts = sf.focus(d_maps, boxes, n_boxes, sources=track_offsets)
    out, status = sb.listen(d_frames, peak[:, :4])          # what the four best-scored detections sound like"""
from interface import config
from lib._native import _torch, call


class SensorFusion:
    """Boxes against the maps of `listener` (a BeamListener or StreamBeamformer; it supplies offset_per_dir and the device).
    image_size: (width, height) of the frames the boxes are in pixels of; conf: the score a row needs to count as a box (the
    decider's 0.5); shape: (rows, cols) of a map, default (config.MAX_RES_X, config.MAX_RES_Y) as in `sources`."""

    def __init__(self, listener, image_size=(640, 640), conf=0.5, shape=None):
        _torch()
        self.offset_per_dir, self.device = int(listener.offset_per_dir), listener.device
        self.image_size, self.conf = (int(image_size[0]), int(image_size[1])), float(conf)
        self.rows, self.cols = (config.MAX_RES_X, config.MAX_RES_Y) if shape is None else (int(shape[0]), int(shape[1]))

    def focus(self, d_power, boxes, n_boxes=None, sources=None, image_size=None):
        """d_power float32 cuda [F, >= rows*cols] power maps; boxes float32 cuda [F, max_boxes, 6] = x1, y1, x2, y2, score, cls and
        n_boxes int32 cuda [F] (or None: every row is a candidate) as `Detector.detect` returns them; sources int32 cuda [F, n_src]
        (n_src <= 64) offsets of `sources` / `SourceTracker.update`, or None ->
        (peak int32 [F, max_boxes]: the offset of the loudest finite cell under each box, -1 where there is none -- ready for listen();
         power float32 [F, max_boxes]: that cell's power, 0 beside a -1; center int32 [F, max_boxes]: the offset under the box's midpoint;
         rects int32 [F, max_boxes, 4] = xa, xb, ya, yb, the cells the box covers; src_box int32 [F, n_src]: the lowest row of a box
         that contains the source, -1 for none (None without sources); counts int32 [F, 3]: boxes, boxes with a peak, sources with a
         box).  image_size overrides the constructor's for this call."""
        torch = _torch()
        if d_power.dim() != 2 or d_power.dtype != torch.float32 or not d_power.is_cuda:
            raise ValueError("d_power must be a float32 cuda tensor [F, D], got %s %s" % (d_power.dtype, tuple(d_power.shape)))
        F = d_power.shape[0]
        if d_power.shape[1] < self.rows * self.cols:
            raise ValueError("d_power rows hold %d entries, a %d x %d map needs %d" % (d_power.shape[1], self.rows, self.cols, self.rows * self.cols))
        if boxes.dim() != 3 or boxes.dtype != torch.float32 or not boxes.is_cuda or boxes.shape[0] != F or boxes.shape[1] < 1 or boxes.shape[2] != 6:
            raise ValueError("boxes must be a float32 cuda tensor [%d, max_boxes, 6], got %s %s" % (F, boxes.dtype, tuple(boxes.shape)))
        if n_boxes is not None and (n_boxes.dim() != 1 or n_boxes.dtype != torch.int32 or not n_boxes.is_cuda or n_boxes.shape[0] != F):
            raise ValueError("n_boxes must be an int32 cuda tensor [%d], got %s %s" % (F, n_boxes.dtype, tuple(n_boxes.shape)))
        if sources is not None and (sources.dim() != 2 or sources.dtype != torch.int32 or not sources.is_cuda or sources.shape[0] != F
                                    or not 1 <= sources.shape[1] <= 64):
            raise ValueError("sources must be an int32 cuda tensor [%d, 1..64], got %s %s" % (F, sources.dtype, tuple(sources.shape)))
        power = d_power if d_power.stride(1) == 1 else d_power.contiguous()
        stride = power.stride(0) if F > 1 else power.shape[1]
        boxes = boxes.contiguous()
        B = boxes.shape[1]
        n_boxes = None if n_boxes is None else n_boxes.contiguous()
        src = None if sources is None else sources.contiguous()
        n_src = 0 if src is None else src.shape[1]
        w, h = self.image_size if image_size is None else (int(image_size[0]), int(image_size[1]))
        peak = torch.empty((F, B), dtype=torch.int32, device=self.device)
        value = torch.empty((F, B), dtype=torch.float32, device=self.device)
        center = torch.empty((F, B), dtype=torch.int32, device=self.device)
        rects = torch.empty((F, B, 4), dtype=torch.int32, device=self.device)
        src_box = None if src is None else torch.empty((F, n_src), dtype=torch.int32, device=self.device)
        counts = torch.empty((F, 3), dtype=torch.int32, device=self.device)
        call("bf_fuse_boxes_device", power.data_ptr(), F, stride, self.rows, self.cols, self.offset_per_dir, boxes.data_ptr(),
             None if n_boxes is None else n_boxes.data_ptr(), B, w, h, self.conf, None if src is None else src.data_ptr(), n_src, peak.data_ptr(),
             value.data_ptr(), center.data_ptr(), rects.data_ptr(), None if src_box is None else src_box.data_ptr(), counts.data_ptr())
        return peak, value, center, rects, src_box, counts
