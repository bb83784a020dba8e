"""Coarse-to-fine localisation on the device path: scan a lattice of the grid, then only the windows around its peaks.

A power map costs one delay-and-sum per direction, and its consumers read a few cells of it.  `CoarseToFine` evaluates every
`step`-th direction of the grid (one shared-list bf_das_select_device call), takes the peaks of that coarse map
(bf_peaks_device), and evaluates the (2 radius + 1)^2 window of the FULL grid around every peak (one per-frame-list call): a few
per cent of the grid's directions.  Every value is the full map's value at that cell bit for bit, so wherever the coarse peaks
lead to the right windows the result is the full map's peak search.  Everything stays on the device and only enqueues on the
current torch stream; `locate` can be captured in a graph after one warm-up call."""
from interface import config
from lib._native import _torch


class CoarseToFine:
    """sb: a BeamListener or a StreamBeamformer (its table, microphones and, for a stream, its carried frame).  The lattice is every
    `step`-th cell from step // 2 on along both axes of the `shape` = (rows, cols) grid (default (config.MAX_RES_X,
    config.MAX_RES_Y)), in the grid's flat order d = x * cols + y as `sources(shape=...)` takes it; its offsets are uploaded once.
    `radius` (default `step`): half the side of the fine window.  `coarse_shape` = (Xc, Yc) is the lattice's own shape."""

    def __init__(self, sb, step, radius=None, shape=None):
        torch = _torch()
        self.sb, self.step = sb, int(step)
        self.radius = self.step if radius is None else int(radius)
        self.shape = (config.MAX_RES_X, config.MAX_RES_Y) if shape is None else (int(shape[0]), int(shape[1]))
        rows, cols = self.shape
        if self.step < 1 or self.radius < 0 or rows < 1 or cols < 1:
            raise ValueError("step must be >= 1, radius >= 0 and the grid not empty, got step %d radius %d shape %s" % (self.step, self.radius, self.shape))
        dev = sb.device
        self._xs = torch.arange(self.step // 2, rows, self.step, dtype=torch.int32, device=dev)
        self._ys = torch.arange(self.step // 2, cols, self.step, dtype=torch.int32, device=dev)
        self.coarse_shape = (int(self._xs.numel()), int(self._ys.numel()))
        self.lattice = ((self._xs[:, None] * cols + self._ys[None, :]) * sb.offset_per_dir).reshape(-1).contiguous()
        side = torch.arange(-self.radius, self.radius + 1, dtype=torch.int32, device=dev)
        self._dx = side.repeat_interleave(side.numel())       # the window in the grid's flat order: x outer, y inner
        self._dy = side.repeat(side.numel())

    def scan(self, d_frames):
        """d_frames float32 cuda [F, M_total, N_SAMPLES] -> coarse maps float32 [F, Xc * Yc]: the full map's values at the lattice."""
        return self.sb.powers(d_frames, self.lattice)[0]

    def windows(self, coarse_offsets):
        """coarse_offsets int32 [F, k] as sources() gives them on a coarse map (lattice index * offset_per_dir, -1: empty slot) ->
        int32 [F, k, W]: the full-grid table offsets of the window around every found lattice cell, -1 where the window leaves
        the grid and for empty slots."""
        torch = _torch()
        rows, cols = self.shape
        opd = self.sb.offset_per_dir
        found = coarse_offsets >= 0
        c = torch.div(coarse_offsets.clamp(min=0), opd, rounding_mode="floor").long()
        yc = self.coarse_shape[1]
        x = self._xs[torch.div(c, yc, rounding_mode="floor")][:, :, None] + self._dx
        y = self._ys[c % yc][:, :, None] + self._dy
        inside = found[:, :, None] & (x >= 0) & (x < rows) & (y >= 0) & (y < cols)
        return torch.where(inside, (x * cols + y) * opd, torch.full_like(x, -1)).to(torch.int32)

    def locate(self, d_frames, k, radius_c=1, floor_rel=0.5, floor_abs=0.0):
        """d_frames float32 cuda [F, M_total, N_SAMPLES] -> (offsets int32 [F, k], values float32 [F, k], counts int32 [F, 3]):
        the peaks of the coarse map -- sources(coarse, k, radius_c, floor_rel, floor_abs), whose counts these are --, each moved to
        the best cell of its fine window in bf_peaks_device's order (value descending, flat index ascending, non-finite never).
        offsets are table offsets of the full grid, ready for listen(), SourceTracker.update and retarget; an empty slot holds
        -1 and value 0.  Two coarse peaks may refine to the same cell: such duplicates are returned as they are.  No host
        synchronisation."""
        torch = _torch()
        sb, opd = self.sb, self.sb.offset_per_dir
        coarse = self.scan(d_frames)
        F = coarse.shape[0]
        k = int(k)
        c_offs, _, counts = sb.sources(coarse, k, radius_c, floor_rel, floor_abs, shape=self.coarse_shape)
        win = self.windows(c_offs)                                              # [F, k, W]
        W = win.shape[2]
        fine, _ = sb.powers(d_frames, win.reshape(F, k * W))
        side = 2 * self.radius + 1
        w_offs, w_vals, _ = sb.sources(fine.reshape(F * k, W), 1, 0, 0.0, 0.0, shape=(side, side))
        hit = w_offs >= 0
        w = torch.div(w_offs.clamp(min=0), opd, rounding_mode="floor").long()   # [F * k, 1]
        best = torch.gather(win.reshape(F * k, W), 1, w)
        offsets = torch.where(hit, best, torch.full_like(best, -1)).reshape(F, k)
        return offsets, w_vals.reshape(F, k), counts
