"""The window-stream contract's Python side: what a batch of windows must look like, and the one frame a stream carries from a
batch to the next.  A frame may continue the one before it by `hop` samples; the history of a batch's first frame is the last frame
of the batch before.  StreamBeamformer, BandFilter and FilterSumListener own such a frame."""
from interface import config
from lib._native import _torch


def check_frames(d_x, name="d_frames", rows="M_total", min_rows=0, min_frames=1):
    """d_x must be a float32 cuda tensor [F >= min_frames, R >= min_rows, N_SAMPLES] -> its contiguous form.  `name` and `rows`
    (the label of the middle dimension) word the refusal."""
    torch = _torch()
    if (d_x.dim() != 3 or d_x.dtype != torch.float32 or not d_x.is_cuda or d_x.shape[2] != config.N_SAMPLES or d_x.shape[0] < min_frames
            or d_x.shape[1] < min_rows):
        raise ValueError("%s must be a float32 cuda tensor [F, %s, %d], got %s %s" % (name, rows, config.N_SAMPLES, d_x.dtype, tuple(d_x.shape)))
    return d_x.contiguous()


class CarriedFrame:
    """Mixin: `_prev`, the last frame of the batch before ([rows, N_SAMPLES], None: silence before the stream).  `advance` sets it,
    `reset` clears it, everything else only reads it.  `_ROWS`: the label and the least count of a frame's rows."""
    _prev = None
    _ROWS = ("M_total", 0)

    def _frames(self, d_frames):
        frames = check_frames(d_frames, "d_frames", *self._ROWS)
        if self._prev is not None and self._prev.shape[0] != frames.shape[1]:
            raise ValueError("the carried frame has %d rows, d_frames %d: reset() before changing the frame layout" % (self._prev.shape[0], frames.shape[1]))
        return frames

    def _prev_ptr(self):
        """The carried frame's address for a launch (None: no history)."""
        return None if self._prev is None or self.hop < 1 else self._prev.data_ptr()

    def advance(self, d_frames):
        """Done with this batch: keep a copy of its last frame as the history of the next batch's first frame (which starts `hop`
        samples after that frame did)."""
        frames = self._frames(d_frames)
        if self._prev is None:
            self._prev = frames[-1].clone()
        else:
            self._prev.copy_(frames[-1])      # in place: the address a captured graph reads stays valid

    def reset(self):
        """Forget the carried frame: the next batch starts a new stream (silence before it)."""
        self._prev = None


class CarriedBeams(CarriedFrame):
    """... of an owner whose windows become beams: `audio` joins them."""

    def audio(self, out):
        """out [F, B, N_SAMPLES] from listen() -> [B, F * hop]: the last `hop` samples of every window joined, the gapless beams of the
        stream from sample N_SAMPLES - hop of the batch's first window on."""
        if self.hop < 1:
            raise ValueError("audio() joins the windows of a stream: this listener has no hop (independent windows)")
        if out.dim() != 3 or out.shape[2] != config.N_SAMPLES:
            raise ValueError("out must be [F, B, %d], got %s" % (config.N_SAMPLES, tuple(out.shape)))
        F, B, N = out.shape
        return out[:, :, N - self.hop:].permute(1, 0, 2).reshape(B, F * self.hop)
