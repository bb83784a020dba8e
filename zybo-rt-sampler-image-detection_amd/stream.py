"""Continuous-stream beams and maps on the device path: delays read the previous window.

Every other delay-and-sum entry point treats a window as if the world began at its first sample, as the reference does: a
microphone delayed by p samples gives nothing to the first p outputs of the window.  Concatenated windows therefore carry a
defect at every boundary (with the shipped tables the first 47 of every 256 samples are sums over a growing subset of the
microphones), and maps lose up to p / N of each microphone's energy.  The reference's own PC/TODO.md names the cure,
"read the last N samples of the previous signal"; `StreamBeamformer` is that for pad and lerp: windows that sit next to each
other in HBM (`PacketIngest.frames`, bf_ingest_stream_device) -> beams and maps in which the samples a delay reaches before
the start of frame f come from frame f - 1, and for the first frame of a batch from the last frame of the batch before it
(`advance`).  include/beamformer_hip.h has the definition; for samples at or past `history` the beams equal BeamListener's
bit for bit."""
from carried import CarriedBeams
from interface import config
from lib import _native as nat
from lib._native import _entry, _torch, call
from listen import ALGOS, BeamListener


class StreamBeamformer(CarriedBeams, BeamListener):
    """Beams and maps of one continuous stream, for the table loaded for `algo` ("pad" or "lerp") over the microphone rows `mics`
    (default as BeamListener).  `hop`: samples between the starts of consecutive frames, as given to the ingest (None: back to
    back, N_SAMPLES).  The carried state is one frame, the last one of the batch before: `advance` sets it, `reset` clears it
    (silence before the stream); `maps` and `listen` only read it."""

    def __init__(self, algo="pad", hop=None, mics=None, device="cuda"):
        if algo not in ("pad", "lerp"):
            raise ValueError("algo must be 'pad' or 'lerp': the FIR flavours read ahead of the window's end, which a causal stream cannot supply")
        super().__init__(algo, mics=mics, device=device)
        N = config.N_SAMPLES
        hop = N if hop is None else int(hop)
        if hop < 1 or hop > N:
            raise ValueError("hop must be in [1, N_SAMPLES = %d], got %d" % (N, hop))
        self.hop = hop

    @property
    def history(self):
        """Samples of the previous window the loaded table reaches (bf_stream_history): the calls want history <= hop."""
        h = _entry("bf_stream_history")(ALGOS[self.algo])
        if h < 0:
            raise nat.BeamformerError("bf_stream_history: the %s table is not loaded" % self.algo)
        return h

    def maps(self, d_frames, dir_begin=0, dir_end=None):
        """d_frames float32 cuda [F, M_total, N_SAMPLES] -> power maps float32 [F, dir_end - dir_begin] of the flat direction range
        (default: the whole grid).  Does not change the carried state."""
        torch = _torch()
        frames = self._frames(d_frames)
        F, m_total, N = frames.shape
        D = config.MAX_RES_X * config.MAX_RES_Y
        dir_end = D if dir_end is None else int(dir_end)
        dir_begin = int(dir_begin)
        if dir_begin < 0 or dir_end > D or dir_begin >= dir_end:
            raise ValueError("bad direction range [%d, %d) of %d" % (dir_begin, dir_end, D))
        img = torch.empty((F, dir_end - dir_begin), dtype=torch.float32, device=self.device)
        call("bf_das_stream_device", ALGOS[self.algo], frames.data_ptr(), m_total, img.data_ptr(), img.shape[1], F, self.hop, self._prev_ptr(),
             nat.iptr(self.mics), self.n, dir_begin, dir_end)
        return img

    def listen(self, d_frames, offsets, mic_gain=0.0):
        """As BeamListener.listen -> (out float32 [F, B, N_SAMPLES], status int32 [F, B]), every sample of every beam a sum over all
        microphones.  Does not change the carried state."""
        torch = _torch()
        frames = self._frames(d_frames)
        F, m_total, N = frames.shape
        offs = self._offsets(offsets, F)
        B = offs.shape[1]
        out = torch.empty((F, B, N), dtype=torch.float32, device=self.device)
        status = torch.empty((F, B), dtype=torch.int32, device=self.device)
        call("bf_miso_stream_device", ALGOS[self.algo], frames.data_ptr(), m_total, F, self.hop, self._prev_ptr(), nat.iptr(self.mics), self.n,
             offs.data_ptr(), B, float(mic_gain), out.data_ptr(), N, status.data_ptr())
        return out, status

    def powers(self, d_frames, offsets):
        """As BeamListener.powers -> (power float32 [F, B], status int32 [F, B]): the values maps() writes at the listed offsets
        (bf_das_select_stream_device).  Does not change the carried state."""
        return self._powers(self._frames(d_frames), offsets, "bf_das_select_stream_device", self.hop, self._prev_ptr())

    def remove(self, *args, **kwargs):
        raise NotImplementedError("StreamBeamformer.remove: stream beams read the previous window, and the adjoint BeamListener.remove applies is "
                                  "that of the zero-prefix delay: it does not match them")

    def separate(self, *args, **kwargs):
        raise NotImplementedError("StreamBeamformer.separate: stream beams read the previous window, and the adjoint BeamListener.remove applies is "
                                  "that of the zero-prefix delay: it does not match them")
