"""The front door of the device path: a stream of FPGA datagrams in, a batch of frames out, in one enqueue.

In the reference a receiver child turns one datagram per sample instant into the mic-major ring buffer (`receive_to_buffer`,
PC/src/receiver.c:94-151) after checking the first header (`receive_header_data`, receiver.c:224-239), and `get_data` zeroes the
dead microphones' rows on the way out (PC/src/api.c:830-859).  `PacketIngest` is the batched, device-resident form: datagrams
already in HBM (a replayed recording, a socket buffer copied over) -> float32 [F, m_total, N_SAMPLES] frames with overlapping
windows (`hop`), the dead rows zeroed and a per-frame header report, all from one kernel launch (bf_ingest_stream_device).  The
frames are what bf_das_device, listen.BeamListener and pipeline.FusedPipeline read.  `frames` only enqueues on the current torch
stream, so ingest, maps and beams can be captured as one graph.  Frame data is bit-identical to the reference's conversion."""
import numpy as np

from interface import config
from lib import _native as nat
from lib._native import _entry, _torch, call


def default_disabled_mics():
    """The 122 rows get_data zeroes (PC/src/api.c:835-851), from the library's one copy of the list."""
    fn = _entry("bf_default_disabled_mics")
    out = np.zeros(fn(None), dtype=np.int32)
    fn(nat.iptr(out))
    return out


class PacketIngest:
    """Frames of `n_arrays` 8 x 8 arrays (config.ROWS x config.COLUMNS) from protocol-v2 datagrams of the configured sizes.
    hop: datagrams between the starts of consecutive frames (None: N_SAMPLES, windows back to back); dead_mics: None, an iterable of
    rows to zero, or "reference" for get_data's list; m_total: rows per output frame (None: N_MICROPHONES; rows past
    n_arrays * ROWS * COLUMNS are zero)."""

    def __init__(self, n_arrays, hop=None, dead_mics=None, m_total=None, device="cuda"):
        self.n_arrays, self.device = int(n_arrays), device
        self.rows, self.columns = config.ROWS, config.COLUMNS
        self.n_samples, self.n_microphones = config.N_SAMPLES, config.N_MICROPHONES
        self.hop = self.n_samples if hop is None else int(hop)
        self.m_total = self.n_microphones if m_total is None else int(m_total)
        self.stride = 8 + 4 * self.n_microphones                     # sizeof(msg), receiver.h:51-59
        self.protocol_ver = int(config.FPGA_PROTOCOL_VERSION)
        mics_out = self.n_arrays * self.rows * self.columns
        if self.n_arrays < 1 or mics_out > self.n_microphones or mics_out > self.m_total:
            raise ValueError("n_arrays = %d: %d rows must fit N_MICROPHONES = %d and m_total = %d" % (self.n_arrays, mics_out, self.n_microphones,
                                                                                                     self.m_total))
        if self.hop < 1:
            raise ValueError("hop = %d < 1" % self.hop)
        # the row mask, built once: a non-zero byte zeroes that row of every frame (rows outside the frame are ignored, as get_data's are)
        self.mask = None
        if dead_mics is not None:
            if isinstance(dead_mics, str):
                if dead_mics != "reference":
                    raise ValueError("dead_mics must be None, an iterable of rows or \"reference\", got %r" % dead_mics)
                dead = default_disabled_mics()
            else:
                dead = np.asarray(list(dead_mics), dtype=np.int64).ravel()
                if dead.size and dead.min() < 0:
                    raise ValueError("dead_mics names row %d" % dead.min())
            self.mask = np.zeros(self.m_total, dtype=np.uint8)
            self.mask[dead[dead < self.m_total]] = 1
        self._d_mask = None

    def n_frames(self, n_datagrams):
        """How many whole frames a stream of n_datagrams holds: the largest F with (F - 1) * hop + N_SAMPLES <= n_datagrams."""
        n_datagrams = int(n_datagrams)
        return 0 if n_datagrams < self.n_samples else (n_datagrams - self.n_samples) // self.hop + 1

    def _datagrams(self, d_packets):
        """Shape check of a [T, stride] or flat uint8 tensor -> T."""
        import torch
        if (config.N_SAMPLES, config.N_MICROPHONES) != (self.n_samples, self.n_microphones):     # the library sizes its reads and writes by these
            raise ValueError("built for %d microphones x %d samples, but the configured sizes are now %d x %d: make a new PacketIngest"
                             % (self.n_microphones, self.n_samples, config.N_MICROPHONES, config.N_SAMPLES))
        if not isinstance(d_packets, torch.Tensor) or d_packets.dtype != torch.uint8 or d_packets.dim() not in (1, 2):
            raise ValueError("d_packets must be a uint8 tensor [T, %d] or flat, got %s %s" % (self.stride, getattr(d_packets, "dtype", type(d_packets)),
                                                                                             tuple(getattr(d_packets, "shape", ()))))
        if d_packets.dim() == 2 and d_packets.shape[1] != self.stride:
            raise ValueError("d_packets must be [T, %d] (8 + 4 * N_MICROPHONES bytes per datagram), got %s" % (self.stride, tuple(d_packets.shape)))
        if d_packets.dim() == 1 and d_packets.numel() % self.stride != 0:
            raise ValueError("a flat d_packets must hold whole datagrams of %d bytes, got %d bytes" % (self.stride, d_packets.numel()))
        T = d_packets.numel() // self.stride
        if self.n_frames(T) < 1:
            raise ValueError("%d datagrams do not fill one frame of N_SAMPLES = %d" % (T, self.n_samples))
        return T

    def frames(self, d_packets):
        """d_packets uint8 cuda [T, 8 + 4 * N_MICROPHONES] (or flat, that many bytes) -> (d_frames float32 [F, m_total, N_SAMPLES],
        status int32 [F, 4]) with F = n_frames(T); status[f] = (datagrams with another protocol version, datagrams with another
        n_arrays, counter steps != 1 inside the frame, counter of the first datagram)."""
        T = self._datagrams(d_packets)
        torch = _torch()
        if not d_packets.is_cuda:
            raise ValueError("d_packets must be a cuda tensor")
        packets = d_packets.contiguous()
        F = self.n_frames(T)
        if self.mask is not None and self._d_mask is None:
            self._d_mask = torch.from_numpy(self.mask).to(self.device)
        out = torch.empty((F, self.m_total, self.n_samples), dtype=torch.float32, device=self.device)
        status = torch.empty((F, 4), dtype=torch.int32, device=self.device)
        call("bf_ingest_stream_device", packets.data_ptr(), T, self.n_arrays, self.rows, self.columns, self.hop, F, self.m_total,
             None if self._d_mask is None else self._d_mask.data_ptr(), self.protocol_ver, out.data_ptr(), status.data_ptr())
        return out, status
