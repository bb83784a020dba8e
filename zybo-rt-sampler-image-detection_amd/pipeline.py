"""Fused acoustic heat-map -> overlay -> detection on one MI355X (BASELINE.json config 4).

Per batch of B (audio window, camera frame) pairs, everything stays in HBM:
  0. (step_packets) datagram stream -> the B windows                 bf_ingest_stream_device (csrc/ingest_kernel.hip)
  1. delay-and-sum power maps of the B windows                      bf_das_device           (csrc/das_pair.hip, das_kernels.hip)
  2. colourise, upscale to the camera size, temporal blend, overlay  bf_heatmap_*_device     (csrc/heatmap_kernels.hip)
  3. YOLOv5s-shaped detector on the overlaid frames                  PyTorch-ROCm module graph, convolutions = csrc/conv_kernels.hip
                                                                     (float32 like the reference's predict call; half=True: float16)
  4. head decode + NMS                                               bf_yolo_decode_device / bf_nms_device (csrc/nms_kernels.hip)
In the reference these are three processes joined by queues (beamformer producer, camera reader, YOLO worker; PC/src/
main.pyx:669-736) and the heat-map is blended onto the frame only for display (visual.py:450-455, sensorfusion/
decider.py:44-49); running the detector on the overlaid frame is this build's composition of the same pieces."""
import numpy as np

from interface import config
from lib import _native as nat
import visual
from image_detection.src.yolo_smooth_tracking import Detector


class FusedPipeline:
    def __init__(self, algo="lerp", size=640, device="cuda", half=False):
        import torch
        self.torch, self.device, self.size = torch, device, size
        self.algo = {"pad": nat.PAD, "lerp": nat.LERP}[algo]
        self.mics = None
        self.stream_state = visual.HeatmapStream(size, size, device)
        self.detector = Detector(device=device, half=half)

    def load_tables(self, delays, mics):
        """Steering tables once, as the reference's producer loops do before their frame loop (main.pyx:172-181)."""
        self.mics = np.ascontiguousarray(mics, dtype=np.int32)
        if self.algo == nat.PAD:
            t = np.ascontiguousarray(delays.astype(int).astype(np.int32)).ravel()
            nat.lib.load_coefficients_pad(nat.iptr(t), t.size)
        else:
            t = np.ascontiguousarray(np.float32(delays)).ravel()
            nat.lib.load_coefficients_lerp(nat.fptr(t), t.size)
        nat.check()

    def step(self, d_windows, d_camera, conf_thres=0.1):
        """d_windows float32 [B, N_MICROPHONES, N_SAMPLES]; d_camera uint8 [B, size, size, 3] (BGR).
        Returns (power maps [B, D], overlaid frames uint8 [B, size, size, 3], boxes [B, 300, 6], counts [B])."""
        t = self.torch
        B, D = d_windows.shape[0], config.MAX_RES_X * config.MAX_RES_Y
        power = t.empty((B, D), dtype=t.float32, device=self.device)
        s = t.cuda.current_stream().cuda_stream
        if nat.lib.bf_das_device(self.algo, d_windows.data_ptr(), d_windows.shape[1], power.data_ptr(), D, B, nat.iptr(self.mics), self.mics.size,
                                 0, D, s) != 0:
            nat.check()
        small, _ = self.stream_state.small_heatmaps(power)
        frames = self.stream_state.overlay(small, d_camera)
        boxes, counts = self.detector.detect(frames, conf_thres)
        return power, frames, boxes, counts

    def step_packets(self, d_packets, d_camera, ingest, conf_thres=0.1):
        """The same batch starting from the datagram stream: d_packets uint8 [T, 8 + 4 * N_MICROPHONES] -> ingest.frames (an
        ingest.PacketIngest: windows, dead-row mask, header report; one launch) -> step.  Returns step's tuple plus the ingest status
        int32 [B, 4]; d_camera holds one frame per window, B = ingest.n_frames(T)."""
        d_windows, status = ingest.frames(d_packets)
        return self.step(d_windows, d_camera, conf_thres) + (status,)

    def track(self, boxes, counts, tracker):
        """step's boxes and counts -> tracker.update (a boxtrack.BoxTracker): rows whose slot s is one object over time, which
        `focus` takes as boxes with counts None (tracks, ids, match, live, counts)."""
        return tracker.update(boxes, counts)

    def smooth(self, d_camera, boxes, counts, smoother):
        """The camera batch with step's boxes and counts -> smoother.update (a smooth.SmoothDetections): the reference's confidence
        hysteresis, low-score rows kept only where the previous frame's boxes are re-found in the image; its `out` feeds `track`
        and `focus` with counts None (out, boosted, counts, moved, score)."""
        return smoother.update(d_camera, boxes, counts)

    def focus(self, power, boxes, counts, fusion, sources=None):
        """step's power maps, boxes and counts -> fusion.focus (a fuse.SensorFusion) at this pipeline's frame size: per box the
        loudest direction under it as a table offset for listen(), per source of `sources` the box it lies in."""
        return fusion.focus(power, boxes, counts, sources=sources, image_size=(self.size, self.size))

    def audio_out(self, out, ao):
        """listen's beams [F, B, N_SAMPLES] -> ao.push (an audio_out.AudioOut): the beams at a sound card's rate, float32 and 16-bit PCM,
        continuous across batches (audio, pcm, count)."""
        return ao.push(out)

    def features(self, out, ao, bfeat):
        """listen's beams [F, B, N_SAMPLES] -> bfeat.push_from(ao, out) (a features.BeamFeatures behind an audio_out.AudioOut): the
        beams as spectral frames at the model's rate, log-mel or band levels, continuous across batches and without a host round
        trip (feat, count)."""
        return bfeat.push_from(ao, out)

    def enhance(self, out, en):
        """listen's beams [F, B, N_SAMPLES] -> en.push (an enhance.Enhancer): the beams' stream with its noise suppressed by short-time
        spectral gains, float32 [B, S], en.delay samples late and continuous across batches (clean, count); AudioOut.push_flat and
        BeamFeatures take it from there."""
        return en.push(out)

    def postfilter(self, frames, out, offsets, pf, en):
        """The frame batch [F, M_total, N_SAMPLES], listen's beams of it [F, B, N_SAMPLES] and the one row of B slot offsets they were
        steered by -> pf.push (a postfilter.SpatialPostFilter in front of an enhance.Enhancer with rows = B): the beams with the gains
        the microphones' coherence gives every (frame, bin), instead of the Enhancer's own noise tracker (clean, count, status)."""
        return pf.push(en, frames, out, offsets)

    def whiten(self, frames, whitener):
        """A frame batch [F, R, N_SAMPLES] -> whitener.frames (a whiten.Whitener): [K, F, R, N_SAMPLES], every in-band bin of every row
        at unit magnitude (the phase transform), for maps and peaks; listen on the raw frames at the offsets those maps give."""
        return whitener.frames(frames)
