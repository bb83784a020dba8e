"""CPU: the host-side contract of bf_peaks_device (every argument is checked before device bring-up, so the refusals run without a
GPU), the Python front end without a GPU, and the NumPy restatement the GPU tests compare with (tests/peaks_np.py) against the
definition read aloud."""
import math

import numpy as np
import pytest

import peaks_np
from support import entry, FAKE, refused


_peaks = entry("bf_peaks_device", d_power=FAKE, frames=2, image_stride=60, rows=6, cols=10, radius=2, k=4, floor_rel=0.5, floor_abs=0.0,
               offset_per_dir=4, d_offsets=FAKE, d_values=FAKE, d_counts=FAKE)


def test_symbol_is_exported(native):
    assert hasattr(native.lib, "bf_peaks_device")


@pytest.mark.parametrize("kw,match", [
    (dict(d_power=None), "bf_peaks_device: d_power is null"),
    (dict(d_offsets=None), "bf_peaks_device: d_offsets is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(frames=-2), "frames = -2 < 1"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(cols=0), "cols = 0 < 1"),
    (dict(cols=-1), "cols = -1 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(k=0), "k = 0 < 1"),
    (dict(k=65), "k = 65 > 64"),
    (dict(radius=-1), "radius = -1 < 0"),
    (dict(rows=65536, cols=32768), r"rows \* cols = 2147483648 does not fit an int"),
    (dict(image_stride=59), r"image_stride = 59 < rows \* cols = 60"),
    (dict(rows=1, cols=3, image_stride=3, offset_per_dir=2 ** 30), r"\(rows \* cols - 1\) \* offset_per_dir = 2147483648 does not fit"),
    (dict(floor_rel=-0.25), r"floor_rel = -0.25 is not in \[0, 1\]"),
    (dict(floor_rel=1.5), r"floor_rel = 1.5 is not in \[0, 1\]"),
    (dict(floor_rel=math.nan), r"floor_rel = -?nan is not in \[0, 1\]"),
    (dict(floor_rel=math.inf), r"floor_rel = inf is not in \[0, 1\]"),
    (dict(floor_abs=math.inf), "floor_abs = inf is not finite"),
    (dict(floor_abs=-math.inf), "floor_abs = -inf is not finite"),
    (dict(floor_abs=math.nan), "floor_abs = -?nan is not finite"),
])
def test_peaks_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _peaks(native, **kw), match)


def test_valid_arguments_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only: with one, valid arguments would enqueue")
    refused(native, _peaks(native), "no usable HIP device")
    # the edges of every range pass the checks; the optional outputs may be null
    refused(native, _peaks(native, k=64, radius=0, floor_rel=0.0, floor_abs=-1e30, d_values=None, d_counts=None), "no usable HIP device")
    refused(native, _peaks(native, k=1, radius=2 ** 31 - 1, floor_rel=1.0, rows=1, cols=2, image_stride=2, offset_per_dir=2 ** 31 - 1), "no usable HIP device")
    refused(native, _peaks(native, rows=361, cols=361, image_stride=361 * 361), "no usable HIP device")


def test_sources_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only")
    import torch
    import listen
    import stream
    bl = listen.BeamListener("pad", mics=[0, 1, 2])
    with pytest.raises(native.BeamformerError, match="no usable HIP device"):
        bl.sources(torch.zeros((1, 12)), k=2, radius=1, shape=(3, 4))
    assert issubclass(stream.StreamBeamformer, listen.BeamListener) and stream.StreamBeamformer.sources is listen.BeamListener.sources


# ------------------------------------------------------------------ the restatement against the definition

def _tied_map(rng, rows, cols):
    """Integer levels 0..3 (plateaus and ties everywhere), 10 % NaN, 5 % +-inf."""
    img = rng.integers(0, 4, (rows, cols)).astype(np.float32)
    u = rng.uniform(0, 1, (rows, cols))
    img[u < 0.10] = np.nan
    img[(u >= 0.10) & (u < 0.125)] = np.inf
    img[(u >= 0.125) & (u < 0.15)] = -np.inf
    return img


@pytest.mark.parametrize("shape", [(11, 11), (13, 7), (1, 20), (20, 1)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("radius", [0, 1, 2, 3, 20])
def test_vectorised_candidates_equal_the_definition(shape, radius):
    rng = np.random.default_rng([shape[0], shape[1], radius])
    for _ in range(6):
        img = _tied_map(rng, *shape)
        got, want = peaks_np.candidates(img, radius), peaks_np.candidates_naive(img, radius)
        assert (got == want).all(), np.argwhere(got != want)[:4]
        assert not got[~np.isfinite(img)].any()
        sep = peaks_np.min_chebyshev(got)
        assert sep is None or sep > radius, (sep, radius)
        if radius == 0:
            assert (got == np.isfinite(img)).all()
        if radius >= max(shape):
            assert got.sum() == (1 if np.isfinite(img).any() else 0)


def test_consequences_of_the_definition():
    const = np.full((9, 5), 0.75, dtype=np.float32)
    for radius in (1, 2, 4, 50):
        c = peaks_np.candidates(const, radius)
        assert c.ravel()[0] and c[: radius + 1, : radius + 1].sum() == 1        # index 0, and nothing else near it
    assert peaks_np.candidates(const, 50).sum() == 1
    zeros = np.zeros((4, 4), dtype=np.float32); zeros[0, 0] = -0.0; zeros[2, 2] = -0.0
    assert np.flatnonzero(peaks_np.candidates(zeros, 4)).tolist() == [0]      # zeros of both signs tie: the first index wins
    nan = np.full((3, 3), np.nan, dtype=np.float32)
    assert not peaks_np.candidates(nan, 1).any()


def test_peaks_outputs():
    rng = np.random.default_rng(5)
    rows, cols, per = 12, 9, 7
    power = rng.uniform(0, 1, (3, rows * cols + 5)).astype(np.float32)
    power[:, rows * cols:] = 99.0                                              # past the map: never looked at
    power[1, :rows * cols] = np.nan
    power[2, 17] = np.inf
    offs, vals, cnt = peaks_np.peaks(power, rows, cols, 2, 4, 0.0, 0.0, per)
    naive = peaks_np.peaks(power, rows, cols, 2, 4, 0.0, 0.0, per, cand_fn=peaks_np.candidates_naive)
    for a, b in zip((offs, vals, cnt), naive):
        assert a.tobytes() == b.tobytes()
    img0 = power[0, :rows * cols]
    assert offs[0, 0] == int(np.argmax(img0)) * per and vals[0, 0] == img0.max()
    assert (np.diff(vals[0, :cnt[0, 0]]) <= 0).all()
    assert (offs[1] == -1).all() and (vals[1] == 0).all() and cnt[1].tolist() == [0, 0, rows * cols]
    assert cnt[2, 2] == 1 and 17 * per not in offs[2]
    # floor_rel 1: only entries equal to the top; a floor_abs above the top: nothing
    o1, v1, c1 = peaks_np.peaks(power[:1], rows, cols, 2, 4, 1.0, 0.0, per)
    assert c1[0].tolist() == [1, 1, 0] and o1[0, 0] == offs[0, 0] and (o1[0, 1:] == -1).all()
    o2, v2, c2 = peaks_np.peaks(power[:1], rows, cols, 2, 4, 0.0, 2.0, per)
    assert c2[0].tolist() == [0, 0, 0] and (o2 == -1).all()
    # k truncates the list: counts[1] still shows all kept candidates
    o3, _, c3 = peaks_np.peaks(power[:1], rows, cols, 0, 4, 0.0, 0.0, per)
    assert c3[0].tolist() == [4, rows * cols, 0]
    assert o3[0].tolist() == (np.argsort(-img0, kind="stable")[:4] * per).tolist()


def test_two_sources_on_the_oracle_map(oracle_lib):
    """The end-to-end case of tests/test_peaks.py on the CPU oracle's map (device maps are bit-identical to it): two plane waves at the
    as-shipped size give exactly two sources, (19, 21) and then (42, 8), and two empty slots."""
    import util
    from test_peaks import two_source_frame
    c = util.CONFIGS["shipped"]
    M, N, X, Y, T = c["M"], c["N"], c["X"], c["Y"], c["T"]
    img = oracle_lib.Oracle(N, X, Y, T).mimo_lerp(two_source_frame(), util.table_for("lerp", "shipped"), np.arange(M, dtype=np.int32)).ravel()
    offs, vals, cnt = peaks_np.peaks(img[None], X, Y, 4, 4, 0.25, 0.0, M)
    assert offs[0].tolist() == [(19 * Y + 21) * M, (42 * Y + 8) * M, -1, -1] and cnt[0].tolist() == [2, 2, 0]
    assert abs(vals[0, 0] - 0.1401) < 5e-5 and abs(vals[0, 1] - 0.0643) < 5e-5
