"""CPU: the host-side contract of bf_track_sources_device (every argument is checked before device bring-up, so the refusals run
without a GPU), the Python front end without a GPU, and the NumPy restatement the GPU tests compare with (tests/track_np.py): against
the reference's filter in float64 matrix form, and against what the definition promises about identity."""
import math

import numpy as np
import pytest

import track_np
from support import entry, FAKE, refused


_track = entry("bf_track_sources_device", d_offsets=FAKE, frames=2, k=4, rows=41, cols=23, offset_per_dir=4, slots=4, gate=3.0, max_miss=5,
               min_hits=3, q=0.1, r=0.1, d_state=FAKE, d_track_offsets=FAKE, d_track_ids=FAKE, d_track_pos=FAKE, d_match=FAKE, d_counts=FAKE)


def test_symbols_are_exported(native):
    assert hasattr(native.lib, "bf_track_sources_device") and hasattr(native.lib, "bf_track_state_words")


def test_state_words(native):
    native.lib.bf_clear_error()
    w = native.lib.bf_track_state_words
    assert w(1) == 16 and w(4) == 52 and w(64) == 772
    assert w(0) == -1 and w(65) == -1 and w(-3) == -1
    native.check()                                                             # the refusals of this one record no error
    assert [track_np.state_words(s) for s in (1, 64, 0, 65)] == [16, 772, -1, -1]


@pytest.mark.parametrize("kw,match", [
    (dict(d_offsets=None), "bf_track_sources_device: d_offsets is null"),
    (dict(d_state=None), "bf_track_sources_device: d_state is null"),
    (dict(d_track_offsets=None), "bf_track_sources_device: d_track_offsets is null"),
    (dict(frames=0), "bf_track_sources_device: frames = 0 < 1"),
    (dict(frames=-2), "frames = -2 < 1"),
    (dict(k=0), "k = 0 < 1"),
    (dict(k=65), "k = 65 > 64"),
    (dict(slots=0), "slots = 0 < 1"),
    (dict(slots=65), "slots = 65 > 64"),
    (dict(rows=0), "rows = 0 < 1"),
    (dict(cols=0), "cols = 0 < 1"),
    (dict(cols=-1), "cols = -1 < 1"),
    (dict(offset_per_dir=0), "offset_per_dir = 0 < 1"),
    (dict(rows=65536, cols=32768), r"rows \* cols = 2147483648 does not fit an int"),
    (dict(rows=1, cols=3, offset_per_dir=2 ** 30), r"\(rows \* cols - 1\) \* offset_per_dir = 2147483648 does not fit"),
    (dict(gate=-0.5), r"gate = -0.5 is not finite and >= 0"),
    (dict(gate=math.inf), r"gate = inf is not finite and >= 0"),
    (dict(gate=math.nan), r"gate = -?nan is not finite and >= 0"),
    (dict(max_miss=-1), "max_miss = -1 < 0"),
    (dict(min_hits=0), "min_hits = 0 < 1"),
    (dict(q=-0.1), r"q = -0.1 is not finite and >= 0"),
    (dict(q=math.inf), r"q = inf is not finite and >= 0"),
    (dict(q=math.nan), r"q = -?nan is not finite and >= 0"),
    (dict(r=0.0), r"r = 0 is not finite and > 0"),
    (dict(r=-1.0), r"r = -1 is not finite and > 0"),
    (dict(r=math.inf), r"r = inf is not finite and > 0"),
    (dict(r=math.nan), r"r = -?nan is not finite and > 0"),
])
def test_track_argument_errors(native, kw, match):
    native.lib.bf_clear_error()
    refused(native, _track(native, **kw), match)


def test_valid_arguments_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only: with one, valid arguments would enqueue")
    refused(native, _track(native), "no usable HIP device")
    # the edges of every range pass the checks; the optional outputs may be null
    refused(native, _track(native, slots=64, k=64, gate=0.0, max_miss=0, min_hits=1, q=0.0), "no usable HIP device")
    refused(native, _track(native, d_track_ids=None, d_track_pos=None, d_match=None, d_counts=None), "no usable HIP device")
    refused(native, _track(native, slots=1, k=1, rows=1, cols=2, offset_per_dir=2 ** 31 - 1, r=1e-30, gate=1e30), "no usable HIP device")
    refused(native, _track(native, rows=361, cols=361, offset_per_dir=256 * 8), "no usable HIP device")


def test_tracker_without_gpu(native):
    if native.gpu_available():
        pytest.skip("without a GPU only")
    import listen
    import track
    bl = listen.BeamListener("pad", mics=[0, 1, 2])
    with pytest.raises(native.BeamformerError, match="no usable HIP device"):
        track.SourceTracker(bl, slots=4)


# ------------------------------------------------------------------ the restatement against the reference's filter

def _kf_hpp_float64(z, q=0.1, r=0.1):
    """PC/src/kf.hpp's update() in float64 matrix form (its A, Q, H, R; P0 = I), started at the first measurement instead of the
    origin -> [len(z), 6] states (x, y, z, vx, vy, vz) after each measurement."""
    A = np.eye(6)
    A[0, 3] = A[1, 4] = A[2, 5] = 1.0
    Q = q * np.eye(6)
    H = np.zeros((3, 6))
    H[0, 0] = H[1, 1] = H[2, 2] = 1.0
    R = r * np.eye(3)
    P = np.eye(6)
    x = np.zeros(6)
    x[:3] = z[0]
    out = [x.copy()]
    for m in z[1:]:
        x = A @ x
        P = A @ P @ A.T + Q
        S = H @ P @ H.T + R
        K = P @ H.T @ np.linalg.inv(S)
        x = x + K @ (m - H @ x)
        P = (np.eye(6) - K @ H) @ P
        out.append(x.copy())
    return np.array(out)


def test_restatement_against_the_reference_filter():
    """One track that is always matched, 361 x 361, 200 frames, q = r = 0.1: positions and velocities of the float32 restatement
    within 8 * 2^-24 * max(rows, cols) of the float64 matrix form.  About ten roundings per step at the coordinate's magnitude, and
    the gain damps earlier error; over these 20 seeded walks the worst difference measured 1.08 of the unit 2^-24 * 361 (printed)."""
    rows = cols = 361
    F, per = 200, 64
    unit = 2.0 ** -24 * max(rows, cols)
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        start = rng.integers(0, rows, 2)
        walk = np.cumsum(np.vstack([start[None], rng.integers(-2, 3, (F - 1, 2))]), axis=0)
        walk = np.clip(walk, 0, rows - 1)
        offs = ((walk[:, 0] * cols + walk[:, 1]) * per).astype(np.int32)[:, None]
        t_off, ids, pos, match, counts, _ = track_np.track(offs, rows, cols, per, 1, gate=1e3, max_miss=5, min_hits=1, q=0.1, r=0.1)
        assert (match[:, 0] == 0).all() and (ids[:, 0] == 1).all() and counts[:, 0].sum() == 1      # born once, matched ever after
        z = np.concatenate([walk.astype(np.float64), np.zeros((F, 1))], axis=1)
        want = _kf_hpp_float64(z)
        diff = np.abs(pos[:, 0].astype(np.float64) - want[:, [0, 1, 3, 4]]).max()
        worst = max(worst, diff)
        assert np.abs(want[:, [2, 5]]).max() == 0                               # the unused third axis stays at rest
    print("worst |float32 restatement - float64 kf.hpp| = %.3f units of 2^-24 * %d" % (worst / unit, rows))
    assert worst <= 8 * unit, worst / unit


# ------------------------------------------------------------------ consequences of the definition

def _xy(off, cols, per):
    d = off // per
    return d // cols, d % cols


def test_swapping_sources_keep_their_slots():
    rows, cols, per = 41, 23, 3
    offs = track_np.scripted_scene(40, 4, rows, cols, per, gap=(0, 0), alarms=())
    assert (offs[0, :2] != offs[7, :2]).all() and offs[0, 1] == offs[7, 0]      # the input does swap
    t_off, ids, pos, match, counts, _ = track_np.track(offs, rows, cols, per, 4, gate=3.0, max_miss=5, min_hits=3)
    assert (ids[:, 0] == 1).all() and (ids[:, 1] == 2).all() and (ids[:, 2:] == 0).all()
    flipped = (np.arange(40) // 7) % 2
    assert (match[:, 0] == flipped).all() and (match[:, 1] == 1 - flipped).all()
    assert counts[:, 0].tolist() == [2] + [0] * 39 and not counts[:, 1:3].any() and (counts[:, 3] == 2).all()
    assert (t_off[:2, :2] == -1).all() and (t_off[2:, :2] >= 0).all()            # confirmed at the third detection
    for f in range(2, 40):
        assert _xy(t_off[f, 1], cols, per) == (30, 15)
        assert abs(_xy(t_off[f, 0], cols, per)[0] - (10 + f // 4)) <= 1 and _xy(t_off[f, 0], cols, per)[1] == 5


def test_a_dropout_is_coasted_through():
    rows, cols, per = 41, 23, 3
    offs = track_np.scripted_scene(40, 4, rows, cols, per, gap=(20, 24), alarms=())
    t_off, ids, pos, match, counts, _ = track_np.track(offs, rows, cols, per, 4, gate=3.0, max_miss=5, min_hits=3)
    assert (ids[:, 0] == 1).all() and (ids[:, 1] == 2).all() and (ids[:, 2:] == 0).all()
    assert (match[20:24, 1] == -1).all() and (match[:20, 1] >= 0).all() and (match[24:, 1] >= 0).all()
    assert (match[:, 0] >= 0).all()
    assert all(_xy(o, cols, per) == (30, 15) for o in t_off[2:, 1])               # the coasting slot keeps pointing at the source
    assert counts[:, 0].sum() == 2 and not counts[:, 1:3].any()


def test_a_one_frame_detection_is_never_reported():
    rows, cols, per, max_miss = 41, 23, 3, 5
    offs = track_np.scripted_scene(40, 4, rows, cols, per, gap=(0, 0), alarms=((5, 35, 2),))
    t_off, ids, pos, match, counts, _ = track_np.track(offs, rows, cols, per, 4, gate=3.0, max_miss=max_miss, min_hits=3)
    assert (t_off[:, 2:] == -1).all()
    shown = np.flatnonzero(ids[:, 2])
    assert shown.tolist() == list(range(5, 5 + max_miss + 1)) and (ids[shown, 2] == 3).all()
    assert match[5, 2] == 2 and (match[6:, 2] == -1).all()
    assert counts[5, 0] == 1 and counts[5 + max_miss + 1, 1] == 1 and counts[:, 1].sum() == 1
    assert (ids[:, 0] == 1).all() and (ids[:, 1] == 2).all()                    # the two sources never notice


def test_one_slot_drops_the_second_source():
    rows, cols, per = 41, 23, 3
    offs = track_np.scripted_scene(40, 4, rows, cols, per, gap=(0, 0), alarms=())
    t_off, ids, pos, match, counts, _ = track_np.track(offs, rows, cols, per, 1, gate=3.0, max_miss=5, min_hits=3)
    assert (counts[:, 2] == 1).all() and (ids[:, 0] == 1).all() and counts[:, 0].sum() == 1


def test_equal_costs_take_the_lower_slot_then_the_lower_column():
    rows, cols, per = 20, 20, 1
    at = lambda x, y: x * cols + y
    # two slots at (10, 10) and (10, 14), one detection half way: cost 4 for both, the lower slot takes it
    offs = np.array([[at(10, 10), at(10, 14)], [at(10, 12), -1]], dtype=np.int32)
    _, ids, _, match, counts, _ = track_np.track(offs, rows, cols, per, 2, gate=2.0, min_hits=1)
    assert match.tolist() == [[0, 1], [0, -1]] and ids[1].tolist() == [1, 2]
    # one slot at (10, 10), detections two to either side: cost 4 for both, the lower column is taken and the other starts a track
    for first, second in ((at(10, 12), at(10, 8)), (at(10, 8), at(10, 12))):
        offs = np.array([[at(10, 10), -1], [first, second]], dtype=np.int32)
        _, ids, pos, match, counts, _ = track_np.track(offs, rows, cols, per, 2, gate=2.0, min_hits=1)
        assert match.tolist() == [[0, -1], [0, 1]] and ids[1].tolist() == [1, 2] and counts[1].tolist() == [1, 0, 0, 0]
        assert pos[1, 1, :2].tolist() == [float(second // cols), float(second % cols)]


def test_state_carries_between_calls_of_the_restatement():
    rows, cols, per = 41, 23, 3
    offs = track_np.scripted_scene()
    whole = track_np.track(offs, rows, cols, per, 4)
    first = track_np.track(offs[:20], rows, cols, per, 4)
    second = track_np.track(offs[20:], rows, cols, per, 4, state=first[5])
    for w, a, b in zip(whole[:5], first[:5], second[:5]):
        assert w.tobytes() == np.concatenate([a, b]).tobytes()
    assert whole[5].tobytes() == second[5].tobytes() and whole[5].size == 52 and whole[5][0] == 4
