"""CPU: the host-side contract of bf_remove_sources_device (every argument but the table is checked before device bring-up, so the
refusals run without a GPU), the Python front end's surface, and the NumPy restatement the GPU tests compare with
(tests/separate_np.py): against the definition read aloud, against the forward operators (the adjoint identity, exactly), and on the
two-source scene of the end-to-end test."""
import ctypes as C
import math

import numpy as np
import pytest

import separate_np as snp
from support import FAKE, refused

MICS = np.array([4, 0, 3, 1], dtype=np.int32)


def _remove(nat, **kw):
    a = dict(algo=1, d_signals=FAKE, m_total=6, frames=3, mics=MICS, n=None, d_offsets=FAKE, beams=3, d_beams=FAKE, beam_stride=None, gain=1.0,
             d_residual=FAKE, d_status=FAKE)
    a.update(kw)
    mics = None if a["mics"] is None else np.ascontiguousarray(a["mics"], dtype=np.int32)
    n = a["n"] if a["n"] is not None else (0 if mics is None else mics.size)
    cfg = (C.c_int * 5)()
    nat.lib.bf_get_config(cfg)
    stride = a["beam_stride"] if a["beam_stride"] is not None else cfg[1]
    return nat.lib.bf_remove_sources_device(a["algo"], a["d_signals"], a["m_total"], a["frames"], None if mics is None else nat.iptr(mics), n,
                                            a["d_offsets"], a["beams"], a["d_beams"], stride, a["gain"], a["d_residual"], a["d_status"], None)


@pytest.fixture()
def nat32(native):
    from interface import config
    config.configure(N_MICROPHONES=6, N_SAMPLES=32, MAX_RES_X=5, MAX_RES_Y=1, N_TAPS=8)
    native.lib.bf_clear_error()
    return native


def test_symbol_and_prototype(native):
    fn = native.lib.bf_remove_sources_device
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_int, C.c_void_p, C.c_int, C.c_int, native.IP, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                           C.c_void_p, C.c_void_p]


@pytest.mark.parametrize("kw,match", [
    (dict(algo=2), r"algo BF_HYBRID \(2\) has no adjoint"),
    (dict(algo=3), r"algo BF_FIR_NAIVE \(3\) has no adjoint"),
    (dict(algo=4), r"algo BF_FIR_VEC \(4\) has no adjoint"),
    (dict(algo=5), "unknown algo 5"),
    (dict(algo=-1), "unknown algo -1"),
    (dict(d_signals=None), "bf_remove_sources_device: d_signals is null"),
    (dict(mics=None, n=4), "bf_remove_sources_device: adaptive_array is null"),
    (dict(d_offsets=None), "bf_remove_sources_device: d_offsets is null"),
    (dict(d_beams=None), "bf_remove_sources_device: d_beams is null"),
    (dict(d_residual=None), "bf_remove_sources_device: d_residual is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(frames=-3), "frames = -3 < 1"),
    (dict(beams=0), "beams = 0 < 1"),
    (dict(beams=65), "beams = 65 > 64"),
    (dict(n=0), "n = 0 < 1"),
    (dict(n=-2), "n = -2 < 1"),
    (dict(beam_stride=31), "beam_stride = 31 < N_SAMPLES = 32"),
    (dict(mics=[4, 0, 6, 1]), r"adaptive_array\[2\] = 6 is not a row of frames with m_total = 6 rows"),
    (dict(mics=[4, -1, 3, 1]), r"adaptive_array\[1\] = -1 is not a row"),
    (dict(mics=[4, 0, 3, 4]), "row 4 is listed twice in adaptive_array"),
    (dict(mics=[2, 5, 1, 5, 2]), "row 2 is listed twice in adaptive_array"),
    (dict(gain=math.inf), "gain = inf is not finite"),
    (dict(gain=-math.inf), "gain = -inf is not finite"),
    (dict(gain=math.nan), "gain = -?nan is not finite"),
])
def test_argument_errors(nat32, kw, match):
    refused(nat32, _remove(nat32, **kw), match)


def test_valid_arguments_reach_the_device_checks(nat32):
    """Valid arguments pass every host check: without a GPU the refusal is the missing device, with one the missing table."""
    nat32.lib.unload_coefficients_lerp()
    nat32.lib.unload_coefficients_pad()
    nat32.lib.bf_clear_error()
    late = "no usable HIP device|has not been called"
    refused(nat32, _remove(nat32), late)
    refused(nat32, _remove(nat32, algo=0, beams=64, gain=0.0, d_status=None, beam_stride=32), late)
    refused(nat32, _remove(nat32, gain=-64.0, beams=1, frames=1, d_residual=FAKE, d_signals=FAKE, beam_stride=4096), late)


def test_front_end_surface(native):
    import listen
    import stream
    for name in ("maps", "remove", "separate"):
        assert callable(getattr(listen.BeamListener, name))
    sb = stream.StreamBeamformer("lerp", mics=[0, 1, 2])
    assert stream.StreamBeamformer.maps is not listen.BeamListener.maps           # the stream's own maps stay
    for call in (lambda: sb.remove(None, [0], None), lambda: sb.separate(None, 2)):
        with pytest.raises(NotImplementedError, match="read the previous window"):
            call()


# ------------------------------------------------------------------ the restatement against the definition read aloud

def _small_case(algo, seed):
    rng = np.random.default_rng(seed)
    M_total, N, D, F, B = 6, 32, 5, 3, 3
    n = MICS.size
    delays = rng.uniform(0, 12, (D, n))
    delays[0, 0], delays[0, 1], delays[1, 0], delays[1, 1], delays[2, 2] = 0.0, 7.0, N - 1 + 0.25, N - 2 + 0.5, N + 3.75
    if algo == snp.PAD:
        whole, h = snp.pad_table(np.floor(delays).astype(np.int32), N)
    else:
        whole, h = snp.lerp_table(np.float32(delays), N)
    x = (rng.standard_normal((F, M_total, N)) * 0.25).astype(np.float32)
    beams = rng.standard_normal((F, B, N + 3)).astype(np.float32)
    offs = np.array([[0, n, 2 * n], [4 * n, -1, 3 * n], [D * n - n + 1, 2 * n, 0]], dtype=np.int32)
    beams[1, 1], beams[2, 0] = np.nan, np.nan
    return x, whole, h, offs, beams


@pytest.mark.parametrize("algo", [snp.PAD, snp.LERP], ids=["pad", "lerp"])
@pytest.mark.parametrize("gain", [1.0, 0.5, 0.0])
def test_restatement_matches_the_definition_read_aloud(algo, gain):
    x, whole, h, offs, beams = _small_case(algo, 5)
    got, st = snp.remove(algo, x, MICS, whole, h, offs, beams, gain)
    want, st2 = snp.remove_naive(algo, x, MICS, whole, h, offs, beams, gain)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert st.tolist() == st2.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0]]
    assert np.isfinite(got).all()                                         # the NaN rows sit at rejected offsets
    assert got[:, [2, 5]].tobytes() == x[:, [2, 5]].tobytes()             # rows outside the adaptive array
    if gain == 0.0:
        assert got.tobytes() == x.tobytes()
    else:
        assert (got[:, MICS] != x[:, MICS]).any()


# ------------------------------------------------------------------ the adjoint identity, exactly

def exact_case(algo, seed, M_total=6, N=32, mics=MICS):
    """Small-integer frames and beam, delays whose fractions lie in {0, .25, .5, .75}: every product and sum of the identity is exact
    in float32 (|values| < 2^24 by a wide margin).  -> (x [M_total, N], o [N], whole [n], h [n], float32 delays [n])"""
    rng = np.random.default_rng(seed)
    n = len(mics)
    delays = rng.integers(0, N - 4, n) + rng.integers(0, 4, n) / 4.0
    delays[0] = 0.0
    delays[1] = 5.0
    delays[-1] = N - 1 + 0.5
    if n > 3:
        delays[2] = N - 2 + 0.25
    x = rng.integers(-8, 9, (M_total, N)).astype(np.float32)
    o = rng.integers(-8, 9, N).astype(np.float32)
    if algo == snp.PAD:
        whole, h = snp.pad_table(np.floor(delays).astype(np.int32), N)
    else:
        whole, h = snp.lerp_table(np.float32(delays), N)
    return x, o, whole, h, np.float32(delays)


@pytest.mark.parametrize("algo", [snp.PAD, snp.LERP], ids=["pad", "lerp"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_adjoint_identity_exact(algo, seed):
    x, o, whole, h, _ = exact_case(algo, seed)
    n = MICS.size
    fwd = snp.beam(algo, x, MICS, whole, h)
    # zeros in, gain = -n: c = -1 and the residual is the adjoint of o itself
    res, _ = snp.remove(algo, np.zeros_like(x)[None], MICS, whole, h, np.zeros((1, 1), np.int32), o[None, None], -float(n))
    adj = res[0]
    assert adj.tobytes() == snp.remove_naive(algo, np.zeros_like(x)[None], MICS, whole, h, np.zeros((1, 1), np.int32), o[None, None], -float(n))[0][0].tobytes()
    lhs = np.sum(fwd.astype(np.float64) * o.astype(np.float64))
    rhs = np.sum(x.astype(np.float64) * adj.astype(np.float64))
    assert lhs == rhs and lhs != 0.0
    assert (adj[[2, 5]] == 0).all()
    # and in float32 itself the products are exact: multiples of 1/16 far below 2^24
    assert np.all(fwd * 16 == np.round(fwd * 16)) and np.all(adj * 16 == np.round(adj * 16))


# ------------------------------------------------------------------ the scene of the end-to-end test, on the restatement alone

@pytest.fixture(scope="module")
def scene_run(oracle_lib):
    frames, _, sep, plain = snp.scene_reference(oracle_lib)
    return frames, sep, plain


def test_scene_property_on_the_restatement(scene_run):
    import peaks_np
    s = snp.SCENE
    frames, (offsets, values, beams, residual), plain = scene_run
    n, cols = s["M"], s["cols"]
    for f, (a_dir, b_dir) in enumerate(((s["A"], s["B"]), (s["B"], s["A"]))):
        da = snp.chebyshev(offsets[f, 0], n, cols, a_dir)
        db = snp.chebyshev(offsets[f, 1], n, cols, b_dir)
        print("frame %d: first component %d from A, second %d from B" % (f, da, db))
        assert da <= 1
        assert db <= 2
    # the plain map's separated peaks (radius 3, no floor) report nothing near B
    offs, _, counts = peaks_np.peaks(plain, s["rows"], cols, 3, 2, 0.0, 0.0, n)
    for f, b_dir in enumerate((s["B"], s["A"])):
        near = [snp.chebyshev(o, n, cols, b_dir) for o in offs[f] if o >= 0]
        print("frame %d: plain peaks at distances %s from B" % (f, near))
        assert all(d > 2 for d in near)
    assert np.isfinite(beams).all() and np.isfinite(residual).all()
    assert float(np.sum(residual.astype(np.float64) ** 2)) < float(np.sum(frames.astype(np.float64) ** 2))
