"""CPU: the C-ABI's refusals that sit BEFORE device bring-up and that no other test pins -- return code, the exact bf_last_error text
and, where an output buffer is passed, that it comes back all-NaN (or untouched, where the entry point returns before it could
poison).  Every call below is refused before anything could dereference a pointer, so the "device pointers" are fake non-null
addresses; host pointers that an entry point may write (poisoning) are real arrays of the size it writes.

Sizes: 16 microphones, 64 samples, 5 x 5 directions, 8 taps."""
import ctypes as C

import numpy as np
import pytest

import util
from support import FAKE

M, N, X, Y, T = 16, 64, 5, 5, 8
D = X * Y
NO_FRAME = "get_data: no frame published (call bf_publish_frame first)"


@pytest.fixture(scope="module")
def lib(native):
    """The library at the sizes above with nothing loaded, published or listening; the suite's usual configuration afterwards."""
    L = native.lib
    assert L.bf_configure(M, 32, X, Y, T) == 0 and L.bf_configure(M, N, X, Y, T) == 0    # (a change of N_SAMPLES drops every table)
    L.unload_coefficients_pad2()
    L.stop_receiving()
    L.stop_miso()
    L.bf_clear_error()
    yield L
    L.unload_coefficients_pad2()
    L.stop_miso()
    L.bf_clear_error()
    util.configure("cfg1")


def _err(lib):
    text = lib.bf_last_error().decode()
    lib.bf_clear_error()
    return text


def _refused(lib, rc, text, want_rc=-1):
    assert rc == want_rc
    assert _err(lib) == text


def _f(n, fill=0.0):
    return np.full(n, fill, dtype=np.float32)


def fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


MICS = np.arange(M, dtype=np.int32)


# ------------------------------------------------------------------ configuration

@pytest.mark.parametrize("sizes,text", [
    ((0, N, X, Y, T), "bf_configure: invalid sizes N_MICROPHONES=0 N_SAMPLES=64 MAX_RES_X=5 MAX_RES_Y=5 N_TAPS=8"),
    ((M, 0, X, Y, T), "bf_configure: invalid sizes N_MICROPHONES=16 N_SAMPLES=0 MAX_RES_X=5 MAX_RES_Y=5 N_TAPS=8"),
    ((M, N, -1, Y, T), "bf_configure: invalid sizes N_MICROPHONES=16 N_SAMPLES=64 MAX_RES_X=-1 MAX_RES_Y=5 N_TAPS=8"),
    ((M, N, X, 0, T), "bf_configure: invalid sizes N_MICROPHONES=16 N_SAMPLES=64 MAX_RES_X=5 MAX_RES_Y=0 N_TAPS=8"),
    ((M, N, X, Y, 0), "bf_configure: invalid sizes N_MICROPHONES=16 N_SAMPLES=64 MAX_RES_X=5 MAX_RES_Y=5 N_TAPS=0"),
    ((M, N, 8192, 4096, T), "bf_configure: invalid sizes N_MICROPHONES=16 N_SAMPLES=64 MAX_RES_X=8192 MAX_RES_Y=4096 N_TAPS=8"),
    ((M, 1025, X, Y, T), "bf_configure: N_SAMPLES=1025 > 1024 is not supported by the gfx950 kernels"),
    ((0, 2048, X, Y, T), "bf_configure: invalid sizes N_MICROPHONES=0 N_SAMPLES=2048 MAX_RES_X=5 MAX_RES_Y=5 N_TAPS=8"),
])
def test_configure(lib, sizes, text):
    _refused(lib, lib.bf_configure(*sizes), text)
    out = (C.c_int * 5)()
    lib.bf_get_config(out)
    assert list(out) == [M, N, X, Y, T]                # a refused call changes nothing


def test_configure_from_json(lib, tmp_path):
    _refused(lib, lib.bf_configure_from_json(b"/nonexistent/config.json"), "cannot open config file /nonexistent/config.json")
    _refused(lib, lib.bf_configure_from_json(None), "")                        # a null path fails without a message
    p = tmp_path / "config.json"
    p.write_text('{"general": {"N_SAMPLES": 4096}}')
    _refused(lib, lib.bf_configure_from_json(str(p).encode()), "bf_configure: N_SAMPLES=4096 > 1024 is not supported by the gfx950 kernels")
    out = (C.c_int * 5)()
    lib.bf_get_config(out)
    assert list(out) == [M, N, X, Y, T]


# ------------------------------------------------------------------ loaders

@pytest.mark.parametrize("name,kind,text", [
    ("load_coefficients_pad", "i", "load_coefficients_pad: null or empty table"),
    ("load_coefficients2", "i", "load_coefficients2: null or empty table"),
    ("load_coefficients_pad2", "i", "load_coefficients_pad2: null or empty table"),
    ("load_coefficients_lerp", "f", "load_coefficients_lerp: null or empty table"),
    ("load_coefficients_convolve", "f", "load_coefficients_convolve: null or empty table"),
    ("load_coefficients_convolve_hybrid", "f", "load_coefficients_convolve_hybrid: null or empty table"),
    ("load_pa", "i", "load_pa: null or empty adaptive_array"),
])
def test_loaders(lib, name, kind, text):
    fn = getattr(lib, name)
    table = np.zeros(8, dtype=np.int32 if kind == "i" else np.float32)
    ptr = ip(table) if kind == "i" else fp(table)
    _refused(lib, fn(None, 8), text, None)
    _refused(lib, fn(ptr, 0), text, None)
    _refused(lib, fn(ptr, -3), text, None)
    _refused(lib, fn(None, 0), text, None)


def test_table_getters_with_nothing_loaded(lib):
    whole = np.zeros(5, dtype=np.int32)
    _refused(lib, lib.bf_get_pad_table(None, 5), "bf_get_pad_table: whole is null")
    _refused(lib, lib.bf_get_pad_table(ip(whole), 5), "bf_get_pad_table: 5 requested, 0 loaded")
    # the lerp and hybrid getters do not check their pointers: the count is what refuses
    _refused(lib, lib.bf_get_lerp_tables(None, None, 5), "bf_get_lerp_tables: 5 requested, 0 loaded")
    _refused(lib, lib.bf_get_lerp_tables(ip(whole), fp(_f(5)), 0), "bf_get_lerp_tables: 0 requested, 0 loaded")
    _refused(lib, lib.bf_get_hybrid_tables(None, None, 7), "bf_get_hybrid_tables: 7 requested, 0 loaded")
    _refused(lib, lib.bf_get_hybrid_tables(ip(whole), fp(_f(5 * T)), 5), "bf_get_hybrid_tables: 5 requested, 0 loaded")
    assert not whole.any()


# ------------------------------------------------------------------ host-pointer beams and maps

@pytest.mark.parametrize("name", ["mimo_pad", "mimo_lerp", "mimo_convolve_naive", "mimo_convolve_vectorized", "mimo_convolve_hybrid"])
def test_mimo_null(lib, name):
    fn = getattr(lib, name)
    sig = _f(M * N)
    for signals, mics in ((None, MICS), (sig, None), (None, None)):
        image = _f(D)
        _refused(lib, fn(fp(signals), fp(image), ip(mics), M), "null argument", None)
        assert np.isnan(image).all()
    _refused(lib, fn(fp(sig), None, ip(MICS), M), "null argument", None)


@pytest.mark.parametrize("name", ["miso_pad", "miso_lerp", "miso_convolve_vectorized", "miso_convolve_hybrid"])
def test_miso_null(lib, name):
    fn = getattr(lib, name)
    sig = _f(M * N)
    for signals, mics in ((None, MICS), (sig, None)):
        out = _f(N)
        _refused(lib, fn(fp(signals), fp(out), ip(mics), M, 0), "null argument", None)
        assert np.isnan(out).all()
    _refused(lib, fn(fp(sig), None, ip(MICS), M, 0), "null argument", None)


def test_delay_helpers_null(lib):
    sig, h = _f(N), _f(T)
    calls = [lambda s, o: lib.pad_delay(s, o, 3), lambda s, o: lib.lerp_delay(s, o, C.c_float(0.5), 3),
             lambda s, o: lib.convolve_delay_naive_add(s, fp(h), o), lambda s, o: lib.convolve_delay_naive(s, o, fp(h)),
             lambda s, o: lib.convolve_delay_vectorized(s, fp(h), o), lambda s, o: lib.convolve_delay_vectorized_add(s, fp(h), o),
             lambda s, o: lib.convolve_hybrid_delay_add(s, fp(h), 3, o)]
    for call in calls:
        out = _f(N)
        _refused(lib, call(None, fp(out)), "null argument", None)
        assert np.isnan(out).all()
        _refused(lib, call(fp(sig), None), "null argument", None)


def test_miso_pad2(lib):
    sig = _f(M * N)
    out = _f(N)
    _refused(lib, lib.miso_pad2(fp(sig), fp(out), None, 4, 0), "miso_pad2: null or empty adaptive_array", None)
    assert np.isnan(out).all()
    out = _f(N)
    _refused(lib, lib.miso_pad2(fp(sig), fp(out), ip(MICS), 0, 0), "miso_pad2: null or empty adaptive_array", None)
    assert np.isnan(out).all()
    _refused(lib, lib.miso_pad2(fp(sig), None, None, 4, 0), "miso_pad2: null or empty adaptive_array", None)
    out = _f(N)
    _refused(lib, lib.miso_pad2(fp(sig), fp(out), ip(MICS), 4, 0), "miso_pad2: mic 0 outside the 0-entry pad2 table", None)
    assert np.isnan(out).all()
    table = np.array([1, 2, 3, 4], dtype=np.int32)
    lib.load_coefficients_pad2(ip(table), 4)
    assert _err(lib) == ""
    for mics, text in (([0, 3, 4], "miso_pad2: mic 4 outside the 4-entry pad2 table"), ([1, -1, 9], "miso_pad2: mic -1 outside the 4-entry pad2 table")):
        out = _f(N)
        _refused(lib, lib.miso_pad2(fp(sig), fp(out), ip(np.array(mics, dtype=np.int32)), 3, 12345), text, None)
        assert np.isnan(out).all()
    lib.unload_coefficients_pad2()


def test_miso_convolve_vectorized_offset(lib):
    for offset, text in ((3, "miso_convolve_vectorized: offset 3 is not a multiple of N_TAPS=8"),
                         (-4, "miso_convolve_vectorized: offset -4 is not a multiple of N_TAPS=8")):
        out = _f(N)
        _refused(lib, lib.miso_convolve_vectorized(fp(_f(M * N)), fp(out), ip(MICS), M, offset), text, None)
        assert np.isnan(out).all()
    _refused(lib, lib.miso_convolve_vectorized(None, None, None, M, 9), "miso_convolve_vectorized: offset 9 is not a multiple of N_TAPS=8", None)


# ------------------------------------------------------------------ api.h shims

def test_nothing_published(lib):
    lib.stop_receiving()
    frame = _f(M * N)
    _refused(lib, lib.get_data(fp(frame)), NO_FRAME, None)
    assert np.isnan(frame).all()
    _refused(lib, lib.get_data(None), "", None)
    _refused(lib, lib.bf_publish_frame(None), "bf_publish_frame: null frame", None)
    for name in ("pad_mimo", "lerp_mimo", "convolve_mimo_naive", "convolve_mimo_vectorized", "mimo_truncated"):
        image = _f(D)
        _refused(lib, getattr(lib, name)(fp(image), ip(MICS), M), NO_FRAME, None)
        assert np.isnan(image).all(), name
        _refused(lib, getattr(lib, name)(None, ip(MICS), M), NO_FRAME, None)
    out = _f(N)
    _refused(lib, lib.miso_steer_listen(fp(out), ip(MICS), M, 0), NO_FRAME, None)
    assert np.isnan(out).all()


def test_load(lib):
    text = "load: the UDP receiver process (PC/src/api.c:874-939) is out of scope of this library; hand frames over with bf_publish_frame"
    _refused(lib, lib.load(True), text)
    _refused(lib, lib.load(False), text)


def test_miso_listen_block(lib):
    lib.stop_miso()
    lib.stop_receiving()
    gain = C.c_float(128.0)
    _refused(lib, lib.bf_miso_listen_block(None, gain), "bf_miso_listen_block: null output")
    out = _f(N)
    _refused(lib, lib.bf_miso_listen_block(fp(out), gain), "bf_miso_listen_block: load_miso / load_pa has not been called")
    assert np.isnan(out).all()
    assert lib.load_miso() == 0
    _refused(lib, lib.bf_miso_listen_block(None, gain), "bf_miso_listen_block: null output")
    out = _f(N)
    _refused(lib, lib.bf_miso_listen_block(fp(out), gain), NO_FRAME)
    assert np.isnan(out).all()
    lib.stop_miso()


def test_set_device_while_no_device_is_in_use(native, lib):
    if not native.gpu_available():                       # (with a GPU another test may have brought a device up: leave it alone)
        _refused(lib, lib.bf_set_device(3), "", 0)
        _refused(lib, lib.bf_set_device(-1), "", 0)      # back to "$BF_DEVICE, else 0"


# ------------------------------------------------------------------ device-resident entry points

def _das(lib, algo=0, d_signals=FAKE, m_total=M, d_images=FAKE, image_stride=D, frames=1, mics=MICS, n=M, dir_begin=0, dir_end=D):
    return lib.bf_das_device(algo, d_signals, m_total, d_images, image_stride, frames, ip(mics), n, dir_begin, dir_end, None)


@pytest.mark.parametrize("kw,text", [
    (dict(algo=5), "bf_das_device: unknown algo 5"),
    (dict(algo=-1), "bf_das_device: unknown algo -1"),
    (dict(algo=7, d_signals=None, frames=0), "bf_das_device: unknown algo 7"),
    (dict(d_signals=None), "bf_das_device: null argument or frames < 1"),
    (dict(d_images=None), "bf_das_device: null argument or frames < 1"),
    (dict(mics=None), "bf_das_device: null argument or frames < 1"),
    (dict(frames=0), "bf_das_device: null argument or frames < 1"),
    (dict(algo=4, frames=-2), "bf_das_device: null argument or frames < 1"),
])
def test_das_device(lib, kw, text):
    _refused(lib, _das(lib, **kw), text)


def _peak_offsets(lib, d_power=FAKE, frames=2, image_stride=D, n_dirs=D, offset_per_dir=M, d_offsets=FAKE):
    return lib.bf_peak_offsets_device(d_power, frames, image_stride, n_dirs, offset_per_dir, d_offsets, None)


@pytest.mark.parametrize("kw,text", [
    (dict(d_power=None), "bf_peak_offsets_device: d_power is null"),
    (dict(d_offsets=None), "bf_peak_offsets_device: d_offsets is null"),
    (dict(d_power=None, d_offsets=None, frames=0), "bf_peak_offsets_device: d_power is null"),
    (dict(frames=0), "bf_peak_offsets_device: frames = 0 < 1"),
    (dict(frames=-1, n_dirs=0), "bf_peak_offsets_device: frames = -1 < 1"),
    (dict(n_dirs=0), "bf_peak_offsets_device: n_dirs = 0 < 1"),
    (dict(n_dirs=-7, offset_per_dir=0), "bf_peak_offsets_device: n_dirs = -7 < 1"),
    (dict(offset_per_dir=0), "bf_peak_offsets_device: offset_per_dir = 0 < 1"),
    (dict(offset_per_dir=-16, image_stride=3), "bf_peak_offsets_device: offset_per_dir = -16 < 1"),
    (dict(image_stride=24), "bf_peak_offsets_device: image_stride = 24 < n_dirs = 25"),
    (dict(image_stride=-1, n_dirs=3, offset_per_dir=2 ** 30), "bf_peak_offsets_device: image_stride = -1 < n_dirs = 3"),
    (dict(n_dirs=3, offset_per_dir=2 ** 30), "bf_peak_offsets_device: (n_dirs - 1) * offset_per_dir = 2147483648 does not fit an int offset"),
    (dict(n_dirs=2 ** 31 - 1, image_stride=2 ** 31 - 1, offset_per_dir=2),
     "bf_peak_offsets_device: (n_dirs - 1) * offset_per_dir = 4294967292 does not fit an int offset"),
])
def test_peak_offsets_device(lib, kw, text):
    _refused(lib, _peak_offsets(lib, **kw), text)


def test_ingest(lib):
    frame = _f(M * N)
    _refused(lib, lib.bf_ingest(None, 1, 4, 4, fp(frame)), "bf_ingest: null argument")
    assert not frame.any()                                # refused before the size of the output is known: nothing is written
    _refused(lib, lib.bf_ingest(FAKE, 1, 4, 4, None), "bf_ingest: null argument")
    _refused(lib, lib.bf_ingest_device(None, 1, 4, 4, FAKE, None), "bf_ingest_device: null argument")
    _refused(lib, lib.bf_ingest_device(FAKE, 1, 4, 4, None, None), "bf_ingest_device: null argument")


def test_heatmap_calls(lib):
    f = C.c_float
    col = lambda power=FAKE, frames=1, small=FAKE, flag=FAKE: lib.bf_heatmap_colorize_device(power, frames, f(1e-2), f(0.5), f(10.0), small, flag, None)
    for kw in (dict(power=None), dict(small=None), dict(flag=None), dict(frames=0)):
        _refused(lib, col(**kw), "bf_heatmap_colorize_device: null argument or frames < 1")
    ovl = lambda small=FAKE, frames=1, w=64, h=36, prev=FAKE, cam=FAKE, out=FAKE: lib.bf_heatmap_overlay_device(small, frames, w, h, prev, cam, out, f(0.9), f(0.1),
                                                                                                             f(0.5), f(0.5), None)
    for kw in (dict(small=None), dict(prev=None), dict(out=None), dict(frames=0), dict(w=0), dict(h=-1)):
        _refused(lib, ovl(**kw), "bf_heatmap_overlay_device: bad argument")
    ctr = lambda power=FAKE, frames=1, centers=FAKE, work=FAKE: lib.bf_power_center_device(power, frames, centers, work, None)
    for kw in (dict(power=None), dict(centers=None), dict(work=None), dict(frames=0)):
        _refused(lib, ctr(**kw), "bf_power_center_device: bad argument")


def _letterbox(lib, d_frame=FAKE, h=360, w=640, d_out=FAKE, out_h=640, out_w=640, new_h=360, new_w=640, top=140, left=0, value=114):
    return lib.bf_letterbox_bgr8_device(d_frame, h, w, d_out, out_h, out_w, new_h, new_w, top, left, value, None)


@pytest.mark.parametrize("kw,text", [
    (dict(d_frame=None), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 640 at (140, 0) of 640 x 640, border 114"),
    (dict(d_out=None), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 640 at (140, 0) of 640 x 640, border 114"),
    (dict(h=0), "bf_letterbox_bgr8_device: 0 x 640 -> 360 x 640 at (140, 0) of 640 x 640, border 114"),
    (dict(new_w=0), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 0 at (140, 0) of 640 x 640, border 114"),
    (dict(top=-1), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 640 at (-1, 0) of 640 x 640, border 114"),
    (dict(top=281), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 640 at (281, 0) of 640 x 640, border 114"),
    (dict(left=1), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 640 at (140, 1) of 640 x 640, border 114"),
    (dict(value=256), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 640 at (140, 0) of 640 x 640, border 256"),
    (dict(value=-1), "bf_letterbox_bgr8_device: 360 x 640 -> 360 x 640 at (140, 0) of 640 x 640, border -1"),
])
def test_letterbox(lib, kw, text):
    _refused(lib, _letterbox(lib, **kw), text)


def _yolo(lib, raw="ok", batch=1, nc=80, anchors="ok", d_boxes=FAKE):
    raw3 = (C.c_void_p * 3)(FAKE, FAKE, None if raw == "third" else FAKE)
    ints = np.array([8, 16, 32], dtype=np.int32)
    anc = _f(18, 1.0)
    return lib.bf_yolo_decode_device(None if raw is None else raw3, ip(ints), ip(ints), ip(ints), None if anchors is None else fp(anc), batch, nc, 0,
                                     C.c_float(0.25), d_boxes, FAKE, FAKE, None)


def test_fd_and_detector_entry(lib):
    """One null and one non-positive size for each entry point of the family that shares one refusal text."""
    f = C.c_float
    cases = {
        "bf_fd_steering_device": (lambda p=FAKE, n=4: lib.bf_fd_steering_device(p, FAKE, n, M, 9, FAKE, FAKE, None)),
        "bf_fd_dft_device": (lambda p=FAKE, n=4: lib.bf_fd_dft_device(p, M, n, ip(MICS), M, 0, 9, FAKE, FAKE, FAKE, FAKE, None)),
        "bf_fd_das_power_device": (lambda p=FAKE, n=4: lib.bf_fd_das_power_device(FAKE, FAKE, FAKE, FAKE, 2, M, n, 9, p, None)),
        "bf_fd_covariance_device": (lambda p=FAKE, n=4: lib.bf_fd_covariance_device(FAKE, p, n, M, 9, FAKE, FAKE, None)),
        "bf_fd_cholesky_inverse_device": (lambda p=FAKE, n=4: lib.bf_fd_cholesky_inverse_device(FAKE, FAKE, M, n, f(1e-3), FAKE, FAKE, p, None)),
        "bf_fd_mvdr_power_device": (lambda p=FAKE, n=4: lib.bf_fd_mvdr_power_device(FAKE, FAKE, FAKE, p, n, D, 9, FAKE, None)),
        "bf_nms_device": (lambda p=FAKE, n=4: lib.bf_nms_device(FAKE, FAKE, FAKE, FAKE, 2, n, f(0.45), 300, p, FAKE, FAKE, None)),
    }
    for name, call in cases.items():
        text = name + ": null pointer or non-positive size"
        _refused(lib, call(p=None), text)
        _refused(lib, call(n=0), text)
        _refused(lib, call(n=-3), text)
    # what the shared text also covers: a null adaptive array, a negative first bin, a refusal that wins over the later range checks
    _refused(lib, lib.bf_fd_dft_device(FAKE, M, 2, None, M, 0, 9, FAKE, FAKE, FAKE, FAKE, None), "bf_fd_dft_device: null pointer or non-positive size")
    _refused(lib, lib.bf_fd_dft_device(FAKE, M, 2, ip(MICS), M, -1, 9, FAKE, FAKE, FAKE, FAKE, None), "bf_fd_dft_device: null pointer or non-positive size")
    _refused(lib, lib.bf_fd_cholesky_inverse_device(None, FAKE, 257, 9, f(1e-3), FAKE, FAKE, FAKE, None),
             "bf_fd_cholesky_inverse_device: null pointer or non-positive size")
    _refused(lib, lib.bf_nms_device(FAKE, FAKE, FAKE, FAKE, 2, 5000, f(0.45), 0, FAKE, FAKE, FAKE, None), "bf_nms_device: null pointer or non-positive size")
    text = "bf_yolo_decode_device: null pointer or non-positive size"
    for kw in (dict(raw=None), dict(raw="third"), dict(anchors=None), dict(d_boxes=None), dict(batch=0), dict(nc=0)):
        _refused(lib, _yolo(lib, **kw), text)


def _topk(lib, batch=2, total=100, k=30, **null):
    p = {n: FAKE for n in ("d_scores", "d_boxes", "d_cls", "d_top_scores", "d_top_boxes", "d_top_cls", "d_counts")}
    p.update(null)
    return lib.bf_topk_candidates_device(p["d_scores"], p["d_boxes"], p["d_cls"], batch, total, k, p["d_top_scores"], p["d_top_boxes"], p["d_top_cls"],
                                         p["d_counts"], None)


@pytest.mark.parametrize("kw,text", [
    (dict(d_scores=None), "bf_topk_candidates_device: null pointer"),
    (dict(d_top_cls=None, k=0), "bf_topk_candidates_device: null pointer"),
    (dict(d_counts=None), "bf_topk_candidates_device: null pointer"),
    (dict(k=0), "bf_topk_candidates_device: batch 2, 100 boxes, k = 0 (1..1024)"),
    (dict(k=1025), "bf_topk_candidates_device: batch 2, 100 boxes, k = 1025 (1..1024)"),
    (dict(batch=0), "bf_topk_candidates_device: batch 0, 100 boxes, k = 30 (1..1024)"),
    (dict(total=-1), "bf_topk_candidates_device: batch 2, -1 boxes, k = 30 (1..1024)"),
])
def test_topk_candidates(lib, kw, text):
    _refused(lib, _topk(lib, **kw), text)


@pytest.mark.parametrize("name,E", [("bf_upsample_concat_device", 8), ("bf_upsample_concat_f32_device", 4)])
def test_upsample_concat(lib, name, E):
    fn = getattr(lib, name)
    call = lambda a=FAKE, b=FAKE, out=FAKE, batch=1, h=4, w=6, ca=2 * E, cb=E: fn(a, b, out, batch, h, w, ca, cb, None)
    t = name + ": batch %d, %d x %d (even), %d + %d channels (multiples of " + str(E) + ")"
    _refused(lib, call(a=None), t % (1, 4, 6, 2 * E, E))
    _refused(lib, call(out=None), t % (1, 4, 6, 2 * E, E))
    _refused(lib, call(batch=0), t % (0, 4, 6, 2 * E, E))
    _refused(lib, call(h=3), t % (1, 3, 6, 2 * E, E))
    _refused(lib, call(w=0), t % (1, 4, 0, 2 * E, E))
    _refused(lib, call(ca=E + 2), t % (1, 4, 6, E + 2, E))
    _refused(lib, call(cb=E // 2), t % (1, 4, 6, 2 * E, E // 2))


@pytest.mark.parametrize("name,E", [("bf_sppf_pool_device", 8), ("bf_sppf_pool_f32_device", 4)])
def test_sppf_pool(lib, name, E):
    fn = getattr(lib, name)
    call = lambda buf=FAKE, batch=1, h=20, w=20, c=4 * E: fn(buf, batch, h, w, c, None)
    t = name + ": batch %d, %d x %d, %d channels (a multiple of " + str(E) + "; at most 2048 pixels per plane)"
    _refused(lib, call(buf=None), t % (1, 20, 20, 4 * E))
    _refused(lib, call(batch=0), t % (0, 20, 20, 4 * E))
    _refused(lib, call(h=0), t % (1, 0, 20, 4 * E))
    _refused(lib, call(c=E + 1), t % (1, 20, 20, E + 1))
    _refused(lib, call(c=E // 2), t % (1, 20, 20, E // 2))
    _refused(lib, call(h=64, w=33), t % (1, 64, 33, 4 * E))


@pytest.mark.parametrize("name", ["bf_preprocess_bgr8_device", "bf_preprocess_bgr8_f32_device"])
def test_preprocess(lib, name):
    fn = getattr(lib, name)
    call = lambda frames=FAKE, out=FAKE, batch=2, h=36, w=64, cpad=4: fn(frames, out, batch, h, w, cpad, None)
    t = name + ": batch %d, %d x %d, %d channels"
    _refused(lib, call(frames=None), t % (2, 36, 64, 4))
    _refused(lib, call(out=None), t % (2, 36, 64, 4))
    _refused(lib, call(batch=0), t % (0, 36, 64, 4))
    _refused(lib, call(w=0), t % (2, 36, 0, 4))
    _refused(lib, call(cpad=2), t % (2, 36, 64, 2))


# ------------------------------------------------------------------ the conv family: six refusal branches

def _conv(lib, name, x=FAKE, wt=FAKE, y=FAKE, batch=1, h=8, w=8, c=16, n=32, kh=3, kw=3, stride=1, pad=1, ldy=None, res=None, ldr=0):
    fn = getattr(lib, name)
    if "_into_" in name:
        return fn(x, wt, FAKE, y, n if ldy is None else ldy, res, ldr, batch, h, w, c, n, kh, kw, stride, pad, 1, None)
    return fn(x, wt, FAKE, y, batch, h, w, c, n, kh, kw, stride, pad, 1, None)


CHANNELS = ("%s: %d input channels, window width %d, stride %d, pad %d, width %d: channels must be a power of two >= 4 with kw * c a multiple of %d; "
            "float16 with 4 channels needs even stride, pad and width")


@pytest.mark.parametrize("name,E", [("bf_conv2d_nhwc_f16_device", 8), ("bf_conv2d_nhwc_f32_device", 4), ("bf_conv2d_nhwc_f16_into_device", 8),
                                    ("bf_conv2d_nhwc_f32_into_device", 4)])
def test_conv2d(lib, name, E):
    for kw in (dict(x=None), dict(wt=None), dict(y=None), dict(x=None, batch=0)):
        _refused(lib, _conv(lib, name, **kw), name + ": null pointer")
    sizes = name + ": batch %d, %d x %d, window %d x %d, stride %d, pad %d"
    _refused(lib, _conv(lib, name, batch=0), sizes % (0, 8, 8, 3, 3, 1, 1))
    _refused(lib, _conv(lib, name, n=0), sizes % (1, 8, 8, 3, 3, 1, 1))
    _refused(lib, _conv(lib, name, stride=0, c=3), sizes % (1, 8, 8, 3, 3, 0, 1))
    _refused(lib, _conv(lib, name, pad=-1), sizes % (1, 8, 8, 3, 3, 1, -1))
    _refused(lib, _conv(lib, name, h=2, kh=5, pad=1), sizes % (1, 2, 8, 5, 3, 1, 1))
    _refused(lib, _conv(lib, name, c=2), CHANNELS % (name, 2, 3, 1, 1, 8, E))
    _refused(lib, _conv(lib, name, c=24), CHANNELS % (name, 24, 3, 1, 1, 8, E))
    if E == 8:
        _refused(lib, _conv(lib, name, c=4, kw=3, x=FAKE + 4), CHANNELS % (name, 4, 3, 1, 1, 8, E))     # 3 * 4 elements: no whole number of chunks
        _refused(lib, _conv(lib, name, c=4, kw=2, kh=2, pad=0, stride=1), CHANNELS % (name, 4, 2, 1, 0, 8, E))
        _refused(lib, _conv(lib, name, c=4, kw=2, kh=2, pad=0, stride=2, w=7), CHANNELS % (name, 4, 2, 2, 0, 7, E))
    if "_into_" in name:
        strides = name + ": row strides %d / %d under %d output channels"
        _refused(lib, _conv(lib, name, ldy=31), strides % (31, 0, 32))
        _refused(lib, _conv(lib, name, ldy=64, res=FAKE, ldr=16, x=FAKE + 4), strides % (64, 16, 32))
    _refused(lib, _conv(lib, name, x=FAKE + 4), name + ": x and w must be 16-byte aligned")
    _refused(lib, _conv(lib, name, wt=FAKE + 8), name + ": x and w must be 16-byte aligned")


def _cat(lib, name, x1=FAKE, ld1=16, c1=16, up1=0, x2=FAKE, ld2=16, wt=FAKE, y=FAKE, ldy=32, res=None, ldr=0, batch=1, h=8, w=8, c=32, n=32):
    return getattr(lib, name)(x1, ld1, c1, up1, x2, ld2, wt, FAKE, y, ldy, res, ldr, batch, h, w, c, n, 1, None)


@pytest.mark.parametrize("name,E", [("bf_conv1x1_cat_nhwc_f16_device", 8), ("bf_conv1x1_cat_nhwc_f32_device", 4)])
def test_conv1x1_cat(lib, name, E):
    _refused(lib, _cat(lib, name, x1=None), name + ": null pointer")
    _refused(lib, _cat(lib, name, batch=0, c1=3), name + ": batch 0, 8 x 8, window 1 x 1, stride 1, pad 0")
    _refused(lib, _cat(lib, name, c=48, c1=3), CHANNELS % (name, 48, 1, 1, 0, 8, E))
    _refused(lib, _cat(lib, name, ldy=16, c1=3), name + ": row strides 16 / 0 under 32 output channels")
    _refused(lib, _cat(lib, name, res=FAKE, ldr=8), name + ": row strides 32 / 8 under 32 output channels")
    _refused(lib, _cat(lib, name, wt=FAKE + 4, c1=3), name + ": x and w must be 16-byte aligned")
    src = (name + ": sources of %d (pitch %d%s) + %d (pitch %d) channels for 32: whole 16-byte chunks of " + str(E) + " elements, 16-byte aligned; an upsampled "
           "source needs even h and w")
    _refused(lib, _cat(lib, name, c1=E // 2), src % (E // 2, 16, "", 32 - E // 2, 16))
    _refused(lib, _cat(lib, name, c1=40), src % (40, 16, "", -8, 16))
    _refused(lib, _cat(lib, name, c1=E + 1), src % (E + 1, 16, "", 31 - E, 16))
    _refused(lib, _cat(lib, name, ld1=18), src % (16, 18, "", 16, 16))
    _refused(lib, _cat(lib, name, ld1=8), src % (16, 8, "", 16, 16))
    _refused(lib, _cat(lib, name, x2=None), src % (16, 16, "", 16, 16))
    _refused(lib, _cat(lib, name, ld2=E + 1), src % (16, 16, "", 16, E + 1))
    _refused(lib, _cat(lib, name, ld2=8), src % (16, 16, "", 16, 8))
    _refused(lib, _cat(lib, name, x2=FAKE + 4), src % (16, 16, "", 16, 16))
    _refused(lib, _cat(lib, name, up1=1, h=7), src % (16, 16, ", upsampled", 16, 16))
    _refused(lib, _cat(lib, name, up1=1, w=5, c1=32, x2=None, ld1=32), src % (32, 32, ", upsampled", 0, 16))


# ------------------------------------------------------------------ the planner

@pytest.mark.parametrize("args,text", [
    ((0, 0, 1, 0, D, 3), "bf_plan_das: empty launch"),
    ((1, M, 0, 0, D, 3), "bf_plan_das: empty launch"),
    ((0, M, 1, 7, 7, 3), "bf_plan_das: empty launch"),
    ((1, M, 1, 9, 2, 3), "bf_plan_das: empty launch"),
])
def test_plan_das_refuses(lib, args, text):
    out = (C.c_longlong * 10)(*([-7] * 10))
    _refused(lib, lib.bf_plan_das(*args, 256, out), text)
    assert list(out) == [-7] * 10


def test_plan_das_refuses_taps(native, lib):
    out = (C.c_longlong * 10)()
    assert lib.bf_configure(M, N, X, Y, 12) == 0
    try:
        _refused(lib, lib.bf_plan_das(native.FIR_VEC, M, 1, 0, D, 0, 256, out), "bf_plan_das: N_TAPS must be in [1, 64] (multiple of 8 for the vectorized FIR)")
        assert lib.bf_plan_das(native.HYBRID, M, 1, 0, D, 0, 256, out) == 0 and _err(lib) == ""
    finally:
        assert lib.bf_configure(M, N, X, Y, T) == 0


def test_strided_plan_exports_refuse(lib):
    """bf_plan_das_stream and bf_last_strided_plan: a null array, what the map planner refuses, and nothing to report in a process that launched
    no stream or listed-direction call; the array stays untouched."""
    out = (C.c_longlong * 12)(*([-7] * 12))
    _refused(lib, lib.bf_plan_das_stream(0, M, 1, 0, D, 3, 256, None), "bf_plan_das_stream: out is null")
    _refused(lib, lib.bf_plan_das_stream(2, M, 1, 0, D, 3, 256, out), "bf_plan_das_stream: continuous mode exists for pad and lerp only")
    _refused(lib, lib.bf_plan_das_stream(1, M, 0, 0, D, 3, 256, out), "bf_plan_das_stream: empty launch")
    _refused(lib, lib.bf_plan_das_stream(0, M, 1, 7, 7, 3, 256, out), "bf_plan_das_stream: empty launch")
    assert list(out) == [-7] * 12
    _refused(lib, lib.bf_last_strided_plan(None), "bf_last_strided_plan: out is null")
    if lib.bf_last_strided_plan(out) == -1:                # (0 where GPU tests of the same process launched one before this test)
        assert _err(lib) == "bf_last_strided_plan: no stream or listed-direction call was launched in this process" and list(out) == [-7] * 12
    else:
        assert out[10] in (0, 1, 2, 3) and out[11] in (0, 1, 2, 4) and out[0] in (1, 2, 4, 8, 16)
    assert lib.bf_plan_das_stream(1, M, 3, 2, D, 3, 256, out) == 0 and _err(lib) == "" and list(out)[:2] == [1, 4]


# ------------------------------------------------------------------ the convolutions' planner

def _plan_conv(lib, out, eb=2, batch=1, h=8, w=8, c=32, n=32, kh=3, kw=3, stride=1, pad=1, ldy=32, has_res=0, ldr=0, c1=None, ld1=None, up1=0, has_x2=0, ld2=0,
               misaligned=0, dma=1, mode=1, n_cus=256):
    return lib.bf_plan_conv2d(eb, batch, h, w, c, n, kh, kw, stride, pad, ldy, has_res, ldr, c if c1 is None else c1, c if ld1 is None else ld1, up1, has_x2, ld2,
                              misaligned, dma, mode, n_cus, out)


@pytest.mark.parametrize("eb", [2, 4])
def test_plan_conv2d_refuses_what_the_entry_points_refuse(lib, eb):
    """bf_plan_conv2d runs the entry points' own argument checks (one copy of them), so a refused layer gives -1, the same sentence with the planner's
    name in front, and an untouched array; bf_last_conv2d_plan has nothing to report in a process that launched no convolution."""
    E, name = 16 // eb, "bf_plan_conv2d"
    out = (C.c_longlong * 16)(*([-7] * 16))
    sizes = name + ": batch %d, %d x %d, window %d x %d, stride %d, pad %d"
    src = (name + ": sources of %d (pitch %d%s) + %d (pitch %d) channels for 32: whole 16-byte chunks of " + str(E) + " elements, 16-byte aligned; an upsampled "
           "source needs even h and w")
    one = dict(kh=1, kw=1, pad=0)
    for kwargs, text in [
        (dict(batch=0), sizes % (0, 8, 8, 3, 3, 1, 1)),
        (dict(n=0), sizes % (1, 8, 8, 3, 3, 1, 1)),
        (dict(stride=0), sizes % (1, 8, 8, 3, 3, 0, 1)),
        (dict(h=2, kh=5), sizes % (1, 2, 8, 5, 3, 1, 1)),
        (dict(c=2), CHANNELS % (name, 2, 3, 1, 1, 8, E)),
        (dict(c=24), CHANNELS % (name, 24, 3, 1, 1, 8, E)),
        (dict(ldy=31), name + ": row strides 31 / 0 under 32 output channels"),
        (dict(ldy=64, has_res=1, ldr=16), name + ": row strides 64 / 16 under 32 output channels"),
        (dict(misaligned=1), name + ": x and w must be 16-byte aligned"),
        (dict(misaligned=2), name + ": x and w must be 16-byte aligned"),
        (dict(one, c1=E // 2, ld1=16, has_x2=1, ld2=16), src % (E // 2, 16, "", 32 - E // 2, 16)),
        (dict(one, c1=16, ld1=18, has_x2=1, ld2=16), src % (16, 18, "", 16, 16)),
        (dict(one, c1=16, ld1=16, has_x2=0, ld2=16), src % (16, 16, "", 16, 16)),
        (dict(one, c1=16, ld1=16, has_x2=1, ld2=8), src % (16, 16, "", 16, 8)),
        (dict(one, c1=16, ld1=16, has_x2=1, ld2=16, misaligned=4), src % (16, 16, "", 16, 16)),
        (dict(one, c1=16, ld1=16, has_x2=1, ld2=16, up1=1, h=7), src % (16, 16, ", upsampled", 16, 16)),
        (dict(c1=16, ld1=16, has_x2=1, ld2=16), name + ": two sources / a pitch / upsampling under a 3 x 3 window, stride 1, pad 1: 1x1 layers only"),
        (dict(one, batch=3, h=32768, w=32768), name + ": the launch refuses this layer (invalid argument)"),          # more than 2^31 - 1 pixels
    ]:
        _refused(lib, _plan_conv(lib, out, eb=eb, **kwargs), text)
        assert list(out) == [-7] * 16
    _refused(lib, _plan_conv(lib, out, eb=3), name + ": element size 3 (2 = float16, 4 = float32)")
    _refused(lib, _plan_conv(lib, None, eb=eb), name + ": out is null")
    if eb == 2:
        _refused(lib, _plan_conv(lib, out, eb=2, c=4, kw=2, kh=2, pad=0, stride=1), CHANNELS % (name, 4, 2, 1, 0, 8, E))
    assert list(out) == [-7] * 16
    _refused(lib, lib.bf_last_conv2d_plan(None), "bf_last_conv2d_plan: out is null")
    if lib.bf_last_conv2d_plan(out) == -1:                 # (0 where GPU tests of the same process launched one before this test)
        assert _err(lib) == "bf_last_conv2d_plan: no convolution was launched in this process" and list(out) == [-7] * 16
    else:
        assert out[0] in (2, 4) and out[1] in (0, 1, 2)
    # the same layer, taken: the switches as given, < 0 as they stand (the library's defaults: LDS-DMA, the split)
    assert _plan_conv(lib, out, eb=eb) == 0 and _err(lib) == "" and list(out)[:9] == [eb, 1, 128, 32, 4, 0, int(eb == 4), 1, 1]
    assert _plan_conv(lib, out, eb=eb, dma=-1, mode=-1) == 0 and list(out)[:9] == [eb, 1, 128, 32, 4, 0, int(eb == 4), 1, 1]
    assert _plan_conv(lib, out, eb=eb, dma=0) == 0 and list(out)[:9] == [eb, 0, 128, 32, 4, 0, 0, 0, 1]
    assert _plan_conv(lib, out, eb=eb, misaligned=8) == 0 and list(out)[8] == 0          # an output off 16 bytes: the scalar store epilogue
