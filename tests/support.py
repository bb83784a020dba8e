"""What the test modules share that needs pytest: the fixtures around the native library and the vocabulary of the refusal tests.
Helpers that need no pytest live in util.py.  A module takes a fixture by importing it, under another name where it wants one:
`from support import nat_restoring as nat`; a module-scoped fixture is then set up and torn down once for that module."""
import pytest

import util

FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": every call that gets it is refused before anything could dereference it


def refused(nat, rc, match):
    assert rc == -1, rc
    with pytest.raises(nat.BeamformerError, match=match):
        nat.check()


def entry(name, **defaults):
    """call(nat, **kw) -> the return code of nat.lib.<name>, given the defaults updated by kw in the order the defaults are written here
    (the entry point's own), then None for the stream."""
    def call(nat, **kw):
        assert set(kw) <= set(defaults), sorted(set(kw) - set(defaults))
        a = dict(defaults)
        a.update(kw)                    # replaces values in place: the order stays that of the defaults
        return getattr(nat.lib, name)(*a.values(), None)
    return call


# ------------------------------------------------------------------ the native library on the GPU

@pytest.fixture(scope="module")
def nat(native):
    assert native.gpu_available(), "these tests need the MI355X"
    return native


@pytest.fixture(scope="module")
def nat_restoring(native):
    """nat for a module that changes the sizes: cfg1 comes back afterwards."""
    assert native.gpu_available(), "these tests need the MI355X"
    yield native
    util.configure("cfg1")


@pytest.fixture(params=[0, 1], ids=["f32_mfma", "bf16_split"])
def gemm_mode(request, native):
    """bf_fd_gemm_f32_mode for the test: the float32 matrix instruction, and the exact three-way bfloat16 split (same bounds for both)."""
    initial = native.lib.bf_fd_gemm_f32_mode(request.param)
    yield request.param
    native.lib.bf_fd_gemm_f32_mode(initial)


# ------------------------------------------------------------------ the native library without a GPU

@pytest.fixture()
def nat_cfg1(native):
    util.configure("cfg1")                 # 64 x 256, 11 x 11 directions
    native.lib.bf_clear_error()
    return native


@pytest.fixture(scope="module")
def lib(native):
    return native.lib


@pytest.fixture(scope="module")
def lib_clearing(native):
    L = native.lib
    L.bf_clear_error()
    yield L
    L.bf_clear_error()


@pytest.fixture(scope="module")
def lib_16x64(native):
    """The library at the refusal tests' sizes (those of test_api_refusals_host.py) with nothing loaded (a change of N_SAMPLES drops every
    table); cfg1 comes back afterwards."""
    M, N, X, Y, T = 16, 64, 5, 5, 8
    L = native.lib
    assert L.bf_configure(M, 32, X, Y, T) == 0 and L.bf_configure(M, N, X, Y, T) == 0
    L.bf_clear_error()
    yield L
    L.bf_clear_error()
    util.configure("cfg1")


@pytest.fixture(scope="module")
def sized(native):
    """The refusals compare with N_SAMPLES = 256."""
    import filtersum_np as fsn
    from interface import config
    config.configure(N_MICROPHONES=64, ACTIVE_TILES=1, N_SAMPLES=256, MAX_RES_X=fsn.GRID[0], MAX_RES_Y=fsn.GRID[1], N_TAPS=8)
    yield native
    util.configure("cfg1")


# ------------------------------------------------------------------ delays

@pytest.fixture(scope="module")
def grid_tau():
    """float64 [directions, 64]: the delays of filtersum_np.GRID on one array."""
    import directions_np as D
    import filtersum_np as fsn
    return D.calculate_delays(fsn.GRID[0], fsn.GRID[1], arrays=1).reshape(-1, 64)


@pytest.fixture(scope="module")
def scene_tau():
    import mvdr_np
    return mvdr_np.scene_tau()
