"""GPU (-m gpu): the batched pad / lerp kernels sweeping in the table's own order (csrc/sweep_order.h) -- every image bit-identical
to the CPU oracle, the digest's re-read count equal to the NumPy count under the NumPy order and below the flat order's.

Shapes: frames of 64 rows with 16 active microphones (every fourth), 9x45 and 13x21 grids (405 and 273 directions: a partial last
run of 8, a partial last pass of 128, forward and reversed segments; 13x21 also has cuts that are no row ends), 256 and 200
samples, 3 frames (an odd count: the last workgroup row owns one frame) and 2."""
import ctypes as C
import functools

import numpy as np
import pytest

import sweep_order_np as SO
from util import ALGOS, REL_TOL, max_rel
import util
from support import nat

pytestmark = pytest.mark.gpu

M_TOTAL, EVERY, T = 64, 4, 8
MICS = (np.arange(M_TOTAL // EVERY) * EVERY).astype(np.int32)
GRIDS = {"9x45": (9, 45), "13x21": (13, 21)}


def _tables(algo, X, Y):
    """(what the loader takes, the whole-sample rows the library keeps) for the 16 active microphones"""
    import directions_np as D
    d = SO.grid_delays(X, Y, EVERY)
    if algo == "pad":
        w = np.ascontiguousarray(D.whole_samples(d))
        return w, w
    return np.float32(d), SO.whole_of(d)


def _load(nat, algo, table, N, X, Y):
    from interface import config
    config.configure(N_MICROPHONES=M_TOTAL, N_SAMPLES=N, MAX_RES_X=X, MAX_RES_Y=Y, N_TAPS=T)
    if algo == "pad":
        t = np.ascontiguousarray(table, dtype=np.int32).ravel()
        nat.lib.load_coefficients_pad(nat.iptr(t), t.size)
    else:
        t = np.ascontiguousarray(table, dtype=np.float32).ravel()
        nat.lib.load_coefficients_lerp(nat.fptr(t), t.size)
    nat.check()


@functools.lru_cache(maxsize=None)
def _frames(N):
    import synth
    f = synth.frame_batch(M_TOTAL, N, 3)
    f.setflags(write=False)
    return f


_WANT = {}


def _want(oracle_lib, algo, table, N, X, Y, key):
    """Oracle images [3][D] of the three frames, computed once per (table, N)."""
    k = (algo, key, N)
    if k not in _WANT:
        orc = oracle_lib.Oracle(N, X, Y, T)
        orc.load(ALGOS[algo], np.asarray(table).reshape(X, Y, -1))
        w = np.stack([orc.mimo_range(ALGOS[algo], _frames(N)[f], MICS, 0, X * Y).reshape(-1) for f in range(3)])
        w.setflags(write=False)
        _WANT[k] = w
    return _WANT[k]


def _das(nat, algo, d_sig, F, lo, hi):
    torch = util.torch_gpu()
    out = torch.full((F, hi - lo), float("nan"), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_device(ALGOS[algo], d_sig.data_ptr(), M_TOTAL, out.data_ptr(), hi - lo, F, nat.iptr(MICS), MICS.size, lo, hi,
                                 torch.cuda.current_stream().cuda_stream) == 0, nat.check()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _reloads(nat):
    ch, st = C.c_longlong(-2), C.c_longlong(-2)
    assert nat.lib.bf_last_das_reloads(C.byref(ch), C.byref(st)) == 0
    return ch.value, st.value


def _check_count(nat, whole, lo, hi):
    """The digest of the last launch counted what NumPy counts under NumPy's order, and less than the flat order costs."""
    order, info = SO.sweep_order(whole, lo, hi)
    changes, steps = _reloads(nat)
    flat = SO.run_changes(whole, np.arange(lo, hi))
    print("range [%d, %d): re-reads %d (numpy %d), flat order %d, of %d steps; %d segments, %d reversed" %
          (lo, hi, changes, info["changes"], flat, steps, info["segments"], info["reversed"]))
    assert not info["identity"] and 0 < info["reversed"] < info["segments"]      # forward and reversed segments
    assert changes == info["changes"] == SO.run_changes(whole, order)
    assert changes < flat
    assert steps == -(-(hi - lo) // SO.DPW) * (SO.DPW - 1) * whole.shape[1]


@pytest.mark.parametrize("F", [3, 2])
@pytest.mark.parametrize("N", [256, 200])
@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_ordered_sweep_is_bit_identical(nat, oracle_lib, algo, grid, N, F):
    torch = util.torch_gpu()
    X, Y = GRIDS[grid]
    D = X * Y
    table, whole = _tables(algo, X, Y)
    want = _want(oracle_lib, algo, table, N, X, Y, grid)[:F]
    _load(nat, algo, table, N, X, Y)
    d_sig = torch.from_numpy(_frames(N)[:F].copy()).cuda()

    got = _das(nat, algo, d_sig, F, 0, D)
    assert nat.lib.bf_last_das_variant() == (8 if algo == "lerp" else 5)
    _check_count(nat, whole, 0, D)
    for f in range(F):
        assert np.array_equal(got[f], want[f]), f

    # a shard whose ends fall inside rows: its own order, the full maps' slice
    part = _das(nat, algo, d_sig, F, 5, D - 3)
    assert nat.lib.bf_last_das_variant() == (8 if algo == "lerp" else 5)
    _check_count(nat, whole, 5, D - 3)
    assert np.array_equal(part, got[:, 5:D - 3])

    # two shards cut inside a row, as two ranks would compute them
    cut = 262 if grid == "9x45" else 130
    assert cut % Y != 0
    both = np.concatenate([_das(nat, algo, d_sig, F, 0, cut), _das(nat, algo, d_sig, F, cut, D)], axis=1)
    assert np.array_equal(both, got)


@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_second_geometry_rebuilds_the_order(nat, oracle_lib, algo):
    """Two tables of one size (405 directions as 9x45, then as 15x27) loaded one after the other: same launch geometry, so the same
    digest key -- the second load must rebuild the order with the digest (the serpentine of rows of 45 would scatter the 15x27 maps)."""
    torch = util.torch_gpu()
    N, F = 256, 2
    d_sig = torch.from_numpy(_frames(N)[:F].copy()).cuda()
    for X, Y in ((9, 45), (15, 27)):
        table, whole = _tables(algo, X, Y)
        want = _want(oracle_lib, algo, table, N, X, Y, "%dx%d" % (X, Y))[:F]
        _load(nat, algo, table, N, X, Y)
        got = _das(nat, algo, d_sig, F, 0, X * Y)
        assert nat.lib.bf_last_das_variant() == (8 if algo == "lerp" else 5)
        order, info = SO.sweep_order(whole, 0, X * Y)
        assert _reloads(nat)[0] == info["changes"] == SO.run_changes(whole, order)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("algo", ["pad", "lerp"])
def test_random_table_still_takes_the_direction_outer_variant(nat, oracle_lib, algo):
    """Independent random delays: the rule returns the identity, more than half of the steps re-read, the digest build picks the
    direction-outer variant (3) as before -- images against the oracle under the bound that variant has always been held to."""
    torch = util.torch_gpu()
    X, Y, N, F = 24, 23, 256, 2
    rng = np.random.default_rng(77)
    delays = rng.uniform(0, 40.0, size=(X * Y, MICS.size))
    table = delays.astype(int).astype(np.int32) if algo == "pad" else np.float32(delays)
    whole = table if algo == "pad" else SO.whole_of(delays)
    assert SO.sweep_order(whole, 0, X * Y)[1]["identity"]
    want = _want(oracle_lib, algo, table, N, X, Y, "random")[:F]
    _load(nat, algo, table, N, X, Y)
    d_sig = torch.from_numpy(_frames(N)[:F].copy()).cuda()
    got = _das(nat, algo, d_sig, F, 0, X * Y)
    assert nat.lib.bf_last_das_variant() == 3
    changes, steps = _reloads(nat)
    assert changes == SO.run_changes(whole, np.arange(X * Y)) and 2 * changes > steps
    for f in range(F):
        assert max_rel(got[f], want[f]) <= REL_TOL, f
