"""CPU: bf_sweep_order (csrc/sweep_order.cpp) against the NumPy restatement of its rule (tests/sweep_order_np.py), and the same
translation unit alone under AddressSanitizer + UBSan in a stand-alone program (tests/sweep_order_main.cpp).

The rule orders the directions of a batched pad / lerp launch so that no run of 8 positions crosses a grid's row end: segments
are cut where more than half of the microphones' whole-sample delays change and alternate segments are reversed (a serpentine on
a rectangular grid), unless that does not lower the number of changes inside runs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sweep_order_np as SO
import util
from util import CONFIGS


def _table(name):
    if name in CONFIGS:
        c = CONFIGS[name]
        return np.ascontiguousarray(np.asarray(util.table_for("pad", name)).reshape(c["X"] * c["Y"], c["M"]))
    X, Y, every = {"9x45": (9, 45, 4), "13x21": (13, 21, 4), "37x31": (37, 31, 1)}[name]
    return SO.whole_of(SO.grid_delays(X, Y, every))


def _native_order(native, whole, lo, hi, dpw=SO.DPW):
    whole = np.ascontiguousarray(whole, dtype=np.int32)
    out = np.full(hi - lo, -1, dtype=np.int32)
    assert native.lib.bf_sweep_order(native.iptr(whole), whole.shape[0], whole.shape[1], lo, hi, dpw, native.iptr(out)) == 0
    return out


NAMES = ["cfg1", "cfg2", "shipped", "9x45", "13x21", "37x31"]


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_order_equals_the_rule(native, name, sub):
    whole = _table(name)
    D = whole.shape[0]
    lo, hi = (5, D - 3) if sub else (0, D)
    want, info = SO.sweep_order(whole, lo, hi)
    got = _native_order(native, whole, lo, hi)
    assert np.array_equal(got, want), info
    assert np.array_equal(np.sort(got), np.arange(lo, hi))            # a permutation of the range
    assert SO.run_changes(whole, got) == info["changes"] <= info["changes_identity"]


# (segments, reversed, changes of the identity, changes of the order): worked out once from the rule, see DESIGN.md section 4.1
EXPECTED = {
    ("cfg2", False): (101, 50, None, None),
    ("9x45", False): (9, 3, 792, 765),
    ("9x45", True): (None, None, 774, 750),
    ("13x21", False): (19, 6, 1135, 1084),       # cuts that are not row ends
    ("37x31", False): (37, 18, 13254, 11810),
}


@pytest.mark.parametrize("name,sub", sorted(EXPECTED))
def test_reference_values(native, name, sub):
    whole = _table(name)
    D = whole.shape[0]
    lo, hi = (5, D - 3) if sub else (0, D)
    _, info = SO.sweep_order(whole, lo, hi)
    got = _native_order(native, whole, lo, hi)
    seg, rev, ch_id, ch = EXPECTED[(name, sub)]
    print(name, sub, info)
    if seg is not None:
        assert (info["segments"], info["reversed"]) == (seg, rev)
    if ch is not None:
        assert (info["changes_identity"], info["changes"]) == (ch_id, ch)
        assert SO.run_changes(whole, got - 0) == ch and SO.run_changes(whole, np.arange(lo, hi)) == ch_id
    assert not info["identity"]


def test_identity_where_the_rule_gains_nothing(native):
    rng = np.random.default_rng(77)
    rand = rng.uniform(0, 40.0, size=(24 * 23, 64)).astype(int).astype(np.int32)   # independent delays: every position its own segment
    for whole in (rand, _table("cfg1")):
        D = whole.shape[0]
        for lo, hi in ((0, D), (5, D - 3), (7, 8)):
            assert np.array_equal(_native_order(native, whole, lo, hi), np.arange(lo, hi))
            assert SO.sweep_order(whole, lo, hi)[1]["identity"]
    # a run length that makes the serpentine pointless: one position per run shares nothing
    assert np.array_equal(_native_order(native, _table("9x45"), 0, 405, dpw=1), np.arange(405))


def test_refusals(native):
    whole = _table("9x45")
    out = np.zeros(405, dtype=np.int32)
    a = (native.iptr(whole), 405, 16)
    for bad in ((0, 406, 8), (-1, 405, 8), (7, 7, 8), (0, 405, 0)):
        assert native.lib.bf_sweep_order(*a, *bad, native.iptr(out)) == -1
        assert b"bf_sweep_order" in native.lib.bf_last_error()
    assert native.lib.bf_sweep_order(None, 405, 16, 0, 405, 8, native.iptr(out)) == -1
    assert native.lib.bf_sweep_order(*a, 0, 405, 8, None) == -1
    native.lib.bf_clear_error()


def test_alone_under_address_and_ub_sanitizers(tmp_path):
    """csrc/sweep_order.cpp and a main() of its own, nothing else, built with -fsanitize=address,undefined: the orders equal the
    rule's on the small tables, and the run reports nothing."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    import __graft_entry__ as ge
    exe = str(tmp_path / "sweep_order_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", ge.CSRC, os.path.join(ge.CSRC, "sweep_order.cpp"), os.path.join(util.ROOT, "tests", "sweep_order_main.cpp"), "-o", exe])
    rng = np.random.default_rng(5)
    tables = {"9x45": _table("9x45"), "13x21": _table("13x21"), "random": rng.integers(0, 40, size=(99, 16)).astype(np.int32),
              "one": _table("13x21")[:1]}
    for name, whole in tables.items():
        D, M = whole.shape
        for lo, hi in {(0, D), (min(5, D - 1), max(D - 3, min(5, D - 1) + 1))}:
            src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
            with open(src, "wb") as f:
                f.write(np.asarray([D, M, lo, hi, SO.DPW], dtype=np.int32).tobytes() + np.ascontiguousarray(whole, dtype=np.int32).tobytes())
            r = subprocess.run([exe, src, dst], stderr=subprocess.PIPE, text=True, timeout=60)
            assert r.returncode == 0 and not r.stderr, (name, lo, hi, r.returncode, r.stderr[-2000:])
            raw = open(dst, "rb").read()
            n = hi - lo
            order = np.frombuffer(raw[:4 * n], dtype=np.int32)
            seg, rev, ident = np.frombuffer(raw[4 * n:4 * n + 12], dtype=np.int32)
            ch_id, ch = np.frombuffer(raw[4 * n + 12:], dtype=np.int64)
            want, info = SO.sweep_order(whole, lo, hi)
            assert np.array_equal(order, want), (name, lo, hi)
            assert (seg, rev, bool(ident), ch_id, ch) == (info["segments"], info["reversed"], info["identity"], info["changes_identity"], info["changes"])
