"""CPU: the oracle (oracle/directions_np.py + oracle/das_oracle.c) against the golden vectors that
oracle/gen_golden.py produced by running the compiled reference.  This is what pins the oracle."""
import os

import numpy as np
import pytest

import util
from util import CONFIGS, golden, sha


@pytest.mark.parametrize("name", list(CONFIGS))
def test_tables_bit_exact(name):
    import directions_np as D
    c, g = CONFIGS[name], golden(name)
    act, n = D.active_microphones(arrays=c["arrays"])
    assert np.array_equal(act, g["active_mics"]) and n == c["M"]
    rp = D.calc_r_prime(float(np.float32(0.02)), arrays=c["arrays"])
    assert rp.tobytes() == g["r_prime"].tobytes()
    d = util.oracle_delays(name)
    assert sha(d) == str(g["delay_sha256"])
    assert np.array_equal(d.reshape(-1, c["M"])[g["delay_rows_idx"]], g["delay_rows"])
    assert sha(D.whole_samples(d)) == str(g["whole_sha256"])
    assert sha(np.float32(d)) == str(g["delay_f32_sha256"])
    assert [d.min(), d.max()] == list(g["delay_minmax"])


def test_tap_generators_bit_exact():
    import directions_np as D
    g = golden("cfg1")
    for x, h1, h2 in zip(g["tap_probe_delay"], g["tap_probe_get_h"], g["tap_probe_get_h2"]):
        assert np.array_equal(D.get_h(float(x)), h1)
        assert np.array_equal(D.get_h2(float(x)), h2)
    d = g["delay"]
    whole, h = D.calculate_coefficients(d)
    assert np.array_equal(h, g["taps_get_h"])
    assert np.array_equal(D.compute_convolve_h(d), g["taps_get_h2"])


def test_inputs_regenerate():
    for name in CONFIGS:
        g, ins = golden(name), util.inputs(name)
        for k, v in ins.items():
            assert sha(v) == str(g["in_sha256_" + k]), (name, k)
        assert np.array_equal(ins["s1"][0], g["s1_row"])


IMAGE_CASES = [(n, a, s) for n in ("cfg1", "cfg2", "shipped") for a in ("pad", "lerp", "hybrid", "fir_vec") for s in ("s1", "s2", "s3")
               if not (a == "fir_vec" and s == "s3")]


@pytest.mark.parametrize("name,algo,sig", IMAGE_CASES)
def test_images_bit_exact(oracle_lib, name, algo, sig):
    """Full images at cfg1; at the larger sizes 48 sampled directions (the full images take minutes on one core
    and are covered on the GPU side, where the HIP path is compared with these same golden images)."""
    c, g = CONFIGS[name], golden(name)
    key = "img_%s_%s" % ({"fir_vec": "convolve"}.get(algo, algo), sig)
    want = g[key].reshape(-1)
    orc = oracle_lib.Oracle(c["N"], c["X"], c["Y"], c["T"])
    s = util.inputs(name)[sig]
    mics = np.arange(c["M"], dtype=np.int32)
    a = util.ALGOS[algo]
    orc.load(a, util.table_for(algo, name))
    D = c["X"] * c["Y"]
    if name == "cfg1":
        got = orc.mimo_range(a, s, mics, 0, D)
        assert np.array_equal(got, want)
    else:
        for d in np.random.default_rng(3).choice(D, 48, replace=False):
            got = orc.mimo_range(a, s, mics, int(d), int(d) + 1)
            assert got[0] == want[d], (name, algo, sig, int(d))


def test_cfg5_sampled_directions(oracle_lib):
    """256 mics x 1024 samples x 361x361: 16 sampled directions of the golden lerp/hybrid images."""
    name = "cfg5"
    c, g = CONFIGS[name], golden(name)
    orc = oracle_lib.Oracle(c["N"], c["X"], c["Y"], c["T"])
    mics = np.arange(c["M"], dtype=np.int32)
    ins = util.inputs(name)
    picks = np.random.default_rng(5).choice(c["X"] * c["Y"], 16, replace=False)
    orc.load(1, util.table_for("lerp", name))
    for sig in ("s1", "s2"):
        want = g["img_lerp_" + sig].reshape(-1)
        for d in picks:
            assert orc.mimo_range(1, ins[sig], mics, int(d), int(d) + 1)[0] == want[d]


# ---- fixtures taken from the reference's C compiled where it lies (oracle/gen_golden_refc.py -> tests/golden/refc.npz)

def test_refc_cfg5_pad_sampled_directions(oracle_lib):
    """mimo_pad at 256 mics x 1024 x 361x361: 32 sampled directions of the compiled reference's images, bit for bit."""
    name = "cfg5"
    c, g = CONFIGS[name], golden("refc")
    orc = oracle_lib.Oracle(c["N"], c["X"], c["Y"], c["T"])
    mics = np.arange(c["M"], dtype=np.int32)
    ins = util.inputs(name)
    whole = util.table_for("pad", name)
    assert sha(whole) == str(g["cfg5/whole_sha256"])
    orc.load(0, whole)
    picks = np.random.default_rng(11).choice(c["X"] * c["Y"], 32, replace=False)
    for sig in ("s1", "s2"):
        assert sha(ins[sig]) == str(g["cfg5/in_sha256_" + sig])
        want = g["cfg5/img_pad_" + sig].reshape(-1)
        for d in picks:
            assert orc.mimo_range(0, ins[sig], mics, int(d), int(d) + 1)[0] == want[d]


@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_refc_convolve_naive(oracle_lib, name):
    """mimo_convolve_naive (convolve_and_sum.c:231-272), which no Cython wrapper of the reference calls: the oracle's naive FIR
    order against the compiled reference -- all of cfg1, 48 sampled directions of cfg2."""
    c, g = CONFIGS[name], golden("refc")
    orc = oracle_lib.Oracle(c["N"], c["X"], c["Y"], c["T"])
    mics = np.arange(c["M"], dtype=np.int32)
    taps = np.ascontiguousarray(util.table_for("fir_naive", name), dtype=np.float32)
    assert sha(taps) == str(g[name + "/taps_sha256"])
    orc.load(3, taps)
    D = c["X"] * c["Y"]
    picks = range(D) if name == "cfg1" else np.random.default_rng(13).choice(D, 48, replace=False)
    for sig in ("s1", "s2"):
        want = g["%s/img_naive_%s" % (name, sig)].reshape(-1)
        x = util.inputs(name)[sig]
        for d in picks:
            assert orc.mimo_range(3, x, mics, int(d), int(d) + 1)[0] == want[d], (name, sig, int(d))


# ---- the oracle against oracle/_ref directly ("equals it bit for bit")

def shared_entry_points(eng, name):
    """Every entry point the oracle and the compiled reference share, on one seeded random block: key -> output array
    (whole images and the tables the loaders build).  oracle/gen_golden_refhash.py records the reference's side of it."""
    c = CONFIGS[name]
    rng = np.random.default_rng(17)
    sig = (rng.standard_normal((c["M"], c["N"])) * 0.25).astype(np.float32)
    mics = np.arange(c["M"], dtype=np.int32)
    d = util.oracle_delays(name)
    whole, d32 = util.table_for("pad", name), np.float32(d)
    out = {"mimo_pad": eng.mimo_pad(sig, whole, mics), "mimo_lerp": eng.mimo_lerp(sig, d32, mics),
           "mimo_hybrid": eng.mimo_hybrid(sig, d32, mics)}
    out["lerp_tables/whole"], out["lerp_tables/frac"] = eng.lerp_tables(d32.ravel())
    out["hybrid_tables/whole"], out["hybrid_tables/taps"] = eng.hybrid_tables(d32.ravel())
    off = (c["X"] * c["Y"] // 3) * c["M"]
    out["miso_pad"] = eng.miso_pad(sig, whole, mics, off)
    out["miso_lerp"] = eng.miso_lerp(sig, d32, mics, off)
    if name == "cfg1":
        taps = np.ascontiguousarray(util.table_for("fir_vec", name), dtype=np.float32)
        for vec in (False, True):
            out["mimo_convolve/vectorized=%d" % vec] = eng.mimo_convolve(sig, taps, mics, vectorized=vec)
    out.update(miso_and_helpers(eng, sig, d32.ravel(), off // c["M"], np.random.default_rng(19)))
    return out


def miso_and_helpers(eng, sig, d32, direction, rng):
    """The MISO entry points the reference's Cython wrappers never call (miso_convolve_vectorized, miso_convolve_hybrid,
    miso_pad2) at table offset `direction`, and the seven single-signal helpers on one row: key -> float32 [N].
    `d32` is the flat float32 delay table [D * M] (D >= direction + 1); the FIR taps, the pad2 table, the microphone list
    of miso_pad2 and the helpers' inputs are drawn from `rng`."""
    M, N, T = sig.shape[0], eng.N, eng.T
    D = d32.size // M
    out = {}
    taps = rng.uniform(-0.5, 0.5, D * M * T).astype(np.float32)
    out["miso_convolve_vectorized"] = eng.miso_convolve_vectorized(sig, taps, np.arange(M, dtype=np.int32), direction * M * T)
    out["miso_convolve_hybrid"] = eng.miso_hybrid(sig, d32, np.arange(M, dtype=np.int32), direction * M)
    # pad2: delays by microphone id (one of them past the block), a permuted subset of the microphones with gaps
    by_mic = np.floor(d32[direction * M:(direction + 1) * M]).astype(np.int32)
    by_mic[rng.integers(M)] = N + 3
    keep = rng.permutation(M)[:(3 * M) // 4].astype(np.int32)
    out["miso_pad2"] = eng.miso_pad2(sig, by_mic, keep, direction * M)
    x = sig[3]
    base = rng.standard_normal(N).astype(np.float32)
    h = rng.uniform(-0.5, 0.5, T).astype(np.float32)
    hyb = rng.uniform(-0.5, 0.5, T).astype(np.float32)
    out["pad_delay"] = eng.pad_delay(x, base, 17)
    out["lerp_delay"] = eng.lerp_delay(x, base, 0.3125, 9)
    out["convolve_delay_naive"] = eng.convolve_delay_naive(x, base, h)
    out["convolve_delay_naive_add"] = eng.convolve_delay_naive_add(x, h, base)
    out["convolve_delay_vectorized"] = eng.convolve_delay_vectorized(x, h, base)      # overwrites: `base` must not show
    out["convolve_delay_vectorized_add"] = eng.convolve_delay_vectorized_add(x, h, base)
    out["convolve_hybrid_delay_add"] = eng.convolve_hybrid_delay_add(x, hyb, 5, base)
    return out


def miso_small_table(eng, name):
    """miso_and_helpers at one size on a small seeded table of five directions (at cfg5 the full 361 x 361 x 256 table takes
    minutes to build): delays up to N + 40 -- some past the block -- and the middle direction.  Plus miso_pad / miso_lerp at
    the last direction of that table.  oracle/gen_golden_refhash.py records the compiled reference's side."""
    c = CONFIGS[name]
    M, N, D = c["M"], c["N"], 5
    rng = np.random.default_rng(23)
    sig = (rng.standard_normal((M, N)) * 0.25).astype(np.float32)
    d32 = rng.uniform(0, N + 40, D * M).astype(np.float32)
    mics = np.arange(M, dtype=np.int32)
    out = miso_and_helpers(eng, sig, d32, D // 2, rng)
    out["miso_pad"] = eng.miso_pad(sig, np.floor(d32).astype(np.int32), mics, (D - 1) * M)
    out["miso_lerp"] = eng.miso_lerp(sig, d32, mics, (D - 1) * M)
    return out


@pytest.mark.parametrize("name", ["cfg1", "shipped"])
def test_oracle_equals_compiled_reference(oracle_lib, name):
    """Same random block through both CPU engines: every entry point the two share, whole images, bit for bit -- against
    the SHA-256 of the compiled reference's outputs recorded in tests/golden/refc_hashes.json (oracle/gen_golden_refhash.py),
    and against the compiled reference itself where oracle/_ref has been built (oracle/build_ref.py)."""
    import json
    c = CONFIGS[name]
    got = shared_entry_points(oracle_lib.Oracle(c["N"], c["X"], c["Y"], c["T"]), name)
    rec = json.load(open(os.path.join(util.GOLDEN, "refc_hashes.json")))["entry_points"][name]
    assert sorted(got) == sorted(rec)
    for key, a in got.items():
        assert sha(a) == rec[key], (name, key)
    if oracle_lib.RefLib.available(name):
        want = shared_entry_points(oracle_lib.RefLib(name), name)
        for key, a in got.items():
            assert a.dtype == want[key].dtype and a.tobytes() == want[key].tobytes(), (name, key)


def test_miso_cfg5_equals_compiled_reference(oracle_lib):
    """N = 1024 (BASELINE config 5): every MISO entry point and single-signal helper on a small seeded table, bit for bit
    against the SHA-256 of the compiled reference's outputs (refc_hashes.json `miso_small_table`), and against the compiled
    reference itself where oracle/_ref has been built."""
    import json
    name = "cfg5"
    c = CONFIGS[name]
    got = miso_small_table(oracle_lib.Oracle(c["N"], c["X"], c["Y"], c["T"]), name)
    rec = json.load(open(os.path.join(util.GOLDEN, "refc_hashes.json")))["miso_small_table"][name]
    assert sorted(got) == sorted(rec)
    for key, a in got.items():
        assert a.dtype == np.float32 and a.shape == (c["N"],), key
        assert sha(a) == rec[key], (name, key)
    if oracle_lib.RefLib.available(name):
        want = miso_small_table(oracle_lib.RefLib(name), name)
        for key, a in got.items():
            assert a.tobytes() == want[key].tobytes(), (name, key)
