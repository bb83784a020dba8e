"""CPU: bf_filter_sum_device without a device -- the restatement against a direct miso_pad (tests/filtersum_np.py), every refusal that
sits before device bring-up, the null-steering designer (filtersum.design_lcmv) at every in-band bin, and the claim the feature
rests on: on the 8 x 8 array a delay-and-sum beam passes a second talker a few dB down, a null-steered beam tens of dB down.

Sizes of the refusals: 16 microphones, 64 samples, as tests/test_band_filter_host.py."""
import numpy as np
import pytest

import filtersum_np as fsn
import util
from support import FAKE, grid_tau as tau, lib_16x64 as lib

M, N, X, Y, T = 16, 64, 5, 5, 8


# ------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("n_samples,taps,n,m_total", [(64, 1, 1, 1), (64, 17, 5, 9), (100, 48, 7, 7), (99, 99, 3, 4)])
def test_delta_taps_are_miso_pad(n_samples, taps, n, m_total):
    rng = np.random.default_rng([n_samples, taps, n])
    F, B = 2, 3
    x = util.wild(rng, (F, m_total, n_samples))
    x[0, 0, :4] = [-0.0, 0.0, -1e-45, 1e-45]                         # signed zeros and denormals pass through a delta chain
    mics = rng.permutation(m_total)[:n]
    delays = rng.integers(0, taps, size=(B, n))
    delays[0, 0] = taps - 1
    got = fsn.filter_sum(x, mics, fsn.delta_taps(delays, taps))
    for f in range(F):
        for b in range(B):
            assert np.array_equal(util.bits(got[f, b]), util.bits(fsn.miso_pad(x[f], mics, delays[b])))


def test_restatement_overlap_and_order():
    rng = np.random.default_rng(4)
    n_samples, taps, hop, F, m_total = 64, 9, 16, 4, 6
    S = util.wild(rng, (m_total, hop * F + n_samples))
    frames = np.stack([S[:, (f + 1) * hop:(f + 1) * hop + n_samples] for f in range(F)])
    prev = np.ascontiguousarray(S[:, :n_samples])
    mics = np.array([4, 0, 5, 2])
    g = util.wild(rng, (2, 4, taps))
    y = fsn.filter_sum(frames, mics, g, hop, prev)
    for f in range(1, F):                                            # overlapping windows agree where both exist
        assert np.array_equal(util.bits(y[f, :, :n_samples - hop]), util.bits(y[f - 1, :, hop:]))
    a = fsn.filter_sum(frames[:2], mics, g, hop, prev)
    b = fsn.filter_sum(frames[2:], mics, g, hop, frames[1])           # the carried window
    assert np.array_equal(util.bits(np.concatenate([a, b])), util.bits(y))
    # the microphone order is part of the definition: the same rows and taps summed backwards round differently somewhere
    back = fsn.filter_sum(frames, mics[::-1], g[:, ::-1], hop, prev)
    assert not np.array_equal(util.bits(back), util.bits(y)) and np.allclose(back, y, rtol=1e-3, atol=1e-3 * np.abs(y).max())


# ------------------------------------------------------------------ refusals before device bring-up


MICS = np.array([3, 0, 15, 7], dtype=np.int32)
D_TAPS, D_OUT = FAKE + 0x100000, FAKE + 0x200000


def _call(native, d_signals=FAKE, m_total=M, frames=2, hop=32, d_prev=None, mics=MICS, n=None, d_taps=D_TAPS, n_taps=9, beams=2, d_out=D_OUT,
          out_stride=N):
    n = (0 if mics is None else len(mics)) if n is None else n
    return native.lib.bf_filter_sum_device(d_signals, m_total, frames, hop, d_prev, None if mics is None else native.iptr(mics), n, d_taps, n_taps, beams,
                                           d_out, out_stride, None)


IN_BYTES = 2 * M * N * 4            # of _call's default batch
OUT_BYTES = 2 * 2 * N * 4
TAP_BYTES = 2 * 4 * 9 * 4
W = "bf_filter_sum_device: "


@pytest.mark.parametrize("kw,text", [
    (dict(d_signals=None), "d_signals is null"),
    (dict(mics=None, n=4), "adaptive_array is null"),
    (dict(d_taps=None), "d_taps is null"),
    (dict(d_out=None), "d_out is null"),
    (dict(d_signals=None, d_out=None, frames=0), "d_signals is null"),
    (dict(frames=0), "frames = 0 < 1"),
    (dict(frames=-3, beams=0), "frames = -3 < 1"),
    (dict(n=0), "n = 0 < 1"),
    (dict(beams=0), "beams = 0 < 1"),
    (dict(n_taps=0), "n_taps = 0 < 1"),
    (dict(n_taps=-1, hop=-1), "n_taps = -1 < 1"),
    (dict(beams=17), "beams = 17 > 16"),
    (dict(n_taps=65, hop=64), "n_taps = 65 > N_SAMPLES = 64"),
    (dict(hop=-1), "hop = -1 < 0"),
    (dict(hop=65), "hop = 65 > N_SAMPLES = 64 (the windows would leave gaps in the stream)"),
    (dict(hop=7), "the filters need n_taps - 1 = 8 samples of history but hop = 7 (continuous mode wants n_taps - 1 <= hop)"),
    (dict(n_taps=64, hop=62), "the filters need n_taps - 1 = 63 samples of history but hop = 62 (continuous mode wants n_taps - 1 <= hop)"),
    (dict(out_stride=63), "out_stride = 63 < N_SAMPLES = 64"),
    (dict(mics=np.array([3, 16, 1], dtype=np.int32)), "adaptive_array[1] = 16 is not a row of frames with m_total = 16 rows"),
    (dict(mics=np.array([-1], dtype=np.int32)), "adaptive_array[0] = -1 is not a row of frames with m_total = 16 rows"),
    (dict(m_total=0), "adaptive_array[0] = 3 is not a row of frames with m_total = 0 rows"),
    (dict(d_out=FAKE), "d_out overlaps d_signals"),
    (dict(d_out=FAKE + IN_BYTES - 4), "d_out overlaps d_signals"),
    (dict(d_signals=D_OUT + OUT_BYTES - 4), "d_out overlaps d_signals"),
    (dict(d_signals=D_OUT + OUT_BYTES + 12 * 4 - 4, out_stride=N + 4), "d_out overlaps d_signals"),
    (dict(d_prev=D_OUT - M * N * 4 + 4), "d_out overlaps d_prev"),
    (dict(d_prev=D_OUT + OUT_BYTES - 4), "d_out overlaps d_prev"),
    (dict(d_taps=D_OUT - TAP_BYTES + 4), "d_out overlaps d_taps"),
    (dict(d_taps=D_OUT + OUT_BYTES - 4), "d_out overlaps d_taps"),
])
def test_refusals(native, lib, kw, text):
    assert _call(native, **kw) == -1
    assert lib.bf_last_error().decode() == W + text
    lib.bf_clear_error()


def test_accepted_arguments_reach_the_device_check(native, lib):
    """Ranges that only touch (the floats behind the last row's N_SAMPLES are not part of d_out's range), hop = 0 with a long filter,
    hop = n_taps - 1, 16 beams, a repeated row: all pass the argument checks, so without a GPU the one refusal left is the missing
    device (with one, fake pointers must not be launched: nothing is called)."""
    assert lib.bf_filter_sum_waves(3) == -1 and lib.bf_filter_sum_waves(8) == 0 and lib.bf_filter_sum_waves(0) == 8      # needs no device
    if native.gpu_available():
        return
    for kw in (dict(d_out=FAKE + IN_BYTES), dict(d_signals=D_OUT + OUT_BYTES), dict(d_prev=D_OUT - M * N * 4), dict(d_taps=D_OUT - TAP_BYTES),
               dict(d_signals=D_OUT + OUT_BYTES + 12 * 4, out_stride=N + 4), dict(hop=0, n_taps=64), dict(hop=8), dict(beams=16), dict(hop=64, n_taps=64),
               dict(mics=np.array([2, 2], dtype=np.int32)), dict(out_stride=1000)):
        assert _call(native, **kw) == -1
        assert lib.bf_last_error().decode().startswith("no usable HIP device")
        lib.bf_clear_error()


# ------------------------------------------------------------------ the designer


def _in_band_rho(tau, a, b, T):
    import filtersum
    w = 2.0 * np.pi * filtersum.band_bins(T, fsn.BAND, fsn.FS) / T
    return np.abs(np.sum(np.exp(1j * w[:, None] * (tau[b] - tau[a])[None, :]), axis=1)) / tau.shape[1]


@pytest.mark.parametrize("T", [33, 65])
def test_design_meets_its_constraints_at_every_bin(native, tau, T):
    """|H(w_k, look) - e^{-j w_k (T-1)/2}| and |H(w_k, null)| against 2^-22 sum|g|: the taps are the float64 design rounded once to
    float32, each tap off by at most 2^-24 |g| ... times four (the float64 design's own residual is about 1e-8)."""
    import filtersum
    look, null = fsn.flat(fsn.LOOK), fsn.flat(fsn.INTERFERER)
    rho = _in_band_rho(tau, look, null, T)
    print("T = %d: largest in-band rho %.3f" % (T, rho.max()))
    assert rho.max() < 0.95
    taps, kept = filtersum.design_lcmv(tau, [look], [[null]], n_taps=T, band=fsn.BAND, fs=fsn.FS)
    bins = filtersum.band_bins(T, fsn.BAND, fsn.FS)
    assert taps.dtype == np.float32 and taps.shape == (1, 64, T) and kept.shape == (1, bins.size, 1) and kept.all()
    assert bins[0] * fsn.FS / T >= fsn.BAND[0] > (bins[0] - 1) * fsn.FS / T and bins[-1] * fsn.FS / T <= fsn.BAND[1] < (bins[-1] + 1) * fsn.FS / T
    bound = 2.0 ** -22 * float(np.abs(taps[0].astype(np.float64)).sum())
    w = 2.0 * np.pi * bins / T
    e_look = np.abs(filtersum.response(taps[0], tau[look], w) - np.exp(-1j * w * (T - 1) / 2.0))
    e_null = np.abs(filtersum.response(taps[0], tau[null], w))
    print("T = %d: look error %.3g, null response %.3g, bound %.3g" % (T, e_look.max(), e_null.max(), bound))
    assert (e_look <= bound).all() and (e_null <= bound).all()
    assert isinstance(filtersum.response(taps[0], tau[look], float(w[0])), complex)
    # no nulls: band-limited delay-and-sum with exact fractional delays
    das, kept0 = filtersum.design_lcmv(tau, [look], None, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    assert kept0.shape == (1, bins.size, 0)
    bound0 = 2.0 ** -22 * float(np.abs(das[0].astype(np.float64)).sum())
    assert (np.abs(filtersum.response(das[0], tau[look], w) - np.exp(-1j * w * (T - 1) / 2.0)) <= bound0).all()
    # outside the band the grid bins are zero
    out_of_band = np.setdiff1d(np.arange(T // 2 + 1), bins)
    assert (np.abs(filtersum.response(taps[0], tau[look], 2.0 * np.pi * out_of_band / T)) <= bound).all()


def test_a_null_too_close_to_the_look_direction_is_dropped(native, tau):
    import filtersum
    look, near, far = fsn.flat(fsn.LOOK), fsn.flat(fsn.NEAR), fsn.flat(fsn.INTERFERER)
    rho = _in_band_rho(tau, look, near, 65)
    print("null at %s: rho %.3f at the lowest in-band bin" % (fsn.NEAR, rho[0]))
    assert rho[0] > 0.95
    taps, kept = filtersum.design_lcmv(tau, [look, look], [[near, far], [far]], n_taps=65, band=fsn.BAND, fs=fsn.FS)
    assert kept.shape == (2, rho.size, 2)
    assert np.array_equal(kept[0, :, 0], rho <= 0.95) and not kept[0, 0, 0] and kept[0, -1, 0]
    assert kept[0, :, 1].all() and kept[1, :, 0].all() and not kept[1, :, 1].any()       # entries past a beam's own list are False
    # where the near null was dropped the look constraint still holds
    w0 = 2.0 * np.pi * filtersum.band_bins(65, fsn.BAND, fsn.FS)[0] / 65
    bound = 2.0 ** -22 * float(np.abs(taps[0].astype(np.float64)).sum())
    assert abs(filtersum.response(taps[0], tau[look], w0) - np.exp(-1j * w0 * 32.0)) <= bound
    with pytest.raises(ValueError):
        filtersum.design_lcmv(tau, [look], [[far], [far]])
    with pytest.raises(ValueError):
        filtersum.design_lcmv(tau, [tau.shape[0]])
    with pytest.raises(ValueError):
        filtersum.design_lcmv(tau, [look], band=(100.0, 200.0), n_taps=9, fs=fsn.FS)


# ------------------------------------------------------------------ the scene

def test_null_steering_takes_the_second_talker_out(native, tau):
    """Float64 throughout.  Two independent 3-8 kHz noise sources at (20, 11) and (28, 14); the beam looks at the first.  Measured
    here: delay-and-sum (the same designer without nulls) passes the interferer 5.0 dB down, the 65-tap null-steered beam 34.6 dB
    down -- 29.6 dB better; floor 20 dB -- and the look source at -0.01 dB; spatially white noise comes out at -22.4 dB against -24.7 dB
    (README)."""
    import filtersum
    rng = np.random.default_rng(0)
    L, T = 8192, 65
    look, null = fsn.flat(fsn.LOOK), fsn.flat(fsn.INTERFERER)
    lcmv, _ = filtersum.design_lcmv(tau, [look], [[null]], n_taps=T, band=fsn.BAND, fs=fsn.FS)
    das, _ = filtersum.design_lcmv(tau, [look], None, n_taps=T, band=fsn.BAND, fs=fsn.FS)
    S_look, S_int = fsn.band_noise(rng, L), fsn.band_noise(rng, L)
    x_look, x_int = fsn.at_microphones(S_look, tau[look], L), fsn.at_microphones(S_int, tau[null], L)
    power = lambda y: float(np.mean(y ** 2))                           # both sources have unit power
    leak_das, leak_lcmv = fsn.db(power(fsn.beam_f64(x_int, das[0]))), fsn.db(power(fsn.beam_f64(x_int, lcmv[0])))
    gain_look = fsn.db(power(fsn.beam_f64(x_look, lcmv[0])))
    white = fsn.db(float(np.sum(lcmv[0].astype(np.float64) ** 2))), fsn.db(float(np.sum(das[0].astype(np.float64) ** 2)))
    print("interferer: delay-and-sum %.1f dB, null-steered %.1f dB (%.1f dB better); look gain %.2f dB; white noise %.1f dB against %.1f dB"
          % (leak_das, leak_lcmv, leak_das - leak_lcmv, gain_look, white[0], white[1]))
    assert leak_das - leak_lcmv >= 20.0
    assert abs(gain_look) <= 0.5
