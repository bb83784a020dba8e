"""GPU: every stage of the frequency-domain beamformers (csrc/freq_kernels.hip) through its own C-ABI call against the float64 references of
tests/fd_cases.py, at the shapes that reach each branch of the launch code (tests/test_fd_stages_host.py checks on the CPU that they do):
steering phasors, covariance, the Cholesky inverse on its register / LDS / blocked routes with the status it reports, the two bin-reducing
GEMMs in both bf_fd_gemm_f32_mode settings, the DFT with gathered rows, and the three MVDR stages chained."""
import numpy as np
import pytest

import fd_cases as FC
import util
from support import gemm_mode

pytestmark = pytest.mark.gpu


def _dev(v):
    import torch
    return torch.from_numpy(np.array(v, order="C")).cuda()         # (a copy: the cases' arrays are read-only)


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _f64(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize("case", FC.names(FC.STEERING))
def test_steering_matches_float64(native, case):
    """bf_fd_steering_device: a[k][m][d] = exp(-j 2 pi freq[k] tau[d][m]) within 2^-23 of the float32 of the float64 value, every element
    written, and the freq = 0 plane exactly (1, 0)."""
    c = FC.BY_NAME[case]
    tau, freq = FC.steering_data(case)
    d_tau, d_freq = _dev(tau), _dev(freq)
    are, aim = _nan(c.K, c.M, c.D), _nan(c.K, c.M, c.D)
    assert native.lib.bf_fd_steering_device(d_tau.data_ptr(), d_freq.data_ptr(), c.D, c.M, c.K, are.data_ptr(), aim.data_ptr(), None) == 0, native.check()
    got_re, got_im = _f64(are), _f64(aim)
    want_re, want_im = FC.steering_want(case)
    err = max(np.max(np.abs(got_re - want_re)), np.max(np.abs(got_im - want_im)))       # (a NaN left behind makes this NaN)
    print("%s: max |error| = %.3g (bound %.3g)" % (case, err, FC.STEERING_TOL))
    assert err <= FC.STEERING_TOL
    assert (got_re[0] == 1.0).all() and (got_im[0] == 0.0).all()


@pytest.mark.parametrize("case", FC.names(FC.COVARIANCE))
def test_covariance_matches_float64(native, case):
    """bf_fd_covariance_device: R[b] = (1/F) sum_f x x^H against complex128, each entry within its own float32 accumulation bound
    (fd_cases.covariance_bound), all B * M * M entries written."""
    c = FC.BY_NAME[case]
    x = FC.covariance_data(case)
    xr, xi = _dev(x.real), _dev(x.imag)
    rr, ri = _nan(c.B, c.M, c.M), _nan(c.B, c.M, c.M)
    assert native.lib.bf_fd_covariance_device(xr.data_ptr(), xi.data_ptr(), c.F, c.M, c.B, rr.data_ptr(), ri.data_ptr(), None) == 0, native.check()
    got_re, got_im = _f64(rr), _f64(ri)
    assert np.isfinite(got_re).all() and np.isfinite(got_im).all()
    want, bound = FC.covariance_f64(x), FC.covariance_bound(x)
    frac = max(np.max(np.abs(got_re - want.real) / bound), np.max(np.abs(got_im - want.imag) / bound))
    print("%s: max error = %.4f of the per-entry bound" % (case, frac))
    assert frac <= 1.0


def _cholesky(native, rr, ri, loading=FC.LOADING):
    """bf_fd_cholesky_inverse_device on float32 planes [B, M, M]: (re, im) planes as float64 [b][c][r] = Linv[r][c], status int [B]."""
    import torch
    B, M = rr.shape[0], rr.shape[1]
    d_rr, d_ri = _dev(rr), _dev(ri)
    lr, li = _nan(B, M, M), _nan(B, M, M)
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    assert native.lib.bf_fd_cholesky_inverse_device(d_rr.data_ptr(), d_ri.data_ptr(), M, B, loading, lr.data_ptr(), li.data_ptr(), st.data_ptr(), None) == 0, native.check()
    return lr.cpu().numpy(), li.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("case", FC.names(FC.CHOLESKY))
def test_cholesky_inverse_matches_float64(native, case):
    """bf_fd_cholesky_inverse_device on three distinct matrices: inverse(cholesky(R + loading tr(R)/M I)) of the float32-rounded input in
    complex128 within 2e-4 of its largest entry, zeros above the diagonal and in the diagonal's imaginary part, status 0, every entry written."""
    c = FC.BY_NAME[case]
    rr, ri = FC.spd(case, c.M)
    lr, li, st = _cholesky(native, rr, ri)
    assert np.isfinite(lr).all() and np.isfinite(li).all()
    assert st.tolist() == [0] * FC.CHOLESKY_BINS
    want = FC.cholesky_want(case)
    worst = 0.0
    for b in range(FC.CHOLESKY_BINS):
        got = (lr[b].astype(np.float64) + 1j * li[b].astype(np.float64)).T
        worst = max(worst, np.max(np.abs(got - want[b])) / np.max(np.abs(want[b])))
        assert np.max(np.abs(np.triu(got, 1)), initial=0.0) == 0.0, b
        assert (np.diag(got).imag == 0.0).all(), b
    print("%s (%s): max error = %.3g of max |want| (bound %.3g)" % (case, c.route, worst, FC.CHOLESKY_TOL))
    assert worst <= FC.CHOLESKY_TOL


@pytest.mark.parametrize("case", FC.names(FC.STATUS))
def test_cholesky_status_names_the_first_bad_pivot(native, case):
    """Three bins, the middle one not positive definite from column j0 on: d_status is [0, want, 0] with want the first column (as j + 1) whose
    pivot is not positive -- the order of the first leading minor of the loaded matrix that is not positive definite -- and the two good bins'
    planes are, byte for byte, those of a call given only these two bins."""
    c = FC.BY_NAME[case]
    rr, ri = FC.status_data(case)
    lr, li, st = _cholesky(native, rr, ri)
    print("%s: status = %s (want [0, %d, 0])" % (case, st.tolist(), c.want))
    assert st.tolist() == [0, c.want, 0]
    lr2, li2, st2 = _cholesky(native, rr[[0, 2]], ri[[0, 2]])
    assert st2.tolist() == [0, 0]
    for plane, alone in ((lr, lr2), (li, li2)):
        assert np.isfinite(alone).all()
        assert plane[0].tobytes() == alone[0].tobytes() and plane[2].tobytes() == alone[1].tobytes()


@pytest.mark.parametrize("case", FC.names(FC.DAS))
def test_das_power_matches_float64(native, gemm_mode, case):
    """bf_fd_das_power_device: P[f, d] = sum_b |sum_k X[b,k,f] A[b,k,d]|^2 against complex128 within 2e-5 of the peak, every entry written."""
    c = FC.BY_NAME[case]
    x, a = FC.das_data(case)
    xr, xi, ar, ai = _dev(x.real), _dev(x.imag), _dev(a.real), _dev(a.imag)
    p = _nan(c.I, c.J)
    assert native.lib.bf_fd_das_power_device(xr.data_ptr(), xi.data_ptr(), ar.data_ptr(), ai.data_ptr(), c.I, c.K, c.J, c.B, p.data_ptr(), None) == 0, native.check()
    want = FC.das_want(case)
    err = np.max(np.abs(_f64(p) - want)) / want.max()
    print("%s mode %d: max error = %.3g of the peak (bound %.3g)" % (case, gemm_mode, err, FC.TOL_OF_PEAK))
    assert err <= FC.TOL_OF_PEAK


@pytest.mark.parametrize("case", FC.names(FC.MVDR))
def test_mvdr_power_matches_float64(native, gemm_mode, case):
    """bf_fd_mvdr_power_device on an upper-triangular stand-in for the transposed inverse factor: P[d] = sum_b 1 / sum_i |sum_k L[b,k,i] conj(A[b,k,d])|^2
    against complex128 within 1e-4 relative."""
    c = FC.BY_NAME[case]
    l, a = FC.mvdr_data(case)
    lr, li, ar, ai = _dev(l.real), _dev(l.imag), _dev(a.real), _dev(a.imag)
    q = _nan(c.J)
    assert native.lib.bf_fd_mvdr_power_device(lr.data_ptr(), li.data_ptr(), ar.data_ptr(), ai.data_ptr(), c.M, c.J, c.B, q.data_ptr(), None) == 0, native.check()
    want = FC.mvdr_want(case)
    err = np.max(np.abs(_f64(q) - want) / want)
    print("%s mode %d: max relative error = %.3g (bound %.3g)" % (case, gemm_mode, err, FC.MVDR_TOL))
    assert err <= FC.MVDR_TOL


@pytest.mark.parametrize("case", FC.names(FC.DFT))
def test_dft_matches_numpy_rfft(native, case):
    """bf_fd_dft_device against numpy.fft.rfft in float64, both layouts: rows gathered in reversed order out of a taller frame with more than 32
    frames, the Nyquist bin alone, and bin ranges A, B, A of one size in turn (each call must use its own range's twiddles)."""
    from interface import config
    c = FC.BY_NAME[case]
    sig, mics = FC.dft_data(case)
    want_all = FC.dft_want(case)
    config.configure(N_MICROPHONES=c.m_total, N_SAMPLES=c.N, MAX_RES_X=3, MAX_RES_Y=3, N_TAPS=8)
    try:
        d = _dev(sig)
        for call, (lo, nb) in enumerate(c.ranges):
            re_mf, im_mf, re_fm, im_fm = _nan(nb, c.M, c.F), _nan(nb, c.M, c.F), _nan(nb, c.F, c.M), _nan(nb, c.F, c.M)
            assert native.lib.bf_fd_dft_device(d.data_ptr(), c.m_total, c.F, native.iptr(mics), c.M, lo, nb, re_mf.data_ptr(), im_mf.data_ptr(), re_fm.data_ptr(),
                                               im_fm.data_ptr(), None) == 0, native.check()
            want = want_all[:, :, lo:lo + nb]                                           # [F, M, nb]
            got_mf = _f64(re_mf) + 1j * _f64(im_mf)                                     # [nb, M, F]
            got_fm = _f64(re_fm) + 1j * _f64(im_fm)                                     # [nb, F, M]
            tol = FC.dft_tol(want, c.N)
            e_mf, e_fm = np.max(np.abs(got_mf - want.transpose(2, 1, 0))), np.max(np.abs(got_fm - want.transpose(2, 0, 1)))
            print("%s call %d bins [%d, %d): max |error| = %.3g / %.3g (bound %.3g)" % (case, call, lo, lo + nb, e_mf, e_fm, tol))
            assert e_mf <= tol and e_fm <= tol, call
    finally:
        util.configure("cfg1")


@pytest.mark.parametrize("case", FC.names(FC.CHAIN))
def test_mvdr_chain_matches_float64(native, gemm_mode, case):
    """bf_fd_covariance_device -> bf_fd_cholesky_inverse_device -> bf_fd_mvdr_power_device, each reading the planes the one before wrote, at
    microphone counts that are no multiple of 32, against the float64 composition; bounds as the whole-map tests of test_freqdomain.py."""
    import torch
    c = FC.BY_NAME[case]
    x, a = FC.chain_data(case)
    B, F, M = x.shape
    xr, xi, ar, ai = _dev(x.real), _dev(x.imag), _dev(a.real), _dev(a.imag)
    rr, ri, lr, li, q = _nan(B, M, M), _nan(B, M, M), _nan(B, M, M), _nan(B, M, M), _nan(c.J)
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    lib = native.lib
    assert lib.bf_fd_covariance_device(xr.data_ptr(), xi.data_ptr(), F, M, B, rr.data_ptr(), ri.data_ptr(), None) == 0, native.check()
    assert lib.bf_fd_cholesky_inverse_device(rr.data_ptr(), ri.data_ptr(), M, B, FC.LOADING, lr.data_ptr(), li.data_ptr(), st.data_ptr(), None) == 0, native.check()
    assert lib.bf_fd_mvdr_power_device(lr.data_ptr(), li.data_ptr(), ar.data_ptr(), ai.data_ptr(), M, c.J, B, q.data_ptr(), None) == 0, native.check()
    assert st.cpu().tolist() == [0] * B
    want = FC.chain_want(case)
    err = np.max(np.abs(_f64(q) - want) / want)
    print("%s mode %d: max relative error = %.3g (bound %.3g)" % (case, gemm_mode, err, c.tol))
    assert err <= c.tol
