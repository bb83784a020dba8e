"""CPU: the case module of the frequency-domain stage tests (tests/fd_cases.py) checked on its own -- the data are the same on every run,
the branch written beside a case is what the restated launch arithmetic of csrc/freq_kernels.hip gives, the cases together reach every
branch, every reference is finite, a float32 NumPy evaluation of each formula meets the bound its GPU test uses (so a correct float32
kernel can), the status cases' pivots cannot be flipped by float32 rounding, and a float32 restatement of the kernels' factorisation loop
shows what "every bad pivot writes, the last write wins" reports."""
import numpy as np
import pytest

import fd_cases as FC


def _arrays(case):
    name = case.name
    if case in FC.STEERING:
        return FC.steering_data(name)
    if case in FC.COVARIANCE:
        return (FC.covariance_data(name),)
    if case in FC.CHOLESKY:
        return FC.spd(name, case.M)
    if case in FC.STATUS:
        return FC.status_data(name)
    if case in FC.DAS:
        return FC.das_data(name)
    if case in FC.MVDR:
        return FC.mvdr_data(name)
    if case in FC.DFT:
        return FC.dft_data(name)
    return FC.chain_data(name)


_CACHES = (FC.steering_data, FC.spectra, FC.spd, FC.status_data, FC.das_data, FC.mvdr_data, FC.dft_data, FC.chain_data)


def test_cases_are_deterministic():
    assert len(FC.BY_NAME) == len(FC.ALL)                       # (the names seed the data: no two alike)
    first = {c.name: [a.copy() for a in _arrays(c)] for c in FC.ALL}
    for f in _CACHES:
        f.cache_clear()
    for c in FC.ALL:
        for a, b in zip(first[c.name], _arrays(c)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), c.name
            assert not b.flags.writeable


def test_branch_beside_each_case_follows_the_launch_arithmetic():
    for c in FC.STEERING:
        assert FC.steering_passes(c.D, c.M, c.K) == c.passes, c.name
    for c in FC.COVARIANCE:
        assert FC.covariance_branch(c.F, c.M, c.B) == c.branch, c.name
    for c in FC.CHOLESKY:
        assert FC.cholesky_route(c.M) == c.route, c.name
    for c in FC.DAS:
        assert FC.das_branch(c.I, c.K, c.J, c.B) == c.branch, c.name
    for c in FC.MVDR:
        assert FC.mvdr_branch(c.M, c.J, c.B) == c.branch, c.name
    for c in FC.DFT:
        for lo, nb in c.ranges:
            assert FC.dft_branch(c.M, c.F, nb) == c.branch, c.name
            assert lo + nb <= c.N // 2 + 1


def test_cases_cover_every_branch():
    das = [c.branch for c in FC.DAS] + [FC.das_branch(*s) for s in FC.EXISTING_GEMM_SHAPES]
    assert {b[0] for b in das} == {1, 2, 3, 4}                                  # every cgemm_bins_kernel<EPI_POWER, rt, *>
    assert {b[0] for b in das[:len(FC.DAS)]} >= {3, 4}
    assert {b[1] for b in das} == {1, 2, 3}                                     # row groups
    assert {b[2] for b in das} == {True, False}                                 # one K panel and several
    assert 1 in {b[3] for b in das} and max(b[3] for b in das) > 1              # direct output and the plane reduction
    assert max(b[4] for b in das) >= 2                                          # tile slots wholly past the last frame
    assert min(c.B for c in FC.DAS) < 4                                         # fewer bins than waves
    mv = [c.branch for c in FC.MVDR]
    assert {b[0] for b in mv} >= {1, 5, 7, 8} and max(b[1] for b in mv) >= 3 and {b[2] for b in mv} == {1, 2}
    routes = {c.route.split("(")[0] + ("->" + c.route.split("->")[1][:-1] if "->" in c.route else "") for c in FC.CHOLESKY}
    assert routes == {"reg", "lds", "blocked->reg", "blocked->lds"}
    reg = sorted(c.M for c in FC.CHOLESKY if c.route == "reg")
    assert {FC.ceil_div(m, 16) for m in reg} == {1, 2, 3, 4}                    # every count of 16-column blocks ...
    assert {15, 16, 17, 48, 63, 64} <= set(reg)                                 # ... and both sides of the block edges
    assert {c.M for c in FC.CHOLESKY if c.route == "lds"} >= {65, 128}
    cov = [c.branch for c in FC.COVARIANCE]
    assert {b[2] for b in cov} == {True, False} and 0 in {b[1] for b in cov} and max(b[1] for b in cov) > 0
    assert any(c.M > 128 for c in FC.COVARIANCE) and any(c.M % 32 for c in FC.COVARIANCE)
    assert {c.passes for c in FC.STEERING} == {1, 2}
    assert max(c.branch[3] for c in FC.DFT) >= 3 and any(c.m_total > c.M for c in FC.DFT)
    # status: both unblocked kernels, either block of the blocked path
    st = {(FC.cholesky_route(c.M).split("(")[0], c.j0 >= 128) for c in FC.STATUS}
    assert st == {("reg", False), ("lds", False), ("blocked", False), ("blocked", True)}


def test_gathered_rows_are_a_real_subset():
    c = FC.BY_NAME["dft_gather"]
    sig, mics = FC.dft_data(c.name)
    assert len(set(mics.tolist())) == c.M and (np.diff(mics) < 0).all() and mics.max() < c.m_total
    assert not np.array_equal(np.sort(mics), np.arange(c.M))


def test_references_are_finite():
    for c in FC.STEERING:
        re, im = FC.steering_want(c.name)
        assert re.shape == (c.K, c.M, c.D) and np.isfinite(re).all() and np.isfinite(im).all()
        assert (re[0] == 1.0).all() and (im[0] == 0.0).all()                    # the freq = 0 plane
        assert np.abs(FC.steering_data(c.name)[0]).max() <= 2e-3 and FC.steering_data(c.name)[1].max() <= 24414.0
    for c in FC.COVARIANCE:
        x = FC.covariance_data(c.name)
        assert np.isfinite(FC.covariance_f64(x)).all() and np.isfinite(FC.covariance_bound(x)).all()
    for c in FC.CHOLESKY:
        w = FC.cholesky_want(c.name)
        assert w.shape == (FC.CHOLESKY_BINS, c.M, c.M) and np.isfinite(w).all()
        assert c.M == 1 or not np.allclose(w[0], w[1])                          # distinct matrices
    for c in FC.DAS:
        assert np.isfinite(FC.das_want(c.name)).all() and FC.das_want(c.name).shape == (c.I, c.J)
    for c in FC.MVDR:
        assert np.isfinite(FC.mvdr_want(c.name)).all() and (FC.mvdr_want(c.name) > 0).all()
    for c in FC.DFT:
        assert np.isfinite(FC.dft_want(c.name)).all()
    for c in FC.CHAIN:
        assert np.isfinite(FC.chain_want(c.name)).all() and (FC.chain_want(c.name) > 0).all()


def test_float32_numpy_meets_every_bound():
    """Each formula evaluated by NumPy in complex64 against its complex128 reference: a fraction of the bound the GPU test applies, so the
    bounds leave a correct float32 kernel room and no more is claimed than that.  Prints the fractions."""
    worst = {}
    for c in FC.COVARIANCE:
        x = FC.covariance_data(c.name)
        got = np.einsum("bfi,bfj->bij", x, np.conj(x)) / np.float32(c.F)
        err = np.abs(got - FC.covariance_f64(x))
        worst[c.name] = float(np.max(np.maximum(np.abs(err.real), np.abs(err.imag)) / FC.covariance_bound(x)))
    for c in FC.CHOLESKY:
        rr, ri = FC.spd(c.name, c.M)
        r = (rr + 1j * ri).astype(np.complex64)
        tr = np.trace(r, axis1=1, axis2=2).real
        rl = r + (np.float32(FC.LOADING) * tr / np.float32(c.M))[:, None, None] * np.eye(c.M, dtype=np.float32)
        got = np.linalg.inv(np.linalg.cholesky(rl.astype(np.complex64)))
        assert got.dtype == np.complex64
        want = FC.cholesky_want(c.name)
        worst[c.name] = max(float(np.max(np.abs(got[b] - want[b])) / (FC.CHOLESKY_TOL * np.max(np.abs(want[b])))) for b in range(len(want)))
    for c in FC.DAS:
        x, a = FC.das_data(c.name)
        got = (np.abs(np.einsum("bki,bkj->bij", x, a)) ** 2).sum(0)
        worst[c.name] = float(np.max(np.abs(got - FC.das_want(c.name))) / (FC.TOL_OF_PEAK * FC.das_want(c.name).max()))
    for c in FC.MVDR:
        l, a = FC.mvdr_data(c.name)
        got = (np.float32(1.0) / (np.abs(np.einsum("bki,bkj->bij", l, np.conj(a))) ** 2).sum(1)).sum(0)
        assert got.dtype == np.float32
        worst[c.name] = float(np.max(np.abs(got - FC.mvdr_want(c.name)) / FC.mvdr_want(c.name)) / FC.MVDR_TOL)
    for c in FC.CHAIN:
        x, a = FC.chain_data(c.name)
        r = np.einsum("bfi,bfj->bij", x, np.conj(x)) / np.float32(x.shape[1])
        rl = r + (np.float32(FC.LOADING) * np.trace(r, axis1=1, axis2=2).real / np.float32(c.M))[:, None, None] * np.eye(c.M, dtype=np.float32)
        y = np.linalg.inv(np.linalg.cholesky(rl.astype(np.complex64))) @ np.conj(a)
        got = (np.float32(1.0) / (np.abs(y) ** 2).sum(1)).sum(0)
        assert got.dtype == np.float32
        worst[c.name] = float(np.max(np.abs(got - FC.chain_want(c.name)) / FC.chain_want(c.name)) / c.tol)
    for name, frac in worst.items():
        print("%-20s float32 NumPy error = %.4f of the bound" % (name, frac))
    for name, frac in worst.items():
        assert frac <= 0.5, name


@pytest.mark.parametrize("case", [c.name for c in FC.STATUS if np.isfinite(c.value)])
def test_status_pivots_are_far_from_zero(case):
    """In float64 every pivot before j0 is above 1e-3 tr/M (float32 rounding, ~1e-7 tr/M per step, cannot flip it), pivot j0 is at most -0.5,
    and the two outer bins are positive definite throughout."""
    c = FC.BY_NAME[case]
    rl = FC.loaded_f64(*FC.status_data(case))
    floor = 1e-3 * np.trace(rl[1]).real / c.M / (1.0 + FC.LOADING)
    d = FC.pivots_f64(rl[1], c.j0)
    assert len(d) == c.j0 + 1 and (d[:-1] > floor).all() and d[-1] <= -0.5
    assert c.want == c.j0 + 1
    for b in (0, 2):
        assert (FC.pivots_f64(rl[b], c.M - 1) > floor).all()


def test_nan_on_the_diagonal_reaches_every_pivot():
    """The loading is a multiple of the trace: a NaN anywhere on the diagonal makes the loaded matrix's first pivot NaN."""
    for c in FC.STATUS:
        if not np.isfinite(c.value):
            rl = FC.loaded_f64(*FC.status_data(c.name))
            assert np.isnan(rl[1, 0, 0]) and c.want == 1 and np.isfinite(rl[0]).all() and np.isfinite(rl[2]).all()


def test_last_write_wins_reports_the_matrix_size():
    """The kernels' float32 loop restated: after the first bad pivot the trailing block goes to 1e30, infinity and NaN, every later pivot
    is flagged too, and a status word that every flagged column overwrites ends as the size of the matrix -- (first, last) below.  The first
    flagged column is j0 + 1: what bf_fd_cholesky_inverse_device has to report."""
    seen = {}
    for c in FC.STATUS:
        if not np.isfinite(c.value):
            continue
        rl = FC.loaded_f64(*FC.status_data(c.name))[1]
        if c.M <= 128:
            flagged = FC.f32_pivot_reports(rl)
            seen[c.name] = (flagged[0], flagged[-1])
            assert (flagged[0], flagged[-1]) == (c.j0 + 1, c.M), c.name
            assert flagged == list(range(c.j0 + 1, c.M + 1))                    # every later pivot
        elif c.j0 < 128:
            flagged = FC.f32_pivot_reports(rl[:128, :128])                      # the first block; the second block's launch wrote over it
            seen[c.name] = (flagged[0], flagged[-1])
            assert (flagged[0], flagged[-1]) == (c.j0 + 1, 128), c.name
        else:
            assert FC.f32_pivot_reports(rl[:128, :128]) == []
            l11 = np.linalg.cholesky(rl[:128, :128])
            l21 = np.linalg.solve(l11, rl[128:, :128].conj().T).conj().T
            flagged = FC.f32_pivot_reports(rl[128:, 128:] - l21 @ l21.conj().T, base=128)
            seen[c.name] = (flagged[0], flagged[-1])
            assert (flagged[0], flagged[-1]) == (c.j0 + 1, c.M), c.name
    print(seen)
    good = FC.loaded_f64(*FC.status_data("status_64_40"))[0]
    assert FC.f32_pivot_reports(good) == []
