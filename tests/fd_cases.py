"""Cases for test_fd_stages.py (GPU) and test_fd_stages_host.py (CPU): every frequency-domain stage of csrc/freq_kernels.hip on its own,
at the smallest shapes that reach each branch of its launch code, with a NumPy restatement of the launch arithmetic (so that the branch
written beside a case is checked on the CPU before a GPU sees it) and the float64 references (complex128 NumPy only).
TEST INFRASTRUCTURE ONLY.

Data are seeded by the case's name, read-only and shared by every test that asks.  Line numbers are those of
zybo-rt-sampler-image-detection_amd/csrc/freq_kernels.hip."""
import collections
import functools
import zlib

import numpy as np

LOADING = 1e-2


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def ceil_div(a, b):
    return -(-a // b)


# ---- the launch arithmetic, restated ------------------------------------------------------------------------------------------

def bin_groups(col_tiles, row_groups, n_bins):
    """(groups, bins per group) of a bin-reducing GEMM: bin_groups (:1021-1027), then run_bins_t's even split (:1034-1037) with the
    workspace the C-ABI always reserves (fd_workspace_floats, :1060-1064)."""
    cap = (n_bins + 7) // 8
    want = min(ceil_div(1536, col_tiles * row_groups), cap)
    groups = max(want, 1)
    per_group = ceil_div(n_bins, groups)
    return ceil_div(n_bins, per_group), per_group


def das_branch(I, K, J, B):
    """launch_fd_das_power (:1075-1084): (rt, row_groups, single, bin groups, tile slots wholly past I).  rt picks the
    cgemm_bins_kernel<EPI_POWER, rt, *> instantiation, `single` (:208) whether a bin's B panel is loaded once or per K panel."""
    tiles = ceil_div(I, 32)
    row_groups = ceil_div(tiles, 4)
    rt = ceil_div(tiles, row_groups)
    groups, _ = bin_groups(ceil_div(J, 32), row_groups, B)
    return rt, row_groups, K <= 64, groups, rt * row_groups - tiles


def mvdr_branch(M, J, B):
    """launch_fd_mvdr_power (:1175-1176) and the kernel's own loops: (row tiles (:209), K panels of the last row tile (:251, :276 / :295),
    bin groups)."""
    groups, _ = bin_groups(ceil_div(J, 32), 1, B)
    return ceil_div(M, 32), ceil_div(M, 64), groups


def covariance_branch(F, M, B):
    """run_gemm<EPI_STORE> (:826) and cgemm_kernel (:67-69, :95-97): (row tiles, waves that return early at `j0 >= J`, odd F -- the last
    MFMA step half empty)."""
    tiles = ceil_div(M, 32)
    return tiles, 4 * ceil_div(M, 128) - tiles, F % 2 == 1


def cholesky_route(M):
    """launch_fd_cholesky_inverse (:1131, :1137, :1148, :1158) and run_cholesky (:1104)."""
    if M <= 64:
        return "reg"
    if M <= 128:
        return "lds"
    m2 = M - 128
    return "blocked(%d->%s)" % (m2, "reg" if m2 <= 64 else "lds")


def steering_passes(D, M, K):
    """launch_fd_steering (:835): 2048 workgroups of 256 threads, grid-stride."""
    return ceil_div(D * M * K, 2048 * 256)


def dft_branch(M, F, nb):
    """launch_fd_dft (:967, :975-976, :982, :990): (32-bin tiles per workgroup, bin groups, 32-row tiles of dft_tile_kernel, 32-frame
    tiles of transpose_planes_kernel)."""
    kt_all = ceil_div(nb, 32)
    kt = min(kt_all, 4)
    return kt, ceil_div(kt_all, kt), ceil_div(F * M, 32), ceil_div(F, 32)


# ---- steering -------------------------------------------------------------------------------------------------------------------

Steering = collections.namedtuple("Steering", "name D M K passes")
STEERING = [
    Steering("steer_odd", 45, 37, 9, 1),            # nothing a power of two: the index decode
    Steering("steer_two_passes", 1201, 64, 7, 2),   # 538,048 elements > 2048 * 256: the grid-stride loop's second pass
]
STEERING_TOL = 2.0 ** -23       # a correctly rounded float32 of a float64 cos / sin that differs in its last places lands on a neighbouring float at most


@functools.lru_cache(maxsize=None)
def steering_data(name):
    """tau float64 [D, M] seconds, freq float64 [K] Hz with freq[0] = 0."""
    c = BY_NAME[name]
    rng = _rng(name)
    tau = rng.uniform(-2e-3, 2e-3, size=(c.D, c.M))
    freq = np.sort(rng.uniform(0.0, 24414.0, size=c.K))
    freq[0] = 0.0
    return _ro(tau, freq)


@functools.lru_cache(maxsize=None)
def steering_want(name):
    """float32 (re, im) [K, M, D] of exp(-j 2 pi f tau), the phase formed in the kernel's product order ((-2 pi) f) tau (:500)."""
    tau, freq = steering_data(name)
    ph = ((-2.0 * 3.14159265358979323846) * freq)[:, None, None] * tau.T[None, :, :]
    return _ro(np.cos(ph).astype(np.float32), np.sin(ph).astype(np.float32))


# ---- covariance -----------------------------------------------------------------------------------------------------------------

Covariance = collections.namedtuple("Covariance", "name F M B branch")
COVARIANCE = [
    #                                       (row tiles, idle waves, odd F)
    Covariance("cov_one", 1, 1, 1, (1, 3, True)),                   # a single entry: |x|^2
    Covariance("cov_ragged", 5, 37, 3, (2, 2, True)),               # ragged second tile, odd F
    Covariance("cov_two_tiles", 96, 64, 2, (2, 2, False)),          # whole tiles, two waves without work
    Covariance("cov_four_tiles", 190, 100, 2, (4, 0, False)),       # every wave busy, last tile ragged
    Covariance("cov_second_block", 33, 130, 2, (5, 3, True)),       # a second workgroup column with one 2-wide tile
]


@functools.lru_cache(maxsize=None)
def spectra(name, F, M, B):
    """complex64 [B, F, M]: the [K][F][M] layout of bf_fd_dft_device."""
    rng = _rng(name)
    x = (rng.standard_normal((B, F, M)) + 1j * rng.standard_normal((B, F, M))).astype(np.complex64)
    return _ro(x)[0]


def covariance_data(name):
    c = BY_NAME[name]
    return spectra(name, c.F, c.M, c.B)


def covariance_f64(x):
    """R[b, i, j] = (1/F) sum_f x[b, f, i] conj(x[b, f, j]) in complex128."""
    x = x.astype(np.complex128)
    return np.einsum("bfi,bfj->bij", x, np.conj(x)) / x.shape[1]


def covariance_bound(x):
    """Per entry, for both planes: 2 (2F + 2) 2^-24 (1/F) sum_f (|re_i| + |im_i|)(|re_j| + |im_j|) -- the accumulation bound of the 2F float32
    terms of a plane plus the scaling, doubled because the matrix instruction's internal summation order is not specified."""
    F = x.shape[1]
    a = np.abs(x.real).astype(np.float64) + np.abs(x.imag).astype(np.float64)
    return 2.0 * (2 * F + 2) * 2.0 ** -24 * np.einsum("bfi,bfj->bij", a, a) / F


# ---- Cholesky inverse -------------------------------------------------------------------------------------------------------------

Cholesky = collections.namedtuple("Cholesky", "name M route")
CHOLESKY = [Cholesky("chol_%d" % M, M, route) for M, route in [
    (1, "reg"), (2, "reg"), (15, "reg"), (16, "reg"), (17, "reg"), (33, "reg"), (48, "reg"), (63, "reg"), (64, "reg"),   # every 16-column block edge
    (65, "lds"), (100, "lds"), (127, "lds"), (128, "lds"),                                     # a whole matrix with relative loading
    (150, "blocked(22->reg)"),                                                                 # the register kernel inside the blocked path
    (200, "blocked(72->lds)"),                                                                 # the LDS kernel with ld_in = m2, ld_out = M
]]
CHOLESKY_BINS = 3
CHOLESKY_TOL = 2e-4             # of max|want|, as test_freqdomain.py::test_gpu_blocked_cholesky_inverse_matches_numpy


@functools.lru_cache(maxsize=None)
def spd(name, M, B=CHOLESKY_BINS):
    """float32 (re, im) [B, M, M] of X X^H / 2M from 2M complex normal columns, B distinct matrices."""
    rng = _rng(name)
    x = rng.standard_normal((B, M, 2 * M)) + 1j * rng.standard_normal((B, M, 2 * M))
    r = (x @ x.conj().transpose(0, 2, 1)) / (2 * M)
    return _ro(np.ascontiguousarray(r.real.astype(np.float32)), np.ascontiguousarray(r.imag.astype(np.float32)))


def loaded_f64(rr, ri, loading=LOADING):
    """The float32 planes as complex128 with loading tr(R)/M on the diagonal, [B, M, M]."""
    r = rr.astype(np.float64) + 1j * ri.astype(np.float64)
    M = r.shape[-1]
    tr = np.trace(r, axis1=-2, axis2=-1).real
    return r + (loading * tr / M)[..., None, None] * np.eye(M)


def cholesky_inverse_f64(rr, ri, loading=LOADING):
    """inverse(cholesky(R + loading tr(R)/M I)) in complex128, [B, M, M] (row, column)."""
    return np.linalg.inv(np.linalg.cholesky(loaded_f64(rr, ri, loading)))


@functools.lru_cache(maxsize=None)
def cholesky_want(name):
    return _ro(cholesky_inverse_f64(*spd(name, BY_NAME[name].M)))[0]


# ---- status -----------------------------------------------------------------------------------------------------------------------

Status = collections.namedtuple("Status", "name M j0 value want")
STATUS = [
    Status("status_16_5", 16, 5, -1.0, 6),
    Status("status_64_40", 64, 40, -1.0, 41),
    Status("status_100_0", 100, 0, -1.0, 1),
    Status("status_128_77", 128, 77, -1.0, 78),
    Status("status_200_30", 200, 30, -1.0, 31),         # in the first block: the second block's launch must not overwrite it
    Status("status_200_150", 200, 150, -1.0, 151),      # in the second block: status_base = 128
    # NaN on the diagonal.  The loading is relative to the trace, so the NaN reaches every diagonal entry of the loaded matrix and the
    # first pivot that is not positive is column 0 wherever the NaN sat: j0 = 0 is the case whose report is j0 + 1
    Status("status_nan_100_0", 100, 0, float("nan"), 1),
    Status("status_nan_64_40", 64, 40, float("nan"), 1),
]


@functools.lru_cache(maxsize=None)
def status_data(name):
    """float32 (re, im) [3, M, M]: three positive-definite bins, the middle one with `value` at [j0][j0]."""
    c = BY_NAME[name]
    rr, ri = (np.array(a) for a in spd(name, c.M, 3))
    rr[1, c.j0, c.j0] = c.value
    return _ro(rr, ri)


def pivots_f64(rl, upto):
    """The pivots d_0 .. d_upto of the factorisation of one complex128 matrix whose leading minor of order `upto` is positive definite."""
    head = np.linalg.cholesky(rl[:upto, :upto]) if upto else np.zeros((0, 0))
    d = list(np.diag(head).real ** 2)
    w = np.linalg.solve(head, rl[:upto, upto]) if upto else np.zeros(0)
    d.append(float(rl[upto, upto].real - np.sum(np.abs(w) ** 2)))
    return np.array(d)


def f32_pivot_reports(rl, base=0):
    """The factorisation loop of both Cholesky kernels (:546-559, :651-669) restated in float32 on one loaded matrix: every column whose pivot
    is not positive, as base + j + 1.  The arithmetic goes on with 1 / max(d, 1e-30) as the kernels' does."""
    a = rl.astype(np.complex64)
    M = a.shape[0]
    flagged = []
    with np.errstate(all="ignore"):
        for j in range(M):
            d = np.float32(a[j, j].real)
            if not d > 0:
                flagged.append(base + j + 1)
            invd = np.float32(1.0) / max(d, np.float32(1e-30))
            col = a[j + 1:, j].copy()
            a[j + 1:, j + 1:] -= np.outer(col * invd, np.conj(col))
    return flagged


# ---- delay-and-sum power ------------------------------------------------------------------------------------------------------------

Das = collections.namedtuple("Das", "name I K J B branch")
DAS = [
    #                                    (rt, row groups, single, bin groups, tile slots past I)
    Das("das_rt4_ragged", 100, 37, 45, 9, (4, 1, True, 2, 0)),      # rt = 4, last tile ragged, odd K, two bin groups
    Das("das_rt4_full", 128, 64, 33, 2, (4, 1, True, 1, 0)),        # rt = 4 full, fewer bins than waves, direct output
    Das("das_three_groups", 257, 70, 40, 5, (3, 3, False, 1, 0)),   # three row groups of 3, second K panel 6 deep
    Das("das_dead_tiles", 300, 16, 64, 1, (4, 3, True, 1, 2)),      # three row groups of 4, the last with two tiles wholly past I, one bin
]
# test_freqdomain.py's GEMM_SHAPES, for the coverage count
EXISTING_GEMM_SHAPES = [(150, 37, 45, 9), (33, 100, 200, 5), (190, 64, 333, 23), (8, 130, 64, 3)]
TOL_OF_PEAK = 2e-5              # test_freqdomain.py's


@functools.lru_cache(maxsize=None)
def das_data(name):
    """x complex64 [B, K, I] (the [K][M][F] layout), a complex64 [B, K, J] unit phasors."""
    c = BY_NAME[name]
    rng = _rng(name)
    x = (rng.standard_normal((c.B, c.K, c.I)) + 1j * rng.standard_normal((c.B, c.K, c.I))).astype(np.complex64)
    a = np.exp(1j * rng.uniform(0, 2 * np.pi, (c.B, c.K, c.J))).astype(np.complex64)
    return _ro(x, a)


def das_power_f64(x, a):
    """P[f, d] = sum_b |sum_k x[b, k, f] a[b, k, d]|^2."""
    return (np.abs(np.einsum("bki,bkj->bij", x.astype(np.complex128), a.astype(np.complex128))) ** 2).sum(0)


@functools.lru_cache(maxsize=None)
def das_want(name):
    return _ro(das_power_f64(*das_data(name)))[0]


# ---- MVDR power ---------------------------------------------------------------------------------------------------------------------

Mvdr = collections.namedtuple("Mvdr", "name M J B branch")
MVDR = [
    #                              (row tiles, K panels, bin groups)
    Mvdr("mvdr_one_mic", 1, 33, 2, (1, 1, 1)),
    Mvdr("mvdr_129", 129, 45, 3, (5, 3, 1)),            # a fifth row tile one row deep, a third K panel one deep
    Mvdr("mvdr_200", 200, 70, 4, (7, 4, 1)),
    Mvdr("mvdr_256", 256, 333, 9, (8, 4, 2)),           # config 5's array: eight row tiles, the plane reduction
]
MVDR_TOL = 1e-4                 # relative, test_freqdomain.py::test_gpu_mvdr_quadratic_form_matches_numpy


@functools.lru_cache(maxsize=None)
def mvdr_data(name):
    """l complex64 [B, M, M] with l[b, k, i] = Linv[i][k], zero for k > i (an upper-triangular stand-in for the transposed planes of
    bf_fd_cholesky_inverse_device); a complex64 [B, M, J] unit phasors."""
    c = BY_NAME[name]
    rng = _rng(name)
    l = np.triu(rng.standard_normal((c.B, c.M, c.M)) + 1j * rng.standard_normal((c.B, c.M, c.M))).astype(np.complex64)
    a = np.exp(1j * rng.uniform(0, 2 * np.pi, (c.B, c.M, c.J))).astype(np.complex64)
    return _ro(l, a)


def mvdr_power_f64(l, a):
    """P[d] = sum_b 1 / sum_i |sum_k l[b, k, i] conj(a[b, k, d])|^2."""
    y = np.einsum("bki,bkj->bij", l.astype(np.complex128), np.conj(a.astype(np.complex128)))
    return (1.0 / (np.abs(y) ** 2).sum(1)).sum(0)


@functools.lru_cache(maxsize=None)
def mvdr_want(name):
    return _ro(mvdr_power_f64(*mvdr_data(name)))[0]


# ---- DFT ----------------------------------------------------------------------------------------------------------------------------

Dft = collections.namedtuple("Dft", "name N m_total M F ranges rows branch")
DFT = [
    #                                                                        (bin tiles per workgroup, bin groups, row tiles, frame tiles)
    Dft("dft_gather", 256, 50, 37, 70, ((3, 33),), "reversed", (2, 1, 81, 3)),      # 37 of 50 rows in reversed order, three 32-frame tiles in the transpose
    Dft("dft_nyquist", 256, 3, 3, 1, ((128, 1),), "all", (1, 1, 1, 1)),             # the Nyquist bin alone
    Dft("dft_twiddle_cache", 256, 5, 5, 2, ((3, 33), (4, 33), (3, 33)), "all", (2, 1, 1, 1)),   # ranges A, B, A of one size: the twiddle table's key
]


@functools.lru_cache(maxsize=None)
def dft_data(name):
    """frames float32 [F, m_total, N], mics int32 [M] (rows of a frame)."""
    c = BY_NAME[name]
    rng = _rng(name)
    sig = rng.standard_normal((c.F, c.m_total, c.N)).astype(np.float32)
    mics = np.sort(rng.choice(c.m_total, c.M, replace=False)).astype(np.int32)
    if c.rows == "reversed":
        mics = np.ascontiguousarray(mics[::-1])
    return _ro(sig, mics)


@functools.lru_cache(maxsize=None)
def dft_want(name):
    """numpy.fft.rfft of the picked rows in float64, complex128 [F, M, N / 2 + 1]."""
    sig, mics = dft_data(name)
    return _ro(np.fft.rfft(sig[:, mics, :].astype(np.float64), axis=2))[0]


def dft_tol(want, N):
    return 2e-6 * np.abs(want).max() * np.sqrt(N)       # test_freqdomain.py::test_gpu_dft_matches_numpy_rfft's


# ---- the chain covariance -> Cholesky inverse -> MVDR power ---------------------------------------------------------------------------

Chain = collections.namedtuple("Chain", "name M J B tol")
CHAIN = [
    # arrays with dead microphones (FrequencyBeamformer(active=...)): sizes that are no multiple of 32.  Bounds: the whole-map tests' own
    Chain("chain_61", 61, 45, 3, 2e-4),
    Chain("chain_100", 100, 45, 3, 2e-4),
    Chain("chain_200", 200, 45, 3, 5e-4),
]


@functools.lru_cache(maxsize=None)
def chain_data(name):
    """x complex64 [B, F = 2M, M] spectra, a complex64 [B, M, J] unit phasors."""
    c = BY_NAME[name]
    x = spectra(name, 2 * c.M, c.M, c.B)
    a = np.exp(1j * _rng(name + "/a").uniform(0, 2 * np.pi, (c.B, c.M, c.J))).astype(np.complex64)
    return x, _ro(a)[0]


@functools.lru_cache(maxsize=None)
def chain_want(name):
    """P[d] = sum_b 1 / || inverse(L_b) conj(a[b, :, d]) ||^2 with L_b L_b^H = R_b + loading tr(R_b)/M I, all in float64."""
    x, a = chain_data(name)
    r = covariance_f64(x)
    M = r.shape[-1]
    rl = r + (LOADING * np.trace(r, axis1=1, axis2=2).real / M)[:, None, None] * np.eye(M)
    y = np.linalg.inv(np.linalg.cholesky(rl)) @ np.conj(a.astype(np.complex128))
    return _ro((1.0 / (np.abs(y) ** 2).sum(1)).sum(0))[0]


ALL = STEERING + COVARIANCE + CHOLESKY + STATUS + DAS + MVDR + DFT + CHAIN
BY_NAME = {c.name: c for c in ALL}


def names(cases):
    return [c.name for c in cases]
