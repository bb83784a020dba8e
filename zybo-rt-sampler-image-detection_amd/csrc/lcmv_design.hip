// lcmv_design.hip -- bf_lcmv_design_device: null-steering filter-and-sum taps designed on the device, float64 on the vector pipes.
//
// Definition (include/beamformer_hip.h; filtersum.design_lcmv / design_slots on the host): beam i belongs to slot i of d_offsets.  For
// every in-band bin k = bin_lo + kk: w = 2 pi k / T, c_d[m] = e^{+jw tau[d][m]}, C = [c_look, kept nulls] with a null dropped when
// |c^H c'| / n > rho against the look vector or a null kept before it, u = C (C^H C)^{-1} conj(f) with f = (e^{-jw(T-1)/2}, 0, ..),
// G_k[m] = conj(u[m]); taps g[i][m][t] = (1/T) sum_k s_k Re(G_k[m] e^{+j 2 pi k t / T}), rounded once to float32.
//
//   lcmv_gains_kernel : one wave per (beam, bin).  Pass 1, the Gram matrix of ALL slots' steering vectors (8 x 8 at most): 64
//       microphones at a time, lane l forms c_s[m0 + l] of every source slot s with one sincos each and parks them in LDS; lane p < 36
//       owns the pair (a <= b) and adds conj(c_a[m]) c_b[m] over the parked microphones in ascending m -- one sequential float64 chain
//       per entry, the same whatever n or the number of slots is.  Lane 0 then walks the candidate nulls in slot order against the Gram
//       entries (the drop rule), gathers C^H C of the kept columns, factors it (Cholesky, in LDS: a dynamically indexed register array
//       would go to scratch) and solves for the p <= 8 coefficients a = (C^H C)^{-1} conj(f).  Pass 2: lane l forms the kept columns'
//       c[m] again (p sincos; parking all of pass 1 would need n x 8 x 16 bytes of LDS for an n that has no bound) and writes
//       G[m] = conj(sum_r c_r[m] a_r).  A slot that is no source gets zero gains, zero kept entries and status 1.
//   lcmv_taps_kernel  : one workgroup per (beam, block of 8 microphones).  It builds cos / sin(2 pi r / T), r in [0, T), in LDS once
//       (sincospi: the argument reduction is exact), then a thread owns one (microphone, t) and sums the in-band bins in ascending k;
//       the table index (k t) mod T advances by t in integers.  Reads the status the gains launch wrote: a silent beam's taps are zeros.
//
// Two launches, no workspace beyond d_gains, no atomics: the same bits from call to call.
#include <hip/hip_runtime.h>

#include "das_kernels.h"
#include "design_device.h"

namespace bf {
namespace {

constexpr int kLanes = 64;
constexpr int kS = kLcmvMaxSources;
constexpr int kPairs = kS * (kS + 1) / 2;      // entries (a <= b) of the Hermitian Gram matrix
constexpr int kTapThreads = 256;
constexpr int kMicBlock = 8;                   // microphones of a taps workgroup: they share one table

__global__ void __launch_bounds__(kLanes)
lcmv_gains_kernel(const double* __restrict__ tau, const int32_t* __restrict__ offsets, int dirs, int n, int S, int offset_per_dir, int T, int bin_lo, int K,
                  double rho, double* __restrict__ gains, int32_t* __restrict__ kept, int32_t* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) double cs[kS][kLanes + 1][2];   // (re, im) of c_s[m0 + lane]; rows 16 bytes apart in the banks
    __shared__ double gram[kS][kS][2];                                     // gram[a][b] = c_a^H c_b
    __shared__ double L[kS][kS][2];                                        // C^H C of the kept columns, then its Cholesky factor (lower)
    __shared__ double coef[kS][2];                                         // a = (C^H C)^{-1} conj(f)
    __shared__ int dir_of[kS], cols[kS], n_cols;

    const int lane = (int)threadIdx.x;
    const int i = (int)blockIdx.x / K, kk = (int)blockIdx.x % K;
    const int k = bin_lo + kk;
    if (lane < kS) dir_of[lane] = lane < S ? slot_direction(offsets[lane], offset_per_dir, dirs) : -1;
    __syncthreads();

    double* __restrict__ g_out = gains + ((size_t)i * K + kk) * (size_t)n * 2;
    int32_t* __restrict__ kept_out = kept + ((size_t)i * K + kk) * S;
    if (dir_of[i] < 0) {                         // (block-uniform) not a source: a silent beam
        for (int m = lane; m < n; m += kLanes) { g_out[2 * (size_t)m] = 0.0; g_out[2 * (size_t)m + 1] = 0.0; }
        if (lane < S) kept_out[lane] = 0;
        if (kk == 0 && lane == 0) status[i] = 1;
        return;
    }
    const double w = kTwoPi * (double)k / (double)T;

    // ---- pass 1: the Gram matrix, entry (pa, pb) on lane p
    int pa = 0, pb = kS;
    {
        int p = lane;
        for (int a = 0; a < kS; ++a) {
            if (p >= 0 && p < kS - a) { pa = a; pb = a + p; }
            p -= kS - a;
        }
    }
    const bool owner = lane < kPairs && pb < S;
    double acc_r = 0.0, acc_i = 0.0;
    for (int m0 = 0; m0 < n; m0 += kLanes) {
        const int m = m0 + lane;
        for (int s = 0; s < S; ++s) {
            const int d = dir_of[s];
            double sn = 0.0, c = 0.0;            // a slot that is no source, a lane past the last microphone: never read / adds nothing
            if (d >= 0 && m < n) sincos(w * tau[(size_t)d * n + m], &sn, &c);
            cs[s][lane][0] = c;
            cs[s][lane][1] = sn;
        }
        __syncthreads();
        if (owner) {
            const int live = min(kLanes, n - m0);
            for (int l = 0; l < live; ++l) {     // ascending m
                const double ar = cs[pa][l][0], ai = cs[pa][l][1], br = cs[pb][l][0], bi = cs[pb][l][1];
                acc_r += ar * br + ai * bi;      // conj(a) b
                acc_i += ar * bi - ai * br;
            }
        }
        __syncthreads();
    }
    if (owner) {
        gram[pa][pb][0] = acc_r; gram[pa][pb][1] = acc_i;
        if (pa != pb) { gram[pb][pa][0] = acc_r; gram[pb][pa][1] = -acc_i; }
    }
    __syncthreads();

    // ---- the drop rule, and the p x p system
    if (lane == 0) {
        int p = 1;
        cols[0] = i;
        for (int j = 0; j < S; ++j) {
            int keep = 0;
            if (j != i && dir_of[j] >= 0) {
                keep = 1;
                for (int c = 0; c < p; ++c)
                    if (!(hypot(gram[j][cols[c]][0], gram[j][cols[c]][1]) / (double)n <= rho)) keep = 0;
                if (keep) cols[p++] = j;
            }
            kept_out[j] = keep;
        }
        n_cols = p;
        for (int r = 0; r < p; ++r)
            for (int c = 0; c <= r; ++c) { L[r][c][0] = gram[cols[r]][cols[c]][0]; L[r][c][1] = gram[cols[r]][cols[c]][1]; }
        for (int c = 0; c < p; ++c) {            // Cholesky, column by column: C^H C = L L^H
            double d = L[c][c][0];
            for (int q = 0; q < c; ++q) d -= L[c][q][0] * L[c][q][0] + L[c][q][1] * L[c][q][1];
            const double diag = sqrt(d);
            L[c][c][0] = diag; L[c][c][1] = 0.0;
            for (int r = c + 1; r < p; ++r) {
                double vr = L[r][c][0], vi = L[r][c][1];
                for (int q = 0; q < c; ++q) {    // - L[r][q] conj(L[c][q])
                    vr -= L[r][q][0] * L[c][q][0] + L[r][q][1] * L[c][q][1];
                    vi -= L[r][q][1] * L[c][q][0] - L[r][q][0] * L[c][q][1];
                }
                L[r][c][0] = vr / diag; L[r][c][1] = vi / diag;
            }
        }
        // conj(f) = (e^{+jw(T-1)/2}, 0, ..);  L y = conj(f), then L^H a = y
        double fs = 0.0, fc = 1.0;
        sincos(w * (double)(T - 1) / 2.0, &fs, &fc);
        for (int r = 0; r < p; ++r) {
            double yr = r == 0 ? fc : 0.0, yi = r == 0 ? fs : 0.0;
            for (int q = 0; q < r; ++q) {
                yr -= L[r][q][0] * coef[q][0] - L[r][q][1] * coef[q][1];
                yi -= L[r][q][0] * coef[q][1] + L[r][q][1] * coef[q][0];
            }
            coef[r][0] = yr / L[r][r][0]; coef[r][1] = yi / L[r][r][0];
        }
        for (int r = p - 1; r >= 0; --r) {
            double ar = coef[r][0], ai = coef[r][1];
            for (int q = r + 1; q < p; ++q) {    // - conj(L[q][r]) a[q]
                ar -= L[q][r][0] * coef[q][0] + L[q][r][1] * coef[q][1];
                ai -= L[q][r][0] * coef[q][1] - L[q][r][1] * coef[q][0];
            }
            coef[r][0] = ar / L[r][r][0]; coef[r][1] = ai / L[r][r][0];
        }
        if (kk == 0) status[i] = 0;
    }
    __syncthreads();

    // ---- pass 2: G[m] = conj(u[m]), u = C a
    const int p = n_cols;
    for (int m = lane; m < n; m += kLanes) {
        double ur = 0.0, ui = 0.0;
        for (int r = 0; r < p; ++r) {
            double sn, c;
            sincos(w * tau[(size_t)dir_of[cols[r]] * n + m], &sn, &c);
            ur += c * coef[r][0] - sn * coef[r][1];
            ui += c * coef[r][1] + sn * coef[r][0];
        }
        g_out[2 * (size_t)m] = ur;
        g_out[2 * (size_t)m + 1] = -ui;
    }
}

__global__ void __launch_bounds__(kTapThreads)
lcmv_taps_kernel(const double* __restrict__ gains, const int32_t* __restrict__ status, int n, int T, int bin_lo, int K, int mic_blocks, float* __restrict__ taps)
{
    extern __shared__ __attribute__((aligned(16))) double tw[];      // [T][2]: cos, sin of 2 pi r / T
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x / mic_blocks;
    const int m0 = ((int)blockIdx.x % mic_blocks) * kMicBlock;
    const int total = min(kMicBlock, n - m0) * T;                    // (at most 8 * 1024)
    float* __restrict__ out = taps + ((size_t)i * n + m0) * T;
    if (status[i] != 0) {                        // (block-uniform) a silent beam
        for (int e = tid; e < total; e += kTapThreads) out[e] = 0.0f;
        return;
    }
    for (int r = tid; r < T; r += kTapThreads) {
        double sn, c;
        sincospi(2.0 * (double)r / (double)T, &sn, &c);
        tw[2 * r] = c;
        tw[2 * r + 1] = sn;
    }
    __syncthreads();
    const double inv_t = 1.0 / (double)T;
    for (int e = tid; e < total; e += kTapThreads) {
        const int mm = e / T, t = e - mm * T;
        const double* __restrict__ g = gains + ((size_t)i * K * n + (size_t)(m0 + mm)) * 2;
        int idx = (bin_lo * t) % T;              // (k t) mod T, k = bin_lo: both below 1024
        double acc = 0.0;
        for (int kk = 0; kk < K; ++kk) {         // ascending k
            const int k = bin_lo + kk;
            const double gr = g[0], gi = g[1];
            g += 2 * (size_t)n;
            const double sk = (k == 0 || 2 * k == T) ? 1.0 : 2.0;
            acc += sk * (gr * tw[2 * idx] - gi * tw[2 * idx + 1]);
            idx += t;
            if (idx >= T) idx -= T;
        }
        out[e] = (float)(inv_t * acc);
    }
}

}  // namespace

hipError_t launch_lcmv_design(const double* d_tau, int dirs, int n, const int32_t* d_offsets, int sources, int offset_per_dir, int n_taps, int bin_lo, int bin_hi,
                              double rho, double* d_gains, float* d_taps, int32_t* d_kept, int32_t* d_status, hipStream_t stream)
{
    if (dirs < 1 || n < 1 || sources < 1 || sources > kLcmvMaxSources || sources > n || offset_per_dir < 1 || n_taps < 1 || n_taps > kLcmvMaxTaps || bin_lo < 0 ||
        bin_hi < bin_lo || bin_hi > n_taps / 2 || !(rho > 0.0 && rho <= 1.0))
        return hipErrorInvalidValue;
    const int K = bin_hi - bin_lo + 1;
    hipLaunchKernelGGL(lcmv_gains_kernel, dim3((unsigned)(sources * K)), dim3(kLanes), 0, stream, d_tau, d_offsets, dirs, n, sources, offset_per_dir, n_taps,
                       bin_lo, K, rho, d_gains, d_kept, d_status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_lcmv_taps(d_gains, d_status, sources, n, n_taps, bin_lo, K, d_taps, stream);
}

hipError_t launch_lcmv_taps(const double* d_gains, const int32_t* d_status, int sources, int n, int n_taps, int bin_lo, int K, float* d_taps, hipStream_t stream)
{
    if (sources < 1 || n < 1 || n_taps < 1 || n_taps > kLcmvMaxTaps || bin_lo < 0 || K < 1 || bin_lo + K - 1 > n_taps / 2) return hipErrorInvalidValue;
    const int mic_blocks = (n + kMicBlock - 1) / kMicBlock;
    if ((long long)sources * mic_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lcmv_taps_kernel, dim3((unsigned)(sources * mic_blocks)), dim3(kTapThreads), (size_t)n_taps * 2 * sizeof(double), stream, d_gains, d_status,
                       n, n_taps, bin_lo, K, mic_blocks, d_taps);
    return hipGetLastError();
}

}  // namespace bf
