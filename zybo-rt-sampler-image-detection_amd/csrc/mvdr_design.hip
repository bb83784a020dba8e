// mvdr_design.hip -- bf_mvdr_design_device: adaptive (MVDR) filter-and-sum taps from the frames' own covariance, float64 on the vector pipes.
//
// Definition (include/beamformer_hip.h; filtersum.design_mvdr / design_mvdr_slots on the host).  T = n_taps, in-band bins k = bin_lo + kk:
//   snapshots   X_p[kk][m] = sum_t win[t] x_f[r_m][s + t] e^{-j 2 pi ((k t) mod T) / T},  p = f segs + q,  s = seg_first + q seg_hop
//   covariance  R_k[a][b]  = (1/P) sum_p X_p[a] conj(X_p[b])
//   loading     R'_k = R_k + (loading tr R_k / n) I, or I where the trace is not finite and > 0 (d_fallback)
//   factor      R'_k = L L^H
//   solve       per source slot, c[m] = e^{+jw tau[d][m]}:  y = L^{-1} c,  z = L^{-H} y,  G_k[m] = conj(z[m] conj(f0) / sum|y|^2)
// and lcmv_design.hip's taps launch on the gains.
//
//   mvdr_snapshot_kernel : one workgroup per (snapshot, block of 32 microphones).  cos / sin(2 pi r / T) and the window go to LDS once
//       (sincospi: the argument reduction is exact); a thread owns one (microphone, bin) and walks t upwards, the table index
//       (k t) mod T advancing by k in integers.  The samples come through the L1: the threads of a microphone read one address.
//   mvdr_cov_kernel      : one workgroup per (bin, 16 x 16 tile of the lower triangle).  Sixteen snapshots of the tile's rows and
//       columns are staged in LDS at a time; a thread owns one entry (a >= b) and adds over p upwards -- one sequential chain per
//       entry -- then writes it and its conjugate mirror: d_cov is Hermitian bit for bit, its diagonal's imaginary part is +0.
//   mvdr_solve_kernel    : one workgroup per bin.  The trace (one thread, a upwards), R' into d_chol (strict upper zero), then the
//       factorisation in place, column by column, right-looking: column c is scaled by 1 / sqrt of its pivot and parked in LDS,
//       every entry (r, cc) behind it loses L[r][c] conj(L[cc][c]) -- so an entry's subtractions happen in ascending q whatever
//       the blocking.  A full matrix of 256 complex float64 is 1 MB: it stays in d_chol (L2), only the pivot column is in LDS.
//       The forward substitutions of all slots ride on the parked column (b[s][r] -= L[r][c] y[s][c]): L is not read again for
//       them.  The back substitutions walk the rows of L downwards, a thread holding its element of the next row in a register
//       while the current one is applied, and the owner of z[q] writes the gain as it falls out.  Right-hand sides live in LDS
//       (a dynamically indexed register array would go to scratch).
//
// Four launches (the fourth is lcmv_taps_kernel), no atomics, no workspace beyond the named buffers: the same bits from call to call.
//
// bf_mvdr_learn_device keeps the covariance as device state (d_acc, d_mass) that carries from call to call: every frame has a weight,
// every learned frame (weight finite and > 0) multiplies the state by `forget` first.  Its stages are the ones above with
//   mvdr_learn_snapshot_kernel : mvdr_snapshot_kernel's snapshots (the same body); thread 0 of workgroup 0 also advances d_mass over the
//       learned frames and counts d_used -- no other thread of that launch reads either, the next launch reads the final mass.
//   mvdr_accumulate_kernel     : in mvdr_cov_kernel's place and shape.  A thread's chain starts from the entry of d_acc it owns, runs
//       over the learned frames in ascending f (acc = forget acc at q = 0, then acc = acc + w_f t over q upwards, t being
//       mvdr_cov_kernel's term), goes back to d_acc with its mirror where a frame was learned, and d_cov = acc / mass (0 where the
//       mass is not > 0: every bin then falls back).  A thread reads only the entry it owns and writes it and its mirror: in place
//       without a race.  A staged chunk whose frames are all skipped is not loaded; a call that learns nothing does not write d_acc.
// With frames == 0 (the re-aim) there are no snapshots: the accumulate launch turns the stored state into d_cov and writes d_used.
#include <hip/hip_runtime.h>

#include "das_kernels.h"
#include "design_device.h"

namespace bf {
namespace {

constexpr int kS = kLcmvMaxSources;
constexpr int kN = kMvdrMaxMics;
constexpr int kSnapThreads = 256;
constexpr int kSnapMics = 32;                  // microphones of a snapshot workgroup: they share one table
constexpr int kTile = 16;                      // a covariance workgroup owns kTile x kTile entries ...
constexpr int kCovThreads = kTile * kTile;
constexpr int kCovP = 16;                      // ... and stages this many snapshots at a time
constexpr int kSolveThreads = 1024;
constexpr int kSolveWaves = kSolveThreads / 64;

// The body of the two snapshot kernels: one workgroup's (snapshot, block of microphones).
__device__ __forceinline__ void snapshot_block(const float* __restrict__ signals, const int32_t* __restrict__ mics, int m_total, int n_samples, int n, int seg_first,
                                               int seg_hop, int segs, const double* __restrict__ window, int T, int bin_lo, int K, int mic_blocks,
                                               double* __restrict__ snap)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];     // [T][2]: cos, sin of 2 pi r / T; then [T]: the window
    double* __restrict__ tw = lds;
    double* __restrict__ win = lds + 2 * (size_t)T;
    const int tid = (int)threadIdx.x;
    const int p = (int)blockIdx.x / mic_blocks;
    const int m0 = ((int)blockIdx.x % mic_blocks) * kSnapMics;
    const int f = p / segs, q = p - f * segs;
    const int s = seg_first + q * seg_hop;       // (the entry point checked s + T <= n_samples for the last segment)
    for (int r = tid; r < T; r += kSnapThreads) {
        double sn, c;
        sincospi(2.0 * (double)r / (double)T, &sn, &c);
        tw[2 * r] = c;
        tw[2 * r + 1] = sn;
        win[r] = window ? window[r] : 1.0;
    }
    __syncthreads();
    const int total = min(kSnapMics, n - m0) * K;
    for (int e = tid; e < total; e += kSnapThreads) {
        const int mm = e / K, kk = e - mm * K;
        const int k = bin_lo + kk;               // k <= T / 2: the index below stays under 2 T
        const float* __restrict__ x = signals + ((size_t)f * m_total + (size_t)mics[m0 + mm]) * n_samples + s;
        double acc_r = 0.0, acc_i = 0.0;
        int idx = 0;
        for (int t = 0; t < T; ++t) {            // ascending t
            const double v = win[t] * (double)x[t];
            acc_r += v * tw[2 * idx];
            acc_i -= v * tw[2 * idx + 1];
            idx += k;
            if (idx >= T) idx -= T;
        }
        double* __restrict__ out = snap + (((size_t)p * K + kk) * n + (size_t)(m0 + mm)) * 2;
        out[0] = acc_r;
        out[1] = acc_i;
    }
}

__global__ void __launch_bounds__(kSnapThreads)
mvdr_snapshot_kernel(const float* __restrict__ signals, const int32_t* __restrict__ mics, int m_total, int n_samples, int n, int seg_first, int seg_hop, int segs,
                     const double* __restrict__ window, int T, int bin_lo, int K, int mic_blocks, double* __restrict__ snap)
{
    snapshot_block(signals, mics, m_total, n_samples, n, seg_first, seg_hop, segs, window, T, bin_lo, K, mic_blocks, snap);
}

// A frame is learned iff its weight is finite and > 0 (a NaN fails both comparisons); the weight of a frame that is not is 0 here.
__device__ __forceinline__ double learned_weight(const double* __restrict__ weights, int f)
{
    const double w = weights ? weights[f] : 1.0;
    return w > 0.0 && w <= 1.79769313486231570815e308 ? w : 0.0;
}

// mvdr_snapshot_kernel, and the mass chain: mass = forget mass + w_f segs over the learned frames in ascending f.  used = (frames
// learned, weights refused: NaN, Inf, negative; a weight of +-0 is skipped without being counted).
__global__ void __launch_bounds__(kSnapThreads)
mvdr_learn_snapshot_kernel(const float* __restrict__ signals, const int32_t* __restrict__ mics, int m_total, int n_samples, int n, int seg_first, int seg_hop, int segs,
                           const double* __restrict__ window, int T, int bin_lo, int K, int mic_blocks, double* __restrict__ snap,
                           const double* __restrict__ weights, int frames, double forget, double* __restrict__ mass, int32_t* __restrict__ used)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double m = mass[0];
        int learned = 0, refused = 0;
        for (int f = 0; f < frames; ++f) {
            const double w = learned_weight(weights, f);
            if (w > 0.0) {
                m = forget * m;
                m = m + w * (double)segs;
                ++learned;
            } else if (weights && !(weights[f] == 0.0)) {
                ++refused;
            }
        }
        mass[0] = m;
        used[0] = learned;
        used[1] = refused;
    }
    snapshot_block(signals, mics, m_total, n_samples, n, seg_first, seg_hop, segs, window, T, bin_lo, K, mic_blocks, snap);
}

__global__ void __launch_bounds__(kCovThreads)
mvdr_cov_kernel(const double* __restrict__ snap, int P, int K, int n, int tiles, double* __restrict__ cov)
{
    __shared__ __attribute__((aligned(16))) double xa[kCovP][kTile][2];   // X_p[a0 + .]
    __shared__ __attribute__((aligned(16))) double xb[kCovP][kTile][2];   // X_p[b0 + .]
    const int tid = (int)threadIdx.x;
    const int kk = (int)blockIdx.x / tiles;
    int ta = 0, tb = (int)blockIdx.x % tiles;    // tile (ta >= tb) of the lower triangle, counted row by row
    while (tb > ta) { tb -= ta + 1; ++ta; }
    const int a0 = ta * kTile, b0 = tb * kTile;
    const int ia = tid / kTile, ib = tid % kTile;
    const int a = a0 + ia, b = b0 + ib;
    double acc_r = 0.0, acc_i = 0.0;
    for (int p0 = 0; p0 < P; p0 += kCovP) {
        {
            const int pp = tid / kTile, j = tid % kTile, p = p0 + pp;      // consecutive threads: consecutive microphones of one snapshot
            double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
            if (p < P) {
                const double* __restrict__ row = snap + ((size_t)p * K + kk) * (size_t)n * 2;
                if (a0 + j < n) { ar = row[2 * (size_t)(a0 + j)]; ai = row[2 * (size_t)(a0 + j) + 1]; }
                if (b0 + j < n) { br = row[2 * (size_t)(b0 + j)]; bi = row[2 * (size_t)(b0 + j) + 1]; }
            }
            xa[pp][j][0] = ar; xa[pp][j][1] = ai;
            xb[pp][j][0] = br; xb[pp][j][1] = bi;
        }
        __syncthreads();
        const int live = min(kCovP, P - p0);
        for (int pp = 0; pp < live; ++pp) {      // ascending p
            const double ar = xa[pp][ia][0], ai = xa[pp][ia][1], br = xb[pp][ib][0], bi = xb[pp][ib][1];
            acc_r += ar * br + ai * bi;          // a conj(b)
            acc_i += ai * br - ar * bi;
        }
        __syncthreads();
    }
    if (a < n && b <= a) {
        const double re = acc_r / (double)P, im = a == b ? 0.0 : acc_i / (double)P;
        double* __restrict__ base = cov + (size_t)kk * n * n * 2;
        base[((size_t)a * n + b) * 2] = re;
        base[((size_t)a * n + b) * 2 + 1] = im;
        if (a != b) {
            base[((size_t)b * n + a) * 2] = re;
            base[((size_t)b * n + a) * 2 + 1] = -im;
        }
    }
}

// `used` is given only where no snapshot launch ran (frames == 0): this launch then writes (0, 0), and nothing reads it.
__global__ void __launch_bounds__(kCovThreads)
mvdr_accumulate_kernel(const double* __restrict__ snap, const double* __restrict__ weights, int frames, int segs, double forget, int K, int n, int tiles,
                       const double* __restrict__ mass, double* acc, double* __restrict__ cov, int32_t* __restrict__ used)
{
    __shared__ __attribute__((aligned(16))) double xa[kCovP][kTile][2];   // X_p[a0 + .]
    __shared__ __attribute__((aligned(16))) double xb[kCovP][kTile][2];   // X_p[b0 + .]
    const int tid = (int)threadIdx.x;
    const int kk = (int)blockIdx.x / tiles;
    int ta = 0, tb = (int)blockIdx.x % tiles;    // tile (ta >= tb) of the lower triangle, counted row by row
    while (tb > ta) { tb -= ta + 1; ++ta; }
    const int a0 = ta * kTile, b0 = tb * kTile;
    const int ia = tid / kTile, ib = tid % kTile;
    const int a = a0 + ia, b = b0 + ib;
    const bool mine = a < n && b <= a;
    double* base = acc + (size_t)kk * n * n * 2;  // (no __restrict__: the entry is read, then it and its mirror are written)
    double acc_r = 0.0, acc_i = 0.0;
    if (mine) { acc_r = base[((size_t)a * n + b) * 2]; acc_i = base[((size_t)a * n + b) * 2 + 1]; }
    if (used && blockIdx.x == 0 && tid == 0) { used[0] = 0; used[1] = 0; }
    const int P = frames * segs;
    bool learned_any = false;
    for (int p0 = 0; p0 < P; p0 += kCovP) {
        const int live = min(kCovP, P - p0);
        int f = p0 / segs, q = p0 - f * segs;    // of snapshot p0; a frame boundary may fall anywhere in the chunk
        bool any = false;
        for (int ff = f; ff <= (p0 + live - 1) / segs; ++ff) any = any || learned_weight(weights, ff) > 0.0;
        if (!any) continue;                      // (the same for every thread of the workgroup)
        learned_any = true;
        {
            const int pp = tid / kTile, j = tid % kTile, p = p0 + pp;      // consecutive threads: consecutive microphones of one snapshot
            double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
            if (p < P) {
                const double* __restrict__ row = snap + ((size_t)p * K + kk) * (size_t)n * 2;
                if (a0 + j < n) { ar = row[2 * (size_t)(a0 + j)]; ai = row[2 * (size_t)(a0 + j) + 1]; }
                if (b0 + j < n) { br = row[2 * (size_t)(b0 + j)]; bi = row[2 * (size_t)(b0 + j) + 1]; }
            }
            xa[pp][j][0] = ar; xa[pp][j][1] = ai;
            xb[pp][j][0] = br; xb[pp][j][1] = bi;
        }
        __syncthreads();
        double w = learned_weight(weights, f);
        for (int pp = 0; pp < live; ++pp) {      // ascending p
            if (w > 0.0) {
                if (q == 0) { acc_r = forget * acc_r; acc_i = forget * acc_i; }
                const double ar = xa[pp][ia][0], ai = xa[pp][ia][1], br = xb[pp][ib][0], bi = xb[pp][ib][1];
                acc_r = acc_r + w * (ar * br + ai * bi);          // w a conj(b)
                acc_i = acc_i + w * (ai * br - ar * bi);
            }
            if (++q == segs) {
                q = 0;
                ++f;
                w = f < frames ? learned_weight(weights, f) : 0.0;
            }
        }
        __syncthreads();
    }
    if (mine) {
        if (a == b) acc_i = 0.0;
        if (learned_any) {                       // a call that learns nothing leaves the state's bytes alone
            base[((size_t)a * n + b) * 2] = acc_r;
            base[((size_t)a * n + b) * 2 + 1] = acc_i;
            if (a != b) {
                base[((size_t)b * n + a) * 2] = acc_r;
                base[((size_t)b * n + a) * 2 + 1] = -acc_i;
            }
        }
        const double m = mass[0];
        const bool some = m > 0.0;               // (a NaN mass is none)
        const double re = some ? acc_r / m : 0.0, im = some && a != b ? acc_i / m : 0.0;
        double* __restrict__ out = cov + (size_t)kk * n * n * 2;
        out[((size_t)a * n + b) * 2] = re;
        out[((size_t)a * n + b) * 2 + 1] = im;
        if (a != b) {
            out[((size_t)b * n + a) * 2] = re;
            out[((size_t)b * n + a) * 2 + 1] = -im;
        }
    }
}

__global__ void __launch_bounds__(kSolveThreads)
mvdr_solve_kernel(const double* __restrict__ cov, const double* __restrict__ tau, const int32_t* __restrict__ offsets, int dirs, int n, int S, int offset_per_dir,
                  int T, int bin_lo, int K, double loading, double* chol, double* __restrict__ gains, int32_t* __restrict__ status,
                  int32_t* __restrict__ fallback)
{
    __shared__ __attribute__((aligned(16))) double rhs[kS][kN][2];   // c, then y = L^{-1} c, then what is left of it in the back substitution
    __shared__ __attribute__((aligned(16))) double col[kN][2];       // the pivot column L[.][c]; before the loop, the diagonal of R
    __shared__ double den[kS];
    __shared__ double load_s;
    __shared__ int dir_of[kS], fall_s;

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = (int)blockIdx.x;
    const int k = bin_lo + kk;
    const double w = kTwoPi * (double)k / (double)T;
    const double* __restrict__ R = cov + (size_t)kk * n * n * 2;
    double* A = chol + (size_t)kk * n * n * 2;      // (no __restrict__: the waves of the workgroup hand entries to each other through it)

    if (tid < kS) dir_of[tid] = tid < S ? slot_direction(offsets[tid], offset_per_dir, dirs) : -1;
    if (tid < n) col[tid][0] = R[((size_t)tid * n + tid) * 2];
    __syncthreads();
    if (tid == 0) {
        double tr = 0.0;
        for (int a = 0; a < n; ++a) tr += col[a][0];                 // ascending a
        const bool ok = tr > 0.0 && tr <= 1.79769313486231570815e308;   // finite and > 0 (a NaN fails both)
        fall_s = ok ? 0 : 1;
        load_s = ok ? loading * tr / (double)n : 0.0;
        fallback[kk] = ok ? 0 : 1;
    }
    if (kk == 0 && tid < S) status[tid] = dir_of[tid] < 0 ? 1 : 0;
    __syncthreads();
    const bool fall = fall_s != 0;
    const double load = load_s;

    // ---- R' into d_chol: the lower triangle of R plus the loading (or I), the strict upper triangle zero
    for (int e = tid; e < n * n; e += kSolveThreads) {
        const int r = e / n, c = e - r * n;
        double re = 0.0, im = 0.0;
        if (fall) {
            re = r == c ? 1.0 : 0.0;
        } else if (c <= r) {
            re = R[2 * (size_t)e];
            im = R[2 * (size_t)e + 1];
            if (r == c) { re = re + load; im = 0.0; }
        }
        A[2 * (size_t)e] = re;
        A[2 * (size_t)e + 1] = im;
    }
    // ---- the right-hand sides c_s[m] = e^{+jw tau[d_s][m]}; zeros for a slot that is no source (they stay zeros)
    for (int e = tid; e < S * n; e += kSolveThreads) {
        const int s = e / n, m = e - s * n;
        const int d = dir_of[s];
        double sn = 0.0, c = 0.0;
        if (d >= 0) sincos(w * tau[(size_t)d * n + m], &sn, &c);
        rhs[s][m][0] = c;
        rhs[s][m][1] = sn;
    }
    __syncthreads();

    // ---- factor in place, column by column; the forward substitutions ride on the parked column
    for (int c = 0; c < n; ++c) {
        const double diag = sqrt(A[((size_t)c * n + c) * 2]);
        if (tid < n - c) {
            const int r = c + tid;
            double* at = A + ((size_t)r * n + c) * 2;
            double lr = diag, li = 0.0;
            if (tid > 0) {                                            // (the pivot itself is written behind the barrier: every wave reads it above)
                lr = at[0] / diag; li = at[1] / diag;
                at[0] = lr; at[1] = li;
            }
            col[r][0] = lr; col[r][1] = li;
        }
        if (wave == kSolveWaves - 1 && lane < S) {                   // y[s][c]: every subtraction of its chain is done
            rhs[lane][c][0] = rhs[lane][c][0] / diag;
            rhs[lane][c][1] = rhs[lane][c][1] / diag;
        }
        __syncthreads();
        if (tid == 0) { A[((size_t)c * n + c) * 2] = diag; A[((size_t)c * n + c) * 2 + 1] = 0.0; }
        for (int r = c + 1 + wave; r < n; r += kSolveWaves) {        // a wave takes a row, its lanes the columns up to the diagonal
            const double ar = col[r][0], ai = col[r][1];
            for (int cc = c + 1 + lane; cc <= r; cc += 64) {
                const double br = col[cc][0], bi = col[cc][1];
                double* at = A + ((size_t)r * n + cc) * 2;
                at[0] = at[0] - (ar * br + ai * bi);                 // - L[r][c] conj(L[cc][c])
                at[1] = cc == r ? 0.0 : at[1] - (ai * br - ar * bi);
            }
        }
        for (int e = tid; e < S * (n - c - 1); e += kSolveThreads) {
            const int s = e / (n - c - 1), r = c + 1 + (e - s * (n - c - 1));
            const double ar = col[r][0], ai = col[r][1], yr = rhs[s][c][0], yi = rhs[s][c][1];
            rhs[s][r][0] = rhs[s][r][0] - (ar * yr - ai * yi);       // - L[r][c] y[c]
            rhs[s][r][1] = rhs[s][r][1] - (ar * yi + ai * yr);
        }
        __syncthreads();
    }

    // ---- den = sum |y_m|^2, ascending m
    if (tid < S) {
        double d = 0.0;
        for (int m = 0; m < n; ++m) d += rhs[tid][m][0] * rhs[tid][m][0] + rhs[tid][m][1] * rhs[tid][m][1];
        den[tid] = d;
    }
    __syncthreads();

    // ---- z = L^{-H} y by rows of L, downwards; thread (s, r) keeps rhs[s][r], the owner of r == q writes the gain
    double fs = 0.0, fc = 1.0;
    sincos(w * (double)(T - 1) / 2.0, &fs, &fc);                     // conj(f0) = e^{+jw(T-1)/2}
    const int r = tid % kN, s0 = tid / kN;                           // (kSolveThreads / kN slots at a time)
    double nr = 0.0, ni = 0.0, nd = 1.0;                             // L[q][r] and L[q][q] of the row about to be applied
    if (r < n) {
        nd = A[((size_t)(n - 1) * n + (n - 1)) * 2];
        if (r < n - 1) { nr = A[((size_t)(n - 1) * n + r) * 2]; ni = A[((size_t)(n - 1) * n + r) * 2 + 1]; }
    }
    for (int q = n - 1; q >= 0; --q) {
        const double lr = nr, li = ni, ld = nd;
        if (q > 0 && r < n) {                                        // row q - 1 is on its way while row q is applied
            nd = A[((size_t)(q - 1) * n + (q - 1)) * 2];
            if (r < q - 1) { nr = A[((size_t)(q - 1) * n + r) * 2]; ni = A[((size_t)(q - 1) * n + r) * 2 + 1]; }
        }
        if (r <= q) {
            for (int s = s0; s < S; s += kSolveThreads / kN) {
                const double zr = rhs[s][q][0] / ld, zi = rhs[s][q][1] / ld;
                if (r < q) {
                    rhs[s][r][0] = rhs[s][r][0] - (lr * zr + li * zi);   // - conj(L[q][r]) z[q]
                    rhs[s][r][1] = rhs[s][r][1] - (lr * zi - li * zr);
                } else {
                    double* __restrict__ g = gains + (((size_t)s * K + kk) * n + (size_t)q) * 2;
                    if (dir_of[s] < 0) {
                        g[0] = 0.0; g[1] = 0.0;
                    } else {
                        const double ur = (zr * fc - zi * fs) / den[s], ui = (zr * fs + zi * fc) / den[s];
                        g[0] = ur;
                        g[1] = -ui;
                    }
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_mvdr_design(const float* d_signals, int m_total, int frames, int n_samples, const int32_t* d_mics, int n, int seg_first, int seg_hop, int segs,
                              const double* d_window, const double* d_tau, int dirs, const int32_t* d_offsets, int sources, int offset_per_dir, int n_taps,
                              int bin_lo, int bin_hi, double loading, double* d_snap, double* d_cov, double* d_chol, double* d_gains, float* d_taps,
                              int32_t* d_status, int32_t* d_fallback, hipStream_t stream)
{
    if (m_total < 1 || frames < 1 || n < 1 || n > kMvdrMaxMics || seg_first < 0 || seg_hop < 1 || segs < 1 || dirs < 1 || sources < 1 || sources > kLcmvMaxSources ||
        offset_per_dir < 1 || n_taps < 1 || n_taps > kLcmvMaxTaps || bin_lo < 0 || bin_hi < bin_lo || bin_hi > n_taps / 2 || !(loading > 0.0) ||
        (long long)seg_first + (long long)(segs - 1) * seg_hop + n_taps > n_samples)
        return hipErrorInvalidValue;
    const int K = bin_hi - bin_lo + 1;
    const long long P = (long long)frames * segs;
    const int snap_blocks = (n + kSnapMics - 1) / kSnapMics;
    const int tiles_1d = (n + kTile - 1) / kTile, tiles = tiles_1d * (tiles_1d + 1) / 2;
    if (P * snap_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mvdr_snapshot_kernel, dim3((unsigned)(P * snap_blocks)), dim3(kSnapThreads), (size_t)n_taps * 3 * sizeof(double), stream, d_signals, d_mics,
                       m_total, n_samples, n, seg_first, seg_hop, segs, d_window, n_taps, bin_lo, K, snap_blocks, d_snap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mvdr_cov_kernel, dim3((unsigned)(K * tiles)), dim3(kCovThreads), 0, stream, d_snap, (int)P, K, n, tiles, d_cov);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mvdr_solve_kernel, dim3((unsigned)K), dim3(kSolveThreads), 0, stream, d_cov, d_tau, d_offsets, dirs, n, sources, offset_per_dir, n_taps,
                       bin_lo, K, loading, d_chol, d_gains, d_status, d_fallback);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_lcmv_taps(d_gains, d_status, sources, n, n_taps, bin_lo, K, d_taps, stream);
}

hipError_t launch_mvdr_learn(const float* d_signals, int m_total, int frames, int n_samples, const int32_t* d_mics, int n, int seg_first, int seg_hop, int segs,
                             const double* d_window, const double* d_weights, double forget, const double* d_tau, int dirs, const int32_t* d_offsets, int sources,
                             int offset_per_dir, int n_taps, int bin_lo, int bin_hi, double loading, double* d_acc, double* d_mass, int32_t* d_used,
                             double* d_snap, double* d_cov, double* d_chol, double* d_gains, float* d_taps, int32_t* d_status, int32_t* d_fallback,
                             hipStream_t stream)
{
    if (m_total < 1 || frames < 0 || n < 1 || n > kMvdrMaxMics || seg_first < 0 || seg_hop < 1 || segs < 1 || dirs < 1 || sources < 1 || sources > kLcmvMaxSources ||
        offset_per_dir < 1 || n_taps < 1 || n_taps > kLcmvMaxTaps || bin_lo < 0 || bin_hi < bin_lo || bin_hi > n_taps / 2 || !(loading > 0.0) ||
        !(forget > 0.0 && forget <= 1.0) || (long long)seg_first + (long long)(segs - 1) * seg_hop + n_taps > n_samples)
        return hipErrorInvalidValue;
    const int K = bin_hi - bin_lo + 1;
    const long long P = (long long)frames * segs;
    const int snap_blocks = (n + kSnapMics - 1) / kSnapMics;
    const int tiles_1d = (n + kTile - 1) / kTile, tiles = tiles_1d * (tiles_1d + 1) / 2;
    if (P * snap_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (frames > 0) {
        hipLaunchKernelGGL(mvdr_learn_snapshot_kernel, dim3((unsigned)(P * snap_blocks)), dim3(kSnapThreads), (size_t)n_taps * 3 * sizeof(double), stream, d_signals,
                           d_mics, m_total, n_samples, n, seg_first, seg_hop, segs, d_window, n_taps, bin_lo, K, snap_blocks, d_snap, d_weights, frames, forget,
                           d_mass, d_used);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mvdr_accumulate_kernel, dim3((unsigned)(K * tiles)), dim3(kCovThreads), 0, stream, d_snap, d_weights, frames, segs, forget, K, n, tiles, d_mass,
                       d_acc, d_cov, frames > 0 ? nullptr : d_used);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mvdr_solve_kernel, dim3((unsigned)K), dim3(kSolveThreads), 0, stream, d_cov, d_tau, d_offsets, dirs, n, sources, offset_per_dir, n_taps,
                       bin_lo, K, loading, d_chol, d_gains, d_status, d_fallback);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_lcmv_taps(d_gains, d_status, sources, n, n_taps, bin_lo, K, d_taps, stream);
}

}  // namespace bf
