// postfilter.hip -- bf_postfilter_device: the multichannel post-filter (Zelinski 1988; Simmer's variant) on bf_enhance_device's frame grid.  After
// steering to a look direction the target is coherent across the microphones and sensor or diffuse noise is not, so the mean cross-spectrum
// of the n (n - 1) / 2 pairs over the mean power is a Wiener gain per (frame, bin) that needs no noise history; the pair sum is
// (|sum Z|^2 - sum |Z|^2) / 2, so no pair loop exists.
//
// Definition (include/beamformer_hip.h), on the frame grid of stream_grid.h, every microphone read `lag` samples late: u = window * x,
// X = DFT(u), q = |X|^2, Z = a X with the slot's steering a; Y = sum_m Z, Q = sum_m q; num = (|Y|^2 - Q) / (n (n - 1)), den = Q / n or
// |Y|^2 / n^2; N and D smooth them per (slot, bin); G = clamp(max(N, 0) / D).
//
// Four launches on the stream.  d_work holds, behind a header of sixteen ints, the frames' flags int32 [slots][cap] and the raw num and den
// [slots][cap][n_bins].
//   postfilter_steer_kernel : a thread per (slot, microphone, bin): sincospi in double, rounded once, into d_steer; zeros for a slot that is
//       no source.
//   postfilter_analysis_kernel : the work.  A workgroup of 256 lanes owns one frame and walks the microphones.  Up to n_fft = 512 (kSplit)
//       each of the four waves transforms its own microphone in its own re / im buffer (lds_fft.h's passes with lanes = 64; all four waves
//       reach the passes' barriers in step, a wave without a microphone in the last round runs them over stale values and adds nothing);
//       above, the whole workgroup takes one microphone, as fft_lanes prescribes.  LDS (dynamic): the waves' buffers and the twiddles,
//       9 n_fft floats split (18 KiB at 512), 3 n_fft otherwise (48 KiB at 4096).  Behind each transform a lane adds q and the slots' Z of
//       its bins (k = lane + lanes * j, j < BPL, a template parameter so that the sums stay in registers) to its running Q and Y; a slot
//       that is no source is skipped.  The split waves' partial sums then meet in LDS, slot by slot, in wave order: ((w0 + w1) + w2) + w3.
//       The order of every sum is fixed by (n, n_fft): the row count of the frames, the rows the microphones occupy, the slot count and
//       the frame's index do not enter.  A frame's flag says whether all of its num and den are finite.  Reads d_state and d_hist only.
//   postfilter_gain_kernel : a thread per (slot, bin) walks the call's frames in order: the recursion in the header's float32 operations
//       (the build has -ffp-contract=off; the fused steps are __fmaf_rn, the division __fdiv_rn).  It reads its own d_num / d_den element
//       first and writes it last.  The thread of bin 0 also writes d_status and the slot's new `seen` behind the grid's header, thread 0 the
//       header.
//   postfilter_carry_kernel : a workgroup per microphone does the history carry; workgroup 0 also writes d_state and d_count.  It alone
//       writes what is carried, so a replayed graph advances the stream.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "das_kernels.h"
#include "design_device.h"
#include "lds_fft.h"
#include "stream_grid.h"

namespace bf {
namespace {

constexpr int kPostfilterMaxGrid = 1 << 20;     // workgroups of the analysis launch; more frames than that are walked
constexpr int kPostfilterLanes = 256;
constexpr int kPostfilterHeader = 16;           // ints in front of d_work: the grid's four, then (seen'[8], 0, 0, 0, 0)
constexpr int kSplitMaxFft = 512;               // up to here a wave transforms a microphone on its own

// The grid of a call: d_state = (c, 0, seen[slots]), seen in {0, 1}: whether the slot's N and D hold a frame yet.
__device__ __forceinline__ FrameGrid postfilter_grid(const int* __restrict__ state, int slots, int S, int hop_s)
{
    const int c = state[0];
    bool ok = frame_phase_ok(c, hop_s);
    for (int b = 0; b < slots; ++b) ok = ok && (state[2 + b] == 0 || state[2 + b] == 1);
    return frame_grid(c, ok, S, hop_s);
}

__global__ void __launch_bounds__(kPostfilterLanes)
postfilter_steer_kernel(const double* __restrict__ tau, const int32_t* __restrict__ offsets, int dirs, int n, int slots, int offset_per_dir, int n_fft, int n_bins,
                        float* __restrict__ steer)
{
    const long long idx = (long long)blockIdx.x * kPostfilterLanes + threadIdx.x;
    if (idx >= (long long)slots * n * n_bins) return;
    const int k = (int)(idx % n_bins), m = (int)((idx / n_bins) % n), b = (int)(idx / ((long long)n_bins * n));
    const int d = slot_direction(offsets[b], offset_per_dir, dirs);
    float ar = 0.0f, ai = 0.0f;
    if (d >= 0) {
        double s, c;
        sincospi(2.0 * (double)k * tau[(size_t)d * n + m] / (double)n_fft, &s, &c);
        ar = (float)c;
        ai = (float)-s;
    }
    steer[2 * idx] = ar;
    steer[2 * idx + 1] = ai;
}

// One (slot, frame, bin): the raw numerator and denominator; whether both are finite.
__device__ __forceinline__ bool postfilter_emit(float yr, float yi, float Q, float pairs, float den_div, int den_mode, float* __restrict__ num_w,
                                                float* __restrict__ den_w, size_t at)
{
    const float yy = yr * yr + yi * yi;
    const float num = __fdiv_rn(yy - Q, pairs);
    const float den = __fdiv_rn(den_mode == 0 ? Q : yy, den_div);
    num_w[at] = num;
    den_w[at] = den;
    return finite_f32(num) && finite_f32(den);
}

template <int BPL, bool SPLIT>
__global__ void __launch_bounds__(kPostfilterLanes)
postfilter_analysis_kernel(const float* __restrict__ in, int m_total, int n_samples, int len, int S, const int32_t* __restrict__ mics, int n,
                           const float* __restrict__ hist, int H, const int32_t* __restrict__ state, const int32_t* __restrict__ offsets, int slots, int offset_per_dir,
                           int dirs, const float* __restrict__ window, int n_fft, int log2n, int hop_s, int lag, const float* __restrict__ steer, int den_mode,
                           float* __restrict__ num_w, float* __restrict__ den_w, int32_t* __restrict__ flag_w, int cap)
{
    extern __shared__ float lds[];
    constexpr int kWaves = SPLIT ? 4 : 1, kRowLanes = kPostfilterLanes / kWaves, kS = kPostfilterMaxSlots;
    const int tid = (int)threadIdx.x, wave = SPLIT ? tid >> 6 : 0, lane = SPLIT ? tid & 63 : tid;
    const int half_n = n_fft >> 1, K = half_n + 1;
    float* re = lds + (size_t)wave * 2 * n_fft;
    float* im = re + n_fft;
    float* twc = lds + (size_t)kWaves * 2 * n_fft;
    float* tws = twc + half_n;
    const FrameGrid st = postfilter_grid(state, slots, S, hop_s);
    const WindowStream ws = window_stream(in, m_total, n_samples, n_samples, len);
    unsigned src = 0;                           // the slots that are sources
    for (int b = 0; b < slots; ++b) src |= slot_direction(offsets[b], offset_per_dir, dirs) >= 0 ? 1u << b : 0u;
    const float pairs = (float)(n * (n - 1)), den_div = den_mode == 0 ? (float)n : (float)(n * n);     // (exact: n <= 256)
    const int rounds = (n + kWaves - 1) / kWaves;

    fft_twiddles(twc, tws, n_fft, half_n, tid, kPostfilterLanes);

    for (int i = (int)blockIdx.x; i < cap; i += (int)gridDim.x) {
        if (i >= st.count) continue;            // (uniform over the workgroup) a slot behind the last frame: the gain launch zeroes it
        const int start = frame_start<int>(i, hop_s, st.c, n_fft, lag);  // >= -H, and start + n_fft <= S - lag
        float Q[BPL], Yr[kS][BPL], Yi[kS][BPL];
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            Q[j] = 0.0f;
#pragma unroll
            for (int b = 0; b < kS; ++b) Yr[b][j] = Yi[b][j] = 0.0f;
        }
        for (int r = 0; r < rounds; ++r) {
            const int m = r * kWaves + wave;    // (uniform over the wave)
            if (m < n) {
                const int row = mics[m];
                const float* hist_m = hist + (size_t)m * H;
                stage_windowed(re, im, window, n_fft, log2n, lane, kRowLanes, [&](int t) { return stream_or_history(ws, row, hist_m, H, start + t); });
            }
            __syncthreads();                    // u is staged (also: the twiddles are there)
            fft_passes(re, im, twc, tws, log2n, half_n, lane, kRowLanes, 1.0f);
            if (m < n) {
#pragma unroll
                for (int j = 0; j < BPL; ++j) {
                    const int k = lane + kRowLanes * j;
                    if (k < K) {
                        const float xr = re[k], xi = im[k];
                        Q[j] = Q[j] + (xr * xr + xi * xi);
#pragma unroll
                        for (int b = 0; b < kS; ++b)
                            if (src >> b & 1u) {
                                const float* a = steer + (((size_t)b * n + m) * K + k) * 2;
                                const float ar = a[0], ai = a[1];
                                Yr[b][j] = Yr[b][j] + (ar * xr - ai * xi);
                                Yi[b][j] = Yi[b][j] + (ar * xi + ai * xr);
                            }
                    }
                }
            }
            __syncthreads();                    // the next microphone (or the meeting of the partial sums) restages re and im
        }
        if (SPLIT) {
            // the waves' partial sums meet in LDS, a slot at a time: [wave][Yr, Yi, Q][K] floats over the waves' buffers (12 K <= 8 n_fft)
            float* meet = lds;
            float Qt[2] = {0.0f, 0.0f};         // of the bins tid and tid + 256 (K <= 257)
            bool first = true;
#pragma unroll
            for (int b = 0; b < kS; ++b) {
                if (!(src >> b & 1u)) continue; // (uniform over the workgroup)
#pragma unroll
                for (int j = 0; j < BPL; ++j) {
                    const int k = lane + kRowLanes * j;
                    if (k < K) {
                        meet[(wave * 3 + 0) * K + k] = Yr[b][j];
                        meet[(wave * 3 + 1) * K + k] = Yi[b][j];
                        if (first) meet[(wave * 3 + 2) * K + k] = Q[j];
                    }
                }
                __syncthreads();                // the four partial sums of the slot are there
                bool fin = true;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int k = tid + kPostfilterLanes * jj;
                    if (k < K) {
                        const float yr = ((meet[0 * K + k] + meet[3 * K + k]) + meet[6 * K + k]) + meet[9 * K + k];
                        const float yi = ((meet[1 * K + k] + meet[4 * K + k]) + meet[7 * K + k]) + meet[10 * K + k];
                        if (first) Qt[jj] = ((meet[2 * K + k] + meet[5 * K + k]) + meet[8 * K + k]) + meet[11 * K + k];
                        fin = postfilter_emit(yr, yi, Qt[jj], pairs, den_div, den_mode, num_w, den_w, ((size_t)b * cap + i) * K + k) && fin;
                    }
                }
                const int all = __syncthreads_and(fin ? 1 : 0);          // (also: the next slot overwrites `meet`)
                if (tid == 0) flag_w[(size_t)b * cap + i] = all;
                first = false;
            }
        } else {
#pragma unroll
            for (int b = 0; b < kS; ++b) {
                if (!(src >> b & 1u)) continue; // (uniform over the workgroup)
                bool fin = true;
#pragma unroll
                for (int j = 0; j < BPL; ++j) {
                    const int k = lane + kRowLanes * j;
                    if (k < K) fin = postfilter_emit(Yr[b][j], Yi[b][j], Q[j], pairs, den_div, den_mode, num_w, den_w, ((size_t)b * cap + i) * K + k) && fin;
                }
                const int all = __syncthreads_and(fin ? 1 : 0);
                if (tid == 0) flag_w[(size_t)b * cap + i] = all;
            }
        }
        __syncthreads();                        // the next frame restages re and im
    }
}

__global__ void __launch_bounds__(kPostfilterLanes)
postfilter_gain_kernel(const int32_t* __restrict__ state, const int32_t* __restrict__ offsets, int slots, int offset_per_dir, int dirs, int S, int n_bins, int hop_s,
                       int cap, const float* __restrict__ num_w, const float* __restrict__ den_w, const int32_t* __restrict__ flag_w, float beta, float g_min,
                       float* __restrict__ d_num, float* __restrict__ d_den, float* __restrict__ gains, float* __restrict__ num_out, float* __restrict__ den_out,
                       int32_t* __restrict__ status, int32_t* __restrict__ header)
{
    const FrameGrid st = postfilter_grid(state, slots, S, hop_s);
    const long long idx = (long long)blockIdx.x * kPostfilterLanes + threadIdx.x;
    if (idx == 0) grid_header_write(header, st);
    if (idx >= (long long)slots * n_bins) return;
    const int b = (int)(idx / n_bins), k = (int)(idx - (long long)b * n_bins);
    const bool source = slot_direction(offsets[b], offset_per_dir, dirs) >= 0;
    const size_t at = ((size_t)b * cap) * n_bins + k;       // (b, frame 0, k); a frame further is n_bins further
    const bool runs = source && st.count > 0;
    int seen = st.ok ? state[2 + b] : 0;
    float N = 0.0f, D = 0.0f;
    if (runs && seen != 0) {
        N = d_num[idx];
        D = d_den[idx];
    }
    for (int i = 0; i < (runs ? st.count : 0); ++i) {
        const size_t o = at + (size_t)i * n_bins;
        const float num = num_w[o], den = den_w[o];
        float G;
        if (flag_w[(size_t)b * cap + i] == 0) { // a frame with a non-finite num or den: the slot's state stays, the frame comes out NaN
            G = __builtin_nanf("");
        } else {
            if (seen == 0) {
                N = num;
                D = den;
                seen = 1;
            } else {
                N = __fmaf_rn(beta, N - num, num);
                D = __fmaf_rn(beta, D - den, den);
            }
            if (D > 0.0f) {
                G = __fdiv_rn(N < 0.0f ? 0.0f : N, D);
                G = G < g_min ? g_min : G;
                G = G > 1.0f ? 1.0f : G;
            } else {
                G = g_min;
            }
        }
        gains[o] = G;
        if (num_out != nullptr) num_out[o] = num;
        if (den_out != nullptr) den_out[o] = den;
    }
    for (int i = runs ? st.count : 0; i < cap; ++i) {
        const size_t o = at + (size_t)i * n_bins;
        gains[o] = 0.0f;
        if (num_out != nullptr) num_out[o] = 0.0f;
        if (den_out != nullptr) den_out[o] = 0.0f;
    }
    if (runs && seen != 0) {
        d_num[idx] = N;
        d_den[idx] = D;
    }
    if (k == 0) {
        status[b] = source ? 0 : 1;
        header[kGridHeader + b] = source ? seen : 0;    // (every bin of a slot sees the same flags: `seen` is the slot's)
    }
}

__global__ void __launch_bounds__(kPostfilterLanes)
postfilter_carry_kernel(const float* __restrict__ in, int m_total, int n_samples, int len, int S, const int32_t* __restrict__ mics, int n, float* hist, int H,
                        int32_t* __restrict__ state, int slots, int hop_s, const int32_t* __restrict__ header, int32_t* __restrict__ count_status)
{
    extern __shared__ float stage[];            // the row's new d_hist [H]
    const int lane = (int)threadIdx.x, m = (int)blockIdx.x;
    const FrameGrid st = grid_header_read(header);
    if (st.ok) {                                // a corrupt state is reported and everything is left as it was
        float* hist_m = hist + (size_t)m * H;
        const int row = mics[m];
        const WindowStream ws = window_stream(in, m_total, n_samples, n_samples, len);
        carry_stage(stage, hist_m, H, S, lane, kPostfilterLanes, [&](long long s) { return stream_at(ws, row, (int)s); });
        __syncthreads();                        // everything that reads the row's old d_hist has read it
        carry_write(hist_m, stage, H, lane, kPostfilterLanes);
    }
    if (m == 0 && lane == 0) {
        if (!st.ok) {
            report(count_status, false, 0);
        } else {
            state[0] = (int)(((long long)st.c + S) % hop_s);
            state[1] = 0;
            for (int b = 0; b < slots; ++b) state[2 + b] = header[kGridHeader + b];
            report(count_status, true, st.count);
        }
    }
}

template <int BPL, bool SPLIT>
void launch_analysis(unsigned grid, size_t lds, hipStream_t stream, const float* in, int m_total, int n_samples, int len, int S, const int32_t* mics, int n,
                     const float* hist, int H, const int32_t* state, const int32_t* offsets, int slots, int offset_per_dir, int dirs, const float* window, int n_fft,
                     int log2n, int hop_s, int lag, const float* steer, int den_mode, float* num_w, float* den_w, int32_t* flag_w, int cap)
{
    hipLaunchKernelGGL((postfilter_analysis_kernel<BPL, SPLIT>), dim3(grid), dim3(kPostfilterLanes), lds, stream, in, m_total, n_samples, len, S, mics, n, hist, H,
                       state, offsets, slots, offset_per_dir, dirs, window, n_fft, log2n, hop_s, lag, steer, den_mode, num_w, den_w, flag_w, cap);
}

}  // namespace

long long postfilter_workspace(int slots, long long samples, int n_fft, int hop_s)
{
    if (slots < 1 || slots > kPostfilterMaxSlots || !frame_grid_ok(samples, n_fft, hop_s)) return -1;
    const long long cells = (long long)slots * frame_cap(samples, hop_s);            // < 2^34
    return kPostfilterHeader + cells * (1 + 2LL * (n_fft / 2 + 1));
}

hipError_t launch_postfilter(const float* d_signals, int m_total, int frames, int n_samples, int hop, const int32_t* d_mics, int n, const double* d_tau, int dirs,
                             const int32_t* d_offsets, int slots, int offset_per_dir, float* d_hist, float* d_num, float* d_den, int32_t* d_state,
                             const float* d_window, int n_fft, int hop_s, int lag, int den_mode, float beta, float g_min, float* d_work, float* d_steer,
                             float* d_gains, float* d_num_out, float* d_den_out, int32_t* d_status, int32_t* d_count, hipStream_t stream)
{
    if (m_total < 1 || frames < 1 || n_samples < 1 || hop < 0 || hop > n_samples || n < 2 || n > kMvdrMaxMics || dirs < 1 || offset_per_dir < 1 || lag < 0 ||
        lag > n_fft || (den_mode != 0 && den_mode != 1))
        return hipErrorInvalidValue;
    const auto [len, S, fits] = stream_len(frames, hop, n_samples);
    if (!fits || postfilter_workspace(slots, S, n_fft, hop_s) < 0) return hipErrorInvalidValue;
    const int log2n = fft_log2(n_fft), n_bins = n_fft / 2 + 1, H = n_fft - 1 + lag;
    const long long cap = frame_cap(S, hop_s), cells = cap * slots;
    int32_t* header = reinterpret_cast<int32_t*>(d_work);
    int32_t* flag_w = header + kPostfilterHeader;
    float* num_w = d_work + kPostfilterHeader + cells;
    float* den_w = num_w + (size_t)cells * n_bins;

    const long long phasors = (long long)slots * n * n_bins;
    hipLaunchKernelGGL(postfilter_steer_kernel, dim3((unsigned)((phasors + kPostfilterLanes - 1) / kPostfilterLanes)), dim3(kPostfilterLanes), 0, stream, d_tau,
                       d_offsets, dirs, n, slots, offset_per_dir, n_fft, n_bins, d_steer);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    const bool split = n_fft <= kSplitMaxFft;
    const unsigned grid = (unsigned)(cap < kPostfilterMaxGrid ? cap : kPostfilterMaxGrid);
    const size_t lds = (split ? 9 : 3) * (size_t)n_fft * sizeof(float);
    const int bpl = (n_bins + (split ? 64 : 256) - 1) / (split ? 64 : 256);           // the bins of a lane: 1, 2, 3, 5 (split), 3, 5, 9
#define BF_POSTFILTER_ANALYSIS(BPL, SPLIT)                                                                                                                    \
    launch_analysis<BPL, SPLIT>(grid, lds, stream, d_signals, m_total, n_samples, len, (int)S, d_mics, n, d_hist, H, d_state, d_offsets, slots, offset_per_dir, \
                                dirs, d_window, n_fft, log2n, hop_s, lag, d_steer, den_mode, num_w, den_w, flag_w, (int)cap)
    if (split) {
        if (bpl == 1) BF_POSTFILTER_ANALYSIS(1, true);
        else if (bpl == 2) BF_POSTFILTER_ANALYSIS(2, true);
        else if (bpl == 3) BF_POSTFILTER_ANALYSIS(3, true);
        else BF_POSTFILTER_ANALYSIS(5, true);
    } else {
        if (bpl == 3) BF_POSTFILTER_ANALYSIS(3, false);
        else if (bpl == 5) BF_POSTFILTER_ANALYSIS(5, false);
        else BF_POSTFILTER_ANALYSIS(9, false);
    }
#undef BF_POSTFILTER_ANALYSIS
    e = hipGetLastError();
    if (e != hipSuccess) return e;

    const long long bins = (long long)slots * n_bins;
    hipLaunchKernelGGL(postfilter_gain_kernel, dim3((unsigned)((bins + kPostfilterLanes - 1) / kPostfilterLanes)), dim3(kPostfilterLanes), 0, stream, d_state,
                       d_offsets, slots, offset_per_dir, dirs, (int)S, n_bins, hop_s, (int)cap, num_w, den_w, flag_w, beta, g_min, d_num, d_den, d_gains, d_num_out,
                       d_den_out, d_status, header);
    e = hipGetLastError();
    if (e != hipSuccess) return e;

    hipLaunchKernelGGL(postfilter_carry_kernel, dim3((unsigned)n), dim3(kPostfilterLanes), (size_t)H * sizeof(float), stream, d_signals, m_total, n_samples, len,
                       (int)S, d_mics, n, d_hist, H, d_state, slots, hop_s, header, d_count);
    return hipGetLastError();
}

}  // namespace bf
