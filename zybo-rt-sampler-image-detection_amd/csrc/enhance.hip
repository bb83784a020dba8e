// enhance.hip -- bf_enhance_device: noise suppression of beam audio by short-time Fourier gains: analysis, a gain per (frame, bin) --
// a decision-directed Wiener rule over a soft-decision recursive noise tracker, or the caller's own -- and overlap-add synthesis,
// continuous across windows and calls.
//
// Definition (include/beamformer_hip.h), on the window stream and the frame grid of stream_grid.h: u = win_a * x, X = DFT(u), P = |X|^2; G
// from the recursion over the frames in order (or d_gain_in); v = win_s / n_fft * IDFT(G X); y = the frames' v added in ascending frame
// order; d_out = y delayed by n_fft.
//
// Four launches on the stream.  d_work holds, behind a header of four ints, X [rows][cap][2][n_bins], P and G [rows][cap][n_bins] and
// v [rows][cap][n_fft].
//   enhance_analysis_kernel : a workgroup takes one (row, frame) item (the grid walks the items): one wave up to n_fft = 512, four waves
//       above.  LDS (dynamic, 3 n_fft floats: 3 KiB at n_fft = 256, 48 KiB at 4096): re[n_fft], im[n_fft] and the twiddles, from double.
//       The transform is lds_fft.h's (its header states the rounding model that the error budget of tests/enhance_np.py rests on, and
//       why the bank conflicts of the passes stay).  X and P go to d_work.  Reads d_state and d_hist only.
//   enhance_gain_kernel : a thread per (row, bin) walks the call's frames in order: the recursion in the header's float32 operations
//       (the build has -ffp-contract=off; the fused steps are written __fmaf_rn, the divisions __fdiv_rn), G to d_work and the
//       observables.  The thread reads its own d_noise / d_prior element first and writes it last; nothing else touches them.  Thread 0
//       also writes the grid's header.
//   enhance_synthesis_kernel : a workgroup per (row, frame) again: Y = G X staged with its Hermitian extension at the bit-reversed
//       index, the inverse passes at n_fft complex points, v to d_work.
//   enhance_overlap_kernel : a lane per output sample gathers the <= 8 frames that cover it, in ascending frame order, behind the
//       carried partial sum where the position lies before the call's x[0].  The first workgroup of every row (the `tail`) takes the
//       n_fft outputs that read d_ola, the row's new d_ola and the history carry, all staged in LDS (2 n_fft floats) before any of them is
//       written; the other workgroups read v only.  Workgroup 0 also writes d_state and d_count.
// Every value is computed by one fixed sequence of float32 operations on its own frame's samples and its own bin's state: the lane
// count depends on n_fft alone, and the row count, the frame's index in the call and the alignment of the pointers do not enter.  The
// bit promises of the definition rest on that.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "das_kernels.h"
#include "lds_fft.h"
#include "stream_grid.h"

namespace bf {
namespace {

constexpr int kEnhanceMaxGrid = 1 << 20;        // workgroups of a launch; more items than that are walked
constexpr int kEnhanceLanes = 256;              // of the gain and the overlap-add launches

// The grid of a call: d_state = (c, seen, 0, 0), seen >= 0 the frames the tracker has taken so far.
__device__ __forceinline__ FrameGrid enhance_grid(const int* __restrict__ state, int S, int hop_s)
{
    const int c = state[0], seen = state[1];
    return frame_grid(c, frame_phase_ok(c, hop_s) && seen >= 0, S, hop_s);
}

__global__ void __launch_bounds__(256)
enhance_analysis_kernel(const float* __restrict__ in, int rows, int n, int in_stride, int len, int S, const float* __restrict__ hist,
                        const int* __restrict__ state, const float* __restrict__ win_a, int n_fft, int log2n, int hop_s, float* __restrict__ spec,
                        float* __restrict__ power, int cap, long long items)
{
    extern __shared__ float lds[];
    float* re = lds;
    float* im = lds + n_fft;
    float* twc = lds + 2 * n_fft;
    float* tws = twc + (n_fft >> 1);
    const int lane = (int)threadIdx.x, lanes = (int)blockDim.x;
    const int H = n_fft - 1, half_n = n_fft >> 1, n_bins = half_n + 1;
    const FrameGrid st = enhance_grid(state, S, hop_s);
    const WindowStream ws = window_stream(in, rows, n, in_stride, len);

    fft_twiddles(twc, tws, n_fft, half_n, lane, lanes);

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / cap);
        const int i = (int)(item - (long long)r * cap);
        if (i >= st.count) continue;            // (uniform over the workgroup) a slot behind the last frame: the gain launch zeroes it
        const long long start = frame_start(i, hop_s, st.c, n_fft);                // >= -H, and start + n_fft <= S
        const float* hist_r = hist + (size_t)r * H;
        stage_windowed(re, im, win_a, n_fft, log2n, lane, lanes, [&](int t) { return stream_or_history(ws, r, hist_r, H, start + t); });
        __syncthreads();                        // u is staged (also: the twiddles are there)
        fft_passes(re, im, twc, tws, log2n, half_n, lane, lanes, 1.0f);
        float* x = spec + (size_t)item * 2 * n_bins;
        float* pw = power + (size_t)item * n_bins;
        for (int k = lane; k < n_bins; k += lanes) {
            const float a = re[k], b = im[k];
            x[k] = a;
            x[n_bins + k] = b;
            pw[k] = a * a + b * b;
        }
        __syncthreads();                        // the next item restages re and im
    }
}

__global__ void __launch_bounds__(kEnhanceLanes)
enhance_gain_kernel(const int* __restrict__ state, int rows, int S, int n_bins, int hop_s, int cap, const float* __restrict__ power,
                    const float* __restrict__ gain_in, float alpha, float a_noise, float g0, float g1, float g_min, int n_init, float* __restrict__ noise,
                    float* __restrict__ prior, float* __restrict__ gain, float* __restrict__ power_out, float* __restrict__ gain_out, int* __restrict__ header)
{
    const FrameGrid st = enhance_grid(state, S, hop_s);
    const long long idx = (long long)blockIdx.x * kEnhanceLanes + threadIdx.x;
    if (idx == 0) grid_header_write(header, st);
    if (idx >= (long long)rows * n_bins) return;
    const int r = (int)(idx / n_bins), k = (int)(idx - (long long)r * n_bins);
    const size_t at = ((size_t)r * cap) * n_bins + k;       // (r, frame 0, k); a frame further is n_bins further
    float lam = 0.0f, pri = 0.0f;
    if (gain_in == nullptr && st.count > 0) {
        lam = noise[idx];
        pri = prior[idx];
    }
    const float one_minus_alpha = 1.0f - alpha, one_minus_a_noise = 1.0f - a_noise, width = g1 - g0;
    for (int i = 0; i < st.count; ++i) {
        const size_t o = at + (size_t)i * n_bins;
        const float P = power[o];
        float G;
        if (gain_in != nullptr) {
            G = gain_in[o];
        } else if (!finite_f32(P)) {            // not finite: the bin's state stays, the frame comes out non-finite
            G = __builtin_nanf("");
        } else {
            const long long seen = (long long)state[1] + i;
            if (seen < n_init) {
                lam = seen == 0 ? P : lam + __fdiv_rn(P - lam, (float)(seen + 1));
            } else {
                const float g = __fdiv_rn(P, lam < FLT_MIN ? FLT_MIN : lam);
                float p = __fdiv_rn(g - g0, width);
                p = p < 0.0f ? 0.0f : p;
                p = p > 1.0f ? 1.0f : p;
                const float a = a_noise + one_minus_a_noise * p;
                lam = __fmaf_rn(1.0f - a, P - lam, lam);
            }
            const float den = lam < FLT_MIN ? FLT_MIN : lam;
            const float gam = __fdiv_rn(P, den);
            float ratio = __fdiv_rn(pri, den);
            ratio = ratio > FLT_MAX ? FLT_MAX : ratio;
            float excess = gam - 1.0f;
            excess = excess < 0.0f ? 0.0f : excess;
            const float xi = __fmaf_rn(alpha, ratio, one_minus_alpha * excess);
            G = 1.0f - __fdiv_rn(1.0f, 1.0f + xi);
            G = G < g_min ? g_min : G;
            pri = (G * G) * P;
        }
        gain[o] = G;
        if (power_out != nullptr) power_out[o] = P;
        if (gain_out != nullptr) gain_out[o] = G;
    }
    for (int i = st.count; i < cap; ++i) {
        const size_t o = at + (size_t)i * n_bins;
        if (power_out != nullptr) power_out[o] = 0.0f;
        if (gain_out != nullptr) gain_out[o] = 0.0f;
    }
    if (gain_in == nullptr && st.count > 0) {
        noise[idx] = lam;
        prior[idx] = pri;
    }
}

__global__ void __launch_bounds__(256)
enhance_synthesis_kernel(const int* __restrict__ state, int S, const float* __restrict__ win_s, int n_fft, int log2n, int hop_s,
                         const float* __restrict__ spec, const float* __restrict__ gain, float* __restrict__ frames, int cap, long long items)
{
    extern __shared__ float lds[];
    float* re = lds;
    float* im = lds + n_fft;
    float* twc = lds + 2 * n_fft;
    float* tws = twc + (n_fft >> 1);
    const int lane = (int)threadIdx.x, lanes = (int)blockDim.x;
    const int half_n = n_fft >> 1, n_bins = half_n + 1;
    const FrameGrid st = enhance_grid(state, S, hop_s);
    const float inv_n = 1.0f / (float)n_fft;    // (a power of two)

    fft_twiddles(twc, tws, n_fft, half_n, lane, lanes);

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int i = (int)(item % cap);
        if (i >= st.count) continue;            // (uniform over the workgroup)
        const float* x = spec + (size_t)item * 2 * n_bins;
        const float* g = gain + (size_t)item * n_bins;
        for (int k = lane; k < n_bins; k += lanes) {
            const float G = g[k];
            fft_stage_hermitian(re, im, k, G * x[k], G * x[n_bins + k], n_fft, half_n, log2n);
        }
        __syncthreads();                        // Y is staged (also: the twiddles are there)
        fft_passes(re, im, twc, tws, log2n, half_n, lane, lanes, -1.0f);
        float* v = frames + (size_t)item * n_fft;
        for (int t = lane; t < n_fft; t += lanes) v[t] = (win_s[t] * inv_n) * re[t];
        __syncthreads();                        // the next item restages re and im
    }
}

// The enhanced stream at position t (relative to the call's x[0], -n_fft <= t < S): the carried partial sum where t < 0, then the
// call's frames that cover t, in ascending order.
__device__ __forceinline__ float enhance_gather(const float* __restrict__ ola_r, const float* __restrict__ frames_r, long long t, int c, int count, int n_fft,
                                                int hop_s)
{
    float acc = t < 0 ? ola_r[t + n_fft] : 0.0f;
    // frame i covers t where (i + 1) hop_s - c - n_fft <= t <= (i + 1) hop_s - c - 1
    const long long first = (t + c + n_fft + hop_s) / hop_s - n_fft / hop_s - 1;       // ceil((t + c + 1) / hop_s) - 1, the numerator kept positive
    const long long last = (t + c + n_fft) / hop_s - 1;
    const int lo = (int)(first < 0 ? 0 : first);
    const int hi = (int)(last < count - 1 ? last : count - 1);
    for (int i = lo; i <= hi; ++i) {
        acc = acc + frames_r[(size_t)i * n_fft + (t - frame_start(i, hop_s, c, n_fft))];
    }
    return acc;
}

__global__ void __launch_bounds__(kEnhanceLanes)
enhance_overlap_kernel(const float* __restrict__ in, int rows, int n, int in_stride, int len, int S, float* hist, float* ola, int* __restrict__ state,
                       const int* __restrict__ header, const float* __restrict__ frames, int n_fft, int hop_s, int cap, bool tracks, int n_init,
                       float* __restrict__ out, int out_stride, int* __restrict__ count_status, int blocks_per_row, long long items)
{
    extern __shared__ float stage[];            // the tail's: the row's new d_ola [n_fft], then its new d_hist [n_fft - 1]
    const int lane = (int)threadIdx.x, H = n_fft - 1;
    const auto [c, count, ok] = grid_header_read(header);
    const WindowStream ws = window_stream(in, rows, n, in_stride, len);

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / blocks_per_row);
        const int b = (int)(item - (long long)r * blocks_per_row);
        const float* frames_r = frames + (size_t)r * cap * n_fft;
        float* ola_r = ola + (size_t)r * n_fft;
        float* out_r = out + (size_t)r * out_stride;
        if (b > 0) {                            // outputs s >= n_fft: positions inside the call, this call's frames only
            const long long s = (long long)n_fft + (long long)(b - 1) * kEnhanceLanes + lane;
            if (s < S) out_r[s] = ok ? enhance_gather(ola_r, frames_r, s - n_fft, c, count, n_fft, hop_s) : 0.0f;
            continue;
        }
        const int head = S < n_fft ? S : n_fft;                  // the outputs that read d_ola
        if (!ok) {                              // a corrupt state is reported and everything is left as it was
            for (int s = lane; s < head; s += kEnhanceLanes) out_r[s] = 0.0f;
        } else {
            float* hist_r = hist + (size_t)r * H;
            float* new_hist = stage + n_fft;
            for (int j = lane; j < n_fft; j += kEnhanceLanes) stage[j] = enhance_gather(ola_r, frames_r, (long long)S - n_fft + j, c, count, n_fft, hop_s);
            carry_stage(new_hist, hist_r, H, S, lane, kEnhanceLanes, [&](long long s) { return stream_at(ws, r, s); });
            for (int s = lane; s < head; s += kEnhanceLanes) out_r[s] = enhance_gather(ola_r, frames_r, (long long)s - n_fft, c, count, n_fft, hop_s);
            __syncthreads();                    // everything that reads the old d_ola and d_hist of the row has read them
            for (int j = lane; j < n_fft; j += kEnhanceLanes) ola_r[j] = stage[j];
            carry_write(hist_r, new_hist, H, lane, kEnhanceLanes);
            __syncthreads();                    // the next item restages
        }
        if (r == 0 && lane == 0) {
            if (!ok) {
                report(count_status, false, 0);
            } else {
                const long long seen = (long long)state[1] + count;
                state[0] = (int)(((long long)c + S) % hop_s);
                if (tracks) state[1] = (int)(seen < n_init ? seen : n_init);
                state[2] = 0;
                state[3] = 0;
                report(count_status, true, count);
            }
        }
    }
}

}  // namespace

long long enhance_workspace(int rows, long long samples, int n_fft, int hop_s)
{
    if (rows < 1 || !frame_grid_ok(samples, n_fft, hop_s)) return -1;
    const long long slots = (long long)rows * frame_cap(samples, hop_s);             // < 2^61
    return kGridHeader + slots * (4LL * (n_fft / 2 + 1) + n_fft);
}

hipError_t launch_enhance(const float* d_in, int rows, int frames, int n, int in_stride, int hop, float* d_hist, float* d_ola, float* d_noise, float* d_prior,
                          int32_t* d_state, const float* d_win_a, const float* d_win_s, int n_fft, int hop_s, const float* d_gain_in, float alpha, float a_noise,
                          float g0, float g1, float g_min, int n_init, float* d_work, float* d_out, int out_stride, float* d_power_out, float* d_gain_out,
                          int32_t* d_count, hipStream_t stream)
{
    if (rows < 1 || frames < 1 || n < 1 || hop < 0 || hop > n || in_stride < n) return hipErrorInvalidValue;
    const auto [len, S, fits] = stream_len(frames, hop, n);
    if (!fits || enhance_workspace(rows, S, n_fft, hop_s) < 0 || out_stride < S) return hipErrorInvalidValue;
    const int log2n = fft_log2(n_fft);
    const int n_bins = n_fft / 2 + 1;
    const long long cap = frame_cap(S, hop_s), items = cap * rows;
    int32_t* header = reinterpret_cast<int32_t*>(d_work);
    float* spec = d_work + kGridHeader;
    float* power = spec + (size_t)items * 2 * n_bins;
    float* gain = power + (size_t)items * n_bins;
    float* v = gain + (size_t)items * n_bins;
    const unsigned grid = (unsigned)(items < kEnhanceMaxGrid ? items : kEnhanceMaxGrid);
    const unsigned lanes = fft_lanes(n_fft);
    const size_t lds = 3 * (size_t)n_fft * sizeof(float);

    hipLaunchKernelGGL(enhance_analysis_kernel, dim3(grid), dim3(lanes), lds, stream, d_in, rows, n, in_stride, len, (int)S, d_hist, d_state, d_win_a, n_fft,
                       log2n, hop_s, spec, power, (int)cap, items);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long cells = (long long)rows * n_bins;
    hipLaunchKernelGGL(enhance_gain_kernel, dim3((unsigned)((cells + kEnhanceLanes - 1) / kEnhanceLanes)), dim3(kEnhanceLanes), 0, stream, d_state, rows, (int)S,
                       n_bins, hop_s, (int)cap, power, d_gain_in, alpha, a_noise, g0, g1, g_min, n_init, d_noise, d_prior, gain, d_power_out, d_gain_out, header);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(enhance_synthesis_kernel, dim3(grid), dim3(lanes), lds, stream, d_state, (int)S, d_win_s, n_fft, log2n, hop_s, spec, gain, v, (int)cap,
                       items);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long inner = S > n_fft ? S - n_fft : 0;
    const long long blocks_per_row = 1 + (inner + kEnhanceLanes - 1) / kEnhanceLanes, blocks = blocks_per_row * rows;
    hipLaunchKernelGGL(enhance_overlap_kernel, dim3((unsigned)(blocks < kEnhanceMaxGrid ? blocks : kEnhanceMaxGrid)), dim3(kEnhanceLanes),
                       (size_t)(2 * n_fft) * sizeof(float), stream, d_in, rows, n, in_stride, len, (int)S, d_hist, d_ola, d_state, header, v, n_fft, hop_s, (int)cap,
                       d_gain_in == nullptr, n_init, d_out, out_stride, d_count, (int)blocks_per_row, blocks);
    return hipGetLastError();
}

}  // namespace bf
