// resample.hip -- bf_resample_device: rational sample-rate conversion (up / down) of the rows of a window stream, continuous across
// windows and calls, as float32 and as 16-bit PCM.
//
// Definition (include/beamformer_hip.h): with (o, phi) = d_state[0..1], output k of row r sits at a_k = phi + k * M of the L-times
// upsampled stream: i_k = o + a_k / L, p_k = a_k % L, and y[r][k] = acc_T with acc_0 = 0, acc_{t+1} = fmaf(h[p_k][t], x[i_k - t], acc_t),
// t = 0 .. T-1 in that order, while i_k < S.  x is the call's stream: the last `len` samples of every window, behind the T - 1 samples
// that end the previous call's last window (d_prev; zeros without one).
//
//   resample_kernel<VEC> : a workgroup of 256 lanes takes `run` <= 256 consecutive outputs [k0, k0 + run) of one row (a work item; the
//       grid walks the items).  Their inputs are the contiguous span x[i_k0 - (T-1) .. i_klast], at most ceil((run - 1) M / L) + T
//       samples: the launch halves `run` until that fits the 16 KiB of LDS (run = 256 up to M / L = 15; 32 at the steepest
//       decimation allowed, M = 64 L, with 128 taps).  The span is staged through the window mapping, sample by sample: it crosses
//       window boundaries every `len` samples and may begin in d_prev.  A lane owns one output and walks its coefficient row h[p_k]
//       -- every lane another row, at most 4 MB of table in all, L2-resident -- with 16-byte loads where T % 4 == 0 and the table is
//       16-byte aligned (VEC), dword loads otherwise; the LDS reads of neighbouring lanes are M / L samples apart, so for the rate
//       changes near 1 that audio needs a wave reads 64 consecutive banks.  The chain runs t = 0 .. T-1 in order either way.
//       Why 256: the streaming call (one window, hop 128, four beams) has 4 x 126 outputs, two waves' worth per row, and is bound by
//       the latency of one chain whatever the shape; a batch wants the T - 1 samples of overlap between neighbouring spans
//       staged as rarely as the LDS allows.
//       The kernel only READS d_state: every workgroup derives count from it, so no launch with many workgroups writes it.
//   resample_advance_kernel : one thread behind it on the same stream: the new state and (count, status).
#include <hip/hip_runtime.h>

#include "das_kernels.h"
#include "stream_grid.h"

namespace bf {
namespace {

constexpr int kResampleLanes = 256;
constexpr int kResampleSpan = 4096;        // floats of LDS a work item's inputs may take
constexpr int kResampleMaxGrid = 1 << 20;  // workgroups of a launch; more items than that are walked

// Outputs a call emits from a valid state: k with o + (phi + k M) / L < S.
__device__ __forceinline__ long long resample_count(int o, int phi, int S, int L, int M)
{
    return o < S ? ((long long)(S - o) * L - phi + M - 1) / M : 0;
}

__device__ __forceinline__ bool resample_state_ok(int o, int phi, int L) { return o >= 0 && phi >= 0 && phi < L; }

template <bool VEC>
__global__ void __launch_bounds__(kResampleLanes)
resample_kernel(const float* __restrict__ in, const float* __restrict__ prev, const float* __restrict__ taps, const int* __restrict__ state, float gain,
                float* __restrict__ out, short* __restrict__ pcm, int* __restrict__ clip, int rows, int n, int in_stride, int len, int S, int L, int M, int T,
                int out_stride, int cap, int run, int blocks_per_row, long long items)
{
    __shared__ __attribute__((aligned(16))) float s[kResampleSpan];
    const int o = state[0], phi = state[1];
    const int count = resample_state_ok(o, phi, L) ? (int)resample_count(o, phi, S, L, M) : 0;   // (<= cap, which fits an int)
    const WindowStream ws = window_stream(in, rows, n, in_stride, len);
    const int lane = (int)threadIdx.x;

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / blocks_per_row);
        const int k0 = (int)(item - (long long)r * blocks_per_row) * run;
        const int k1 = (int)min((long long)k0 + run, (long long)cap);      // this item's slots [k0, k1): outputs up to kc, zeros behind
        const int kc = min(k1, count);
        long long i0 = 0;
        if (kc > k0) {                          // (uniform over the workgroup)
            i0 = o + (phi + (long long)k0 * M) / L;
            const long long i1 = o + (phi + (long long)(kc - 1) * M) / L;      // < S
            const int i_lo = (int)i0 - (T - 1);
            const int span = min((int)i1 - i_lo + 1, kResampleSpan);           // (the launch chose `run` so that the span fits)
            for (int j = lane; j < span; j += kResampleLanes) {
                const int si = i_lo + j;
                float v = 0.0f;
                if (si >= 0) {
                    v = stream_at(ws, r, si);
                } else if (prev != nullptr) {
                    v = prev[(size_t)r * in_stride + n + si];
                }
                s[j] = v;
            }
        }
        __syncthreads();
        const int k = k0 + lane;
        bool clipped = false;
        if (lane < run && k < k1) {
            float v = 0.0f;
            if (k < kc) {
                const long long a = phi + (long long)k * M;
                const long long q = a / L;
                const int p = (int)(a - q * L);
                const float* x = s + ((int)(o + q - i0) + (T - 1));            // x[-t] = the stream's x[i_k - t]
                const float* __restrict__ h = taps + (size_t)p * T;
                float acc = 0.0f;
                if (VEC) {
                    const float4* __restrict__ h4 = reinterpret_cast<const float4*>(h);
#pragma unroll 2
                    for (int t4 = 0; t4 < (T >> 2); ++t4) {
                        const float4 c = h4[t4];
                        const float* xt = x - 4 * t4;
                        acc = __fmaf_rn(c.x, xt[0], acc);
                        acc = __fmaf_rn(c.y, xt[-1], acc);
                        acc = __fmaf_rn(c.z, xt[-2], acc);
                        acc = __fmaf_rn(c.w, xt[-3], acc);
                    }
                } else {
                    for (int t = 0; t < T; ++t) acc = __fmaf_rn(h[t], x[-t], acc);
                }
                v = acc * gain;
            }
            if (out != nullptr) out[(size_t)r * out_stride + k] = v;
            if (pcm != nullptr) {
                const float rounded = rintf(v * 32768.0f);     // ties to even
                int q16;
                if (rounded != rounded) { q16 = 0; clipped = true; }
                else if (rounded > 32767.0f) { q16 = 32767; clipped = true; }
                else if (rounded < -32768.0f) { q16 = -32768; clipped = true; }
                else q16 = (int)rounded;
                pcm[(size_t)k * rows + r] = (short)q16;
            }
        }
        if (clip != nullptr) {                  // (uniform; all lanes of the wave are here)
            const int hits = __popcll(__ballot(clipped));
            if ((lane & 63) == 0 && hits > 0) atomicAdd(clip + r, hits);
        }
        __syncthreads();                        // the next item restages s
    }
}

__global__ void resample_advance_kernel(int* __restrict__ state, int* __restrict__ count_status, int S, int L, int M)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int o = state[0], phi = state[1];
    if (!resample_state_ok(o, phi, L)) {        // a corrupt state is reported and left as it was
        report(count_status, false, 0);
        return;
    }
    const long long count = resample_count(o, phi, S, L, M);
    const long long A = phi + count * M;        // (count = 0 for o >= S: A = phi < L, and the state moves back by S)
    state[0] = (int)(o + A / L - S);
    state[1] = (int)(A % L);
    state[2] = 0;
    state[3] = 0;
    report(count_status, true, (int)count);
}

}  // namespace

long long resample_capacity(long long samples_in, int up, int down)
{
    if (samples_in < 0 || up < 1 || down < 1 || samples_in > 0x7fffffffffffffffLL / up - down) return -1;
    return (samples_in * up + down - 1) / down;
}

hipError_t launch_resample(const float* d_in, int rows, int frames, int n, int in_stride, int hop, const float* d_prev, const float* d_taps, int up, int down,
                           int n_taps, int32_t* d_state, float gain, float* d_out, int out_stride, short* d_pcm, int32_t* d_clip, int32_t* d_count,
                           hipStream_t stream)
{
    const int L = up, M = down, T = n_taps;
    if (rows < 1 || frames < 1 || n < 1 || L < 1 || L > kResampleMaxPhases || M < 1 || M > 64LL * L || T < 1 || T > kResampleMaxTaps || hop < 0 || hop > n ||
        in_stride < n || (d_out == nullptr && d_pcm == nullptr))
        return hipErrorInvalidValue;
    const auto [len, S, fits] = stream_len(frames, hop, n);
    if (!fits) return hipErrorInvalidValue;
    const long long cap = resample_capacity(S, L, M);
    if (T - 1 > len || cap < 1 || cap > 0x7fffffffLL || (d_out != nullptr && out_stride < cap)) return hipErrorInvalidValue;
    int run = kResampleLanes;
    while (run > 1 && ((long long)(run - 1) * M + L - 1) / L + T > kResampleSpan) run >>= 1;      // (run = 1: T <= 128 samples always fit)
    const long long blocks_per_row = (cap + run - 1) / run, items = blocks_per_row * rows;
    const unsigned grid = (unsigned)(items < kResampleMaxGrid ? items : kResampleMaxGrid);
    const bool vec = (T % 4 == 0) && (reinterpret_cast<uintptr_t>(d_taps) % 16 == 0);
    int32_t* clip = d_pcm != nullptr ? d_clip : nullptr;      // the meter counts PCM samples
#define BF_RESAMPLE_ARGS dim3(grid), dim3(kResampleLanes), 0, stream, d_in, d_prev, d_taps, d_state, gain, d_out, d_pcm, clip, rows, n, in_stride, len, (int)S, L, M, T, \
                         out_stride, (int)cap, run, (int)blocks_per_row, items
    if (vec) hipLaunchKernelGGL(resample_kernel<true>, BF_RESAMPLE_ARGS);
    else hipLaunchKernelGGL(resample_kernel<false>, BF_RESAMPLE_ARGS);
#undef BF_RESAMPLE_ARGS
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(resample_advance_kernel, dim3(1), dim3(1), 0, stream, d_state, d_count, (int)S, L, M);
    return hipGetLastError();
}

}  // namespace bf
