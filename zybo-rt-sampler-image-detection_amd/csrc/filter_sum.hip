// filter_sum.hip -- bf_filter_sum_device: filter-and-sum beams, one FIR per (beam, microphone), then a sum over the microphones.
//
// Definition (include/beamformer_hip.h): c_m[j] = acc_T with acc_0 = 0, acc_{t+1} = fmaf(g[b][m][t], x~_f[r_m][j - t], acc_t), t = 0 .. T-1
// in that order; out[f][b][j] = s_n with s_0 = 0, s_{m+1} = s_m + c_m[j], m = 0 .. n-1 in that order.  x~ is band_filter.hip's: the row
// behind the T - 1 samples that precede it in the stream.
//
//   filter_sum_kernel : one workgroup of W waves (W = blockDim.x / 64, a power of two) per (frame, chunk of 256 outputs, beam).  The
//       microphones go round the waves: in pass p wave w takes microphone m = p W + w.  It stages that row's chunk once into its own
//       LDS region behind its history, s[hp + i] = x~[c0 + i] for i in [-(T-1), 256) with hp = 4 * ceil(T / 4), and runs
//       band_filter.hip's inner loop on it: a lane owns the four consecutive outputs c0 + 4 lane .. + 3 and slides an eight-float register
//       window down the row, ONE ds_read_b128 per four taps (lane l reads 16 bytes at 16 l + const: every bank once); the taps are
//       wave-uniform, scalar loads of g[b][m][4q .. 4q+3].  Every c_m chain runs t = 0 .. T-1 in order whatever the blocking, and a
//       tap past T - 1 is skipped, never multiplied by zero.
//       The wave parks its quad of c_m in LDS (park[w][256], 16-byte stores).  After a barrier wave 0, the OWNER of the outputs, adds
//       the parked quads of the pass to its running s in wave order, which is microphone order; the barrier behind the next pass's
//       staging keeps the next parked values off the ones still being read.  Two barriers per W microphones, n adds beside n T
//       multiply-adds per output, no atomics; which wave computed which microphone cannot show in the result.
//       A workgroup takes ONE beam.  An earlier form with blocks of 2, 4 and 8 beams sharing the LDS reads was measured and dropped
//       (profiles/filter_sum_beam_blocks.txt: at best 14 % ahead, up to 8x behind at one frame) -- the loop waits on latencies, not
//       on the LDS port, and more workgroups hide them better.
//       LDS: W (hp + 256) floats of rows, at most 32 KiB, and W 256 floats of parked quads.
#include <hip/hip_runtime.h>

#include <atomic>

#include "das_kernels.h"
#include "fir_window.h"

namespace bf {
namespace {

constexpr int kLanes = 64;
constexpr int kChunk = 4 * kLanes;        // outputs of a workgroup: a lane owns four
constexpr int kMaxWaves = 16;
constexpr int kLdsRowBytes = 32 * 1024;   // the staged rows of a workgroup

std::atomic<int> g_waves{0};              // filter_sum_waves: 0 = the launch decides

__global__ void __launch_bounds__(kMaxWaves * kLanes)
filter_sum_kernel(const float* __restrict__ signals, const float* __restrict__ prev0, const int32_t* __restrict__ mics, const float* __restrict__ taps,
                  float* __restrict__ out, int m_total, int N, int n, int T, int beams, int hop, int chunks, int out_stride, int vec_in, int vec_out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    int id = (int)blockIdx.x;
    const int b = id % beams; id /= beams;
    const int c0 = (id % chunks) * kChunk;
    const int f = id / chunks;
    const int hp = (T + 3) & ~3;             // floats in front of the chunk's first sample: the T - 1 history samples end at hp
    const int hist = T - 1;
    float* s = lds + wave * (hp + kChunk);
    float* park = lds + W * (hp + kChunk);   // [W][kChunk]
    const int full = T >> 2, rem = T & 3;

    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};

    for (int m0 = 0; m0 < n; m0 += W) {
        const int m = m0 + wave;
        const bool live = m < n;             // (wave-uniform: the last pass may have fewer microphones than waves)
        if (live) {
            const int r = mics[m];
            const float* __restrict__ row = signals + ((size_t)f * m_total + r) * N;
            if (vec_in) {
                const float4* __restrict__ src4 = reinterpret_cast<const float4*>(row + c0);
                const int q_end = (N - c0) >> 2;                     // (N % 4 == 0 here)
                reinterpret_cast<float4*>(s + hp)[lane] = lane < q_end ? src4[lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else {
                for (int i = lane; i < kChunk; i += kLanes) s[hp + i] = c0 + i < N ? row[c0 + i] : 0.0f;
            }
            const float* prev = nullptr;
            if (hop > 0) prev = f > 0 ? row - (size_t)m_total * N : (prev0 != nullptr ? prev0 + (size_t)r * N : nullptr);
            float* h0 = s + (hp - hist);
            for (int i = lane; i < hist; i += kLanes) {
                const int idx = c0 - hist + i;                       // >= -hist >= -hop where there is a hop
                h0[i] = idx >= 0 ? row[idx] : (prev != nullptr ? prev[hop + idx] : 0.0f);
            }
            for (int i = lane; i < hp - hist; i += kLanes) s[i] = 0.0f;
        }
        __syncthreads();     // the row is staged; every owner is done with the quads parked in the pass before
        if (live) {
            const float* const gm[1] = {taps + ((size_t)b * n + m) * T};
            float acc[1][4] = {{0.0f, 0.0f, 0.0f, 0.0f}};
            const float* p = s + hp + 4 * lane;
            float w[8];
            {
                const float4 a = *reinterpret_cast<const float4*>(p);
                w[4] = a.x; w[5] = a.y; w[6] = a.z; w[7] = a.w;
            }
#pragma unroll 2
            for (int q = 0; q < full; ++q) {
                const float4 a = *reinterpret_cast<const float4*>(p - 4 * q - 4);
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
                fir_taps4<1>(acc, w, gm, 4 * q, 4);
                w[4] = w[0]; w[5] = w[1]; w[6] = w[2]; w[7] = w[3];
            }
            if (rem) {
                const float4 a = *reinterpret_cast<const float4*>(p - 4 * full - 4);
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
                fir_taps4<1>(acc, w, gm, 4 * full, rem);
            }
            *reinterpret_cast<float4*>(park + (wave * kChunk + 4 * lane)) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
        }
        __syncthreads();     // the pass's quads are parked
        if (wave == 0) {     // the owner of the workgroup's outputs
            const int n_pass = min(W, n - m0);
            for (int v = 0; v < n_pass; ++v) {                       // microphones m0 .. m0 + n_pass - 1, in order
                const float4 c = *reinterpret_cast<const float4*>(park + (v * kChunk + 4 * lane));
                sum[0] = sum[0] + c.x; sum[1] = sum[1] + c.y; sum[2] = sum[2] + c.z; sum[3] = sum[3] + c.w;
            }
        }
    }

    const int j0 = c0 + 4 * lane;
    if (wave != 0 || j0 >= N) return;
    float* __restrict__ o = out + ((size_t)f * beams + b) * out_stride + j0;
    if (vec_out && j0 + 3 < N) {
        *reinterpret_cast<float4*>(o) = make_float4(sum[0], sum[1], sum[2], sum[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j0 + i < N) o[i] = sum[i];
    }
}

}  // namespace

int filter_sum_waves(int waves)
{
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4 && waves != 8 && waves != 16) return -1;
    return g_waves.exchange(waves);
}

hipError_t launch_filter_sum(const float* d_signals, int m_total, int frames, int n_samples, int hop, const float* d_prev, const int32_t* d_mics, int n,
                             const float* d_taps, int n_taps, int beams, float* d_out, int out_stride, int n_cus, hipStream_t stream)
{
    const int N = n_samples, T = n_taps;
    if (m_total < 1 || frames < 1 || N < 1 || N > 1024 || n < 1 || T < 1 || T > N || beams < 1 || beams > kFilterSumMaxBeams || hop < 0 || hop > N ||
        (hop > 0 && T - 1 > hop) || out_stride < N)
        return hipErrorInvalidValue;
    const int chunks = (N + kChunk - 1) / kChunk;
    const long long groups = (long long)frames * chunks * beams;
    if (groups > 0x7fffffffLL) return hipErrorInvalidValue;
    const int hp = (T + 3) & ~3;
    const int row_bytes = (hp + kChunk) * (int)sizeof(float), park_bytes = kChunk * (int)sizeof(float);
    // waves of a workgroup, as measured (scripts/dev/filter_sum_time.py): a launch of at most one workgroup per compute unit -- the
    // live, one-window case -- splits its microphones over 16 waves, up to four per compute unit over 8, a larger one over 4.
    // Either way only as many as the rows' LDS holds, and no more than twice the microphones.
    int waves = g_waves.load();
    if (waves == 0) waves = groups <= n_cus ? kMaxWaves : groups <= 4LL * n_cus ? 8 : 4;
    while (waves > 1 && (waves * row_bytes > kLdsRowBytes || waves / 2 >= n)) waves >>= 1;
    const size_t lds_bytes = (size_t)waves * (row_bytes + park_bytes);
    // 16-byte accesses: a row starts a multiple of N floats after the base, an output row a multiple of out_stride
    const int vec_in = (N % 4 == 0) && (reinterpret_cast<uintptr_t>(d_signals) % 16 == 0);
    const int vec_out = (out_stride % 4 == 0) && (reinterpret_cast<uintptr_t>(d_out) % 16 == 0);
    hipLaunchKernelGGL(filter_sum_kernel, dim3((unsigned)groups), dim3(waves * kLanes), lds_bytes, stream, d_signals, d_prev, d_mics, d_taps, d_out, m_total, N, n,
                       T, beams, hop, chunks, out_stride, vec_in, vec_out);
    return hipGetLastError();
}

}  // namespace bf
