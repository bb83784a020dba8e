// band_filter.hip -- bf_band_filter_device: one FIR per band on every row of a frame batch, continuous across windows.
//
// Definition (include/beamformer_hip.h): out[b][f][r][j] = acc_T with acc_0 = 0, acc_{t+1} = fmaf(h[b][t], x~_f[r][j - t], acc_t),
// t = 0 .. T-1 in that order; x~ is the row behind the T - 1 samples that precede it in the stream (the previous frame's
// [hop - (T-1), hop), d_prev for frame 0, zeros without one or with hop = 0).
//
//   band_filter_kernel<KB> : one workgroup of kBandWaves waves per (frame, kBandWaves rows); a wave takes one row.  The wave stages
//       its row once into its own LDS region, s[hp + i] = x~[i] for i in [-(T-1), N) with hp = 4 * ceil(T / 4): the row with
//       16-byte loads where N % 4 == 0 and the pointer allows, the history slice (it starts at an arbitrary sample) and every
//       other shape with dword loads.  A lane owns four consecutive outputs j0 .. j0+3 of a 256-output chunk and slides an
//       eight-float register window down the row: four taps t = 4q .. 4q+3 need x~[j0 - 4q - 3 .. j0 - 4q + 3], the quad read for
//       the step before plus ONE new ds_read_b128 (lane l reads 16 bytes at 16 l + const: every bank once).  That is one LDS
//       read per 16 * KB multiply-adds, and all bands share it.  The taps are wave-uniform: scalar loads of h[b][4q .. 4q+3].
//       Every output's chain runs t = 0 .. T-1 in order whatever the blocking: the q loop ascends, the four taps of a step are
//       applied in order, and a tap past T - 1 is skipped (never multiplied by zero: fmaf(0, x, -0) is +0).
//       KB = 1, 2, 4, 8 or 16 is the smallest of those that holds the call's bands; rows of the tap table past the last band
//       repeat the last band and are not stored.
#include <hip/hip_runtime.h>

#include "das_kernels.h"
#include "fir_window.h"

namespace bf {
namespace {

constexpr int kBandWaves = 4;
constexpr int kLanes = 64;

template <int KB>
__global__ void __launch_bounds__(kBandWaves * kLanes)
band_filter_kernel(const float* __restrict__ signals, const float* __restrict__ prev0, const float* __restrict__ taps, float* __restrict__ out, int rows,
                   int frames, int N, int T, int K, int hop, int groups, int vec_in, int vec_out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int f = (int)(blockIdx.x / (unsigned)groups);
    const int r = ((int)blockIdx.x - f * groups) * kBandWaves + wave;
    const int hp = (T + 3) & ~3;            // floats in front of sample 0: the T - 1 history samples end at hp
    const int n4 = (N + 3) & ~3;
    float* s = lds + wave * (hp + n4);
    const bool live = r < rows;             // (wave-uniform: the last workgroup of a frame may have fewer rows than waves)

    if (live) {
        const float* __restrict__ row = signals + ((size_t)f * rows + r) * N;
        if (vec_in) {
            const float4* __restrict__ row4 = reinterpret_cast<const float4*>(row);
            float4* dst4 = reinterpret_cast<float4*>(s + hp);
            for (int i = lane; i < (N >> 2); i += kLanes) dst4[i] = row4[i];
        } else {
            for (int i = lane; i < N; i += kLanes) s[hp + i] = row[i];
            for (int i = N + lane; i < n4; i += kLanes) s[hp + i] = 0.0f;
        }
        const int hist = T - 1;
        const float* prev = nullptr;
        if (hop > 0) prev = f > 0 ? row - (size_t)rows * N : (prev0 != nullptr ? prev0 + (size_t)r * N : nullptr);
        float* h0 = s + (hp - hist);
        if (prev != nullptr) {
            const float* __restrict__ src = prev + (hop - hist);
            for (int i = lane; i < hist; i += kLanes) h0[i] = src[i];
        } else {
            for (int i = lane; i < hist; i += kLanes) h0[i] = 0.0f;
        }
        for (int i = lane; i < hp - hist; i += kLanes) s[i] = 0.0f;
    }
    __syncthreads();
    if (!live) return;

    const float* hk[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) hk[k] = taps + (size_t)min(k, K - 1) * T;
    const int full = T >> 2, rem = T & 3;

    for (int c0 = 0; c0 < N; c0 += 4 * kLanes) {
        const int j0 = c0 + 4 * lane;
        if (j0 >= N) continue;
        float acc[KB][4];
#pragma unroll
        for (int k = 0; k < KB; ++k)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[k][o] = 0.0f;
        const float* p = s + hp + j0;
        float w[8];
        {
            const float4 b = *reinterpret_cast<const float4*>(p);
            w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        }
#pragma unroll 2
        for (int q = 0; q < full; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(p - 4 * q - 4);
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            fir_taps4<KB>(acc, w, hk, 4 * q, 4);
            w[4] = w[0]; w[5] = w[1]; w[6] = w[2]; w[7] = w[3];
        }
        if (rem) {
            const float4 a = *reinterpret_cast<const float4*>(p - 4 * full - 4);
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            fir_taps4<KB>(acc, w, hk, 4 * full, rem);
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (k < K) {
                float* __restrict__ o = out + (((size_t)k * frames + f) * rows + r) * N + j0;
                if (vec_out) {
                    *reinterpret_cast<float4*>(o) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (j0 + i < N) o[i] = acc[k][i];
                }
            }
        }
    }
}

template <int KB>
void band_filter_enqueue(dim3 grid, size_t lds_bytes, hipStream_t stream, const float* d_signals, const float* d_prev, const float* d_taps, float* d_out,
                         int rows, int frames, int N, int T, int K, int hop, int groups, int vec_in, int vec_out)
{
    hipLaunchKernelGGL(band_filter_kernel<KB>, grid, dim3(kBandWaves * kLanes), lds_bytes, stream, d_signals, d_prev, d_taps, d_out, rows, frames, N, T, K, hop,
                       groups, vec_in, vec_out);
}

}  // namespace

hipError_t launch_band_filter(const float* d_signals, int rows, int frames, int n_samples, int hop, const float* d_prev, const float* d_taps, int n_taps,
                              int bands, float* d_out, hipStream_t stream)
{
    const int N = n_samples, T = n_taps;
    if (rows < 1 || frames < 1 || N < 1 || N > 1024 || T < 1 || T > N || bands < 1 || bands > kBandMaxBands || hop < 0 || hop > N || (hop > 0 && T - 1 > hop))
        return hipErrorInvalidValue;
    const long long groups = ((long long)rows + kBandWaves - 1) / kBandWaves;
    if (frames * groups > 0x7fffffffLL) return hipErrorInvalidValue;
    const int hp = (T + 3) & ~3, n4 = (N + 3) & ~3;
    const size_t lds_bytes = (size_t)kBandWaves * (hp + n4) * sizeof(float);     // at most 4 * 2048 floats = 32 KiB
    // 16-byte accesses: every row starts N floats after the one before, so they need N % 4 == 0 and an aligned base
    const int vec_in = (N % 4 == 0) && (reinterpret_cast<uintptr_t>(d_signals) % 16 == 0);
    const int vec_out = (N % 4 == 0) && (reinterpret_cast<uintptr_t>(d_out) % 16 == 0);
    const dim3 grid((unsigned)(frames * groups));
#define BF_BAND_ARGS grid, lds_bytes, stream, d_signals, d_prev, d_taps, d_out, rows, frames, N, T, bands, hop, (int)groups, vec_in, vec_out
    if (bands <= 1) band_filter_enqueue<1>(BF_BAND_ARGS);
    else if (bands <= 2) band_filter_enqueue<2>(BF_BAND_ARGS);
    else if (bands <= 4) band_filter_enqueue<4>(BF_BAND_ARGS);
    else if (bands <= 8) band_filter_enqueue<8>(BF_BAND_ARGS);
    else band_filter_enqueue<16>(BF_BAND_ARGS);
#undef BF_BAND_ARGS
    return hipGetLastError();
}

}  // namespace bf
