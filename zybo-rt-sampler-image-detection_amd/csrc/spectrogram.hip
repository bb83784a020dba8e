// spectrogram.hip -- bf_spectrogram_device: the rows of a continuous float32 stream (beam audio) as spectral frames: windowed STFT power
// through a filterbank, linear or on a log scale, continuous across calls.
//
// Definition (include/beamformer_hip.h): with s0 = d_state[0] and L = the call's new samples, frame j covers x[s0 + j hop .. + n_win) of
// hist || x[0 .. L); u = window * x, zero-padded to n_fft; P_k = |DFT(u)_k|^2 for k <= n_fft / 2; E_b = sum_k bank[b][k] P_k over the band's
// support; out = E or scale * log10f(max(E, floor)).
//
//   spectrogram_kernel : a workgroup takes one (row, frame) slot (a work item; the grid walks the items): one wave up to n_fft = 512, four
//       waves above.  LDS (dynamic, 3 n_fft floats: 1.5 KiB at n_fft = 128, 48 KiB at 4096): re[n_fft], im[n_fft], and the twiddles,
//       from sincospif.  The transform is lds_fft.h's (its header states the rounding model that the error budget of
//       tests/spectrogram_np.py rests on, and why the bank conflicts of the passes stay).  P overwrites re[0 .. n_fft / 2].  Then a lane
//       owns a band and walks its support in ascending k, one multiply and one add per bin.  Every value of a frame is computed by one
//       fixed sequence of float32 operations on the frame's own n_win samples: the workgroup size, the frame's index, the row count and
//       the alignment of the pointers do not enter it, which is what the bit-exact promises of the definition rest on.
//       The kernel only READS d_state, d_hist and d_len: every workgroup derives count from them.
//   spectrogram_advance_kernel : one workgroup per row behind it on the same stream: the row's new history, staged whole in LDS before
//       any of it is written (with L < n_win - 1 the history shifts inside itself); workgroup 0 also writes the state and (count, status).
//       The other workgroups read d_state[0] only to learn whether the state is valid, which the write cannot change (a valid s0 is
//       followed by a valid s0', an invalid one is left alone), so it does not matter on which side of the write they read it; both
//       sides use relaxed atomic accesses.
#include <hip/hip_runtime.h>

#include "das_kernels.h"
#include "lds_fft.h"
#include "stream_grid.h"

namespace bf {
namespace {

constexpr int kSpectrogramMaxGrid = 1 << 20;   // workgroups of a launch; more items than that are walked
constexpr int kSpectrogramAdvanceLanes = 256;

__device__ __forceinline__ int spectrogram_len(const int* __restrict__ d_len, int len)
{
    return d_len != nullptr ? min(max(d_len[0], 0), len) : len;
}

// Frames a call completes from a valid state: j with s0 + j hop + n_win <= L.
__device__ __forceinline__ int spectrogram_count(int s0, int L, int n_win, int hop)
{
    const long long room = (long long)L - n_win - s0;
    return room >= 0 ? (int)(room / hop) + 1 : 0;       // (<= ceil(L / hop) as s0 >= -(n_win - 1))
}

__global__ void __launch_bounds__(256)
spectrogram_kernel(const float* __restrict__ in, int rows, int in_stride, int len, const int* __restrict__ d_len, const float* __restrict__ hist,
                   const int* __restrict__ state, const float* __restrict__ window, int n_win, int n_fft, int log2n, int hop,
                   const float* __restrict__ bank, const int* __restrict__ support, int n_bands, float scale, float floor_,
                   float* __restrict__ out, int out_frames, int cap, long long items)
{
    extern __shared__ float lds[];
    float* re = lds;
    float* im = lds + n_fft;
    float* twc = lds + 2 * n_fft;               // cos, then -sin, of 2 pi m / n_fft for m < n_fft / 2
    float* tws = twc + (n_fft >> 1);
    const int lane = (int)threadIdx.x, lanes = (int)blockDim.x;
    const int H = n_win - 1, half_n = n_fft >> 1, n_bins = half_n + 1;
    const int s0 = state[0];
    const int L = spectrogram_len(d_len, len);
    const int count = s0 >= -H ? spectrogram_count(s0, L, n_win, hop) : 0;

    fft_twiddles_f32(twc, tws, n_fft, half_n, lane, lanes);

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)(item / cap);
        const int j = (int)(item - (long long)r * cap);
        float* o = out + ((size_t)r * out_frames + j) * n_bands;
        if (j >= count) {                       // (uniform over the workgroup) a slot behind the last frame
            for (int b = lane; b < n_bands; b += lanes) o[b] = 0.0f;
            continue;
        }
        const long long sj = (long long)s0 + (long long)j * hop;           // >= -H, and sj + n_win <= L
        const float* x = in + (size_t)r * in_stride;
        const float* h = hist + (size_t)r * H;
        for (int t = lane; t < n_fft; t += lanes) {           // (stage_windowed, zero-padded behind n_win)
            float u = 0.0f;
            if (t < n_win) {
                const long long s = sj + t;
                u = window[t] * (s < 0 ? h[H + s] : x[s]);
            }
            const int rev = fft_rev(t, log2n);
            re[rev] = u;
            im[rev] = 0.0f;
        }
        __syncthreads();                        // (also: the twiddles are there)
        fft_passes(re, im, twc, tws, log2n, half_n, lane, lanes, 1.0f);
        for (int k = lane; k < n_bins; k += lanes) re[k] = re[k] * re[k] + im[k] * im[k];     // P_k, each by the lane that read it
        __syncthreads();
        for (int b = lane; b < n_bands; b += lanes) {
            float e;
            if (bank == nullptr) {
                e = re[b];                      // (n_bands == n_bins)
            } else {
                int lo = 0, hi = n_bins;
                if (support != nullptr) {
                    lo = max(support[2 * b], 0);
                    hi = min(support[2 * b + 1], n_bins);
                }
                const float* w = bank + (size_t)b * n_bins;
                e = 0.0f;
                for (int k = lo; k < hi; ++k) e = e + w[k] * re[k];
            }
            o[b] = scale == 0.0f ? e : scale * log10f(e < floor_ ? floor_ : e);      // (a NaN stays a NaN)
        }
        __syncthreads();                        // the next item restages re and im
    }
}

__global__ void __launch_bounds__(kSpectrogramAdvanceLanes)
spectrogram_advance_kernel(const float* __restrict__ in, int in_stride, int len, const int* __restrict__ d_len, float* __restrict__ hist, int* state,
                           int* __restrict__ count_status, int n_win, int hop)
{
    extern __shared__ float stage[];            // n_win - 1 floats: the row's new history
    const int H = n_win - 1, lane = (int)threadIdx.x, r = (int)blockIdx.x;
    const int s0 = __atomic_load_n(state, __ATOMIC_RELAXED);
    const bool ok = s0 >= -H;                   // (the same answer before and after workgroup 0's write)
    const int L = spectrogram_len(d_len, len);
    if (ok) {                                   // a corrupt state is reported and everything is left as it was
        float* h = hist + (size_t)r * H;
        const float* x = in + (size_t)r * in_stride;
        carry_stage(stage, h, H, L, lane, kSpectrogramAdvanceLanes, [&](long long s) { return x[s]; });
        __syncthreads();                        // everything that reads the row's old d_hist has read it
        carry_write(h, stage, H, lane, kSpectrogramAdvanceLanes);
    }
    if (r == 0 && lane == 0) {
        if (!ok) {
            count_status[0] = 0;
            count_status[1] = 1;
            return;
        }
        const int count = spectrogram_count(s0, L, n_win, hop);
        __atomic_store_n(state, (int)((long long)s0 + (long long)count * hop - L), __ATOMIC_RELAXED);
        state[1] = 0;
        state[2] = 0;
        state[3] = 0;
        count_status[0] = count;
        count_status[1] = 0;
    }
}

}  // namespace

long long spectrogram_capacity(long long len, int hop)
{
    if (len < 0 || hop < 1) return -1;
    return len / hop + (len % hop != 0);
}

hipError_t launch_spectrogram(const float* d_in, int rows, int in_stride, int len, const int32_t* d_len, float* d_hist, int32_t* d_state, const float* d_window,
                              int n_win, int n_fft, int hop, const float* d_bank, const int32_t* d_support, int n_bands, float scale, float floor_,
                              float* d_out, int out_frames, int32_t* d_count, hipStream_t stream)
{
    const int log2n = fft_log2(n_fft);
    if (rows < 1 || len < 0 || in_stride < len || n_fft < kSpectrogramMinFft || n_fft > kSpectrogramMaxFft || log2n < 0 || n_win < 1 ||
        n_win > n_fft || hop < 1 || n_bands < 1 || n_bands > kSpectrogramMaxBands || (d_bank == nullptr && n_bands != n_fft / 2 + 1))
        return hipErrorInvalidValue;
    const long long cap = spectrogram_capacity(len, hop);
    if (out_frames < cap) return hipErrorInvalidValue;
    if (cap > 0) {
        const long long items = cap * rows;
        const unsigned grid = (unsigned)(items < kSpectrogramMaxGrid ? items : kSpectrogramMaxGrid);
        hipLaunchKernelGGL(spectrogram_kernel, dim3(grid), dim3(fft_lanes(n_fft)), 3 * (size_t)n_fft * sizeof(float), stream, d_in, rows, in_stride, len, d_len, d_hist,
                           d_state, d_window, n_win, n_fft, log2n, hop, d_bank, d_support, n_bands, scale, floor_, d_out, out_frames, (int)cap, items);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(spectrogram_advance_kernel, dim3((unsigned)rows), dim3(kSpectrogramAdvanceLanes), (size_t)(n_win - 1) * sizeof(float), stream, d_in,
                       in_stride, len, d_len, d_hist, d_state, d_count, n_win, hop);
    return hipGetLastError();
}

}  // namespace bf
