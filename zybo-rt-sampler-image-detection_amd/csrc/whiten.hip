// whiten.hip -- bf_whiten_device: the rows of a frame batch with every in-band DFT bin weighted by |X_k|^-beta (beta = 1: the phase
// transform, PHAT), K bands in one launch.  The weighting is zero-phase and per row, so it leaves every inter-microphone delay intact:
// a PHAT map is the existing map of whitened frames.
//
// Definition (include/beamformer_hip.h): u = window * x; X_k = DFT(u)_k for k <= N / 2; band b keeps lo <= k < hi, with
// d_k = max(|X_k|, max(floor_abs, floor_rel * rms_b)) and W_k = X_k (beta == 0), X_k / d_k (beta == 1) or d_k^-beta X_k; out = gain / N times
// the real inverse transform of the Hermitian extension of W.
//
//   whiten_kernel : a workgroup takes one (frame, row) item (the grid walks the items): one wave up to N = 512, four waves above.
//       LDS (dynamic, 4.5 N + 8 floats: 4.6 KiB at N = 256, 18 KiB at N = 1024, 72 KiB at N = 4096):
//           re[N], im[N]           the working arrays of both transforms
//           twc[N / 2], tws[N / 2] the twiddles, from double
//           xr, xi, mag [N / 2 + 1] the kept half spectrum and |X_k|, shared by all bands of the item
//           red[4]                 a band's power sum, one partial per wave
//       Both transforms are lds_fft.h's (its header states the rounding model that the error budget of tests/whiten_np.py rests on,
//       and why the bank conflicts of the passes stay): the inverse runs at N complex points on the Hermitian extension of W and its
//       real part is the output.
//       Every value of a row is computed by one fixed sequence of float32 operations on the row's own N samples and the band's own
//       scalars: the lane count depends on N alone, the band's power sum has a fixed shape (lane-strided partials in ascending k, an
//       xor butterfly over the wave, then the waves' partials in order), and nothing is shared between bands but X.  The bit promises
//       of the definition rest on that.  Scaling a row by 2^e scales X, |X| (a correctly rounded sqrtf of an exactly scaled sum), the
//       rms (an IEEE division by the bin count) and the floor exactly, so X_k / d_k keeps its bits.
#include <hip/hip_runtime.h>

#include "das_kernels.h"
#include "lds_fft.h"

namespace bf {
namespace {

constexpr int kWhitenMaxGrid = 2048;            // workgroups of a launch; more items than that are walked

__global__ void __launch_bounds__(256)
whiten_kernel(const float* __restrict__ in, const float* __restrict__ window, WhitenBands bands, int n_bands, float floor_rel, float floor_abs, int n,
              int log2n, float* __restrict__ out, long long items)
{
    extern __shared__ float lds[];
    const int half_n = n >> 1, n_bins = half_n + 1;
    float* re = lds;
    float* im = re + n;
    float* twc = im + n;
    float* tws = twc + half_n;
    float* xr = tws + half_n;
    float* xi = xr + n_bins;
    float* mag = xi + n_bins;
    float* red = mag + n_bins;
    const int lane = (int)threadIdx.x, lanes = (int)blockDim.x, wave = lane >> 6, waves = lanes >> 6;

    fft_twiddles(twc, tws, n, half_n, lane, lanes);

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const float* x = in + (size_t)item * n;
        for (int t = lane; t < n; t += lanes) {
            const float u = window != nullptr ? window[t] * x[t] : x[t];
            const int rev = fft_rev(t, log2n);
            re[rev] = u;
            im[rev] = 0.0f;
        }
        __syncthreads();                        // u is staged (also: the twiddles are there)
        fft_passes(re, im, twc, tws, log2n, half_n, lane, lanes, 1.0f);
        for (int k = lane; k < n_bins; k += lanes) {
            const float a = re[k], b = im[k];
            xr[k] = a;
            xi[k] = b;
            mag[k] = sqrtf(a * a + b * b);
        }
        __syncthreads();                        // the half spectrum is kept; re / im are free for the bands

        for (int b = 0; b < n_bands; ++b) {     // (everything read from `bands` is uniform over the workgroup)
            const int lo = bands.lo[b], hi = bands.hi[b];
            const float beta = bands.beta[b];
            float* o = out + ((size_t)b * (size_t)items + (size_t)item) * n;
            float floor_b = 0.0f;
            if (beta != 0.0f) {
                float part = 0.0f;
                for (int k = lo + lane; k < hi; k += lanes) part = part + (xr[k] * xr[k] + xi[k] * xi[k]);
                for (int m = 32; m >= 1; m >>= 1) part = part + __shfl_xor(part, m);        // every lane of the wave holds the same sum
                if ((lane & 63) == 0) red[wave] = part;
                __syncthreads();                // the waves' partials are there (behind the band before: its passes' barriers)
                float sum = red[0];
                for (int w = 1; w < waves; ++w) sum = sum + red[w];
                const float rms = sqrtf(sum / (float)(hi - lo));
                const float rel = floor_rel * rms;
                floor_b = floor_abs > rel ? floor_abs : rel;     // (a NaN rms leaves floor_abs: the row is NaN anyway)
            }
            for (int k = lane; k < n_bins; k += lanes) {
                float wr = 0.0f, wi = 0.0f;
                if (k >= lo && k < hi) {
                    const float a = xr[k], c = xi[k];
                    if (beta == 0.0f) {
                        wr = a;
                        wi = c;
                    } else {
                        const float m = mag[k];
                        const float d = m < floor_b ? floor_b : m;           // (a NaN |X_k| stays)
                        if (d == 0.0f) {
                            wr = 0.0f;
                            wi = 0.0f;
                        } else if (beta == 1.0f) {
                            wr = a / d;
                            wi = c / d;
                        } else {
                            const float g = powf(d, -beta);
                            wr = g * a;
                            wi = g * c;
                        }
                    }
                }
                fft_stage_hermitian(re, im, k, wr, wi, n, half_n, log2n);
            }
            __syncthreads();                    // Y is staged
            fft_passes(re, im, twc, tws, log2n, half_n, lane, lanes, -1.0f);
            const float scale = bands.gain[b] * (1.0f / (float)n);           // (1 / N is a power of two: gain / N exactly)
            for (int j = lane; j < n; j += lanes) o[j] = scale * re[j];
            __syncthreads();                    // the next band, or the next item, restages re and im
        }
    }
}

}  // namespace

hipError_t launch_whiten(const float* d_signals, long long items, int n_samples, const float* d_window, const WhitenBands& bands, int n_bands, float floor_rel,
                         float floor_abs, float* d_out, hipStream_t stream)
{
    const int log2n = fft_log2(n_samples);
    if (items < 1 || n_samples < kWhitenMinN || n_samples > kWhitenMaxN || log2n < 0 || n_bands < 1 || n_bands > kWhitenMaxBands)
        return hipErrorInvalidValue;
    for (int b = 0; b < n_bands; ++b)
        if (bands.lo[b] < 0 || bands.hi[b] > n_samples / 2 + 1 || bands.lo[b] >= bands.hi[b]) return hipErrorInvalidValue;
    const size_t lds = (size_t)(4 * n_samples + n_samples / 2 + 8) * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(whiten_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned grid = (unsigned)(items < kWhitenMaxGrid ? items : kWhitenMaxGrid);
    hipLaunchKernelGGL(whiten_kernel, dim3(grid), dim3(fft_lanes(n_samples)), lds, stream, d_signals, d_window, bands, n_bands, floor_rel, floor_abs, n_samples, log2n, d_out,
                       items);
    return hipGetLastError();
}

}  // namespace bf
