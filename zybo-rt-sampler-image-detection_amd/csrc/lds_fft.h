// lds_fft.h -- the one radix-2 transform of the stream stages (whiten.hip, enhance.hip, spectrogram.hip): a workgroup transforms n complex
// points, n a power of two, in place in LDS.
//
// Layout, the caller's: re[n], im[n], and the twiddles twc[n / 2], tws[n / 2] = cos and -sin of 2 pi m / n, which a workgroup fills
// once before it walks its items.  The input is staged at the bit-reversed index (fft_rev), so the decimation-in-time butterflies of
// fft_passes run in place: log2 n passes of n / 2 butterflies, lane-strided, with a barrier behind each pass.  The inverse is the same
// passes with the conjugate twiddle (sign = -1), unnormalised; a real output comes from the full-length transform of the Hermitian
// extension (fft_stage_hermitian): twice the arithmetic a real-output transform of half length would need, for one pass routine and
// one rounding model.
//
// Rounding model (the error budgets of tests/whiten_np.py, tests/enhance_np.py and tests/spectrogram_np.py rest on it): a butterfly is
// the four multiplies and six adds of the textbook, each rounded on its own (the build has -ffp-contract=off), in the operand order
// written below; sign * tws is exact.  The twiddles come in two precisions, which give different bits and stay apart:
//   fft_twiddles      sincospi in double, rounded once to float32: each component within half a float32 step of the true value
//                     (whiten, enhance)
//   fft_twiddles_f32  sincospif (spectrogram)
// Every value is computed by one fixed sequence of float32 operations: the lane count (fft_lanes) depends on n alone, and which lane
// takes which butterfly cannot show in the result.
//
// Bank conflicts: passes with a half-length under 64 read LDS at a stride of 2 * half floats within a wave (2-way to 32-way conflicts
// on the first five passes), and the bit-reversed staging writes scatter the same way.  They are not padded away: a padded index is
// other address arithmetic in every butterfly of every pass, and each of these calls is a small fraction of the launch it feeds
// (profiles/whiten_time.json, profiles/spectrogram_time.json, profiles/enhance_time.json).
#pragma once

#include <hip/hip_runtime.h>

namespace bf {

// The exponent of a transform length, -1 where n is no power of two.
inline int fft_log2(int n)
{
    if (n < 1 || (n & (n - 1)) != 0) return -1;
    int log2n = 0;
    while ((1 << log2n) < n) ++log2n;
    return log2n;
}

// Lanes of the workgroup that transforms n points: one wave up to n = 512, four waves above.
inline unsigned fft_lanes(int n) { return n <= 512 ? 64 : 256; }

__device__ __forceinline__ int fft_rev(int t, int log2n) { return (int)(__brev((unsigned)t) >> (32 - log2n)); }

__device__ __forceinline__ void fft_twiddles(float* twc, float* tws, int n, int half_n, int lane, int lanes)
{
    for (int m = lane; m < half_n; m += lanes) {
        double s, c;
        sincospi((double)m * (2.0 / (double)n), &s, &c);         // (the argument is exact: m / 2^k)
        twc[m] = (float)c;
        tws[m] = (float)-s;
    }
}

__device__ __forceinline__ void fft_twiddles_f32(float* twc, float* tws, int n, int half_n, int lane, int lanes)
{
    for (int m = lane; m < half_n; m += lanes) {
        float s, c;
        sincospif((float)m * (2.0f / (float)n), &s, &c);         // (the argument is exact: m / 2^k)
        twc[m] = c;
        tws[m] = -s;
    }
}

// One in-place transform over re / im (staged at the bit-reversed index), a barrier behind every pass.
// sign = +1: exp(-2 pi i ..) (forward); -1: the conjugate twiddles (inverse, unnormalised).
__device__ __forceinline__ void fft_passes(float* re, float* im, const float* twc, const float* tws, int log2n, int half_n, int lane, int lanes, float sign)
{
    for (int p = 0; p < log2n; ++p) {
        const int half = 1 << p, tw_shift = log2n - 1 - p;
        for (int i = lane; i < half_n; i += lanes) {
            const int pos = i & (half - 1);
            const int a = ((i >> p) << (p + 1)) + pos, b = a + half;
            const float wr = twc[pos << tw_shift], wi = sign * tws[pos << tw_shift];
            const float br = re[b], bi = im[b], ar = re[a], ai = im[a];
            const float tr = wr * br - wi * bi;
            const float ti = wr * bi + wi * br;
            re[a] = ar + tr;
            im[a] = ai + ti;
            re[b] = ar - tr;
            im[b] = ai - ti;
        }
        __syncthreads();                        // the next pass (or the reader behind the last one) sees this pass's butterflies
    }
}

// Bin k <= n / 2 of a real signal's spectrum, staged for the inverse passes with its mirror: Y_k = (yr, yi), Y_{n-k} = conj Y_k.
__device__ __forceinline__ void fft_stage_hermitian(float* re, float* im, int k, float yr, float yi, int n, int half_n, int log2n)
{
    if (k == 0 || k == half_n) yi = 0.0f;       // only Re Y_0 and Re Y_{n/2} enter a real signal
    const int rev = fft_rev(k, log2n);
    re[rev] = yr;
    im[rev] = yi;
    if (k != 0 && k != half_n) {
        const int rev2 = fft_rev(n - k, log2n);
        re[rev2] = yr;
        im[rev2] = -yi;
    }
}

}  // namespace bf
