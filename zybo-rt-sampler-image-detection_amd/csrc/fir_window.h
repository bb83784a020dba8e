// fir_window.h -- the one tap step of the sliding-window FIR loops of band_filter.hip (KB bands share the window) and filter_sum.hip
// (KB = 1).
//
// A lane owns four consecutive outputs j0 .. j0+3 of a row staged in LDS and holds an eight-float register window of it: four taps
// t0 .. t0+3 need x~[j0 - t0 - 3 .. j0 - t0 + 3].  The taps are wave-uniform: scalar loads of hk[k][t0 .. t0+3].
// The order of the fmaf chain is the contract (both kernels are pinned to their NumPy models by equality): the four taps of a step
// are applied in order, and a tap past T - 1 is skipped (never multiplied by zero: fmaf(0, x, -0) is +0).
// The loop round this step -- one ds_read_b128 per step, `#pragma unroll 2`, the rem tail -- is written out in both kernels: stated
// as one function it compiled to other code in each of them, and measured outside the parent's band in some shapes (band filter, 4
// bands: up to 1.4 % slower; filter-and-sum, 190 frames, 129 taps, one beam: 10 % slower).
#pragma once

#include <hip/hip_runtime.h>

namespace bf {

template <int KB>
__device__ __forceinline__ void fir_taps4(float (&acc)[KB][4], const float (&w)[8], const float* const (&hk)[KB], int t0, int n_u)
{
    // w[4 + d] = x~[j0 - t0 + d]; output o at tap t0 + u reads x~[j0 + o - t0 - u]
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < n_u) {   // (wave-uniform; n_u = 4 in the main loop)
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const float h = hk[k][t0 + u];
#pragma unroll
                for (int o = 0; o < 4; ++o) acc[k][o] = __fmaf_rn(h, w[4 + o - u], acc[k][o]);
            }
        }
    }
}

}  // namespace bf
