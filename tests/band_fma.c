/* The one operation tests/band_np.py cannot write in NumPy: acc[i] = fmaf(h, x[i], acc[i]), a fused multiply-add with ONE float32
 * rounding (C99 7.12.13.1), over an array of outputs.  Compiled by band_np.py with the host compiler, -ffp-contract=off. */
#include <math.h>

void band_fma_step(float h, const float *x, float *acc, long n)
{
    for (long i = 0; i < n; ++i) acc[i] = fmaf(h, x[i], acc[i]);
}
