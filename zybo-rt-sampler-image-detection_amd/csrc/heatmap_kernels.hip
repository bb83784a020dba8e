// heatmap_kernels.hip -- power map -> colour heat-map -> upscaled, temporally blended overlay, all on the device.
//
// Reference (display side of the hot path): PC/src/visual.py
//   calculate_heatmap            :143-188  clip 1e-12, log10, subtract log10(min), divide by max, keep levels >= amount,
//                                          ((l - amount) / amount) ** exponent, int(255 * .) -> reversed-jet LUT,
//                                          written at [MAX_RES_Y-1-y, MAX_RES_X-1-x] (the flip), should_overlay = max > threshold
//   cv2.resize(..., INTER_LINEAR)  :186    uint8 bilinear upscale to the display size
//   cv2.addWeighted(prev,.5,new,.5):450    temporal blend, then addWeighted(frame, .9, res, .9) onto the camera frame :452
//   find_power_center            :295-322  5x5 Gaussian (sigma 1), >= 95 % mask, cube-weighted centroid
// cv2 is not available where this was built (and its version is not pinned by the reference), so resize / blend /
// blur follow OpenCV's documented uint8 algorithms (11-bit fixed-point bilinear weights, half-pixel centres,
// saturate_cast<uchar>(lrint(.)), BORDER_REFLECT_101): parity for those three is "unpinned" -- see DESIGN.md.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdint.h>
#include "das_kernels.h"

namespace bf {

namespace {

struct Rgb { unsigned char r, g, b; };
__constant__ Rgb kJet[256] = {
#include "jet_lut.inc"
};

__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = is_max ? fmaxf(v, o) : fminf(v, o);
    }
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < nw; ++w) r = is_max ? fmaxf(r, red[w]) : fminf(r, red[w]);
    return r;
}

// One workgroup per frame: statistics of the map, then the small colour image [res_y][res_x][3] (flipped, as the
// reference indexes it) and the should_overlay flag.
__global__ void __launch_bounds__(1024) colorize_kernel(const float* __restrict__ power, int res_x, int res_y, float threshold,
                                                       float amount, float exponent, unsigned char* __restrict__ small,
                                                       int* __restrict__ should_overlay)
{
    __shared__ float red[16];                 // (one slot per wave: up to 1024 threads)
    const int D = res_x * res_y;
    const float* img = power + (size_t)blockIdx.x * D;
    unsigned char* out = small + (size_t)blockIdx.x * D * 3;
    float vmax = -INFINITY, smin = INFINITY;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        const float v = img[i];
        vmax = fmaxf(vmax, v);
        // fmaxf / fminf drop a NaN where np.max keeps it: a NaN rides through the min reduction as -inf (the clipped values are >= 1e-12)
        smin = v != v ? -INFINITY : fminf(smin, fmaxf(v, 1e-12f));
    }
    vmax = block_reduce(vmax, red, true);
    smin = block_reduce(smin, red, false);
    // np.max of a map with a NaN is NaN and `NaN > threshold` is false: blank image, flag 0 (visual.py:156-162)
    const bool overlay = smin != -INFINITY && vmax > threshold;
    const float lmin = log10f(smin);
    // max over the image of log10(clip(v)) - log10(min): log10 is monotonic, so it is log10(clip(max)) - lmin
    const float lmax = log10f(fmaxf(vmax, 1e-12f)) - lmin;
    if (threadIdx.x == 0) should_overlay[blockIdx.x] = overlay ? 1 : 0;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        const int x = i / res_y, y = i - x * res_y;          // image[x, y], flat x*res_y + y
        Rgb c{0, 0, 0};
        if (overlay) {
            float l = (log10f(fmaxf(img[i], 1e-12f)) - lmin) / lmax;
            if (l >= amount) {
                l = (l - amount) / amount;
                int cv = (int)(255.0f * powf(l, exponent));
                cv = cv < 0 ? 0 : cv > 255 ? 255 : cv;
                c = kJet[cv];
            }
        }
        unsigned char* p = out + ((size_t)(res_y - 1 - y) * res_x + (res_x - 1 - x)) * 3;
        p[0] = c.r; p[1] = c.g; p[2] = c.b;
    }
}

__device__ __forceinline__ unsigned char sat_u8(float v)
{
    const float r = rintf(v);   // cv::saturate_cast<uchar>(double) rounds to nearest even
    return (unsigned char)(r < 0.f ? 0.f : r > 255.f ? 255.f : r);
}

// One thread per output pixel (all 3 channels); the frames of the batch are walked in order because the temporal
// blend is a recurrence: res_f = sat(0.5 prev + 0.5 new_f), prev = res_f.
__global__ void __launch_bounds__(256) overlay_kernel(const unsigned char* __restrict__ small, int frames, int sw, int sh, int ow, int oh,
                                                      unsigned char* __restrict__ prev, const unsigned char* __restrict__ camera,
                                                      unsigned char* __restrict__ out, float w_prev, float w_new, float w_cam, float w_heat)
{
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= ow * oh) return;
    const int oy = px / ow, ox = px - oy * ow;
    // cv2.resize INTER_LINEAR, 8-bit: fx = (ox + 0.5) * sw/ow - 0.5, clamp, weights in 11-bit fixed point
    auto coord = [](int o, int ssz, int dsz, int& i0, int& i1, int& w0, int& w1) {
        float f = (float)((o + 0.5) * ((double)ssz / dsz) - 0.5);
        int i = (int)floorf(f);
        f -= i;
        if (i < 0) { i = 0; f = 0.f; }
        if (i >= ssz - 1) { i = ssz - 1; f = 0.f; i1 = i; } else i1 = i + 1;
        i0 = i;
        w0 = (int)rintf((1.0f - f) * 2048.0f);   // each weight is rounded on its own (saturate_cast<short>)
        w1 = (int)rintf(f * 2048.0f);
    };
    int x0, x1, wx0, wx1, y0, y1, wy0, wy1;
    coord(ox, sw, ow, x0, x1, wx0, wx1);
    coord(oy, sh, oh, y0, y1, wy0, wy1);
    float pv[3];
    const size_t o3 = (size_t)px * 3;
    for (int ch = 0; ch < 3; ++ch) pv[ch] = prev[o3 + ch];
    for (int f = 0; f < frames; ++f) {
        const unsigned char* s = small + (size_t)f * sw * sh * 3;
        for (int ch = 0; ch < 3; ++ch) {
            const int a = s[((size_t)y0 * sw + x0) * 3 + ch], b = s[((size_t)y0 * sw + x1) * 3 + ch];
            const int c = s[((size_t)y1 * sw + x0) * 3 + ch], d = s[((size_t)y1 * sw + x1) * 3 + ch];
            const int up = (((wy0 * ((a * wx0 + b * wx1) >> 4)) >> 16) + ((wy1 * ((c * wx0 + d * wx1) >> 4)) >> 16) + 2) >> 2;   // OpenCV's VResizeLinear<uchar>
            const unsigned char res = sat_u8(w_prev * pv[ch] + w_new * (float)up);
            pv[ch] = res;
            const size_t oi = ((size_t)f * ow * oh + px) * 3 + ch;
            out[oi] = camera ? sat_u8(w_cam * (float)camera[oi] + w_heat * (float)res) : res;
        }
    }
    for (int ch = 0; ch < 3; ++ch) prev[o3 + ch] = (unsigned char)pv[ch];
}

// The same recurrence as a tiled kernel: a workgroup owns a 128 x 8 tile of the output (256 threads x 4 pixels of a row) and first copies the few source
// pixels the tile's bilinear taps touch -- for EVERY frame of the chunk -- into LDS as one dword per pixel (101 -> 640 upscaling: 23 x 4 source pixels per
// frame, 23 KB for 64 frames).  The frame loop then reads its taps from LDS (16 ds_read_b32 instead of 48 global byte loads per thread and frame), moves
// camera / output / prev as three dwords per thread instead of nine single bytes, and has the camera words of the next kOvAhead frames in flight while it
// blends (the loop is a recurrence per pixel, so without that every frame waits for an HBM round trip).  The one-pixel kernel above took 0.19 ms for 64
// frames of 640 x 640; the bytes alone are 0.03.  Needs out_w % 4 == 0 and 4-byte aligned buffers (launch_overlay checks and falls back to the kernel above);
// identical arithmetic, identical results.
constexpr int kOvTW = 128, kOvTH = 8, kOvAhead = 8, kOvLdsBytes = 48 * 1024;

__global__ void __launch_bounds__(256) overlay_tile_kernel(const unsigned char* __restrict__ small, int frames, int sw, int sh, int ow, int oh,
                                                           unsigned char* __restrict__ prev, const unsigned char* __restrict__ camera,
                                                           unsigned char* __restrict__ out, float w_prev, float w_new, float w_cam, float w_heat,
                                                           int bx, int by, int chunk)
{
    extern __shared__ unsigned ov_lds[];                          // [chunk][by][bx] source pixels, r | g << 8 | b << 16
    auto coord = [](int o, int ssz, int dsz, int& i0, int& i1, int& w0, int& w1) {
        float f = (float)((o + 0.5) * ((double)ssz / dsz) - 0.5);
        int i = (int)floorf(f);
        f -= i;
        if (i < 0) { i = 0; f = 0.f; }
        if (i >= ssz - 1) { i = ssz - 1; f = 0.f; i1 = i; } else i1 = i + 1;
        i0 = i;
        w0 = (int)rintf((1.0f - f) * 2048.0f);
        w1 = (int)rintf(f * 2048.0f);
    };
    const int tx0 = blockIdx.x * kOvTW, ty0 = blockIdx.y * kOvTH;
    int sx_lo, sy_lo, t0, t1, t2;
    coord(tx0, sw, ow, sx_lo, t0, t1, t2);                        // the tile's first tap column / row (coord is monotonic in o)
    coord(ty0, sh, oh, sy_lo, t0, t1, t2);
    const int ox = tx0 + (threadIdx.x & 31) * 4, oy = ty0 + (threadIdx.x >> 5);
    const bool live = ox < ow && oy < oh;                         // ow % 4 == 0: a group of four is inside or outside as a whole
    int x0[4], x1[4], wx0[4], wx1[4], y0 = 0, y1 = 0, wy0 = 0, wy1 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) coord(min(ox + i, ow - 1), sw, ow, x0[i], x1[i], wx0[i], wx1[i]);
    coord(min(oy, oh - 1), sh, oh, y0, y1, wy0, wy1);
    const int P = bx * by;
    int ta[4], tb[4];                                             // LDS word of the (y0, x0) / (y0, x1) tap; the y1 row is dy words further
#pragma unroll
    for (int i = 0; i < 4; ++i) { ta[i] = (y0 - sy_lo) * bx + (x0[i] - sx_lo); tb[i] = (y0 - sy_lo) * bx + (x1[i] - sx_lo); }
    const int dy = (y1 - y0) * bx;
    const size_t o3 = ((size_t)oy * ow + ox) * 3, fstride = (size_t)ow * oh * 3;
    union B12 { unsigned u[3]; unsigned char b[12]; };
    float pv[12];
    if (live) {
        B12 pw;
#pragma unroll
        for (int k = 0; k < 3; ++k) pw.u[k] = reinterpret_cast<const unsigned*>(prev + o3)[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) pv[k] = pw.b[k];
    }
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    u16x2 wxp[4];                                                 // (wx0, wx1) as the second operand of v_dot2_u32_u16
#pragma unroll
    for (int i = 0; i < 4; ++i) wxp[i] = u16x2{(unsigned short)wx0[i], (unsigned short)wx1[i]};
    // sat_u8 without leaving float: rint, clamp (the operands are finite), and the byte is packed by v_cvt_pk_u8_f32 from an exact integer
    auto blend = [](float wa, float a, float wb, float b) { return __builtin_amdgcn_fmed3f(rintf(wa * a + wb * b), 0.f, 255.f); };
    for (int f0 = 0; f0 < frames; f0 += chunk) {
        const int nf = min(chunk, frames - f0);
        __syncthreads();                                          // the previous chunk's taps have been read
        for (int r = threadIdx.x; r < P; r += 256) {
            const int sy = r / bx, sx = r - sy * bx;
            const unsigned char* g = small + ((size_t)f0 * sh * sw + (size_t)min(sy_lo + sy, sh - 1) * sw + min(sx_lo + sx, sw - 1)) * 3;
#pragma unroll 8
            for (int f = 0; f < nf; ++f, g += (size_t)sh * sw * 3) ov_lds[f * P + r] = (unsigned)g[0] | ((unsigned)g[1] << 8) | ((unsigned)g[2] << 16);
        }
        __syncthreads();
        if (!live) continue;
        const unsigned char* cam_p = camera ? camera + (size_t)f0 * fstride + o3 : nullptr;
        unsigned char* out_p = out + (size_t)f0 * fstride + o3;
        for (int g0 = 0; g0 < nf; g0 += kOvAhead) {
            unsigned cam[kOvAhead][3];
            if (camera) {
#pragma unroll
                for (int u = 0; u < kOvAhead; ++u, cam_p += fstride)
                    if (g0 + u < nf) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) cam[u][k] = reinterpret_cast<const unsigned*>(cam_p)[k];
                    }
            }
#pragma unroll
            for (int u = 0; u < kOvAhead; ++u, out_p += fstride) {
                if (g0 + u >= nf) break;
                const unsigned* s = ov_lds + (g0 + u) * P;
                unsigned res[3] = {0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned a4 = s[ta[i]], b4 = s[tb[i]], c4 = s[ta[i] + dy], d4 = s[tb[i] + dy];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int e = 3 * i + ch;
                        const unsigned sel = 0x0c000c00u | ((4u + ch) << 16) | (unsigned)ch;          // (a | b << 16) of channel ch
                        const unsigned h0 = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, __builtin_amdgcn_perm(b4, a4, sel)), wxp[i], 0u, false);
                        const unsigned h1 = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, __builtin_amdgcn_perm(d4, c4, sel)), wxp[i], 0u, false);
                        const unsigned up = ((__umul24(wy0, h0 >> 4) >> 16) + (__umul24(wy1, h1 >> 4) >> 16) + 2u) >> 2;
                        const float r = blend(w_prev, pv[e], w_new, (float)up);
                        pv[e] = r;
                        const float o = camera ? blend(w_cam, (float)((cam[u][e >> 2] >> (8 * (e & 3))) & 255u), w_heat, r) : r;
                        res[e >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(o, e & 3, res[e >> 2]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned*>(out_p)[k] = res[k];
            }
        }
    }
    if (live) {
        B12 pw;
#pragma unroll
        for (int k = 0; k < 12; ++k) pw.b[k] = (unsigned char)pv[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned*>(prev + o3)[k] = pw.u[k];
    }
}

// The detector's letterbox (what ultralytics' predict does to a frame before the network, yolo_smooth_tracking.py:13-23): the frame resized with
// cv2.resize(INTER_LINEAR) to new_w x new_h -- the same 8-bit fixed-point bilinear as above -- centred in an out_w x out_h canvas of the border value.
// One thread per output pixel, 3 channels.
__global__ void __launch_bounds__(256) letterbox_kernel(const unsigned char* __restrict__ src, int sh, int sw, unsigned char* __restrict__ out, int oh, int ow, int new_h,
                                                        int new_w, int top, int left, int value)
{
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= ow * oh) return;
    const int oy = px / ow, ox = px - oy * ow;
    unsigned char* o = out + (size_t)px * 3;
    const int y = oy - top, x = ox - left;
    if (y < 0 || y >= new_h || x < 0 || x >= new_w) { o[0] = o[1] = o[2] = (unsigned char)value; return; }
    if (new_h == sh && new_w == sw) {                          // (no resampling: cv2.resize is skipped for equal shapes)
        const unsigned char* s = src + ((size_t)y * sw + x) * 3;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        return;
    }
    auto coord = [](int d, int ssz, int dsz, int& i0, int& i1, int& w0, int& w1) {
        float f = (float)((d + 0.5) * ((double)ssz / dsz) - 0.5);
        int i = (int)floorf(f);
        f -= i;
        if (i < 0) { i = 0; f = 0.f; }
        if (i >= ssz - 1) { i = ssz - 1; f = 0.f; i1 = i; } else i1 = i + 1;
        i0 = i;
        w0 = (int)rintf((1.0f - f) * 2048.0f);
        w1 = (int)rintf(f * 2048.0f);
    };
    int x0, x1, wx0, wx1, y0, y1, wy0, wy1;
    coord(x, sw, new_w, x0, x1, wx0, wx1);
    coord(y, sh, new_h, y0, y1, wy0, wy1);
    for (int ch = 0; ch < 3; ++ch) {
        const int a = src[((size_t)y0 * sw + x0) * 3 + ch], b = src[((size_t)y0 * sw + x1) * 3 + ch];
        const int c = src[((size_t)y1 * sw + x0) * 3 + ch], d = src[((size_t)y1 * sw + x1) * 3 + ch];
        o[ch] = (unsigned char)((((wy0 * ((a * wx0 + b * wx1) >> 4)) >> 16) + ((wy1 * ((c * wx0 + d * wx1) >> 4)) >> 16) + 2) >> 2);
    }
}

// find_power_center: one workgroup per frame.  image[x][y] float32 (rows = x).  Returns (center_x, center_y) in the
// reference's naming: centroid over columns then rows of the smoothed map.
__global__ void __launch_bounds__(256) power_center_kernel(const float* __restrict__ power, int rows, int cols, float* __restrict__ centers,
                                                           float* __restrict__ smooth_ws)
{
    __shared__ float red[8];
    const int D = rows * cols;
    const float* img = power + (size_t)blockIdx.x * D;
    float* sm = smooth_ws + (size_t)blockIdx.x * D;
    // cv2.getGaussianKernel(5, 1.0): exp(-(i-2)^2/2) normalised
    const float g0 = 0.05448868f, g1 = 0.24420134f, g2 = 0.40261996f;
    const float gk[5] = {g0, g1, g2, g1, g0};
    auto refl = [](int i, int n) { if (n == 1) return 0; while (i < 0 || i >= n) { i = i < 0 ? -i : 2 * (n - 1) - i; } return i; };   // BORDER_REFLECT_101
    float vmax = -INFINITY;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        const int r = i / cols, c = i - r * cols;
        float acc = 0.f;
        for (int dr = -2; dr <= 2; ++dr) {
            float rowacc = 0.f;
            const int rr = refl(r + dr, rows);
            for (int dc = -2; dc <= 2; ++dc) rowacc += gk[dc + 2] * fmaxf(img[rr * cols + refl(c + dc, cols)], 1e-12f);
            acc += gk[dr + 2] * rowacc;
        }
        sm[i] = acc;
        vmax = fmaxf(vmax, acc);
    }
    vmax = block_reduce(vmax, red, true);
    const float thr = vmax * 0.95f;
    // weighted centroid in float64 like NumPy's float32*bool -> float32 weights, int64 indices * float32 -> float64 sums
    double sw = 0.0, sx = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        const float v = sm[i];
        if (v >= thr) {
            const float w = v * v * v;
            const int r = i / cols, c = i - r * cols;
            sw += (double)w; sx += (double)c * (double)w; sy += (double)r * (double)w;
        }
    }
    __shared__ double dred[3][4];
    for (int off = 32; off > 0; off >>= 1) { sw += __shfl_xor(sw, off, 64); sx += __shfl_xor(sx, off, 64); sy += __shfl_xor(sy, off, 64); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { dred[0][threadIdx.x >> 6] = sw; dred[1][threadIdx.x >> 6] = sx; dred[2][threadIdx.x >> 6] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, b = 0, c = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { a += dred[0][w]; b += dred[1][w]; c += dred[2][w]; }
        centers[blockIdx.x * 2 + 0] = (float)(b / a);
        centers[blockIdx.x * 2 + 1] = (float)(c / a);
    }
}

}  // namespace

hipError_t launch_colorize(const float* d_power, int frames, int res_x, int res_y, float threshold, float amount, float exponent,
                           unsigned char* d_small, int* d_overlay, hipStream_t stream)
{
    // one workgroup per frame (two reductions over the map, then the mapping): 1024 threads -- a batch of 64 frames occupies 64 CUs either way, and the
    // log10 / pow per pixel is what a frame's workgroup spends its time on (51 -> 26 us per 64 frames of 101 x 101)
    const int threads = (long long)res_x * res_y >= 4096 ? 1024 : 256;
    hipLaunchKernelGGL(colorize_kernel, dim3(frames), dim3(threads), 0, stream, d_power, res_x, res_y, threshold, amount, exponent, d_small, d_overlay);
    return hipGetLastError();
}

hipError_t launch_overlay(const unsigned char* d_small, int frames, int small_w, int small_h, int out_w, int out_h, unsigned char* d_prev,
                          const unsigned char* d_camera, unsigned char* d_out, float w_prev, float w_new, float w_cam, float w_heat,
                          hipStream_t stream)
{
    const int px = out_w * out_h;
    // source pixels under one tile: a tile spans at most ceil(tile * scale) source steps, plus the tap to the right / below and one for the rounding of the first
    const int bx = (int)std::ceil((double)kOvTW * small_w / out_w) + 2, by = (int)std::ceil((double)kOvTH * small_h / out_h) + 2;
    const int chunk = std::min(frames, kOvLdsBytes / (bx * by * 4));
    const bool tiled = (out_w & 3) == 0 && chunk >= std::min(frames, 8) &&
                       ((reinterpret_cast<uintptr_t>(d_prev) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_camera)) & 3) == 0;
    if (tiled)
        hipLaunchKernelGGL(overlay_tile_kernel, dim3((out_w + kOvTW - 1) / kOvTW, (out_h + kOvTH - 1) / kOvTH), dim3(256), (size_t)chunk * bx * by * 4, stream, d_small,
                           frames, small_w, small_h, out_w, out_h, d_prev, d_camera, d_out, w_prev, w_new, w_cam, w_heat, bx, by, chunk);
    else
        hipLaunchKernelGGL(overlay_kernel, dim3((px + 255) / 256), dim3(256), 0, stream, d_small, frames, small_w, small_h, out_w, out_h, d_prev,
                           d_camera, d_out, w_prev, w_new, w_cam, w_heat);
    return hipGetLastError();
}

hipError_t launch_letterbox(const unsigned char* d_src, int sh, int sw, unsigned char* d_out, int oh, int ow, int new_h, int new_w, int top, int left, int value,
                            hipStream_t stream)
{
    if (sh < 1 || sw < 1 || oh < 1 || ow < 1 || new_h < 1 || new_w < 1 || top < 0 || left < 0 || top + new_h > oh || left + new_w > ow) return hipErrorInvalidValue;
    hipLaunchKernelGGL(letterbox_kernel, dim3((unsigned)((oh * ow + 255) / 256)), dim3(256), 0, stream, d_src, sh, sw, d_out, oh, ow, new_h, new_w, top, left, value);
    return hipGetLastError();
}

hipError_t launch_power_center(const float* d_power, int frames, int rows, int cols, float* d_centers, float* d_workspace, hipStream_t stream)
{
    hipLaunchKernelGGL(power_center_kernel, dim3(frames), dim3(256), 0, stream, d_power, rows, cols, d_centers, d_workspace);
    return hipGetLastError();
}

namespace {

// np.argmax order on (value, index) pairs: a NaN beats every number, a larger value beats a smaller one, and among equals (two
// NaNs included) the lower index wins.  (-inf, INT_MAX) loses to every real entry.
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi)
{
    const bool nan_v = v != v, nan_o = ov != ov;
    const bool take = nan_o ? (!nan_v || oi < i) : (!nan_v && (ov > v || (ov == v && oi < i)));
    if (take) { v = ov; i = oi; }
}

// One workgroup per frame: the loudest direction of the map -> its table offset (bf_peak_offsets_device).
__global__ void __launch_bounds__(256) peak_offsets_kernel(const float* __restrict__ power, int image_stride, int n_dirs, int offset_per_dir,
                                                           int* __restrict__ offsets)
{
    __shared__ float rv[4];
    __shared__ int ri[4];
    const float* img = power + (size_t)blockIdx.x * image_stride;
    float v = -INFINITY;
    int i = INT32_MAX;
    for (int j = threadIdx.x; j < n_dirs; j += blockDim.x) argmax_merge(v, i, img[j], j);
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        argmax_merge(v, i, ov, oi);
    }
    if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = v; ri[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) argmax_merge(v, i, rv[w], ri[w]);
        offsets[blockIdx.x] = i * offset_per_dir;
    }
}

}  // namespace

hipError_t launch_peak_offsets(const float* d_power, int frames, int image_stride, int n_dirs, int offset_per_dir, int* d_offsets, hipStream_t stream)
{
    hipLaunchKernelGGL(peak_offsets_kernel, dim3(frames), dim3(256), 0, stream, d_power, image_stride, n_dirs, offset_per_dir, d_offsets);
    return hipGetLastError();
}

// ---------------------------------------------------------------- bf_peaks_device: the K loudest separated sources of every map
//
// The order of include/beamformer_hip.h -- value descending, flat index ascending, non-finite entries below everything -- as ONE
// unsigned 64-bit key, so that "comes before" is `>` and the best of a window is an integer maximum (argmax_merge's ordering with the
// NaN rule turned round: here a NaN never wins).  High word: the float's bits mapped monotonically to unsigned (both zeros share a
// code; the smallest finite value maps to 0x00800000, so 0 is free for "non-finite"); low word: ~index.  Keys of different entries
// differ, key 0 is "nothing".  The maximum of a total order over a square window is the maximum over the rows of the per-row maxima:
// a row pass leaves each entry's best key over its horizontal window, a column pass over those gives the best over the square, and an
// entry is a candidate iff that is its own key -- 2 (2r + 1) reads per entry instead of (2r + 1)^2.
namespace {

typedef unsigned long long PeakKey;

__device__ __forceinline__ unsigned peak_code(float v)
{
    unsigned b = __float_as_uint(v);
    if ((b & 0x7f800000u) == 0x7f800000u) return 0u;        // NaN, +inf, -inf
    if (b == 0x80000000u) b = 0u;                           // -0.0f == 0.0f
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the value of a non-zero code (a -0.0f comes back as 0.0f, which compares the same)
__device__ __forceinline__ float peak_value(unsigned code) { return __uint_as_float((code & 0x80000000u) ? (code ^ 0x80000000u) : ~code); }
__device__ __forceinline__ PeakKey peak_key(unsigned code, int index) { return code ? ((PeakKey)code << 32) | (PeakKey)(0xffffffffu - (unsigned)index) : 0ull; }
__device__ __forceinline__ int peak_index(PeakKey key) { return (int)(0xffffffffu - (unsigned)key); }

// thr = fmaxf(floor_abs, floor_rel * top): one float32 multiplication (the build has -ffp-contract=off; there is nothing to fuse with anyway)
__device__ __forceinline__ float peak_threshold(PeakKey top, float floor_rel, float floor_abs)
{
    return top ? fmaxf(floor_abs, floor_rel * peak_value((unsigned)(top >> 32))) : floor_abs;
}

// Block-wide maximum / sum, the same value in every thread.  red: one slot per wave; safe to call back to back.
__device__ __forceinline__ PeakKey block_max_key(PeakKey v, PeakKey* red)
{
    for (int off = 32; off > 0; off >>= 1) {
        const PeakKey o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    PeakKey r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = red[w] > r ? red[w] : r;
    return r;
}

__device__ __forceinline__ int block_sum_int(int v, int* red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += red[w];
    return r;
}

__device__ __forceinline__ void peak_write(PeakKey key, size_t slot, const float* __restrict__ img, int offset_per_dir, int* __restrict__ offsets,
                                           float* __restrict__ values)
{
    const int d = peak_index(key);
    offsets[slot] = key ? d * offset_per_dir : -1;
    if (values) values[slot] = key ? img[d] : 0.0f;
}

// Maps that fit LDS: one workgroup per frame, the map is read from HBM once.  LDS: best[D] keys (row-pass results), code[D] (the
// entries' codes; after the column pass: the kept candidates' codes, 0 everywhere else).  The ordered top k is then k rounds of
// "largest key below the previous one" over code[] -- exact for any number of candidates (radius 0: every finite entry), no list,
// no atomics.  radius has been clamped to max(rows, cols) by the launcher.
__global__ void __launch_bounds__(1024) peaks_frame_kernel(const float* __restrict__ power, int image_stride, int rows, int cols, int radius, int k,
                                                          float floor_rel, float floor_abs, int offset_per_dir, int* __restrict__ offsets,
                                                          float* __restrict__ values, int* __restrict__ counts)
{
    extern __shared__ PeakKey pk_lds[];
    __shared__ PeakKey red[16];
    __shared__ int redi[16];
    const int D = rows * cols, tid = threadIdx.x, nt = blockDim.x;
    PeakKey* best = pk_lds;
    unsigned* code = reinterpret_cast<unsigned*>(pk_lds + D);
    const float* img = power + (size_t)blockIdx.x * image_stride;
    PeakKey top = 0;
    int bad = 0;
    for (int i = tid; i < D; i += nt) {
        const unsigned c = peak_code(img[i]);
        code[i] = c;
        bad += c == 0u;
        const PeakKey key = peak_key(c, i);
        top = key > top ? key : top;
    }
    top = block_max_key(top, red);          // (its barriers also publish code[])
    bad = block_sum_int(bad, redi);
    for (int i = tid; i < D; i += nt) {
        const int x = i / cols, y = i - x * cols;
        const int lo = y - min(radius, y), hi = y + min(radius, cols - 1 - y);
        const unsigned* row = code + x * cols;
        unsigned bc = 0u;
        int by = 0;
        for (int j = lo; j <= hi; ++j) {     // ascending index: only a larger code replaces the best so far
            const unsigned c = row[j];
            if (c > bc) { bc = c; by = j; }
        }
        best[i] = peak_key(bc, x * cols + by);
    }
    __syncthreads();
    const float thr = peak_threshold(top, floor_rel, floor_abs);
    int kept = 0;
    for (int i = tid; i < D; i += nt) {
        const unsigned c = code[i];
        if (c == 0u) continue;
        const int x = i / cols, y = i - x * cols;
        const int lo = x - min(radius, x), hi = x + min(radius, rows - 1 - x);
        PeakKey m = 0;
        for (int j = lo; j <= hi; ++j) {
            const PeakKey b = best[j * cols + y];
            m = b > m ? b : m;
        }
        const bool keep = m == peak_key(c, i) && peak_value(c) >= thr;
        if (!keep) code[i] = 0u;             // (only this thread reads code[i] in this pass)
        kept += keep;
    }
    kept = block_sum_int(kept, redi);       // (publishes the edited code[])
    PeakKey last = ~0ull;
    for (int s = 0; s < k; ++s) {
        PeakKey m = 0;
        if (s < kept) {                      // uniform
            for (int i = tid; i < D; i += nt) {
                const PeakKey key = peak_key(code[i], i);
                if (key < last && key > m) m = key;
            }
            m = block_max_key(m, red);
        }
        if (tid == 0) peak_write(m, (size_t)blockIdx.x * k + s, img, offset_per_dir, offsets, values);
        last = m;
    }
    if (tid == 0 && counts) {
        counts[(size_t)blockIdx.x * 3 + 0] = min(k, kept);
        counts[(size_t)blockIdx.x * 3 + 1] = kept;
        counts[(size_t)blockIdx.x * 3 + 2] = bad;
    }
}

// Larger maps, any radius: the same three steps as three launches over tiles of kPeakTile consecutive entries, the row-pass results
// in a library-owned buffer.  A tile's window reaches into its neighbours through that buffer (and through the map itself in the row
// pass), so no halo is staged and a radius as large as the grid needs nothing special.
//   1. peaks_row_kernel   : best[f][i] = best key of entry i's horizontal window; per tile: the best own key and the non-finite count
//   2. peaks_col_kernel   : frame top (from the tiles' partials) -> threshold; candidates by the column pass; per tile: the number of
//                           kept candidates and their ordered top k
//   3. peaks_merge_kernel : per frame: counts summed, the ordered top k of the tiles' lists
// Every partial is written by one workgroup and read by later launches: nothing depends on the order workgroups run in.
constexpr int kPeakTile = 1024;

__global__ void __launch_bounds__(kPeakTile) peaks_row_kernel(const float* __restrict__ power, int image_stride, int D, int cols, int radius, int tiles,
                                                             PeakKey* __restrict__ best, PeakKey* __restrict__ tile_top, int* __restrict__ tile_bad)
{
    __shared__ PeakKey red[16];
    __shared__ int redi[16];
    const int f = blockIdx.x / tiles, tile = blockIdx.x - f * tiles;
    const int i = tile * kPeakTile + threadIdx.x;
    const float* img = power + (size_t)f * image_stride;
    PeakKey own = 0;
    int bad = 0;
    if (i < D) {
        const int x = i / cols, y = i - x * cols;
        const int lo = y - min(radius, y), hi = y + min(radius, cols - 1 - y);
        const float* row = img + (size_t)x * cols;
        unsigned bc = 0u;
        int by = 0;
        for (int j = lo; j <= hi; ++j) {
            const unsigned c = peak_code(row[j]);
            if (c > bc) { bc = c; by = j; }
        }
        best[(size_t)f * D + i] = peak_key(bc, x * cols + by);
        own = peak_key(peak_code(img[i]), i);
        bad = own == 0ull;
    }
    own = block_max_key(own, red);
    bad = block_sum_int(bad, redi);
    if (threadIdx.x == 0) { tile_top[blockIdx.x] = own; tile_bad[blockIdx.x] = bad; }
}

__global__ void __launch_bounds__(kPeakTile) peaks_col_kernel(const float* __restrict__ power, int image_stride, int D, int rows, int cols, int radius, int k,
                                                             float floor_rel, float floor_abs, int tiles, const PeakKey* __restrict__ best,
                                                             const PeakKey* __restrict__ tile_top, PeakKey* __restrict__ tile_keys,
                                                             int* __restrict__ tile_kept)
{
    __shared__ PeakKey red[16];
    __shared__ int redi[16];
    const int f = blockIdx.x / tiles, tile = blockIdx.x - f * tiles;
    const int i = tile * kPeakTile + threadIdx.x;
    const float* img = power + (size_t)f * image_stride;
    PeakKey top = 0;
    for (int t = threadIdx.x; t < tiles; t += kPeakTile) {
        const PeakKey o = tile_top[(size_t)f * tiles + t];
        top = o > top ? o : top;
    }
    top = block_max_key(top, red);
    const float thr = peak_threshold(top, floor_rel, floor_abs);
    PeakKey own = 0;
    if (i < D) {
        const unsigned c = peak_code(img[i]);
        if (c) {
            const int x = i / cols, y = i - x * cols;
            const int lo = x - min(radius, x), hi = x + min(radius, rows - 1 - x);
            const PeakKey* col = best + (size_t)f * D + y;
            PeakKey m = 0;
            for (int j = lo; j <= hi; ++j) {
                const PeakKey b = col[(size_t)j * cols];
                m = b > m ? b : m;
            }
            if (m == peak_key(c, i) && peak_value(c) >= thr) own = m;
        }
    }
    const int kept = block_sum_int(own != 0ull, redi);
    PeakKey last = ~0ull;
    for (int s = 0; s < k; ++s) {
        PeakKey m = 0;
        if (s < kept) m = block_max_key(own < last ? own : 0ull, red);
        if (threadIdx.x == 0) tile_keys[(size_t)blockIdx.x * k + s] = m;
        last = m;
    }
    if (threadIdx.x == 0) tile_kept[blockIdx.x] = kept;
}

__global__ void __launch_bounds__(256) peaks_merge_kernel(const float* __restrict__ power, int image_stride, int k, int offset_per_dir, int tiles,
                                                         const PeakKey* __restrict__ tile_keys, const int* __restrict__ tile_kept,
                                                         const int* __restrict__ tile_bad, int* __restrict__ offsets, float* __restrict__ values,
                                                         int* __restrict__ counts)
{
    __shared__ PeakKey red[4];
    __shared__ int redi[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* img = power + (size_t)f * image_stride;
    int kept = 0, bad = 0;
    for (int t = tid; t < tiles; t += 256) { kept += tile_kept[(size_t)f * tiles + t]; bad += tile_bad[(size_t)f * tiles + t]; }
    kept = block_sum_int(kept, redi);
    bad = block_sum_int(bad, redi);
    const PeakKey* keys = tile_keys + (size_t)f * tiles * k;
    const long long n = (long long)tiles * k;
    PeakKey last = ~0ull;
    for (int s = 0; s < k; ++s) {
        PeakKey m = 0;
        if (s < kept) {
            for (long long j = tid; j < n; j += 256) {
                const PeakKey key = keys[j];
                if (key < last && key > m) m = key;
            }
            m = block_max_key(m, red);
        }
        if (tid == 0) peak_write(m, (size_t)f * k + s, img, offset_per_dir, offsets, values);
        last = m;
    }
    if (tid == 0 && counts) {
        counts[(size_t)f * 3 + 0] = min(k, kept);
        counts[(size_t)f * 3 + 1] = kept;
        counts[(size_t)f * 3 + 2] = bad;
    }
}

// LDS of the one-workgroup form: 12 bytes per entry, beside the 192 bytes of the reduction slots, within the CU's 160 KiB
constexpr long long kPeakLdsBudget = 160 * 1024 - 256;

inline bool peaks_fit_lds(long long D) { return D * 12 <= kPeakLdsBudget; }
inline long long peaks_tiles(long long D) { return (D + kPeakTile - 1) / kPeakTile; }

}  // namespace

// Workspace of the tiled form in 8-byte words (0: the map fits LDS, no workspace): best[frames][D], tile_top[frames][tiles],
// tile_keys[frames][tiles][k], then tile_kept and tile_bad as int [frames][tiles] each.
size_t peaks_workspace_words(int frames, int rows, int cols, int k)
{
    const long long D = (long long)rows * cols;
    if (peaks_fit_lds(D)) return 0;
    const long long tiles = peaks_tiles(D);
    return (size_t)frames * (size_t)(D + tiles + tiles * k + tiles);
}

hipError_t launch_peaks(const float* d_power, int frames, int image_stride, int rows, int cols, int radius, int k, float floor_rel, float floor_abs,
                        int offset_per_dir, int* d_offsets, float* d_values, int* d_counts, unsigned long long* d_workspace, size_t workspace_words,
                        hipStream_t stream)
{
    const long long D = (long long)rows * cols;
    radius = std::min(radius, std::max(rows, cols));       // a window past the grid's edge is the window to the edge; keeps y + radius an int
    if (peaks_fit_lds(D)) {
        const size_t lds = (size_t)D * 12;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(peaks_frame_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        // a frame's workgroup is alone on the critical path of its map: sixteen waves as soon as each has more than one entry to look at
        const int threads = D > 1024 ? 1024 : 256;
        hipLaunchKernelGGL(peaks_frame_kernel, dim3(frames), dim3(threads), lds, stream, d_power, image_stride, rows, cols, radius, k, floor_rel, floor_abs,
                           offset_per_dir, d_offsets, d_values, d_counts);
        return hipGetLastError();
    }
    const long long tiles = peaks_tiles(D);
    if (!d_workspace || workspace_words < peaks_workspace_words(frames, rows, cols, k) || frames * tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    PeakKey* best = d_workspace;
    PeakKey* tile_top = best + (size_t)frames * D;
    PeakKey* tile_keys = tile_top + (size_t)frames * tiles;
    int* tile_kept = reinterpret_cast<int*>(tile_keys + (size_t)frames * tiles * k);
    int* tile_bad = tile_kept + (size_t)frames * tiles;
    const dim3 grid((unsigned)(frames * tiles));
    hipLaunchKernelGGL(peaks_row_kernel, grid, dim3(kPeakTile), 0, stream, d_power, image_stride, (int)D, cols, radius, (int)tiles, best, tile_top, tile_bad);
    hipLaunchKernelGGL(peaks_col_kernel, grid, dim3(kPeakTile), 0, stream, d_power, image_stride, (int)D, rows, cols, radius, k, floor_rel, floor_abs, (int)tiles,
                       best, tile_top, tile_keys, tile_kept);
    hipLaunchKernelGGL(peaks_merge_kernel, dim3(frames), dim3(256), 0, stream, d_power, image_stride, k, offset_per_dir, (int)tiles, tile_keys, tile_kept, tile_bad,
                       d_offsets, d_values, d_counts);
    return hipGetLastError();
}

// ---------------------------------------------------------------- bf_track_sources_device: identity over time for bf_peaks_device's sources
//
// The frame loop is sequential by definition (a frame's association reads the state the previous frame left), so the launch is ONE
// wave: lane s owns slot s and keeps its track in registers from the first frame to the last; the state buffer is read once and
// written once.  Per frame: lanes j < k decode the detection row into LDS (512 bytes, read back by broadcast), the row of frame
// f + 1 is already in flight; the greedy association runs as wave-wide rounds -- every unassigned lane holds its best unassigned
// eligible detection, the 64-bit key (cost bits << 32) | (slot << 8) | column is reduced to its minimum across the wave (cost >= 0,
// so the bits order as the floats do, and the low bytes are the definition's tie rule), the winner is assigned and only lanes whose
// best detection was just taken look again; at most min(slots, k) rounds.  Births are serial over the few detections left, lowest
// free slot by ballot.  No atomics, no workspace.  The kernel is bound by latency, not by throughput.
namespace {

constexpr unsigned kTrackNone = 0xffffffffu;       // no eligible detection (a cost's bits are at most +inf's, 0x7f800000)

// lane's best (cost bits, column) among the detections of `avail`: ascending columns, only a smaller cost replaces the best so far
__device__ __forceinline__ void track_best(unsigned long long avail, const float* zx, const float* zy, float x, float y, float gate2, unsigned& bc, int& bj)
{
    bc = kTrackNone;
    bj = -1;
    for (; avail; avail &= avail - 1) {
        const int j = __ffsll((long long)avail) - 1;
        const float dx = zx[j] - x, dy = zy[j] - y;
        const float cost = dx * dx + dy * dy;
        if (cost <= gate2) {
            const unsigned cb = __float_as_uint(cost);
            if (cb < bc) { bc = cb; bj = j; }
        }
    }
}

// clamp((int)rintf(v), 0, n - 1), the clamp to the int range done in float: no conversion overflows, a NaN gives 0
__device__ __forceinline__ int track_pixel(float v, int n)
{
    const float r = rintf(v);
    if (!(r >= 0.0f)) return 0;
    return min((int)fminf(r, 2147483520.0f), n - 1);
}

__global__ void __launch_bounds__(64) track_sources_kernel(const int* __restrict__ offsets, int frames, int k, int rows, int cols, int offset_per_dir,
                                                         int slots, float gate2, int max_miss, int min_hits, float q, float r, int* __restrict__ state,
                                                         int* __restrict__ track_offsets, int* __restrict__ track_ids, float* __restrict__ track_pos,
                                                         int* __restrict__ match, int* __restrict__ counts)
{
    __shared__ float zx[64], zy[64];
    const int lane = threadIdx.x;
    const bool mine = lane < slots;
    const int D = rows * cols;
    int* const sw = state + 4 + 12 * lane;
    float* const sf = reinterpret_cast<float*>(sw);
    int next_id = state[0];
    int id = 0, hits = 0, misses = 0;
    float x = 0.0f, vx = 0.0f, y = 0.0f, vy = 0.0f, p00 = 0.0f, p01 = 0.0f, p11 = 0.0f;
    if (mine) {
        id = sw[0]; hits = sw[1]; misses = sw[2];
        x = sf[4]; vx = sf[5]; y = sf[6]; vy = sf[7]; p00 = sf[8]; p01 = sf[9]; p11 = sf[10];
    }
    int raw = lane < k ? offsets[lane] : -1;
    for (int f = 0; f < frames; ++f) {
        const int cur = raw;
        if (f + 1 < frames && lane < k) raw = offsets[(size_t)(f + 1) * k + lane];      // in flight while this frame is worked on
        bool det = false;
        if (cur >= 0) {                                  // (lanes >= k hold -1)
            const int d = cur / offset_per_dir;
            det = d * offset_per_dir == cur && d < D;
            if (det) {
                const int dx = d / cols;
                zx[lane] = (float)dx;
                zy[lane] = (float)(d - dx * cols);
            }
        }
        unsigned long long avail = __ballot(det);        // detections no slot has taken yet
        const int invalid = k - __popcll(avail);
        // 1. predict
        if (id != 0) {
            x = x + vx;
            y = y + vy;
            const float a = p00 + p01, b = p01 + p11;
            p00 = (a + b) + q;
            p01 = b;
            p11 = p11 + q;
        }
        __syncthreads();                                 // zx, zy visible
        // 2. associate
        int took = -1;
        bool want = id != 0;
        unsigned bc = kTrackNone;
        int bj = -1;
        if (want) track_best(avail, zx, zy, x, y, gate2, bc, bj);
        for (;;) {
            unsigned long long key = bj >= 0 ? ((unsigned long long)bc << 32) | (unsigned)(lane << 8) | (unsigned)bj : ~0ull;
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(key, off, 64);
                key = o < key ? o : key;
            }
            if (key == ~0ull) break;                     // uniform: every lane holds the minimum
            const int win = __builtin_amdgcn_readfirstlane((int)(unsigned)key);
            const int ws = (win >> 8) & 0xff, wj = win & 0xff;
            avail &= ~(1ull << wj);
            if (lane == ws) { took = wj; want = false; bj = -1; }
            const bool redo = want && bj == wj;
            if (__any(redo)) {
                if (redo) track_best(avail, zx, zy, x, y, gate2, bc, bj);
            }
        }
        // 3. update / 4. coast
        bool ends = false;
        if (took >= 0) {
            const float S = p00 + r;
            const float k0 = p00 / S, k1 = p01 / S;
            const float ex = zx[took] - x;
            x = x + k0 * ex;
            vx = vx + k1 * ex;
            const float ey = zy[took] - y;
            y = y + k0 * ey;
            vy = vy + k1 * ey;
            const float o00 = p00, o01 = p01;
            p00 = o00 - k0 * o00;
            p01 = o01 - k0 * o01;
            p11 = p11 - k1 * o01;
            hits += 1;
            misses = 0;
        } else if (id != 0) {
            misses += 1;
            ends = misses > max_miss;
            if (ends) id = 0;
        }
        const int ended = __popcll(__ballot(ends));
        // 5. birth: the detections left, in column order, each into the lowest free slot
        unsigned long long free_slots = __ballot(mine && id == 0);
        int born = 0, dropped = 0;
        for (; avail; avail &= avail - 1) {
            if (!free_slots) { dropped = __popcll(avail); break; }
            const int j = __ffsll((long long)avail) - 1;
            const int s = __ffsll((long long)free_slots) - 1;
            free_slots &= free_slots - 1;
            next_id += 1;
            born += 1;
            if (lane == s) {
                id = next_id; hits = 1; misses = 0; took = j;
                x = zx[j]; y = zy[j]; vx = 0.0f; vy = 0.0f;
                p00 = 1.0f; p01 = 0.0f; p11 = 1.0f;
            }
        }
        // 6. write
        if (mine) {
            const size_t o = (size_t)f * slots + lane;
            const bool live = id != 0;
            track_offsets[o] = live && hits >= min_hits ? (track_pixel(x, rows) * cols + track_pixel(y, cols)) * offset_per_dir : -1;
            if (track_ids) track_ids[o] = id;
            if (track_pos) {
                track_pos[o * 4 + 0] = live ? x : 0.0f;
                track_pos[o * 4 + 1] = live ? y : 0.0f;
                track_pos[o * 4 + 2] = live ? vx : 0.0f;
                track_pos[o * 4 + 3] = live ? vy : 0.0f;
            }
            if (match) match[o] = live ? took : -1;
        }
        if (counts && lane < 4) counts[(size_t)f * 4 + lane] = lane == 0 ? born : lane == 1 ? ended : lane == 2 ? dropped : invalid;
        __syncthreads();                                 // every read of zx, zy is done before the next row lands
    }
    if (lane == 0) { state[0] = next_id; state[1] = 0; state[2] = 0; state[3] = 0; }
    if (mine) {
        const bool live = id != 0;                       // a free slot is stored as zeros
        sw[0] = id; sw[1] = live ? hits : 0; sw[2] = live ? misses : 0; sw[3] = 0;
        sf[4] = live ? x : 0.0f; sf[5] = live ? vx : 0.0f; sf[6] = live ? y : 0.0f; sf[7] = live ? vy : 0.0f;
        sf[8] = live ? p00 : 0.0f; sf[9] = live ? p01 : 0.0f; sf[10] = live ? p11 : 0.0f; sw[11] = 0;
    }
}

}  // namespace

hipError_t launch_track_sources(const int* d_offsets, int frames, int k, int rows, int cols, int offset_per_dir, int slots, float gate2, int max_miss,
                                int min_hits, float q, float r, int* d_state, int* d_track_offsets, int* d_track_ids, float* d_track_pos, int* d_match,
                                int* d_counts, hipStream_t stream)
{
    if (k < 1 || k > 64 || slots < 1 || slots > 64) return hipErrorInvalidValue;   // one wave: a lane per slot and per column (das_kernels.h: kTrackMaxSlots)
    hipLaunchKernelGGL(track_sources_kernel, dim3(1), dim3(64), 0, stream, d_offsets, frames, k, rows, cols, offset_per_dir, slots, gate2, max_miss, min_hits,
                       q, r, d_state, d_track_offsets, d_track_ids, d_track_pos, d_match, d_counts);
    return hipGetLastError();
}

// ---------------------------------------------------------------- bf_fuse_boxes_device: detector boxes meet the acoustic map
//
// A box's footprint is the nearest-cell inverse of the display path (colourise's flip, then the half-pixel upscale of the overlay):
// integer arithmetic after four float32 roundings, see include/beamformer_hip.h.  Two kernels on the stream:
//   fuse_boxes_kernel   : one workgroup of four waves per (frame, kFuseBoxesPerGroup rows).  A wave takes rows in a strided loop, its
//                         lanes stride over the footprint's cells, and the first cell in bf_peaks_device's order is the maximum of
//                         peak_key over the wave.  Maps of at most kFuseStageMax directions are staged into LDS once per workgroup
//                         (a group without a box skips that), larger ones are read through L2: the same bits either way.
//   fuse_sources_kernel : one wave per frame, only when sources or counts are asked for.  Lane l of a 64-row chunk holds row l's
//                         rect, lane s holds source s; a ballot per source over the chunk gives the lowest row that contains it, and
//                         chunks go in ascending order.  counts[1] reads the peak offsets the first kernel wrote (stream order).
// Every output entry has one writer and every reduction is a maximum or a sum of integers: nothing depends on the split of rows
// over workgroups or on the order they run in.  No atomics, no workspace.
namespace {

constexpr int kFuseBoxesPerGroup = 32;

struct FuseGrid { int rows, cols, img_w, img_h; };

// (int)u for a float u in [0, (float)(n - 1)], clamped to n - 1: (float)(n - 1) rounds up above 2^24
__device__ __forceinline__ int fuse_pixel(float u, int n) { return min((int)fminf(u, 2147483520.0f), n - 1); }

// small-image index of display pixel u: ((2u + 1) * cells) / (2 * img), in [0, cells - 1] for u in [0, img - 1]
__device__ __forceinline__ int fuse_cell(int u, int cells, int img) { return (int)(((2ll * u + 1) * cells) / (2ll * img)); }

// the grid range [lo, hi] of the display pixels whose centres lie in [a, b]; false: none
__device__ __forceinline__ bool fuse_axis(float a, float b, int img, int cells, int& lo, int& hi)
{
    if (a != a || b != b) return false;
    float ua = ceilf(a - 0.5f), ub = floorf(b - 0.5f);
    ua = fmaxf(ua, 0.0f);
    ub = fminf(ub, (float)(img - 1));
    if (!(ua <= ub)) return false;
    lo = cells - 1 - fuse_cell(fuse_pixel(ub, img), cells, img);
    hi = cells - 1 - fuse_cell(fuse_pixel(ua, img), cells, img);
    return true;
}

// the grid index of the display pixel under the midpoint of [a, b]; -1: the midpoint is outside the frame (or NaN)
__device__ __forceinline__ int fuse_mid(float a, float b, int img, int cells)
{
    const float um = floorf((a + b) * 0.5f);
    if (!(um >= 0.0f && um <= (float)(img - 1))) return -1;
    return cells - 1 - fuse_cell(fuse_pixel(um, img), cells, img);
}

__device__ __forceinline__ bool fuse_is_box(const float* __restrict__ row, int b, int nb, float conf) { return b < nb && row[4] >= conf; }

__device__ __forceinline__ int fuse_box_count(const int* __restrict__ box_counts, int f, int max_boxes)
{
    return box_counts ? min(max(box_counts[f], 0), max_boxes) : max_boxes;
}

template <bool kStaged>
__global__ void __launch_bounds__(256) fuse_boxes_kernel(const float* __restrict__ power, int image_stride, FuseGrid g, int offset_per_dir,
                                                         const float* __restrict__ boxes, const int* __restrict__ box_counts, int max_boxes, int groups,
                                                         float conf, int* __restrict__ peak_offsets, float* __restrict__ peak_power,
                                                         int* __restrict__ center_offsets, int* __restrict__ rects)
{
    extern __shared__ float fuse_lds[];
    __shared__ int any_box;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x / groups, b0 = (blockIdx.x - f * groups) * kFuseBoxesPerGroup;
    const int b1 = min(b0 + kFuseBoxesPerGroup, max_boxes);
    const int nb = fuse_box_count(box_counts, f, max_boxes);
    const float* img = power + (size_t)f * image_stride;
    const float* frame_boxes = boxes + (size_t)f * max_boxes * 6;
    const float* cells = img;
    if (kStaged) {
        if (tid == 0) any_box = 0;
        __syncthreads();
        if (b0 + tid < b1 && fuse_is_box(frame_boxes + (size_t)(b0 + tid) * 6, b0 + tid, nb, conf)) any_box = 1;
        __syncthreads();
        if (any_box) {                           // uniform
            const int D = g.rows * g.cols;
            for (int i = tid; i < D; i += 256) fuse_lds[i] = img[i];
        }
        __syncthreads();
        cells = fuse_lds;
    }
    for (int b = b0 + wave; b < b1; b += 4) {    // everything but the cell loop is uniform over the wave
        const float* row = frame_boxes + (size_t)b * 6;
        const bool is_box = fuse_is_box(row, b, nb, conf);
        int xa = -1, xb = -1, ya = -1, yb = -1, center = -1;
        PeakKey key = 0;
        if (is_box) {
            const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
            const int cx = fuse_mid(x1, x2, g.img_w, g.rows), cy = fuse_mid(y1, y2, g.img_h, g.cols);
            if (cx >= 0 && cy >= 0) center = (cx * g.cols + cy) * offset_per_dir;
            const bool hx = fuse_axis(x1, x2, g.img_w, g.rows, xa, xb), hy = fuse_axis(y1, y2, g.img_h, g.cols, ya, yb);
            if (hx && hy) {
                // cell i of the footprint, row-major: (xa + i / w, ya + i % w); a lane steps by 64 cells without dividing again
                const int w = yb - ya + 1, n = (xb - xa + 1) * w;
                const int sx = 64 / w, sy = 64 - sx * w;
                int x = lane / w, y = lane - x * w;
                for (int i = lane; i < n; i += 64) {
                    const int d = (xa + x) * g.cols + ya + y;
                    const PeakKey k = peak_key(peak_code(cells[d]), d);
                    key = k > key ? k : key;
                    x += sx;
                    y += sy;
                    if (y >= w) { y -= w; x += 1; }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const PeakKey o = __shfl_xor(key, off, 64);
                    key = o > key ? o : key;
                }
            } else {
                xa = xb = ya = yb = -1;
            }
        }
        if (lane == 0) {
            const size_t slot = (size_t)f * max_boxes + b;
            peak_write(key, slot, img, offset_per_dir, peak_offsets, peak_power);
            if (center_offsets) center_offsets[slot] = center;
            if (rects) { rects[slot * 4 + 0] = xa; rects[slot * 4 + 1] = xb; rects[slot * 4 + 2] = ya; rects[slot * 4 + 3] = yb; }
        }
    }
}

__global__ void __launch_bounds__(64) fuse_sources_kernel(FuseGrid g, int offset_per_dir, const float* __restrict__ boxes, const int* __restrict__ box_counts,
                                                        int max_boxes, float conf, const int* __restrict__ src_offsets, int n_src,
                                                        const int* __restrict__ peak_offsets, int* __restrict__ src_box, int* __restrict__ counts)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int nb = fuse_box_count(box_counts, f, max_boxes);
    const float* frame_boxes = boxes + (size_t)f * max_boxes * 6;
    int sx = -1, sy = -1;                        // a lane without a source is inside no rect
    if (lane < n_src) {
        const int o = src_offsets[(size_t)f * n_src + lane];
        if (o >= 0) {
            const int d = o / offset_per_dir;
            if (d * offset_per_dir == o && d < g.rows * g.cols) { sx = d / g.cols; sy = d - sx * g.cols; }
        }
    }
    int best = -1, n_boxes = 0, n_peaks = 0;
    for (int base = 0; base < nb; base += 64) {
        const int b = base + lane;
        const float* row = frame_boxes + (size_t)b * 6;
        const bool is_box = b < nb && fuse_is_box(row, b, nb, conf);
        int xa = 0, xb = -1, ya = 0, yb = -1;
        bool has = false;
        if (is_box) {
            n_boxes += 1;
            n_peaks += peak_offsets[(size_t)f * max_boxes + b] >= 0;
            const bool hx = fuse_axis(row[0], row[2], g.img_w, g.rows, xa, xb), hy = fuse_axis(row[1], row[3], g.img_h, g.cols, ya, yb);
            has = hx && hy;
        }
        if (!__any(has)) continue;
        for (int s = 0; s < n_src; ++s) {
            const int X = __shfl(sx, s, 64), Y = __shfl(sy, s, 64);
            const unsigned long long in = __ballot(has && xa <= X && X <= xb && ya <= Y && Y <= yb);
            if (in && lane == s && best < 0) best = base + __ffsll((long long)in) - 1;
        }
    }
    if (lane < n_src) src_box[(size_t)f * n_src + lane] = best;
    if (counts) {
        for (int off = 32; off > 0; off >>= 1) {
            n_boxes += __shfl_xor(n_boxes, off, 64);
            n_peaks += __shfl_xor(n_peaks, off, 64);
        }
        const int with_box = __popcll(__ballot(best >= 0));
        if (lane < 3) counts[(size_t)f * 3 + lane] = lane == 0 ? n_boxes : lane == 1 ? n_peaks : with_box;
    }
}

}  // namespace

hipError_t launch_fuse_boxes(const float* d_power, int frames, int image_stride, int rows, int cols, int offset_per_dir, const float* d_boxes,
                             const int* d_box_counts, int max_boxes, int img_w, int img_h, float conf, const int* d_src_offsets, int n_src,
                             int* d_peak_offsets, float* d_peak_power, int* d_center_offsets, int* d_rects, int* d_src_box, int* d_counts, hipStream_t stream)
{
    if (n_src < 0 || n_src > kFuseMaxSources) return hipErrorInvalidValue;     // one wave: a lane per source
    const long long D = (long long)rows * cols;
    const long long groups = ((long long)max_boxes + kFuseBoxesPerGroup - 1) / kFuseBoxesPerGroup;
    if (frames * groups > 0x7fffffffLL) return hipErrorInvalidValue;
    const FuseGrid g{rows, cols, img_w, img_h};
    const dim3 grid((unsigned)(frames * groups));
    if (D <= kFuseStageMax)
        hipLaunchKernelGGL(fuse_boxes_kernel<true>, grid, dim3(256), (size_t)D * sizeof(float), stream, d_power, image_stride, g, offset_per_dir, d_boxes,
                           d_box_counts, max_boxes, (int)groups, conf, d_peak_offsets, d_peak_power, d_center_offsets, d_rects);
    else
        hipLaunchKernelGGL(fuse_boxes_kernel<false>, grid, dim3(256), 0, stream, d_power, image_stride, g, offset_per_dir, d_boxes, d_box_counts, max_boxes,
                           (int)groups, conf, d_peak_offsets, d_peak_power, d_center_offsets, d_rects);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || (n_src == 0 && !d_counts)) return e;
    hipLaunchKernelGGL(fuse_sources_kernel, dim3(frames), dim3(64), 0, stream, g, offset_per_dir, d_boxes, d_box_counts, max_boxes, conf, d_src_offsets, n_src,
                       d_peak_offsets, d_src_box, d_counts);
    return hipGetLastError();
}

}  // namespace bf
