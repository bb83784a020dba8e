// patch_match.hip -- bf_match_boxes_device and bf_smooth_boxes_device: a box of the previous image re-found in the current one by
// normalised cross-correlation, and the reference's confidence hysteresis on top of it (image-detection/src/yolo_smooth_tracking.py,
// track_with_correlation and process_video).
//
// Definition (include/beamformer_hip.h): integer patches around the box, a template of at most kMatchMaxPixels decimated pixels,
// exact integer sums per window position, three float64 operations for the score, first maximum in row-major order.
//
//   match_kernel : one workgroup per (frame, row).  After decimation by q the problem is a dense one: a pw x ph template slid over a
//       decimated search image.  Both are kept in LDS as the camera's own interleaved bytes (3 per pixel), a row padded with zeros
//       to whole dwords, because the sum of products and the sum of squares run over all three channels alike: a template row is
//       3 pw consecutive bytes and so is every window row, 3 u bytes further on.
//       template   staged once (at most 72 KiB), its channel sums and square sum reduced over the workgroup on the way.
//       tiles      the search image is staged in tiles of UT x VT positions, (VT + ph - 1) rows of 3 (pw + UT - 1) bytes, sized to the
//                  LDS that the template leaves; at the default scales one tile is the whole search area, at s_pct = 400 the area is
//                  walked tile by tile through L2.  One code path for both.
//       positions  a lane per position; a tile with fewer positions than half the lanes gives every position several lanes, each a
//                  share of the template's rows, and adds their integer sums through LDS; a tile with more positions than lanes is
//                  cut to whole trips.  Per template dword: one LDS read of the template (the same address in every lane, a
//                  broadcast), one of the window, v_alignbyte_b32 on the window's two adjacent dwords (the window starts 3 u mod 4
//                  bytes into its dword), then v_dot4_u32_u8 five times: template x window, window x window, and the window against
//                  the three byte masks that pick a channel (byte b of a row belongs to channel b mod 3, whatever u is; the masks
//                  repeat every three dwords, so the sweep takes three at a time and they are literals).  A row's last group is
//                  masked to the row's own bytes, so what it reads beyond them -- the next pixels, the next row, three dwords
//                  past the tile -- never counts.  32-bit accumulators hold all sums (the header's bounds); N, A, B are int64.
//       argmax     (r, row-major index), the lower index on equality: per lane, across the wave by shuffles, across the waves in LDS.
//   smooth_kernel : one workgroup, one frame: classify the rows, boost the candidates, compact the kept rows into the state.
// No scratch, no atomics, no workspace; the kernels are deterministic whatever the workgroup size.
#include <hip/hip_runtime.h>

#include <climits>

#include "das_kernels.h"

namespace bf {
namespace {

constexpr int kLanes = 64;
constexpr int kMatchThreads = 1024;
constexpr int kMatchWaves = kMatchThreads / kLanes;
constexpr int kMatchLdsDwords = 38912;     // 152 KiB: the template (<= 18432 dwords) and a tile of the search image
constexpr int kMatchMaxUT = 64;
constexpr int kSmoothThreads = 256;
// the template's dwords: ph rows of ceil(3 pw / 4) <= (3 P + 3 ph) / 4 with P <= kMatchMaxPixels, ph <= kMatchMaxSide; the smallest tile (one position) is as large
static_assert(2 * ((3 * kMatchMaxPixels + 3 * kMatchMaxSide) / 4) + 3 <= kMatchLdsDwords, "template and the smallest tile fit");

struct Patch { int a, b, c, d; };          // columns [a, b), rows [c, d)

// the reference's extract_patch in integers: PATCH(pct) of the header
__device__ __forceinline__ Patch patch_of(int ix1, int iy1, int w, int h, int pct, int width, int height)
{
    const int nw = w * pct / 100, nh = h * pct / 100;
    const int cx = ix1 + w / 2, cy = iy1 + h / 2;
    Patch p;
    p.a = max(0, cx - nw / 2); p.b = min(width, cx + nw / 2);
    p.c = max(0, cy - nh / 2); p.d = min(height, cy + nh / 2);
    return p;
}

__device__ __forceinline__ bool coord_ok(float v) { return fabsf(v) < 1048576.0f; }   // finite and of magnitude < 2^20 (false for a NaN)

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int o = kLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kLanes);
    return v;
}

// Four bytes of a decimated image row, bytes [4 k, 4 k + 4) of its interleaved pixels from column x0 on in steps of q; pixels at or
// beyond `limit` (counted in decimated columns from x0) read as zero.
__device__ __forceinline__ unsigned gather_dword(const unsigned char* __restrict__ row, int x0, int q, int k, int limit)
{
    unsigned v = 0;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int b = 4 * k + jj, pix = b / 3, c = b - 3 * pix;
        if (pix < limit) v |= (unsigned)row[(size_t)(x0 + q * pix) * 3 + c] << (8 * jj);
    }
    return v;
}

// The sums of one window position over template rows [r0, r1): tp the template's row r0, wp the window's first dword in that row.
struct Sums { unsigned X, Q, s0, s1, s2; };

// Three dwords = four pixels, so the channel masks are literals.  kLast: the row's last group, masked to the row's own bytes.
template <bool kLast>
__device__ __forceinline__ void sweep_group(const unsigned* tp, const unsigned* wp, unsigned& lo, unsigned shl, unsigned e0, unsigned e1, unsigned e2, Sums& a)
{
    const unsigned h0 = wp[1], h1 = wp[2], h2 = wp[3];
    const unsigned t0 = tp[0], t1 = tp[1], t2 = tp[2];
    unsigned w0 = __builtin_amdgcn_alignbyte(h0, lo, shl);
    unsigned w1 = __builtin_amdgcn_alignbyte(h1, h0, shl);
    unsigned w2 = __builtin_amdgcn_alignbyte(h2, h1, shl);
    lo = h2;
    if (kLast) { w0 &= e0; w1 &= e1; w2 &= e2; }
    a.X = __builtin_amdgcn_udot4(t0, w0, a.X, false);
    a.X = __builtin_amdgcn_udot4(t1, w1, a.X, false);
    a.X = __builtin_amdgcn_udot4(t2, w2, a.X, false);
    a.Q = __builtin_amdgcn_udot4(w0, w0, a.Q, false);
    a.Q = __builtin_amdgcn_udot4(w1, w1, a.Q, false);
    a.Q = __builtin_amdgcn_udot4(w2, w2, a.Q, false);
    a.s0 = __builtin_amdgcn_udot4(w0, 0x01000001u, a.s0, false);
    a.s0 = __builtin_amdgcn_udot4(w1, 0x00010000u, a.s0, false);
    a.s0 = __builtin_amdgcn_udot4(w2, 0x00000100u, a.s0, false);
    a.s1 = __builtin_amdgcn_udot4(w0, 0x00000100u, a.s1, false);
    a.s1 = __builtin_amdgcn_udot4(w1, 0x01000001u, a.s1, false);
    a.s1 = __builtin_amdgcn_udot4(w2, 0x00010000u, a.s1, false);
    a.s2 = __builtin_amdgcn_udot4(w0, 0x00010000u, a.s2, false);
    a.s2 = __builtin_amdgcn_udot4(w1, 0x00000100u, a.s2, false);
    a.s2 = __builtin_amdgcn_udot4(w2, 0x01000001u, a.s2, false);
}

__device__ __forceinline__ Sums sweep_rows(const unsigned* tp, const unsigned* wp, int n_rows, int trow, int srow, int ng, unsigned shl, unsigned e0, unsigned e1,
                                           unsigned e2)
{
    Sums a = {0, 0, 0, 0, 0};
    for (int r = 0; r < n_rows; ++r) {
        unsigned lo = wp[0];
        int g = 0;
#pragma unroll 2
        for (; g < ng - 1; ++g) sweep_group<false>(tp + 3 * g, wp + 3 * g, lo, shl, e0, e1, e2, a);
        sweep_group<true>(tp + 3 * g, wp + 3 * g, lo, shl, e0, e1, e2, a);
        tp += trow; wp += srow;
    }
    return a;
}

__global__ void __launch_bounds__(kMatchThreads) match_kernel(const unsigned char* __restrict__ images, const unsigned char* __restrict__ prev, int height,
                                                              int width, const float* __restrict__ boxes, int box_stride, const int* __restrict__ n_boxes,
                                                              int max_boxes, int t_pct, int s_pct, float* __restrict__ moved, float* __restrict__ score,
                                                              int* __restrict__ shift, int* __restrict__ status)
{
    __shared__ unsigned lds[kMatchLdsDwords];
    __shared__ unsigned part[4][kMatchWaves];
    __shared__ double best_r[kMatchWaves];
    __shared__ int best_i[kMatchWaves];

    const int tid = threadIdx.x, lane = tid & (kLanes - 1), wave = tid / kLanes;
    const int f = blockIdx.x / max_boxes, j = blockIdx.x % max_boxes;
    const size_t row_out = (size_t)f * max_boxes + j;
    const float* bx = boxes + row_out * box_stride;
    const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];

    int st = 0, sx = 0, sy = 0;
    float mv0 = 0.0f, mv1 = 0.0f, mv2 = 0.0f, mv3 = 0.0f, sc_out = 0.0f;

    int n = max_boxes;
    if (n_boxes) n = min(max(n_boxes[f], 0), max_boxes);
    int ix1 = 0, iy1 = 0, w = 0, h = 0;
    if (j < n && coord_ok(x1) && coord_ok(y1) && coord_ok(x2) && coord_ok(y2)) {
        ix1 = (int)x1; iy1 = (int)y1;
        w = (int)x2 - ix1; h = (int)y2 - iy1;
    }
    Patch T = {0, 0, 0, 0}, S = {0, 0, 0, 0};
    int tw = 0, th = 0;
    if (w < 1 || h < 1) {
        st = 1;
    } else {
        T = patch_of(ix1, iy1, w, h, t_pct, width, height);
        S = patch_of(ix1, iy1, w, h, s_pct, width, height);
        tw = T.b - T.a; th = T.d - T.c;
        if (tw < 1 || th < 1) st = 2;
        else if (f == 0 && !prev) st = 4;
    }

    if (st == 0) {                                             // (uniform over the workgroup from here on: every lane holds the same box)
        const size_t image_bytes = (size_t)height * width * 3;
        const unsigned char* cur = images + (size_t)f * image_bytes;
        const unsigned char* old = f == 0 ? prev : cur - image_bytes;
        int q = 1;
        while (((tw + q - 1) / q) * ((th + q - 1) / q) > kMatchMaxPixels) ++q;
        const int pw = (tw + q - 1) / q, ph = (th + q - 1) / q, P = pw * ph;
        const int sw = S.b - S.a, sh = S.d - S.c;
        const int dx0 = T.a - S.a, dy0 = T.c - S.c;
        const int dxb = dx0 % q, dyb = dy0 % q;
        const int nu = (sw - tw - dxb) / q + 1, nv = (sh - th - dyb) / q + 1;       // window positions; the zero displacement is (dx0 / q, dy0 / q)
        const int swp = pw + nu - 1;                                              // the decimated search image's columns
        const int trow = (3 * pw + 3) / 4;                                        // dwords of a template row
        const int tail = 3 * pw - 4 * (trow - 1);                                 // bytes of its last dword that belong to it, 1..4
        const unsigned lastmask = tail == 4 ? 0xffffffffu : (1u << (8 * tail)) - 1u;
        const int tdw = ph * trow;
        // the sweep takes a row three dwords (four pixels) at a time; the last group's dwords keep: everything, the row's tail, nothing
        const int ng = (trow + 2) / 3, kl = 3 * (ng - 1);
        const unsigned e0 = kl < trow - 1 ? 0xffffffffu : lastmask;
        const unsigned e1 = kl + 1 < trow - 1 ? 0xffffffffu : kl + 1 == trow - 1 ? lastmask : 0u;
        const unsigned e2 = kl + 2 == trow - 1 ? lastmask : 0u;
        unsigned* tmpl = lds;
        unsigned* tile = lds + tdw;

        // ---- the template, and its sums
        unsigned s0 = 0, s1 = 0, s2 = 0, qq = 0;
#pragma unroll 2
        for (int e = tid; e < tdw; e += kMatchThreads) {
            const int r = e / trow, k = e - r * trow;
            const unsigned v = gather_dword(old + (size_t)(T.c + q * r) * width * 3, T.a, q, k, pw);
            tmpl[e] = v;
            const int km = k % 3;
            const unsigned m0 = km == 0 ? 0x01000001u : km == 1 ? 0x00010000u : 0x00000100u;
            const unsigned m1 = km == 0 ? 0x00000100u : km == 1 ? 0x01000001u : 0x00010000u;
            const unsigned m2 = km == 0 ? 0x00010000u : km == 1 ? 0x00000100u : 0x01000001u;
            s0 = __builtin_amdgcn_udot4(v, m0, s0, false);
            s1 = __builtin_amdgcn_udot4(v, m1, s1, false);
            s2 = __builtin_amdgcn_udot4(v, m2, s2, false);
            qq = __builtin_amdgcn_udot4(v, v, qq, false);
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); qq = wave_sum(qq);
        if (lane == 0) { part[0][wave] = s0; part[1][wave] = s1; part[2][wave] = s2; part[3][wave] = qq; }
        __syncthreads();
        long long ST0 = 0, ST1 = 0, ST2 = 0, QT = 0;
        for (int i = 0; i < kMatchWaves; ++i) { ST0 += part[0][i]; ST1 += part[1][i]; ST2 += part[2][i]; QT += part[3][i]; }
        const long long A = (long long)P * QT - (ST0 * ST0 + ST1 * ST1 + ST2 * ST2);

        if (A == 0) {
            st = 3;
            mv0 = x1; mv1 = y1; mv2 = x2; mv3 = y2;
        } else {
            // ---- the tile: as many columns of positions as kMatchMaxUT allows, halved until the rows it needs fit beside the template
            const int budget = kMatchLdsDwords - tdw - 3;                         // (three dwords of slack: the last group reads on past the last window, masked)
            int UT = min(nu, kMatchMaxUT), srow, VT;
            for (;;) {
                srow = (3 * (UT - 1) + 4 * trow + 3) / 4;
                const int rows = budget / srow;
                if (rows >= ph) { VT = min(nv, rows - ph + 1); break; }
                UT = max(1, UT / 2);                                              // (UT = 1 always fits: srow = trow)
            }
            // whole trips: a tile of more positions than lanes takes a multiple of the lanes, and what is left over forms a small last tile
            if (UT * VT > kMatchThreads) VT = (UT * VT / kMatchThreads) * kMatchThreads / UT;
            const double dA = (double)A;
            double my_r = -HUGE_VAL;
            int my_i = INT_MAX;
            for (int v0 = 0; v0 < nv; v0 += VT)
                for (int u0 = 0; u0 < nu; u0 += UT) {
                    const int ut = min(UT, nu - u0), vt = min(VT, nv - v0);
                    const int rows = vt + ph - 1;
                    __syncthreads();                                              // the previous tile has been read
#pragma unroll 4
                    for (int e = tid; e < rows * srow; e += kMatchThreads) {
                        const int r = e / srow, k = e - r * srow;
                        tile[e] = gather_dword(cur + (size_t)(S.c + dyb + q * (v0 + r)) * width * 3, S.a + dxb + q * u0, q, k, swp - u0);
                    }
                    __syncthreads();
                    // A tile with fewer positions than half the lanes splits every position's rows over C lanes (each lane C-th of the
                    // rows; integer partial sums through LDS, so the split changes no bit), where the LDS behind the tile has the room.
                    const int npos = ut * vt;
                    int C = min(kMatchThreads / npos, ph);
                    if (C < 2 || tdw + rows * srow + 3 + 5 * kMatchThreads > kMatchLdsDwords) C = 1;
                    unsigned* red = tile + rows * srow + 3;
                    for (int p0 = 0; p0 < npos; p0 += kMatchThreads) {            // (one trip when C > 1)
                        const int item = p0 + tid;
                        const int c = C > 1 ? item / npos : 0, p = item - c * npos;
                        const bool work = c < C && p < npos;
                        const int vv = p / ut, uu = p - vv * ut;
                        Sums sm = {0, 0, 0, 0, 0};
                        if (work) {
                            const int r0 = c * ph / C, r1 = (c + 1) * ph / C;
                            sm = sweep_rows(tmpl + r0 * trow, tile + (vv + r0) * srow + ((3 * uu) >> 2), r1 - r0, trow, srow, ng, (3 * uu) & 3, e0, e1, e2);
                        }
                        if (C > 1) {
                            red[tid] = sm.X; red[kMatchThreads + tid] = sm.Q; red[2 * kMatchThreads + tid] = sm.s0; red[3 * kMatchThreads + tid] = sm.s1;
                            red[4 * kMatchThreads + tid] = sm.s2;
                            __syncthreads();
                            if (c == 0 && work)
                                for (int i = 1; i < C; ++i) {
                                    const int o = tid + i * npos;
                                    sm.X += red[o]; sm.Q += red[kMatchThreads + o]; sm.s0 += red[2 * kMatchThreads + o]; sm.s1 += red[3 * kMatchThreads + o];
                                    sm.s2 += red[4 * kMatchThreads + o];
                                }
                        }
                        if (c == 0 && work) {
                            const long long SI0 = sm.s0, SI1 = sm.s1, SI2 = sm.s2;
                            const long long N = (long long)P * (long long)sm.X - (ST0 * SI0 + ST1 * SI1 + ST2 * SI2);
                            const long long B = (long long)P * (long long)sm.Q - (SI0 * SI0 + SI1 * SI1 + SI2 * SI2);
                            const double r = B == 0 ? 0.0 : (double)N / sqrt(dA * (double)B);
                            const int idx = (v0 + vv) * nu + (u0 + uu);
                            if (r > my_r || (r == my_r && idx < my_i)) { my_r = r; my_i = idx; }
                        }
                    }
                }
            for (int o = kLanes / 2; o > 0; o >>= 1) {
                const double r2 = __shfl_xor(my_r, o, kLanes);
                const int i2 = __shfl_xor(my_i, o, kLanes);
                if (r2 > my_r || (r2 == my_r && i2 < my_i)) { my_r = r2; my_i = i2; }
            }
            if (lane == 0) { best_r[wave] = my_r; best_i[wave] = my_i; }
            __syncthreads();
            for (int i = 0; i < kMatchWaves; ++i)
                if (best_r[i] > my_r || (best_r[i] == my_r && best_i[i] < my_i)) { my_r = best_r[i]; my_i = best_i[i]; }
            const int bv = my_i / nu, bu = my_i - bv * nu;
            sx = (dxb + q * bu) - dx0; sy = (dyb + q * bv) - dy0;
            const float fx = (float)sx, fy = (float)sy;
            mv0 = x1 + fx; mv1 = y1 + fy; mv2 = x2 + fx; mv3 = y2 + fy;
            sc_out = (float)my_r;
        }
    }

    if (tid == 0) {
        float* mo = moved + row_out * 4;
        mo[0] = mv0; mo[1] = mv1; mo[2] = mv2; mo[3] = mv3;
        score[row_out] = sc_out;
        if (shift) { shift[row_out * 2] = sx; shift[row_out * 2 + 1] = sy; }
        status[row_out] = st;
    }
}

// ---------------------------------------------------------------- the hysteresis

__device__ __forceinline__ float sm_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float sm_min(float a, float b) { return a < b ? a : b; }

// compute_iou(moved box p, candidate g) of the reference, in float32
__device__ __forceinline__ float sm_iou(const float4 p, const float4 g)
{
    const float dw = sm_min(p.z, g.z) - sm_max(p.x, g.x), dh = sm_min(p.w, g.w) - sm_max(p.y, g.y);
    const float iw = dw > 0.0f ? dw : 0.0f, ih = dh > 0.0f ? dh : 0.0f;
    const float inter = iw * ih;
    const float a1 = (p.z - p.x) * (p.w - p.y), a2 = (g.z - g.x) * (g.w - g.y);
    const float uni = (a1 + a2) - inter;
    return uni > 0.0f ? inter / uni : 0.0f;
}

enum : unsigned char { ROW_NONE = 0, ROW_VALID = 1, ROW_CANDIDATE = 2, ROW_BOOSTED = 3 };

__global__ void __launch_bounds__(kSmoothThreads) smooth_kernel(const float* __restrict__ boxes, const int* __restrict__ n_boxes, int max_boxes, float conf_low,
                                                                float conf_high, float iou_threshold, float corr_threshold, int slots,
                                                                const float* __restrict__ moved, const float* __restrict__ score,
                                                                const int* __restrict__ status, int* __restrict__ state, float* __restrict__ out,
                                                                int* __restrict__ boosted, int* __restrict__ counts)
{
    __shared__ unsigned char kind[kMatchMaxBoxes];
    __shared__ float4 pbox[kSmoothMaxSlots];
    __shared__ int pany[kSmoothMaxSlots];       // previous box p takes part
    __shared__ int any_valid, any_corr;

    const int tid = threadIdx.x;
    int n = max_boxes;
    if (n_boxes) n = min(max(n_boxes[0], 0), max_boxes);
    const int m = min(max(state[0], 0), slots);
    if (tid == 0) { any_valid = 0; any_corr = 0; }
    __syncthreads();
    if (tid < slots) {
        const bool in = tid < m && status[tid] == 0;
        pany[tid] = in;
        pbox[tid] = in ? make_float4(moved[4 * tid], moved[4 * tid + 1], moved[4 * tid + 2], moved[4 * tid + 3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (in && score[tid] > corr_threshold) any_corr = 1;
    }
    for (int j = tid; j < max_boxes; j += kSmoothThreads) {
        const float* b = boxes + (size_t)j * 6;
        unsigned char k = ROW_NONE;
        if (j < n && isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]) && b[2] > b[0] && b[3] > b[1] && isfinite(b[4])) {
            if (b[4] > conf_high) { k = ROW_VALID; any_valid = 1; }
            else if (b[4] > conf_low) k = ROW_CANDIDATE;
        }
        kind[j] = k;
    }
    __syncthreads();
    const bool valid_branch = any_valid != 0;
    for (int j = tid; j < max_boxes; j += kSmoothThreads) {
        const float* b = boxes + (size_t)j * 6;
        unsigned char k = kind[j];
        float s = 0.0f;
        if (valid_branch) {
            if (k == ROW_VALID) s = b[4];
        } else if (k == ROW_CANDIDATE) {
            bool boost = any_corr != 0;
            const float4 g = make_float4(b[0], b[1], b[2], b[3]);
            for (int p = 0; p < slots && !boost; ++p)
                if (pany[p] && sm_iou(pbox[p], g) > iou_threshold) boost = true;
            if (boost) { kind[j] = ROW_BOOSTED; s = conf_high; }
        }
        float* o = out + (size_t)j * 6;
        o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3]; o[4] = s; o[5] = b[5];
        if (boosted) boosted[j] = !valid_branch && kind[j] == ROW_BOOSTED;
    }
    __syncthreads();
    if (tid < kLanes) {                              // the kept rows in row order: wave 0, 64 rows a step, slots by ballot
        const unsigned char keep = valid_branch ? ROW_VALID : ROW_BOOSTED;
        int total = 0, n_valid = 0, n_cand = 0, n_boost = 0;
        float* rows = reinterpret_cast<float*>(state + 4);
        for (int base = 0; base < max_boxes; base += kLanes) {
            const int j = base + tid;
            const unsigned char k = j < max_boxes ? kind[j] : (unsigned char)ROW_NONE;
            const unsigned long long mine = __ballot(k == keep);
            n_valid += __popcll(__ballot(k == ROW_VALID));
            n_cand += __popcll(__ballot(k == ROW_CANDIDATE || k == ROW_BOOSTED));
            n_boost += __popcll(__ballot(k == ROW_BOOSTED));
            const int slot = total + __popcll(mine & ((1ull << tid) - 1ull));
            if (k == keep && k != ROW_NONE && slot < slots) {
                const float* b = boxes + (size_t)j * 6;
                for (int c = 0; c < 4; ++c) rows[4 * slot + c] = b[c];
            }
            total += __popcll(mine);
        }
        const int kept = min(total, slots);
        for (int i = 4 * kept + tid; i < 4 * slots; i += kLanes) rows[i] = 0.0f;
        if (tid == 0) {
            state[0] = kept; state[1] = 0; state[2] = 0; state[3] = 0;
            if (counts) { counts[0] = n_valid; counts[1] = n_cand; counts[2] = n_boost; counts[3] = total - kept; }
        }
    }
}

}  // namespace

hipError_t launch_match_boxes(const unsigned char* d_images, const unsigned char* d_prev, int frames, int height, int width, const float* d_boxes, int box_stride,
                              const int* d_n_boxes, int max_boxes, int t_pct, int s_pct, float* d_moved, float* d_score, int* d_shift, int* d_status,
                              hipStream_t stream)
{
    if (frames < 1 || height < 1 || height > kMatchMaxSide || width < 1 || width > kMatchMaxSide || max_boxes < 1 || max_boxes > kMatchMaxBoxes || box_stride < 4 ||
        t_pct < 100 || s_pct < t_pct || s_pct > 400 || (long long)frames * max_boxes > INT_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)(frames * max_boxes)), dim3(kMatchThreads), 0, stream, d_images, d_prev, height, width, d_boxes, box_stride,
                       d_n_boxes, max_boxes, t_pct, s_pct, d_moved, d_score, d_shift, d_status);
    return hipGetLastError();
}

hipError_t launch_smooth_boxes(const float* d_boxes, const int* d_n_boxes, int max_boxes, float conf_low, float conf_high, float iou_threshold, float corr_threshold,
                               int slots, const float* d_moved, const float* d_score, const int* d_status, int* d_state, float* d_out, int* d_boosted,
                               int* d_counts, hipStream_t stream)
{
    if (max_boxes < 1 || max_boxes > kMatchMaxBoxes || slots < 1 || slots > kSmoothMaxSlots) return hipErrorInvalidValue;
    hipLaunchKernelGGL(smooth_kernel, dim3(1), dim3(kSmoothThreads), 0, stream, d_boxes, d_n_boxes, max_boxes, conf_low, conf_high, iou_threshold, corr_threshold,
                       slots, d_moved, d_score, d_status, d_state, d_out, d_boosted, d_counts);
    return hipGetLastError();
}

}  // namespace bf
