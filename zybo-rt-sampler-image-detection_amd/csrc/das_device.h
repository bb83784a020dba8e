// das_device.h -- what the delay-and-sum kernel units (das_kernels.hip, das_strided.hip, das_pair.hip) share on the device -- the
// kernel argument block, staging, the ordered power sum, the helpers of the shifted-copies layout -- and the host helpers of their
// launchers.  das_kernels.hip has the overview.
//
// Everything here sits in the unnamed namespace: KArgs is a kernel parameter, so it is part of every kernel's symbol, and no function
// that crosses units takes one -- the per-family launchers (das_geometry.h) take the launch and its plan and call make_args themselves.
#pragma once
#include "das_geometry.h"

namespace bf {

namespace {

// Scalars of one launch (kernel argument, lives in SGPRs).
struct KArgs {
    long long miso_row;                   // launch_miso only: flat table offset (the reference's `offset`)
    int n_mics, m_total, n_samples, n_taps;
    int dir_begin, dir_end, image_stride, image_origin;
    int lead, row_stride, mic_chunk, n_chunks, tile_dirs, n_tiles;
    int scratch_off, srow, pbw;           // per-wave power scratch: float offset in LDS, row stride, rows per wave
    int n_is_pow2;
    float inv_n;
    int n_frames;   // frames of the launch (das_pair_kernel: whether a workgroup's second frame exists)
    int wg_frames, frame_inner;   // workgroup id -> (tile, frame [pair]): see tile_and_frame()
    long long digest_h_off;   // shifted-copies pad / lerp: where the grouped lerp weights start in the digest buffer (floats)
    long long digest_t_off;   // the 8-tap FIR pair kernel: where the taps regrouped per 8 directions start in the digest buffer (floats)
    long long digest_o_off;   // pad / lerp pair kernels: where the sweep order (flat direction of every position) starts in the digest buffer; 0 = positions are directions
};

// Workgroup id -> (direction tile, frame or frame pair).  Ids go round-robin over the 8 XCDs.
//   frame_inner == 0:  tile = id % n_tiles, frame = id / n_tiles.  With n_tiles a multiple of 8 a tile's workgroups stay on
//                      one XCD (tile % 8 == id % 8); an XCD walks its tiles frame by frame, so a tile's table slice is
//                      re-used out of L2 only if the XCD's share of the whole table stays resident (cfg2: 650 KB).
//   frame_inner == 1:  tables beyond that (cfg5: 33 MB per XCD): XCD x = id % 8 walks tile x, x + 8, .. and runs ALL frames of
//                      a tile back to back (its 32 CUs hold 32 frames of the same tile at a time), so the slice comes from
//                      HBM once instead of once per frame.
__device__ __forceinline__ void tile_and_frame(const KArgs& a, int* tile, int* frame)
{
    const unsigned id = blockIdx.x;
    if (a.frame_inner) {
        const unsigned x = id & 7u, j = id >> 3;
        *tile = (int)(x + 8u * (j / (unsigned)a.wg_frames));
        *frame = (int)(j % (unsigned)a.wg_frames);
    } else {
        *tile = (int)(id % (unsigned)a.n_tiles);
        *frame = (int)(id / (unsigned)a.n_tiles);
    }
}

// The read-only tables are separate `const __restrict__` kernel parameters on purpose: only then can the
// compiler prove that no store in the kernel clobbers them and fetch the wave-uniform table entries with
// scalar loads (s_load_*) instead of 64-lane vector loads.
#define BF_TABLE_PARAMS                                                                                   \
    const float* __restrict__ signals, float* __restrict__ images, const int32_t* __restrict__ mics,     \
        const int32_t* __restrict__ whole, const float* __restrict__ frac, const float* __restrict__ taps
#define BF_TABLE_ARGS signals, images, mics, whole, frac, taps

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// Copy mic rows [m0, m0+mc) of one frame into LDS rows 0..mc-1 at column `lead`.  One wave per row, lanes
// stride the row in 16-byte pieces (coalesced global_load_dwordx4 -> ds_write_b128).
__device__ __forceinline__ void stage_chunk(float* lds, const KArgs& a, const int32_t* __restrict__ mics,
                                            const float* __restrict__ frame, int m0, int mc, int wave, int nwaves, int lane)
{
    const int n = a.n_samples;
    for (int r = wave; r < mc; r += nwaves) {
        const int mic = mics[m0 + r];
        const float* src = frame + (size_t)mic * n;
        float* dst = lds + r * a.row_stride + a.lead;
        if ((n & 3) == 0) {
            const float4* s4 = reinterpret_cast<const float4*>(src);
            float4* d4 = reinterpret_cast<float4*>(dst);
            for (int i = lane; i < (n >> 2); i += kWave) d4[i] = s4[i];
        } else {
            for (int i = lane; i < n; i += kWave) dst[i] = src[i];
        }
    }
}

// ---- mean power, in the reference's summation order ------------------------------------------------------
// (the one statement of the rule, for both layouts: park_squares / flush_powers are the strided kernels' form of it, mic_mean /
// row_mean_power below them the shifted-copies kernels')
// The reference finishes a direction with (pad_and_sum.c:122-131)
//     for k: out[k] /= n; sum += out[k]^2          (gcc: vdivps, vmulps, then one vaddss per k, in k order)
//     image = sum / N
// A float32 sum of N squares taken in another order differs from that by up to ~N*2^-24 relative (2e-5 observed
// at N = 1024), which is more than the 1e-5 parity bar.  So the squares are summed in k order here too:
// every wave parks the squares of `pbw` finished directions as rows of a private LDS scratch, then lanes
// 0..pbw-1 each walk one row front to back (ds_read_b128, four ordered adds per read).
//
// REF_TAIL: the last N % 4 samples as the compiled reference sums them.  gcc vectorises the loop above by 8, then by 4, and runs
// the rest through a scalar epilogue in which its contraction default fuses square and add: sum = fma(out[k], out[k], sum) for
// k >= N - N % 4 (measured on the reference compiled at N = 202 and N = 450; oracle/das_oracle.c states the same rule).  Those
// samples are parked unsquared and the summing lane fuses them.  The reference's own sizes are multiples of 8: nothing is fused there.
// The stream maps are defined with every square rounded (include/beamformer_hip.h): REF_TAIL = false.
template <int NC, bool REF_TAIL = false>
__device__ __forceinline__ void park_squares(const float (&acc)[NC], float* scratch_row, const KArgs& a, int d, int lane)
{
    float sq[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        // out[k] /= (float)n: for a power-of-two n the reciprocal multiply is exact; otherwise a true division
        const float o = a.n_is_pow2 ? acc[c] * a.inv_n : acc[c] / (float)a.n_mics;
        sq[c] = (REF_TAIL && lane + c * kWave >= (a.n_samples & ~3)) ? o : o * o;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) scratch_row[lane + c * kWave] = sq[c];
    if (lane == 0) scratch_row[a.srow - 4] = __int_as_float(d);   // the pad column carries the direction id
}

// Rows are 16-byte aligned and 4 (mod 64) dwords apart, so up to 16 lanes can each stream their own row with
// ds_read_b128 without sharing a bank; the additions stay strictly in k order.
template <bool REF_TAIL = false>
__device__ __forceinline__ void flush_powers(const float* scratch, int filled, float* __restrict__ img, const KArgs& a, int lane)
{
    if (lane < filled) {
        const float* row = scratch + lane * a.srow;
        const float4* row4 = reinterpret_cast<const float4*>(row);
        const int n = a.n_samples;
        float sum = 0.0f;
        int k = 0;
#pragma unroll 4
        for (; k + 4 <= n; k += 4) {
            const float4 v = row4[k >> 2];
            sum += v.x; sum += v.y; sum += v.z; sum += v.w;
        }
        for (; k < n; ++k) sum = REF_TAIL ? __fmaf_rn(row[k], row[k], sum) : sum + row[k];   // k >= n - n % 4 (REF_TAIL: parked unsquared)
        const int d = __float_as_int(row[a.srow - 4]);
        img[d - a.image_origin] = sum / (float)n;
    }
}

// The same rule for the shifted-copies kernels (das_kernels.hip, das_pair.hip), whose lanes hold four samples of a direction each and
// whose rows alias the staging buffer: a kernel keeps its row layout, its barriers and its rounds, and takes the arithmetic here.
//
// out[k] /= (float)n for a lane's four sums.  MUL (the count is a power of two): the reciprocal multiply, exact.  Otherwise a true
// division like the reference's, by a divisor passed through an empty asm: that is not speculatable, so the division sequence stays
// behind the caller's branch on a.n_is_pow2.
template <bool MUL>
__device__ __forceinline__ void mic_mean(float x0, float x1, float x2, float x3, int n_mics, float inv_n, float& o0, float& o1, float& o2, float& o3)
{
    if constexpr (MUL) {
        o0 = x0 * inv_n; o1 = x1 * inv_n; o2 = x2 * inv_n; o3 = x3 * inv_n;
    } else {
        float fm = (float)n_mics;
        asm volatile("" : "+v"(fm));
        o0 = x0 / fm; o1 = x1 / fm; o2 = x2 / fm; o3 = x3 / fm;
    }
}

__device__ __forceinline__ float add_in_order(const float4* row4, float sum)   // 32 squares: eight reads in flight, then 32 ordered adds
{
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = row4[u];
#pragma unroll
    for (int u = 0; u < 8; ++u) { sum += v[u].x; sum += v[u].y; sum += v[u].z; sum += v[u].w; }
    return sum;
}

// image = sum / N of one parked row (squares in k order, 16-byte aligned), walked by one lane.  ONE_TRIP: the 32-sample trip is not
// unrolled further, for the kernels that have no registers for two trips' reads (each says why where it asks for it).  No REF_TAIL
// form: the kernels that come here take N % 4 == 0 only (plan_das); das_copies_kernel, which takes any N, writes its sum out.
template <bool ONE_TRIP>
__device__ __forceinline__ float row_mean_power(const float* row, int n)
{
    const float4* row4 = reinterpret_cast<const float4*>(row);
    float sum = 0.0f;
    int k = 0;
    if constexpr (ONE_TRIP) {
#pragma unroll 1
        for (; k + 32 <= n; k += 32) sum = add_in_order(row4 + (k >> 2), sum);
    } else {
        for (; k + 32 <= n; k += 32) sum = add_in_order(row4 + (k >> 2), sum);
    }
    for (; k < n; ++k) sum += row[k];
    return sum / (float)n;
}

// sum + the first 4 * `quads` (quads = 1..32) squares of a half row parked at LDS byte address `ad`, in k order.
// The row holds its 128 samples as [the 64 even ones][the 64 odd ones] (that is how a lane that owns samples 2l, 2l+1 stores them
// without a bank conflict: one dword per lane, side by side, twice), so samples 8p .. 8p+7 are the p-th 16-byte quad of each part,
// E and O, added E0 O0 E1 O1 E2 O2 E3 O3.
// Rolling: the reads of four such pairs are in flight, and a pair is requested again, four pairs on, right behind the eight adds that
// consumed it -- after the first wait the chain never meets an LDS latency, and no wait inside the loop is a full one.  The last 1..8
// quads of samples drain without refills.  The reads run up to 7 quads of samples past `quads`, never past the row's 128 samples.
// One statement, because the adds name the registers of a read tuple singly, which asm operands cannot express: the reads land in
// HARD-WIRED v96..v111 (E) and v112..v127 (O), named as clobbers (tests/test_isa_hazards.py: nothing touches a register between a
// read into it and its wait).
#define BF_R_ADD4(e0, o0, e1, o1) "v_add_f32 %[s], %[s], v" #e0 "\n\tv_add_f32 %[s], %[s], v" #o0 "\n\tv_add_f32 %[s], %[s], v" #e1 "\n\tv_add_f32 %[s], %[s], v" #o1 "\n\t"
#define BF_R_READ(e0, e3, o0, o3, off) "ds_read_b128 v[" #e0 ":" #e3 "], %[ad] offset:" #off "\n\tds_read_b128 v[" #o0 ":" #o3 "], %[ad] offset:256 + " #off "\n\t"
#define BF_R_ROLL(e0, e1, e2, e3, o0, o1, o2, o3, off) "s_waitcnt lgkmcnt(6)\n\t" BF_R_ADD4(e0, o0, e1, o1) BF_R_ADD4(e2, o2, e3, o3) BF_R_READ(e0, e3, o0, o3, off)
#define BF_R_DONE(n) "s_cmp_eq_u32 %[nq], " #n "\n\ts_cbranch_scc1 .Le_%=\n\t"
#define BF_R_DRAIN(e0, e1, e2, e3, o0, o1, o2, o3, left, n) "s_waitcnt lgkmcnt(" #left ")\n\t" BF_R_ADD4(e0, o0, e1, o1) BF_R_DONE(n) BF_R_ADD4(e2, o2, e3, o3)
__device__ __forceinline__ float add_in_order_rolling(unsigned ad, int quads, float sum)
{
    asm volatile(BF_R_READ(96, 99, 112, 115, 0) BF_R_READ(100, 103, 116, 119, 16) BF_R_READ(104, 107, 120, 123, 32) BF_R_READ(108, 111, 124, 127, 48)
                 "s_cmp_le_u32 %[nq], 8\n\ts_cbranch_scc1 .Ld_%=\n"
                 ".Lt_%=:\n\t"      // a trip of four pairs (32 samples), each requested again from 64 bytes on
                 BF_R_ROLL(96, 97, 98, 99, 112, 113, 114, 115, 64) BF_R_ROLL(100, 101, 102, 103, 116, 117, 118, 119, 80)
                 BF_R_ROLL(104, 105, 106, 107, 120, 121, 122, 123, 96) BF_R_ROLL(108, 109, 110, 111, 124, 125, 126, 127, 112)
                 "v_add_u32 %[ad], 64, %[ad]\n\ts_sub_u32 %[nq], %[nq], 8\n\ts_cmp_gt_u32 %[nq], 8\n\ts_cbranch_scc1 .Lt_%=\n"
                 ".Ld_%=:\n\t"      // the drain: 1..8 quads of samples are left, all of them requested; it ends behind any half pair
                 BF_R_DRAIN(96, 97, 98, 99, 112, 113, 114, 115, 6, 1) BF_R_DONE(2) BF_R_DRAIN(100, 101, 102, 103, 116, 117, 118, 119, 4, 3) BF_R_DONE(4)
                 BF_R_DRAIN(104, 105, 106, 107, 120, 121, 122, 123, 2, 5) BF_R_DONE(6) BF_R_DRAIN(108, 109, 110, 111, 124, 125, 126, 127, 0, 7)
                 ".Le_%=:\n\ts_waitcnt lgkmcnt(0)"      // (an early end: the reads beyond it land before the registers are anyone else's)
                 : [s] "+v"(sum), [ad] "+v"(ad), [nq] "+s"(quads)
                 :
                 : "memory", "scc", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111",
                   "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
    return sum;
}
#undef BF_R_ADD4
#undef BF_R_READ
#undef BF_R_ROLL
#undef BF_R_DONE
#undef BF_R_DRAIN

namespace copies {

__device__ __forceinline__ float dpp_prev(float x)   // lane-1's value, 0 in lane 0
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_next(float x)   // lane+1's value, 0 in lane 63
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x130, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_value(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }

// Write the NC shifted copies of a segment: copy c holds the row shifted right by c samples, i.e. its aligned
// quad i is (x[4i-c], ..., x[4i-c+3]); (py, pz, pw) are x[4q-3 .. 4q-1] (previous lane, or the segment edge).
// NC = 4 serves 16-byte reads at any delay (the FIR flavours' ds_read_b128), NC = 2 the 8-byte reads of pad / lerp.
template <int NC>
__device__ __forceinline__ void write_copies(float* row0, int rs, int col, int lane, float4 v, float py, float pz, float pw)
{
    float4* q0 = reinterpret_cast<float4*>(row0 + 0 * rs + col) + lane;
    float4* q1 = reinterpret_cast<float4*>(row0 + 1 * rs + col) + lane;
    *q0 = v;
    *q1 = make_float4(pw, v.x, v.y, v.z);
    if constexpr (NC == 4) {
        float4* q2 = reinterpret_cast<float4*>(row0 + 2 * rs + col) + lane;
        float4* q3 = reinterpret_cast<float4*>(row0 + 3 * rs + col) + lane;
        *q2 = make_float4(pz, pw, v.x, v.y);
        *q3 = make_float4(py, pz, pw, v.x);
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// The quad (two register pairs) of one 256-sample segment of a staged mic row, and of its difference row for lerp.
struct Quad { f32x2 lo, hi; };

}  // namespace copies

// The sweeps keep LDS reads in flight in hard-wired registers across asm statements: sound only in a build that does not spill
// (tests/test_isa_hazards.py checks the build the tests run on; this checks the one that is about to launch).
template <typename K>
static hipError_t refuse_scratch(K kernel, int* cached)
{
    if (*cached < 0) {
        hipFuncAttributes fa{};
        hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel));
        if (e != hipSuccess) return e;
        *cached = (int)fa.localSizeBytes;
    }
#ifdef BF_STAMPS
    return hipSuccess;              // (the profiling build's stamp registers may spill: its phase shares are read, never its images)
#else
    return *cached != 0 ? hipErrorInvalidDeviceFunction : hipSuccess;
#endif
}

// Raise the kernel's dynamic-LDS limit to what the plan asks for and enqueue it.  `scratch`: the cache slot of refuse_scratch for
// the kernels that keep reads in flight across asm statements, null for the others.
template <typename K, typename... Args>
hipError_t launch_with_lds(K kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, int* scratch, Args... args)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    if (scratch != nullptr && (e = refuse_scratch(kernel, scratch)) != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    return hipGetLastError();
}

inline KArgs make_args(const DasLaunch& L, const DasPlan& plan)
{
    KArgs a{};
    a.miso_row = 0;
    a.n_mics = L.n_mics; a.m_total = L.m_total; a.n_samples = L.n_samples; a.n_taps = L.n_taps;
    a.dir_begin = L.dir_begin; a.dir_end = L.dir_end; a.image_stride = L.image_stride; a.image_origin = L.image_origin;
    a.lead = plan.lead; a.row_stride = plan.row_stride; a.mic_chunk = plan.mic_chunk; a.n_chunks = plan.n_chunks;
    a.tile_dirs = plan.tile_dirs; a.n_tiles = plan.n_tiles;
    a.scratch_off = plan.scratch_off; a.srow = plan.srow; a.pbw = plan.pbw;
    a.n_is_pow2 = (L.n_mics & (L.n_mics - 1)) == 0;
    a.inv_n = 1.0f / (float)L.n_mics;
    a.n_frames = L.frames;
    a.wg_frames = wg_frames(plan.family, L.frames);
    a.frame_inner = plan.frame_inner;
    const DigestLayout dig = digest_layout(L, plan);
    a.digest_h_off = dig.h_off;
    a.digest_t_off = dig.t_off;
    a.digest_o_off = L.tab.digest_order_off;
    return a;
}

}  // namespace

}  // namespace bf
