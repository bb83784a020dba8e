// das_cells.hip -- the lerp sweep with two frames per workgroup on rows of 16-byte CELLS: copies::das_pair2_cells_kernel, the second
// kernel of das_pair2_kernel's family (das_pair.hip), for microphone counts that are a multiple of 32.  das_kernels.hip has the
// overview, das_pair.hip the kernel this one grew out of.
#include "das_device.h"

namespace bf {

namespace {

// sum + the first 4 * `quads` (quads = 1..32) squares of a half row parked at LDS byte address `ad`, in k order: add_in_order_rolling
// (das_device.h) for a row that holds its 128 samples IN ORDER -- a lane of the cells kernel owns samples l and 64 + l of a half, so
// its two dwords per store already land where k order wants them.  Samples 8p .. 8p+7 are the quads A = 2p and B = 2p + 1, added
// A0 A1 A2 A3 B0 B1 B2 B3.  Rolling as there: the reads of four such pairs are in flight, a pair is requested again, four pairs on,
// right behind the eight adds that consumed it, and no wait inside the loop is a full one.  The reads run up to 7 quads past `quads`,
// never past the row's 128 samples.  The reads land in HARD-WIRED v96..v111 (A) and v112..v127 (B), named as clobbers.
#define BF_L_ADD4(r0, r1, r2, r3) "v_add_f32 %[s], %[s], v" #r0 "\n\tv_add_f32 %[s], %[s], v" #r1 "\n\tv_add_f32 %[s], %[s], v" #r2 "\n\tv_add_f32 %[s], %[s], v" #r3 "\n\t"
#define BF_L_READ(a0, a3, b0, b3, off) "ds_read_b128 v[" #a0 ":" #a3 "], %[ad] offset:" #off "\n\tds_read_b128 v[" #b0 ":" #b3 "], %[ad] offset:16 + " #off "\n\t"
#define BF_L_ROLL(a0, a1, a2, a3, b0, b1, b2, b3, off) "s_waitcnt lgkmcnt(6)\n\t" BF_L_ADD4(a0, a1, a2, a3) BF_L_ADD4(b0, b1, b2, b3) BF_L_READ(a0, a3, b0, b3, off)
#define BF_L_DONE(n) "s_cmp_eq_u32 %[nq], " #n "\n\ts_cbranch_scc1 .Le_%=\n\t"
#define BF_L_DRAIN(a0, a1, a2, a3, b0, b1, b2, b3, left, n) "s_waitcnt lgkmcnt(" #left ")\n\t" BF_L_ADD4(a0, a1, a2, a3) BF_L_DONE(n) BF_L_ADD4(b0, b1, b2, b3)
__device__ __forceinline__ float add_in_order_linear(unsigned ad, int quads, float sum)
{
    asm volatile(BF_L_READ(96, 99, 112, 115, 0) BF_L_READ(100, 103, 116, 119, 32) BF_L_READ(104, 107, 120, 123, 64) BF_L_READ(108, 111, 124, 127, 96)
                 "s_cmp_le_u32 %[nq], 8\n\ts_cbranch_scc1 .Ld_%=\n"
                 ".Lt_%=:\n\t"      // a trip of four pairs (32 samples), each requested again from 128 bytes on
                 BF_L_ROLL(96, 97, 98, 99, 112, 113, 114, 115, 128) BF_L_ROLL(100, 101, 102, 103, 116, 117, 118, 119, 160)
                 BF_L_ROLL(104, 105, 106, 107, 120, 121, 122, 123, 192) BF_L_ROLL(108, 109, 110, 111, 124, 125, 126, 127, 224)
                 "v_add_u32 %[ad], 128, %[ad]\n\ts_sub_u32 %[nq], %[nq], 8\n\ts_cmp_gt_u32 %[nq], 8\n\ts_cbranch_scc1 .Lt_%=\n"
                 ".Ld_%=:\n\t"      // the drain: 1..8 quads are left, all of them requested; it ends behind any quad
                 BF_L_DRAIN(96, 97, 98, 99, 112, 113, 114, 115, 6, 1) BF_L_DONE(2) BF_L_DRAIN(100, 101, 102, 103, 116, 117, 118, 119, 4, 3) BF_L_DONE(4)
                 BF_L_DRAIN(104, 105, 106, 107, 120, 121, 122, 123, 2, 5) BF_L_DONE(6) BF_L_DRAIN(108, 109, 110, 111, 124, 125, 126, 127, 0, 7)
                 ".Le_%=:\n\ts_waitcnt lgkmcnt(0)"      // (an early end: the reads beyond it land before the registers are anyone else's)
                 : [s] "+v"(sum), [ad] "+v"(ad), [nq] "+s"(quads)
                 :
                 : "memory", "scc", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111",
                   "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
    return sum;
}
#undef BF_L_ADD4
#undef BF_L_READ
#undef BF_L_ROLL
#undef BF_L_DONE
#undef BF_L_DRAIN

namespace copies {

// ==================================================================================================
// Two frames per workgroup on rows of CELLS (lerp, N <= 256, a multiple of 32 mics).
//
// das_pair2_kernel keeps four rows per mic -- samples and differences, each in two shifted copies -- because its 16-byte reads
// bring two samples and must be aligned at every delay.  Here a mic is ONE row of 16-byte cells, one per sample:
//     cell i = (s f0[i], s f1[i], D f0[i], D f1[i]),   D[i] = s[i+1] - s[i]
// A ds_read_b128 of a cell is aligned at every delay, so there is no shifted copy: a mic takes 4,992 bytes instead of 9,984, the same
// LDS holds 32 mic slots, and a half is 16 mics -- half the staging stores per mic, each of them a whole KiB of contiguous cells
// (conflict-free, where a lane's 32 contiguous bytes of an interleaved row made every store of das_pair2_kernel a two-way conflict),
// and half the barriers.
//   * lane l owns samples l, 64 + l, 128 + l, 192 + l: a (re)load is four reads of 1 KiB contiguous each, at v120 and 1, 2, 3 KiB on;
//   * v[96:97] is (frame 0, frame 1) of sample l, v[98:99] its difference, and so on to v[110:111]: the packed operations are the
//     same 8 per direction step, fma(h, D, s) as the reference contracts it;
//   * one wave stages one mic of a half: eight 4-byte loads a half ahead (lane l: s f[l + 64 q]), the differences from the next lane
//     (lane 63: lane 0 of the next register), four stores of whole cells;
//   * a parked half row of the power pass is in k order as it is stored (add_in_order_linear above).
// The group loop, the ladder, the statements S1 / S2 with their markers, the entry rotation and the power pass are das_pair2_kernel's.
// (CellGeo: das_geometry.h)

#define BF_C_ACC(n, j) [a##n##0] "+v"(acc[j][0]), [a##n##1] "+v"(acc[j][1]), [a##n##2] "+v"(acc[j][2]), [a##n##3] "+v"(acc[j][3])
#define BF_C_READ                                                                                   \
    "ds_read_b128 v[96:99], v120\n\tds_read_b128 v[100:103], v120 offset:1024\n\t"                   \
    "ds_read_b128 v[104:107], v120 offset:2048\n\tds_read_b128 v[108:111], v120 offset:3072\n\ts_waitcnt lgkmcnt(0)\n\t"
#define BF_C_STEP(n, h, mods)                                                                       \
    "v_pk_fma_f32 v[112:113], %[" #h "], v[98:99], v[96:97] " mods "\n\tv_pk_fma_f32 v[114:115], %[" #h "], v[102:103], v[100:101] " mods "\n\t" \
    "v_pk_fma_f32 v[116:117], %[" #h "], v[106:107], v[104:105] " mods "\n\tv_pk_fma_f32 v[118:119], %[" #h "], v[110:111], v[108:109] " mods "\n\t" \
    "v_pk_add_f32 %[a" #n "0], %[a" #n "0], v[112:113]\n\tv_pk_add_f32 %[a" #n "1], %[a" #n "1], v[114:115]\n\t" \
    "v_pk_add_f32 %[a" #n "2], %[a" #n "2], v[116:117]\n\tv_pk_add_f32 %[a" #n "3], %[a" #n "3], v[118:119]\n\t"
// A mic's first reads with direction step 0 behind them, each half of the step waiting only for its own reads (LDS returns in order;
// a counted wait bounds the outstanding operations of any kind, hence the outstanding reads).
#define BF_C_FIRST(h, mods)                                                                         \
    "ds_read_b128 v[96:99], v120\n\tds_read_b128 v[100:103], v120 offset:1024\n\t"                   \
    "ds_read_b128 v[104:107], v120 offset:2048\n\tds_read_b128 v[108:111], v120 offset:3072\n\ts_waitcnt lgkmcnt(2)\n\t" \
    "v_pk_fma_f32 v[112:113], %[" #h "], v[98:99], v[96:97] " mods "\n\tv_pk_fma_f32 v[114:115], %[" #h "], v[102:103], v[100:101] " mods "\n\t" \
    "v_pk_add_f32 %[a00], %[a00], v[112:113]\n\tv_pk_add_f32 %[a01], %[a01], v[114:115]\n\ts_waitcnt lgkmcnt(0)\n\t" \
    "v_pk_fma_f32 v[116:117], %[" #h "], v[106:107], v[104:105] " mods "\n\tv_pk_fma_f32 v[118:119], %[" #h "], v[110:111], v[108:109] " mods "\n\t" \
    "v_pk_add_f32 %[a02], %[a02], v[116:117]\n\tv_pk_add_f32 %[a03], %[a03], v[118:119]\n\t"
#define BF_C_EVEN "op_sel_hi:[0,1,1]"
#define BF_C_ODD "op_sel:[1,0,0] op_sel_hi:[1,1,1]"
#define BF_C_CHECK(n, ep, ec) "s_cmp_lg_u32 %[" #ec "], %[" #ep "]\n\ts_cbranch_scc1 .Lr" #n "_%=\n.Lb" #n "_%=:\n\t"
#define BF_C_STUB(n, ec) ".Lr" #n "_%=:\n\tv_add_u32 v120, %[" #ec "], %[lb]\n\t" BF_C_READ "s_branch .Lb" #n "_%=\n"
#define BF_C_CLOB "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", \
                  "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120"

// S1: a mic's first cells, read in place, and direction step 0
// lerp_and_sum.c:50-56  out[k] += s[i] + h * (s[i+1] - s[i]),  i = k - p - 1   (gcc contracts it into one fma)
__device__ __forceinline__ void cells_first(f32x2 (&acc)[8][4], int e0, unsigned long long h01, int lbase)
{
    asm volatile("v_add_u32 v120, %[e0], %[lb]\n\t" BF_C_FIRST(h01, BF_C_EVEN) ";BF_S1_END"
                 : BF_C_ACC(0, 0) : [e0] "s"(e0), [h01] "s"(h01), [lb] "v"(lbase) : BF_C_CLOB);
}
// S2: direction steps 1..7, each behind the test of its LDS offset against the previous step's
__device__ __forceinline__ void cells_rest(f32x2 (&acc)[8][4], const int (&e)[8], const unsigned long long (&hp)[4], int lbase)
{
    asm volatile(";BF_S2_BEGIN\n\t"
                 BF_C_CHECK(1, e0, e1) BF_C_STEP(1, h01, BF_C_ODD) BF_C_CHECK(2, e1, e2) BF_C_STEP(2, h23, BF_C_EVEN)
                 BF_C_CHECK(3, e2, e3) BF_C_STEP(3, h23, BF_C_ODD) BF_C_CHECK(4, e3, e4) BF_C_STEP(4, h45, BF_C_EVEN)
                 BF_C_CHECK(5, e4, e5) BF_C_STEP(5, h45, BF_C_ODD) BF_C_CHECK(6, e5, e6) BF_C_STEP(6, h67, BF_C_EVEN)
                 BF_C_CHECK(7, e6, e7) BF_C_STEP(7, h67, BF_C_ODD)
                 ".subsection 1\n" BF_C_STUB(1, e1) BF_C_STUB(2, e2) BF_C_STUB(3, e3) BF_C_STUB(4, e4) BF_C_STUB(5, e5) BF_C_STUB(6, e6) BF_C_STUB(7, e7)
                 "\t.subsection 0"
                 : BF_C_ACC(1, 1), BF_C_ACC(2, 2), BF_C_ACC(3, 3), BF_C_ACC(4, 4), BF_C_ACC(5, 5), BF_C_ACC(6, 6), BF_C_ACC(7, 7)
                 : [e0] "s"(e[0]), [e1] "s"(e[1]), [e2] "s"(e[2]), [e3] "s"(e[3]), [e4] "s"(e[4]), [e5] "s"(e[5]), [e6] "s"(e[6]), [e7] "s"(e[7]), [lb] "v"(lbase),
                   [h01] "s"(hp[0]), [h23] "s"(hp[1]), [h45] "s"(hp[2]), [h67] "s"(hp[3])
                 : "scc", BF_C_CLOB);
}
#undef BF_C_ACC
#undef BF_C_READ
#undef BF_C_FIRST
#undef BF_C_STEP
#undef BF_C_EVEN
#undef BF_C_ODD
#undef BF_C_CHECK
#undef BF_C_STUB
#undef BF_C_CLOB

template <int ALGO, int HC>
__global__ void __launch_bounds__(1024, 4) das_pair2_cells_kernel(BF_TABLE_PARAMS, KArgs a)
{
    static_assert(ALGO == ALGO_LERP, "das_pair2_cells_kernel: lerp (pad runs das_pair_kernel)");
    using G = CellGeo;
    static_assert(HC == G::kHalf && (HC == 16 || HC == 8), "one wave per mic and half, or (HC = 8, the measuring aid) two");
    constexpr int LEAD = G::kLead, W = 16, DW = 8, kGroup = DW * W, kParkHalf = Geo<1>::kParkHalf;
    constexpr int QW = HC / 4;                                  // registers per frame a wave stages: all four, or (HC = 8) the two of its part
    static_assert(2 * kGroup * kParkHalf <= Pair2Geo::kMc * Pair2Geo::kSlot && G::kMc * G::kSlot <= Pair2Geo::kMc * Pair2Geo::kSlot,
                  "both frames' parked half rows and the rows fit the LDS image of the family (the plan's lds_bytes)");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kWave - 1);               // (set-up only: inside the group loop lane_id() recomputes it, a register less to carry through the sweep)
    auto lane_id = []() -> int {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int tile, fpair;
    tile_and_frame(a, &tile, &fpair);
    const int f0 = 2 * fpair;
    const bool two = f0 + 1 < a.n_frames;                      // an odd frame count: the last workgroup row computes its frame twice
    const int f1 = two ? f0 + 1 : f0;
    const int tile_begin = a.dir_begin + tile * a.tile_dirs;
    if (tile_begin >= a.dir_end) return;
    const int tile_end = min(tile_begin + a.tile_dirs, a.dir_end);
    const int M = a.n_mics, N = a.n_samples;                   // M % (2 HC) == 0, N % 4 == 0, 128 < N <= 256 (plan_das, launch_pair_cells)
    const int n_half = M / HC;
    const float* __restrict__ sig0 = signals + (size_t)f0 * a.m_total * N;
    const float* __restrict__ sig1 = signals + (size_t)f1 * a.m_total * N;
    float* __restrict__ img0 = images + (size_t)f0 * a.image_stride;
    float* __restrict__ img1 = images + (size_t)f1 * a.image_stride;
    const int32_t* __restrict__ dig = reinterpret_cast<const int32_t*>(taps);   // the digest rides in the unused `taps` slot

    // (HC = 8, built with -DBF_CELLS_HC=8 to tell the bytes' share of the gain from the barriers': halves of 8 mics in 16 slots, waves w and w + 8
    //  share mic w & 7 -- part 0 stages samples 0..127, part 1 the rest, two registers per frame and two stores each; the ladder at mics 2, 4, 6)
    const int my_mic = HC == 16 ? wave : (wave & (HC - 1)), part = HC == 16 ? 0 : wave / HC;
    // Staging: wave w stages mic w of every half, both frames.  Straight-line code: the row base from the mic id (a scalar, loaded a
    // half ahead), eight loads through a scalar base and a 32-bit lane offset (das_pair2_kernel says why), the differences, four stores.
    constexpr unsigned kHalfBytes = HC * G::kSlot * 4;          // from a row of half 0 to the same row of half 1
    const bool full = N == 256;                                 // every lane has a sample in every register (wave-uniform, once per workgroup)
    const unsigned row_bytes = 4u * (unsigned)N, hoff_end = (unsigned)n_half * (HC * 4u);
    unsigned voff = 4u * (unsigned)lane;
    const char* mic_ids = reinterpret_cast<const char*>(mics + my_mic);
    unsigned hoff = 0;                                          // the half the next fetch reads (byte offset into mic_ids) ...
    int mic_a = *reinterpret_cast<const int32_t*>(mic_ids);     // ... and its mic id: a scalar load, consumed half a sweep later
    struct Staged { float s[2][QW]; float seam[2]; };           // [frame][q]: sample lane + 64 q (HC = 8: + 128 part, and the sample behind the wave's last)
    auto fetch_next = [&]() -> Staged {
        const size_t row = (size_t)(unsigned)mic_a * row_bytes;
        const char* r0 = reinterpret_cast<const char*>(sig0) + row;
        const char* r1 = reinterpret_cast<const char*>(sig1) + row;
        asm volatile("" : "+v"(voff));                          // (opaque: or hipcc folds it back into hoisted 64-bit lane pointers)
        // samples 0..127 are in every row (N > 128); a lane beyond a short row reads the row's last sample instead, and `stage` zeroes
        // what it brought
        Staged st;
        if constexpr (HC == 8) {
            const unsigned pb = 512u * (unsigned)part;
            const unsigned o0 = min(voff + pb, row_bytes - 4u), o1 = min(voff + pb + 256u, row_bytes - 4u), os = min(pb + 512u, row_bytes - 4u);
            st.s[0][0] = *reinterpret_cast<const float*>(r0 + o0);
            st.s[1][0] = *reinterpret_cast<const float*>(r1 + o0);
            st.s[0][1] = *reinterpret_cast<const float*>(r0 + o1);
            st.s[1][1] = *reinterpret_cast<const float*>(r1 + o1);
            st.seam[0] = *reinterpret_cast<const float*>(r0 + os);      // s[128] for part 0; part 1: the row's last sample (D[255] = 0)
            st.seam[1] = *reinterpret_cast<const float*>(r1 + os);
        } else {
        const unsigned o2 = min(voff + 512u, row_bytes - 4u), o3 = min(voff + 768u, row_bytes - 4u);
        st.seam[0] = st.seam[1] = 0.f;
        st.s[0][0] = *reinterpret_cast<const float*>(r0 + voff);
        st.s[1][0] = *reinterpret_cast<const float*>(r1 + voff);
        st.s[0][1] = *reinterpret_cast<const float*>(r0 + voff + 256u);
        st.s[1][1] = *reinterpret_cast<const float*>(r1 + voff + 256u);
        st.s[0][2] = *reinterpret_cast<const float*>(r0 + o2);
        st.s[1][2] = *reinterpret_cast<const float*>(r1 + o2);
        st.s[0][3] = *reinterpret_cast<const float*>(r0 + o3);
        st.s[1][3] = *reinterpret_cast<const float*>(r1 + o3);
        }
        hoff = hoff + HC * 4u < hoff_end ? hoff + HC * 4u : 0u;  // (after the last half: half 0 again, the next group's first -- or for nothing)
        mic_a = *reinterpret_cast<const int32_t*>(mic_ids + hoff);
        return st;
    };
    const int lb = 16 * lane + (int)(unsigned)(size_t)((__attribute__((address_space(3))) char*)lds);   // the sweep's lane base
    // this wave's row: lb + row0 is the lane's cell of samples 0..63 in half 0, lb + row1 in half 1; samples 64 q on are q KiB further
    const int row0 = (my_mic * G::kSlot + 4 * LEAD) * 4 + part * (QW * 1024), row1 = row0 + (int)kHalfBytes;
    auto stage = [&](int row, const Staged& st) {
        typedef __attribute__((address_space(3))) f32x4 lds_cell;
        lds_cell* cell = reinterpret_cast<lds_cell*>((uintptr_t)(unsigned)(lb + row));
        float s[2][4], d[2][4];
        if constexpr (HC == 8) {
            const int k0 = 128 * part + lane_id();               // the lane's sample of its first register
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int q = 0; q < QW; ++q) s[f][q] = (full || k0 + 64 * q < N) ? st.s[f][q] : 0.f;
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int q = 0; q < QW; ++q) {
                    const int cur = __float_as_int(s[f][q]);
                    const int old = q + 1 < QW ? __builtin_amdgcn_readlane(__float_as_int(s[f][q + 1]), 0) : __float_as_int(st.seam[f]);
                    const float dq = __int_as_float(__builtin_amdgcn_update_dpp(old, cur, 0x130, 0xf, 0xf, false)) - s[f][q];
                    d[f][q] = (full || k0 + 64 * q + 1 < N) ? dq : 0.f;
                }
#pragma unroll
            for (int q = 0; q < QW; ++q) cell[64 * q] = f32x4{s[0][q], s[1][q], d[0][q], d[1][q]};
            return;
        } else {
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int q = 0; q < 4; ++q) s[f][q] = st.s[f][q];
        if (!full) {
            asm volatile(";BF_STAGE_MASKED");
            const int l = lane_id();
#pragma unroll
            for (int f = 0; f < 2; ++f) { s[f][2] = 128 + l < N ? s[f][2] : 0.f; s[f][3] = 192 + l < N ? s[f][3] : 0.f; }
        }
        // D[i] = s[i+1] - s[i], the reference's own subtraction (lerp_and_sum.c:54).  s[i+1] is the next lane's sample (DPP wave_shl:1); lane
        // 63 has no next lane and keeps the move's old value: lane 0 of the next register, and for the last register its own sample,
        // which stores D[255] = 0 (D[N-1] is never read).  Builtins: the compiler places the hazards of the scalar and of the DPP operand.
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cur = __float_as_int(s[f][q]);
                const int old = q < 3 ? __builtin_amdgcn_readlane(__float_as_int(s[f][q + 1]), 0) : cur;
                d[f][q] = __int_as_float(__builtin_amdgcn_update_dpp(old, cur, 0x130, 0xf, 0xf, false)) - s[f][q];
            }
        if (!full) {
            asm volatile(";BF_STAGE_MASKED");
            const int l = lane_id();
#pragma unroll
            for (int f = 0; f < 2; ++f) { d[f][2] = 129 + l < N ? d[f][2] : 0.f; d[f][3] = 193 + l < N ? d[f][3] : 0.f; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) cell[64 * q] = f32x4{s[0][q], s[1][q], d[0][q], d[1][q]};
        }
    };
    // the zero prefix (56 cells per row) of this wave's row, in both halves: only the parked rows of the power pass overwrite it, so a
    // group restores it once, before its first half is staged
    auto wipe_prefix = [&]() {
        static_assert(LEAD <= kWave, "one lane per prefix cell");
        const int l = lane_id();
        if (l < LEAD && (HC == 16 || part == 0)) {
            float4* q = reinterpret_cast<float4*>(lds + my_mic * G::kSlot) + l;
            q[0] = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(reinterpret_cast<char*>(q) + kHalfBytes) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    Staged st = fetch_next();

    for (int g0 = tile_begin; g0 < tile_end; g0 += kGroup) {
        f32x2 acc[DW][4];                                       // (frame 0, frame 1) of samples l, 64+l, 128+l, 192+l
#pragma unroll
        for (int j = 0; j < DW; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[j][q] = f32x2{0.0f, 0.0f};

        __syncthreads();   // the previous group's parked rows have been summed
        wipe_prefix();
        stage(row0, st);
        st = fetch_next();                                      // half 1
        __syncthreads();

        const int dw0 = g0 + wave * DW;                         // wave-uniform
        const bool busy = dw0 < tile_end;
        const size_t grp = busy ? (size_t)(dw0 - a.dir_begin) / DW : 0;
        const int32_t* __restrict__ etg = dig + grp * M * DW;
        const float* __restrict__ htg = reinterpret_cast<const float*>(dig) + a.digest_h_off + grp * M * DW;
        int row_next = row1;                                    // where the next half is staged: halves alternate
        for (int h = 0; h < n_half; ++h) {
            // The priority ladder of das_pair2_kernel (see there) on halves of 16 mics: 3 from the barrier on (the staging included), 2,
            // 1, 0 at mics 4, 8, 12.  One scalar instruction where it changes, before a mic's first statement: never while the
            // hard-wired cells are in flight.
            asm volatile("s_setprio 3");
            asm volatile(";BF_STAGE_BEGIN");                    // (;BF_STAGE_*: path markers for scripts/dev/pair2_instruction_budget.py, comments in the assembly)
            if (h + 1 < n_half) {
                stage(row_next, st);                            // into the half whose sweeps ended before the last barrier
                row_next = row0 + row1 - row_next;
                st = fetch_next();                              // staged an iteration from now: half h + 2, or the next group's first half
            }
            asm volatile(";BF_STAGE_END");
            if (busy) {
                // one table base per half: the sixteen mics' entries and weights are immediate offsets off it
                const int32_t* __restrict__ et = etg + (size_t)h * (HC * DW);
                const float* __restrict__ ht = htg + (size_t)h * (HC * DW);
                struct Entries { int e[DW]; unsigned long long hp[DW / 2]; };
                auto request = [&](Entries& t, int m) {
                    // (reads past the half's last mic stay inside the slack-padded table and are dropped)
#pragma unroll
                    for (int j = 0; j < DW; ++j) t.e[j] = et[m * DW + j];
#pragma unroll
                    for (int j = 0; j < DW / 2; ++j) t.hp[j] = *reinterpret_cast<const unsigned long long*>(ht + m * DW + 2 * j);
                };
                Entries E[3];
                request(E[0], 0);
                request(E[1], 1);
                auto mic = [&](int m, auto kc) {
                    constexpr int K = decltype(kc)::value, K2 = (K + 2) % 3;
                    const Entries& cur = E[K];
                    cells_first(acc, cur.e[0], cur.hp[0], lb);
                    request(E[K2], m + 2);      // after the first statement's wait, so that it does not sit on these loads
                    cells_rest(acc, cur.e, cur.hp, lb);
                };
                using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
                if constexpr (HC == 8) {
                    mic(0, I0{}); mic(1, I1{});
                    asm volatile("s_setprio 2");
                    mic(2, I2{}); mic(3, I0{});
                    asm volatile("s_setprio 1");
                    mic(4, I1{}); mic(5, I2{});
                    asm volatile("s_setprio 0");
                    mic(6, I0{}); mic(7, I1{});
                } else {
                mic(0, I0{}); mic(1, I1{}); mic(2, I2{}); mic(3, I0{});
                asm volatile("s_setprio 2");
                mic(4, I1{}); mic(5, I2{}); mic(6, I0{}); mic(7, I1{});
                asm volatile("s_setprio 1");
                mic(8, I2{}); mic(9, I0{}); mic(10, I1{}); mic(11, I2{});
                asm volatile("s_setprio 0");
                mic(12, I0{}); mic(13, I1{}); mic(14, I2{}); mic(15, I0{});
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);             // the entries requested past the half's end have landed (and are dropped)
            }
            __syncthreads();   // half h is free, half h + 1 is staged
        }
        asm volatile("s_setprio 0");    // (a wave without directions of its own kept 3 from barrier to barrier, where it issues next to nothing)

        // ---- k-ordered mean power (pad_and_sum.c:120-128), both frames at once, one HALF of the samples at a time: das_pair2_kernel's
        // pass (rounds, barriers, waves, parking store; the whole pass once per way of dividing, behind the real branch on a.n_is_pow2 --
        // see there).  A lane holds samples l and 64 + l of a half, so the same two-dword store leaves the parked row in k order.
        auto power_pass = [&](auto mul_c) __attribute__((always_inline)) {
        constexpr bool MUL = decltype(mul_c)::value;
        if constexpr (MUL) asm volatile(";BF_POWER_POW2"); else asm volatile(";BF_POWER_DIV");      // (;BF_POWER_*: markers for scripts/dev/pair2_instruction_budget.py, comments in the assembly)
        int wv = wave;
        asm volatile("" : "+s"(wv));
        float sum = 0.0f;               // of this lane's (frame, direction), carried from round 0 to round 1 (waves 0..3)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1) __syncthreads();        // round 0's rows have been summed
            {
                // out[k] /= n and the squares of direction j's half, both frames at once: a register pair is one sample of frames 0 and 1,
                // and v_pk_mul_f32 rounds each component as v_mul_f32 does
                auto squares = [&](int j, f32x2& s0, f32x2& s1) __attribute__((always_inline)) {
                    if constexpr (MUL) {
                        const f32x2 inv2 = {a.inv_n, a.inv_n};
                        s0 = acc[j][2 * r] * inv2; s1 = acc[j][2 * r + 1] * inv2;
                    } else {
                        float o0, o1, o2, o3;
                        mic_mean<false>(acc[j][2 * r].x, acc[j][2 * r + 1].x, acc[j][2 * r].y, acc[j][2 * r + 1].y, M, a.inv_n, o0, o1, o2, o3);
                        s0 = f32x2{o0, o2}; s1 = f32x2{o1, o3};
                    }
                    s0 = s0 * s0; s1 = s1 * s1;
                };
                // lane l holds samples l and 64 + l of the half, one frame's two floats in two register pairs.  ds_write2_b32 stores
                // them from where they are, 64 dwords apart: the lanes of either store cover 64 banks, and the row is in k order.
                static_assert(kParkHalf + 64 < 256, "a row and the next one off one address");
                const unsigned rows = (unsigned)(size_t)((__attribute__((address_space(3))) char*)lds) + (unsigned)((wv * DW) * kParkHalf + lane_id()) * 4u;
                auto park2 = [](unsigned ad, const f32x2& s0, const f32x2& s1, const f32x2& t0, const f32x2& t1, auto fc) __attribute__((always_inline)) {
                    constexpr bool F1 = decltype(fc)::value;
                    asm volatile("ds_write2_b32 %[ad], %[s0], %[s1] offset1:64\n\tds_write2_b32 %[ad], %[t0], %[t1] offset0:%[o0] offset1:%[o1]"
                                 : : [ad] "v"(ad), [s0] "v"(F1 ? s0.y : s0.x), [s1] "v"(F1 ? s1.y : s1.x), [t0] "v"(F1 ? t0.y : t0.x), [t1] "v"(F1 ? t1.y : t1.x),
                                     [o0] "n"(kParkHalf), [o1] "n"(kParkHalf + 64) : "memory");
                };
#pragma unroll
                for (int j = 0; j < DW; j += 2) {
                    f32x2 s0, s1, t0, t1;
                    squares(j, s0, s1);
                    squares(j + 1, t0, t1);
                    const unsigned ad = rows + (unsigned)j * (kParkHalf * 4u);
                    park2(ad, s0, s1, t0, t1, std::false_type{});
                    park2(ad + kGroup * kParkHalf * 4u, s0, s1, t0, t1, std::true_type{});
                }
            }
            __syncthreads();
            if (wv < 2 * (kGroup / kWave)) {
                const int lane_o = lane_id();                 // (recomputed: keeps the per-lane row address out of the registers the sweep needs)
                const int g = (wv & 1) * kWave + lane_o;    // this lane's direction of the group; its parked row is wave * 64 + lane: frame 1's rows follow frame 0's
                const int d = g0 + g;
                if (d < tile_end && (wv < kGroup / kWave || two)) {
                    const unsigned row = (unsigned)(size_t)((__attribute__((address_space(3))) char*)lds) + (unsigned)(wv * kWave + lane_o) * (kParkHalf * 4u);
                    sum = add_in_order_linear(row, r == 0 ? 32 : (N - 128) >> 2, sum);      // round 1 stops at N
                    if (r == 1) {
                        // the direction swept at position d - dir_begin (wave-uniform branch; one 4-byte load in the four summing waves)
                        const int dd = a.digest_o_off != 0 ? dig[a.digest_o_off + (d - a.dir_begin)] : d;
                        (wv < kGroup / kWave ? img0 : img1)[dd - a.image_origin] = sum / (float)N;
                    }
                }
            }
        }
        asm volatile(";BF_POWER_END");
        };
        if (__builtin_expect(a.n_is_pow2, 1)) power_pass(std::true_type{}); else power_pass(std::false_type{});
    }
}

}  // namespace copies

}  // namespace

hipError_t launch_pair_cells(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream)
{
    using G = copies::CellGeo;
    if (L.algo != ALGO_LERP || plan.family != DAS_PAIR_CELLS || L.tab.digest_direct || plan.waves != copies::kWaves ||
        plan.lead != G::kLead || (L.n_mics % G::kMc) != 0 || (L.n_samples % 4) != 0 || L.n_samples <= 128 || L.n_samples > 256 ||
        plan.lds_bytes < (size_t)copies::Pair2Geo::kMc * copies::Pair2Geo::kSlot * sizeof(float))     // the family's image: the rows and the parked rows fit it
        return hipErrorInvalidValue;
    static int cells_scratch = -1;
    const dim3 grid((unsigned)plan.n_tiles * (unsigned)((frames + 1) / 2));
    return launch_with_lds(copies::das_pair2_cells_kernel<ALGO_LERP, G::kHalf>, grid, dim3((unsigned)plan.waves * kWave), plan.lds_bytes, stream, &cells_scratch,
                           L.signals, L.images, L.mics, L.tab.whole, L.tab.frac, reinterpret_cast<const float*>(L.tab.digest), make_args(L, plan));
}

}  // namespace bf
