// das_pair.hip -- the pad / lerp sweep with two frames per workgroup: copies::das_pair_kernel (pad) and das_pair2_kernel (lerp),
// what the bench and every multi-frame caller at N <= 256 run.  das_kernels.hip has the overview and the one-frame sweep
// (das_copies_kernel) these kernels grew out of.
#include "das_device.h"

namespace bf {

namespace {

namespace copies {

// ==================================================================================================
// Two frames per workgroup (pad, N <= 256, fixed row stride, mic count a multiple of 16, two or more frames; lerp runs
// das_pair2_kernel below).
//
// The sweep above is bound by the number of instructions a SIMD issues, and per (direction, mic) step only 2 of them (pad) are
// arithmetic: the rest -- table loads, the address, the offset tests, waits -- depends on the tables alone.  A wave that
// carries its eight directions through TWO frames pays that part once per 4 packed operations.
// Same layout as das_copies_kernel<pad, NSEG = 1, RS = kRs, W = 16> (two shifted copies), with the two frames' rows of a mic
// next to each other: frame 1's quads sit kFoff bytes after frame 0's, an immediate offset off the same address.  16 mics x 2
// frames per chunk; the 64 accumulator registers leave no room for quads in flight across a mic, so a mic's first quads are
// read (and waited for) in place -- the other three waves of the SIMD cover that.
// Mic order and operation order per frame are those of the one-frame kernel: bit-identical maps.
// (PairGeo: das_geometry.h)

#define BF_P_ACC(n, j, f) [a##n##0] "+v"(acc[j][f][0]), [a##n##1] "+v"(acc[j][f][1])
// two direction steps x two frames; a0/a1 = step A frame 0/1, a2/a3 = step B frame 0/1
#define BF_P_PAD_STEP(n0, n1)                                                                             \
    "v_pk_add_f32 %[a" #n0 "0], %[a" #n0 "0], %[s0l]\n\tv_pk_add_f32 %[a" #n0 "1], %[a" #n0 "1], %[s0h]\n\t" \
    "v_pk_add_f32 %[a" #n1 "0], %[a" #n1 "0], %[s1l]\n\tv_pk_add_f32 %[a" #n1 "1], %[a" #n1 "1], %[s1h]\n\t"
#define BF_P_PAD_READ                                                                                     \
    "ds_read_b64 %[s0l], %[ad] offset:0\n\tds_read_b64 %[s0h], %[ad] offset:8\n\t"                         \
    "ds_read_b64 %[s1l], %[ad] offset:%[f0]\n\tds_read_b64 %[s1h], %[ad] offset:%[f8]\n\t"                 \
    "s_waitcnt lgkmcnt(0)\n\t"
#define BF_P_ADDR(e) "v_add_u32 %[ad], %[" #e "], %[lb]\n\t"
#define BF_P_CHECK(n, ep, ec) "s_cmp_lg_u32 %[" #ec "], %[" #ep "]\n\ts_cbranch_scc1 .Lr" #n "_%=\n.Lb" #n "_%=:\n\t"
#define BF_P_STUB(n, ec, READ) ".Lr" #n "_%=:\n\t" BF_P_ADDR(ec) READ "s_branch .Lb" #n "_%=\n"

// Direction steps 0 and 1 of a mic for both frames: the mic's first quads are read in place (offset eb) before step 0, step 1
// tests eb -> ec first.
__device__ __forceinline__ void pair_pad_first(f32x2 (&acc)[8][2][2], Quad& S0, Quad& S1, int eb, int ec, int lbase)
{
    using G = PairGeo;
    int ad;
    // pad_and_sum.c:41-47   out[k] += s[k - p]
    // (step 0: each frame's adds wait only for that frame's two reads -- LDS returns in order)
    asm volatile(BF_P_ADDR(eb)
                 "ds_read_b64 %[s0l], %[ad] offset:0\n\tds_read_b64 %[s0h], %[ad] offset:8\n\t"
                 "ds_read_b64 %[s1l], %[ad] offset:%[f0]\n\tds_read_b64 %[s1h], %[ad] offset:%[f8]\n\ts_waitcnt lgkmcnt(2)\n\t"
                 "v_pk_add_f32 %[a00], %[a00], %[s0l]\n\tv_pk_add_f32 %[a01], %[a01], %[s0h]\n\ts_waitcnt lgkmcnt(0)\n\t"
                 "v_pk_add_f32 %[a10], %[a10], %[s1l]\n\tv_pk_add_f32 %[a11], %[a11], %[s1h]\n\t"
                 BF_P_CHECK(1, eb, ec) BF_P_PAD_STEP(2, 3)
                 ".subsection 1\n" BF_P_STUB(1, ec, BF_P_PAD_READ) "\t.subsection 0"
                 // (the quads are pure outputs here: as in-out operands they are carried around the mic loop -- and copied at its back-edge)
                 : BF_P_ACC(0, 0, 0), BF_P_ACC(1, 0, 1), BF_P_ACC(2, 1, 0), BF_P_ACC(3, 1, 1), [s0l] "=&v"(S0.lo), [s0h] "=&v"(S0.hi),
                   [s1l] "=&v"(S1.lo), [s1h] "=&v"(S1.hi), [ad] "=&v"(ad)
                 : [eb] "s"(eb), [ec] "s"(ec), [lb] "v"(lbase), [f0] "n"(G::kFoff), [f8] "n"(G::kFoff + 8) : "scc");
}

// pad, direction steps 2..7 of a mic for both frames as ONE statement (between two statements the hazard recogniser puts an s_nop:
// three issue slots per mic with one statement per pair of steps).
__device__ __forceinline__ void pair_pad_rest(f32x2 (&acc)[8][2][2], Quad& S0, Quad& S1, const int (&e)[8], int lbase)
{
    using G = PairGeo;
    int ad;
#define BF_P_ACC2(n, j) [a##n##0] "+v"(acc[j][0][0]), [a##n##1] "+v"(acc[j][0][1]), [b##n##0] "+v"(acc[j][1][0]), [b##n##1] "+v"(acc[j][1][1])
#define BF_P_PAD1(n) "v_pk_add_f32 %[a" #n "0], %[a" #n "0], %[s0l]\n\tv_pk_add_f32 %[a" #n "1], %[a" #n "1], %[s0h]\n\t" \
                     "v_pk_add_f32 %[b" #n "0], %[b" #n "0], %[s1l]\n\tv_pk_add_f32 %[b" #n "1], %[b" #n "1], %[s1h]\n\t"
    asm volatile(BF_P_CHECK(2, e1, e2) BF_P_PAD1(2) BF_P_CHECK(3, e2, e3) BF_P_PAD1(3) BF_P_CHECK(4, e3, e4) BF_P_PAD1(4)
                 BF_P_CHECK(5, e4, e5) BF_P_PAD1(5) BF_P_CHECK(6, e5, e6) BF_P_PAD1(6) BF_P_CHECK(7, e6, e7) BF_P_PAD1(7)
                 ".subsection 1\n" BF_P_STUB(2, e2, BF_P_PAD_READ) BF_P_STUB(3, e3, BF_P_PAD_READ) BF_P_STUB(4, e4, BF_P_PAD_READ)
                 BF_P_STUB(5, e5, BF_P_PAD_READ) BF_P_STUB(6, e6, BF_P_PAD_READ) BF_P_STUB(7, e7, BF_P_PAD_READ) "\t.subsection 0"
                 : BF_P_ACC2(2, 2), BF_P_ACC2(3, 3), BF_P_ACC2(4, 4), BF_P_ACC2(5, 5), BF_P_ACC2(6, 6), BF_P_ACC2(7, 7),
                   [s0l] "+v"(S0.lo), [s0h] "+v"(S0.hi), [s1l] "+v"(S1.lo), [s1h] "+v"(S1.hi), [ad] "=&v"(ad)
                 : [e1] "s"(e[1]), [e2] "s"(e[2]), [e3] "s"(e[3]), [e4] "s"(e[4]), [e5] "s"(e[5]), [e6] "s"(e[6]), [e7] "s"(e[7]), [lb] "v"(lbase),
                   [f0] "n"(G::kFoff), [f8] "n"(G::kFoff + 8)
                 : "scc");
#undef BF_P_ACC2
#undef BF_P_PAD1
}

// Profiling build only (-DBF_STAMPS, scripts/dev/phase_stamps.py): every wave sums the time it spends in each phase of
// das_pair_kernel / das_pair2_kernel (s_memtime at the phase boundaries, which are barrier neighbours anyway) and adds the totals to
// g_stamps[phase] when its workgroup ends.  BF_STAMP(k) closes the phase that was running and charges it to slot k:
//   0 sweep  1 wait (chunk free)  2 staging  3 wait (chunk staged)  4 wait (power: rows free)  5 parking  6 wait (rows parked)  7 ordered sum
#ifdef BF_STAMPS
__device__ unsigned long long g_stamps[64 * 16];         // (sums over all waves, in 64 replicas picked by workgroup id: nine atomics per wave on one
                                                         //  line would make the flush longer than the kernel)
#define BF_STAMP_DECL unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long st_prev = __builtin_amdgcn_s_memtime();
#define BF_STAMP(k) do { const unsigned long long st_now = __builtin_amdgcn_s_memtime(); st_acc[k] += st_now - st_prev; st_prev = st_now; } while (0)
// Beside the totals, one row per wave index of the workgroup (16 rows of 8): its sweep (0) and its wait for the staged chunk (1),
// summed over the workgroups, and how often it ran on SIMD 0..3 (2..5; HW_ID[5:4], read once: a wave stays where it was placed).
// g_wave_simd keeps the SIMDs of the 16 waves of one workgroup side by side (0x80 | SIMD; the last launch's workgroups, 4096 of
// them at the most): which wave indices share a SIMD is read off these.
__device__ unsigned long long g_wave_stamps[64 * 16 * 8];
__device__ unsigned char g_wave_simd[4096 * 16];
#define BF_STAMP_FLUSH do { if (lane == 0) { unsigned long long* gs = g_stamps + 16 * (blockIdx.x & 63); for (int i = 0; i < 8; ++i) atomicAdd(&gs[i], st_acc[i]); atomicAdd(&gs[8], 1ull); \
                            unsigned simd; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 4, 2)" : "=s"(simd)); \
                            unsigned long long* gw = g_wave_stamps + 128 * (blockIdx.x & 63) + 8 * (wave & 15); \
                            atomicAdd(&gw[0], st_acc[0]); atomicAdd(&gw[1], st_acc[3]); atomicAdd(&gw[2 + (simd & 3)], 1ull); \
                            g_wave_simd[16 * (blockIdx.x & 4095) + (wave & 15)] = (unsigned char)(0x80 | (simd & 3)); } } while (0)
#else
#define BF_STAMP_DECL
#define BF_STAMP(k)
#define BF_STAMP_FLUSH
#endif

template <int ALGO>   // (pad only: the parameter keeps the kernel's symbol, which the profiles and ISA checks name)
__global__ void __launch_bounds__(1024, 4) das_pair_kernel(BF_TABLE_PARAMS, KArgs a)
{
    static_assert(ALGO == ALGO_PAD, "das_pair_kernel: pad (lerp runs das_pair2_kernel)");
    using G = PairGeo;
    constexpr int C = G::kC, RS = G::kRs, LEAD = G::kLead, HC = G::kHalf, W = 16, DW = 8, kGroup = DW * W, kPark = Geo<1>::kPark;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int tile, fpair;
    tile_and_frame(a, &tile, &fpair);
    const int f0 = 2 * fpair;
    const bool two = f0 + 1 < a.n_frames;                      // an odd frame count: the last workgroup row computes its frame twice
    const int f1 = two ? f0 + 1 : f0;
    const int tile_begin = a.dir_begin + tile * a.tile_dirs;
    if (tile_begin >= a.dir_end) return;
    const int tile_end = min(tile_begin + a.tile_dirs, a.dir_end);
    const int M = a.n_mics, N = a.n_samples;                   // M % 16 == 0, N % 4 == 0, N <= 256 (plan_das)
    const int n_half = M / HC;                                  // half chunks of 8 mics
    const float* __restrict__ sig0 = signals + (size_t)f0 * a.m_total * N;
    const float* __restrict__ sig1 = signals + (size_t)f1 * a.m_total * N;
    float* __restrict__ img0 = images + (size_t)f0 * a.image_stride;
    float* __restrict__ img1 = images + (size_t)f1 * a.image_stride;
    const int32_t* __restrict__ dig = reinterpret_cast<const int32_t*>(taps);   // the digest rides in the unused `taps` slot

    // The LDS image is the 16-mic chunk the digest was built for (mic m -> slot m % 16), used as TWO halves of 8 mics: while
    // the waves sweep half h, each of them also writes its row of half h + 1 into the other half -- ONE barrier per 8 mics,
    // and the staging stores (slow: 13 cycles per ds_write_b128 and wave on the LDS store path) run under other waves' adds
    // instead of between two barriers with every SIMD idle.
    // This wave stages row `wave` of every half: mic (wave >> 1) of the half, frame (wave & 1).
    // Lane c holds half c's mic id (first 64 halves): the per-half prefetch is then one independent load.
    const int vmic = (lane < n_half) ? mics[lane * HC + (wave >> 1)] : 0;
    auto fetch = [&](int h) -> float4 {
        const int mic = (h < kWave) ? __builtin_amdgcn_readlane(vmic, h) : mics[h * HC + (wave >> 1)];
        const float* src = ((wave & 1) ? sig1 : sig0) + (size_t)mic * N;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * lane < N) v = *reinterpret_cast<const float4*>(src + 4 * lane);
        return v;
    };
    auto stage = [&](int h, const float4 v, bool wipe) {
        float* row0 = lds + (((h & 1) * W) + wave) * G::kSlot;  // slot (h & 1) * 8 + (wave >> 1), frame wave & 1
        const float py = dpp_prev(v.y), pz = dpp_prev(v.z), pw = dpp_prev(v.w);
        write_copies<C>(row0, RS, LEAD, lane, v, py, pz, pw);
        if (wipe) {
            // the zero prefix: nothing but the parked rows of the power pass ever overwrites it, so only a group's first
            // visit of a half restores it -- one store: lane -> (copy row lane / 14, quad lane % 14) of the C rows
            static_assert((LEAD >> 2) * C <= kWave, "one lane per prefix quad");
            constexpr int PQ = LEAD >> 2;
            if (lane < PQ * C) reinterpret_cast<float4*>(row0 + (lane / PQ) * RS)[lane % PQ] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    float4 st = fetch(0);
    const int lb = 16 * lane + (int)(unsigned)(size_t)((__attribute__((address_space(3))) char*)lds);
    BF_STAMP_DECL

    for (int g0 = tile_begin; g0 < tile_end; g0 += kGroup) {
        f32x2 acc[DW][2][2];
#pragma unroll
        for (int j = 0; j < DW; ++j)
#pragma unroll
            for (int f = 0; f < 2; ++f) { acc[j][f][0] = f32x2{0.0f, 0.0f}; acc[j][f][1] = f32x2{0.0f, 0.0f}; }

        BF_STAMP(7);
        __syncthreads();   // the previous group's parked rows have been summed
        BF_STAMP(1);
        stage(0, st, true);
        st = fetch(1);
        BF_STAMP(2);
        __syncthreads();
        BF_STAMP(3);

        for (int h = 0; h < n_half; ++h) {
            // the priority ladder of das_pair2_kernel (see there), on this kernel's trips of three mics: 3 from the barrier on, 1 behind
            // either trip (mics 3 and 6), 0 for the last two mics (-9.3 %)
            asm volatile("s_setprio 3");
            if (h + 1 < n_half) {
                stage(h + 1, st, h == 0);                       // into the half whose sweeps ended before the last barrier
                // request what is staged an iteration from now: half h + 2, or the next group's first half (the same rows)
                if (h + 2 < n_half) st = fetch(h + 2);
                else if (g0 + kGroup < tile_end) st = fetch(0);
                BF_STAMP(2);
            }
            const int dw0 = g0 + wave * DW;                     // wave-uniform
            if (dw0 < tile_end) {
                const size_t grp = (size_t)(dw0 - a.dir_begin) / DW;
                const int32_t* __restrict__ et = dig + (grp * M + (size_t)h * HC) * DW;
                struct Entries { int e[DW]; };
                auto request = [&](Entries& t, int m) {
                    // (reads past the half's last mic stay inside the slack-padded table and are dropped)
#pragma unroll
                    for (int j = 0; j < DW; ++j) t.e[j] = et[m * DW + j];
                };
                Entries E[3];
                Quad S0, S1;
                S0.lo = S0.hi = S1.lo = S1.hi = f32x2{0.0f, 0.0f};
                request(E[0], 0);
                request(E[1], 1);
                auto mic = [&](int m, auto kc) {
                    constexpr int K = decltype(kc)::value, K2 = (K + 2) % 3;
                    const Entries& cur = E[K];
                    pair_pad_first(acc, S0, S1, cur.e[0], cur.e[1], lb);
                    request(E[K2], m + 2);      // after the first statement's wait, so that it does not sit on these loads
                    pair_pad_rest(acc, S0, S1, cur.e, lb);
                };
                using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
                static_assert(HC == 8, "eight mics: two trips of three and two more");
#pragma unroll 1
                for (int t = 0; t < 2; ++t) {
                    mic(0, I0{}); mic(1, I1{}); mic(2, I2{});
                    et += 3 * DW;
                    asm volatile("s_setprio 1");
                }
                asm volatile("s_setprio 0");
                mic(0, I0{});
                mic(1, I1{});
            }
            BF_STAMP(0);       // sweep -> waiting for the others
            __syncthreads();   // half h is free, half h + 1 is staged
            BF_STAMP(h + 1 < n_half ? 3 : 4);
        }
        asm volatile("s_setprio 0");    // (a wave without directions of its own kept 3; every wave enters the power pass at 0)

        // ---- k-ordered mean power (pad_and_sum.c:120-128), one frame at a time: the 16 waves park the squared means of their
        // directions (row = direction; the rows alias the chunk buffer), then one direction per lane runs the sequential sum.
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            if (f == 1) {
                __syncthreads();        // frame 0's rows have been summed
                BF_STAMP(4);
            }
            auto park = [&](auto mul_c) {
#pragma unroll
                for (int j = 0; j < DW; ++j) {
                    float* row = lds + (wave * DW + j) * kPark;
                    const f32x2 a0 = acc[j][f][0], a1 = acc[j][f][1];
                    float o0, o1, o2, o3;
                    mic_mean<decltype(mul_c)::value>(a0.x, a0.y, a1.x, a1.y, M, a.inv_n, o0, o1, o2, o3);
                    reinterpret_cast<float4*>(row)[lane] = make_float4(o0 * o0, o1 * o1, o2 * o2, o3 * o3);
                }
            };
            if (__builtin_expect(a.n_is_pow2, 1)) park(std::true_type{}); else park(std::false_type{});
            BF_STAMP(5);                // -> waiting
            __syncthreads();
            BF_STAMP(6);                // -> ordered sum (two waves; the others go on to the next barrier)
            const int g = wave * kWave + lane;            // parked row of this lane
            const int d = g0 + g;
            if (g < kGroup && d < tile_end && (f == 0 || two)) {
                // the direction swept at position d - dir_begin (wave-uniform branch; one 4-byte load in the two summing waves)
                const int dd = a.digest_o_off != 0 ? dig[a.digest_o_off + (d - a.dir_begin)] : d;
                (f == 0 ? img0 : img1)[dd - a.image_origin] = row_mean_power<false>(lds + g * kPark, N);
            }
        }
    }
    BF_STAMP(7);
    BF_STAMP_FLUSH;
}
#undef BF_P_ACC
#undef BF_P_PAD_STEP
#undef BF_P_PAD_READ
#undef BF_P_ADDR
#undef BF_P_CHECK
#undef BF_P_STUB

// ==================================================================================================
// Two frames per workgroup, frames INTERLEAVED sample by sample in the LDS rows (lerp, N <= 256; das_pair_kernel's successor).
//
// Every instruction costs a SIMD a quad-cycle, so what is left to gain on the sweep is instruction count.  With the
// row of a mic holding (f0 s0, f1 s0, f0 s1, f1 s1, ..):
//   * one ds_read_b128 brings two samples of BOTH frames: a (re)load is 4 LDS instructions instead of 8, and with lane l owning
//     the sample pairs (2l, 2l+1) and (128+2l, 128+2l+1) every read covers 1 KiB of contiguous LDS (no bank conflicts; the
//     16-byte lane stride of ds_read_b64 pairs was a two-way conflict on every read);
//   * a register pair is (frame 0, frame 1) of one sample, so the packed operations are the same 8 per direction step, the
//     lerp weight still one scalar operand for both lanes;
//   * the quads live in HARD-WIRED registers v[96:111] (+ products v[112:119], address v120), named as clobbers: 16-byte reads
//     need 4-register tuples whose halves the packed operations address, which inline-asm operands cannot express.  A mic is
//     two statements -- S1: address, reads, wait, step 0;  S2: steps 1..7 with their tests and out-of-line re-reads -- and the
//     quads must survive from S1 to S2 across the table requests the compiler places between them (scalar instructions only;
//     tests/test_isa_hazards.py checks that nothing between the two markers touches a vector register).
// Halves of 8 mics staged under the sweep, power pass, digest: as das_pair_kernel (digest offsets scaled for the 2-float samples).
// (pad, which reads half as much to begin with, measured 2 % slower on interleaved rows: it runs das_pair_kernel)
// (Pair2Geo: das_geometry.h)

#define BF_I_ACC(n, j) [a##n##0] "+v"(acc[j][0]), [a##n##1] "+v"(acc[j][1]), [a##n##2] "+v"(acc[j][2]), [a##n##3] "+v"(acc[j][3])
#define BF_I_READ                                                                                   \
    "ds_read_b128 v[96:99], v120\n\tds_read_b128 v[100:103], v120 offset:1024\n\t"                   \
    "ds_read_b128 v[104:107], v120 offset:%[g0]\n\tds_read_b128 v[108:111], v120 offset:%[g1]\n\ts_waitcnt lgkmcnt(0)\n\t"
#define BF_I_STEP(n, h, mods)                                                                       \
    "v_pk_fma_f32 v[112:113], %[" #h "], v[104:105], v[96:97] " mods "\n\tv_pk_fma_f32 v[114:115], %[" #h "], v[106:107], v[98:99] " mods "\n\t" \
    "v_pk_fma_f32 v[116:117], %[" #h "], v[108:109], v[100:101] " mods "\n\tv_pk_fma_f32 v[118:119], %[" #h "], v[110:111], v[102:103] " mods "\n\t" \
    "v_pk_add_f32 %[a" #n "0], %[a" #n "0], v[112:113]\n\tv_pk_add_f32 %[a" #n "1], %[a" #n "1], v[114:115]\n\t" \
    "v_pk_add_f32 %[a" #n "2], %[a" #n "2], v[116:117]\n\tv_pk_add_f32 %[a" #n "3], %[a" #n "3], v[118:119]\n\t"
// A mic's first reads with direction step 0 behind them, each half of the step waiting only for its own reads (LDS returns in order;
// a counted wait bounds the outstanding operations of any kind, hence the outstanding reads).
#define BF_I_FIRST(h, mods)                                                                         \
    "ds_read_b128 v[96:99], v120\n\tds_read_b128 v[104:107], v120 offset:%[g0]\n\t"                \
    "ds_read_b128 v[100:103], v120 offset:1024\n\tds_read_b128 v[108:111], v120 offset:%[g1]\n\ts_waitcnt lgkmcnt(2)\n\t" \
    "v_pk_fma_f32 v[112:113], %[" #h "], v[104:105], v[96:97] " mods "\n\tv_pk_fma_f32 v[114:115], %[" #h "], v[106:107], v[98:99] " mods "\n\t" \
    "v_pk_add_f32 %[a00], %[a00], v[112:113]\n\tv_pk_add_f32 %[a01], %[a01], v[114:115]\n\ts_waitcnt lgkmcnt(0)\n\t" \
    "v_pk_fma_f32 v[116:117], %[" #h "], v[108:109], v[100:101] " mods "\n\tv_pk_fma_f32 v[118:119], %[" #h "], v[110:111], v[102:103] " mods "\n\t" \
    "v_pk_add_f32 %[a02], %[a02], v[116:117]\n\tv_pk_add_f32 %[a03], %[a03], v[118:119]\n\t"
#define BF_I_EVEN "op_sel_hi:[0,1,1]"
#define BF_I_ODD "op_sel:[1,0,0] op_sel_hi:[1,1,1]"
#define BF_I_CHECK(n, ep, ec) "s_cmp_lg_u32 %[" #ec "], %[" #ep "]\n\ts_cbranch_scc1 .Lr" #n "_%=\n.Lb" #n "_%=:\n\t"
#define BF_I_STUB(n, ec) ".Lr" #n "_%=:\n\tv_add_u32 v120, %[" #ec "], %[lb]\n\t" BF_I_READ "s_branch .Lb" #n "_%=\n"
#define BF_I_CLOB "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", \
                  "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120"

// S1: a mic's first quads, read in place, and direction step 0
// lerp_and_sum.c:50-56  out[k] += s[i] + h * (s[i+1] - s[i]),  i = k - p - 1   (gcc contracts it into one fma)
__device__ __forceinline__ void pair2_first(f32x2 (&acc)[8][4], int e0, unsigned long long h01, int lbase)
{
    using G = Pair2Geo;
    asm volatile("v_add_u32 v120, %[e0], %[lb]\n\t" BF_I_FIRST(h01, BF_I_EVEN) ";BF_S1_END"
                 : BF_I_ACC(0, 0) : [e0] "s"(e0), [h01] "s"(h01), [lb] "v"(lbase), [g0] "n"(G::kDoff), [g1] "n"(G::kDoff + 1024) : BF_I_CLOB);
}
// S2: direction steps 1..7, each behind the test of its LDS offset against the previous step's
__device__ __forceinline__ void pair2_rest(f32x2 (&acc)[8][4], const int (&e)[8], const unsigned long long (&hp)[4], int lbase)
{
    using G = Pair2Geo;
    asm volatile(";BF_S2_BEGIN\n\t"
                 BF_I_CHECK(1, e0, e1) BF_I_STEP(1, h01, BF_I_ODD) BF_I_CHECK(2, e1, e2) BF_I_STEP(2, h23, BF_I_EVEN)
                 BF_I_CHECK(3, e2, e3) BF_I_STEP(3, h23, BF_I_ODD) BF_I_CHECK(4, e3, e4) BF_I_STEP(4, h45, BF_I_EVEN)
                 BF_I_CHECK(5, e4, e5) BF_I_STEP(5, h45, BF_I_ODD) BF_I_CHECK(6, e5, e6) BF_I_STEP(6, h67, BF_I_EVEN)
                 BF_I_CHECK(7, e6, e7) BF_I_STEP(7, h67, BF_I_ODD)
                 ".subsection 1\n" BF_I_STUB(1, e1) BF_I_STUB(2, e2) BF_I_STUB(3, e3) BF_I_STUB(4, e4) BF_I_STUB(5, e5) BF_I_STUB(6, e6) BF_I_STUB(7, e7)
                 "\t.subsection 0"
                 : BF_I_ACC(1, 1), BF_I_ACC(2, 2), BF_I_ACC(3, 3), BF_I_ACC(4, 4), BF_I_ACC(5, 5), BF_I_ACC(6, 6), BF_I_ACC(7, 7)
                 : [e0] "s"(e[0]), [e1] "s"(e[1]), [e2] "s"(e[2]), [e3] "s"(e[3]), [e4] "s"(e[4]), [e5] "s"(e[5]), [e6] "s"(e[6]), [e7] "s"(e[7]), [lb] "v"(lbase),
                   [h01] "s"(hp[0]), [h23] "s"(hp[1]), [h45] "s"(hp[2]), [h67] "s"(hp[3]), [g0] "n"(G::kDoff), [g1] "n"(G::kDoff + 1024)
                 : "scc", BF_I_CLOB);
}
#undef BF_I_ACC
#undef BF_I_READ
#undef BF_I_FIRST
#undef BF_I_STEP
#undef BF_I_EVEN
#undef BF_I_ODD
#undef BF_I_CHECK
#undef BF_I_STUB
#undef BF_I_CLOB

template <int ALGO>   // (lerp only: the parameter keeps the kernel's symbol, which the profiles and ISA checks name)
__global__ void __launch_bounds__(1024, 4) das_pair2_kernel(BF_TABLE_PARAMS, KArgs a)
{
    static_assert(ALGO == ALGO_LERP, "das_pair2_kernel: lerp (pad runs das_pair_kernel)");
    using G = Pair2Geo;
    constexpr int C = G::kC, RS = G::kRs, LEAD = G::kLead, HC = G::kHalf, W = 16, DW = 8, kGroup = DW * W, kParkHalf = Geo<1>::kParkHalf;
    static_assert(2 * kGroup * kParkHalf <= G::kMc * G::kSlot, "both frames' parked half rows fit the LDS image they alias");
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
    const int M = a.n_mics, N = a.n_samples;                   // M % 16 == 0, N % 4 == 0, N <= 256 (plan_das)
    const int n_half = M / HC;
    const float* __restrict__ sig0 = signals + (size_t)f0 * a.m_total * N;
    const float* __restrict__ sig1 = signals + (size_t)f1 * a.m_total * N;
    float* __restrict__ img0 = images + (size_t)f0 * a.image_stride;
    float* __restrict__ img1 = images + (size_t)f1 * a.image_stride;
    const int32_t* __restrict__ dig = reinterpret_cast<const int32_t*>(taps);   // the digest rides in the unused `taps` slot

    // Staging: waves w and w + 8 share mic (w & 7) of every half (both fetch its two frames): part 0 writes the sample rows, part 1
    // the difference rows.  A wave's share of a half is straight-line code: the row base from the mic id (a scalar, loaded a half
    // ahead), two loads, the interleaved quads built in v96.. (free between two sweeps) where the four stores read them.
    const int my_mic = wave & 7, part = wave >> 3;
    constexpr unsigned kHalfBytes = HC * G::kSlot * 4;          // from a row of half 0 to the same row of half 1
    const bool full = N == 256;                                 // every lane has a quad of the row (wave-uniform, once per workgroup)
    // scalar row base + one 32-bit lane offset (global_load saddr form): the per-lane 64-bit pointers of the two frames, hoisted out
    // of the group loop, used to be spilled around the sweep (16 bytes of scratch per lane, stored once per workgroup and
    // reloaded per group: WRITE_SIZE 5x the image bytes).  The load is unconditional: a lane beyond a short row reads the row's last
    // quad instead, and `stage` zeroes what it brought (a load under a lane mask is merged with zeros -- eight moves -- on the spot).
    const unsigned row_bytes = 4u * (unsigned)N, hoff_end = (unsigned)n_half * (HC * 4u);
    unsigned voff = min(16u * (unsigned)lane, row_bytes - 16u);
    const bool in_row = 16u * (unsigned)lane < row_bytes;
    const char* mic_ids = reinterpret_cast<const char*>(mics + my_mic);
    unsigned hoff = 0;                                          // the half the next fetch reads (byte offset into mic_ids) ...
    int mic_a = *reinterpret_cast<const int32_t*>(mic_ids);     // ... and its mic id: a scalar load, consumed half a sweep later
    struct Staged2 { float4 v0, v1; };
    auto fetch_next = [&]() -> Staged2 {
        const size_t row = (size_t)(unsigned)mic_a * row_bytes;
        const char* r0 = reinterpret_cast<const char*>(sig0) + row;
        const char* r1 = reinterpret_cast<const char*>(sig1) + row;
        asm volatile("" : "+v"(voff));                          // (opaque: or hipcc folds it back into two hoisted 64-bit lane pointers)
        Staged2 st;
        st.v0 = *reinterpret_cast<const float4*>(r0 + voff);
        st.v1 = *reinterpret_cast<const float4*>(r1 + voff);
        hoff = hoff + HC * 4u < hoff_end ? hoff + HC * 4u : 0u;  // (after the last half: half 0 again, the next group's first -- or for nothing)
        mic_a = *reinterpret_cast<const int32_t*>(mic_ids + hoff);
        return st;
    };
    // rows of a mic: [s copy 0][s copy 1][d copy 0][d copy 1]; copy c holds sample i - c at position i; position i = floats 2 i, 2 i + 1.
    // With x = frame 0's quad and y = frame 1's (part 1: their differences), v[98:105] = (x.x, y.x, x.y, y.y, x.z, y.z, x.w, y.w) is the
    // lane's piece of copy 0; with v[96:97] = the previous lane's (x.w, y.w) (0 in lane 0: the prefix), v[96:103] is its piece of copy 1.
    // One statement for both parts (part 0's moves out of line): a C++ branch costs five scalar instructions here.
    // (each DPP operand is written two or more instructions before it is read)
#define BF_I_DPP " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    const int lb = 16 * lane + (int)(unsigned)(size_t)((__attribute__((address_space(3))) char*)lds);   // the sweep's lane base
    // a lane's 32 bytes of this wave's first row: 2 lb + row0 in half 0, 2 lb + row1 in half 1
    const int row0 = (my_mic * G::kSlot + part * C * RS) * 4 - (int)(unsigned)(size_t)((__attribute__((address_space(3))) char*)lds), row1 = row0 + (int)kHalfBytes;
    auto stage = [&](int row, const Staged2& st) {
        const int ad = 2 * lb + row;
        float4 x = st.v0, y = st.v1;
        if (!full) {
            asm volatile(";BF_STAGE_MASKED");
            x = make_float4(in_row ? x.x : 0.f, in_row ? x.y : 0.f, in_row ? x.z : 0.f, in_row ? x.w : 0.f);
            y = make_float4(in_row ? y.x : 0.f, in_row ? y.y : 0.f, in_row ? y.z : 0.f, in_row ? y.w : 0.f);
        }
        asm volatile("s_cmp_eq_u32 %[part], 0\n\ts_cbranch_scc1 .Lp0_%=\n\t"
                     // D[i] = s[i+1] - s[i], the reference's own subtraction (lerp_and_sum.c:54); D[-1] stays 0 (prefix)
                     "v_sub_f32 v98, %[xy], %[xx]\n\tv_sub_f32 v99, %[yy], %[yx]\n\t"
                     "v_sub_f32_dpp v104, %[xx], %[xw] wave_shl:1" BF_I_DPP "v_sub_f32_dpp v105, %[yx], %[yw] wave_shl:1" BF_I_DPP
                     "v_sub_f32 v100, %[xz], %[xy]\n\tv_sub_f32 v101, %[yz], %[yy]\n\t"
                     "v_sub_f32 v102, %[xw], %[xz]\n\tv_sub_f32 v103, %[yw], %[yz]\n"
                     ".Lst_%=:\n\t"
                     "v_mov_b32_dpp v96, v104 wave_shr:1" BF_I_DPP "v_mov_b32_dpp v97, v105 wave_shr:1" BF_I_DPP
                     "ds_write_b128 %[ad], v[98:101] offset:%[c0]\n\tds_write_b128 %[ad], v[102:105] offset:%[c0] + 16\n\t"
                     "ds_write_b128 %[ad], v[96:99] offset:%[c1]\n\tds_write_b128 %[ad], v[100:103] offset:%[c1] + 16\n\t"
                     ".subsection 1\n"
                     ".Lp0_%=:\n\t;BF_STAGE_PART0\n\t"
                     "v_mov_b32 v104, %[xw]\n\tv_mov_b32 v105, %[yw]\n\tv_mov_b32 v98, %[xx]\n\tv_mov_b32 v99, %[yx]\n\t"
                     "v_mov_b32 v100, %[xy]\n\tv_mov_b32 v101, %[yy]\n\tv_mov_b32 v102, %[xz]\n\tv_mov_b32 v103, %[yz]\n\t"
                     "s_branch .Lst_%=\n\t.subsection 0"
                     : : [xx] "v"(x.x), [xy] "v"(x.y), [xz] "v"(x.z), [xw] "v"(x.w), [yx] "v"(y.x), [yy] "v"(y.y), [yz] "v"(y.z), [yw] "v"(y.w),
                         [ad] "v"(ad), [part] "s"(part), [c0] "n"(2 * LEAD * 4), [c1] "n"((RS + 2 * LEAD) * 4)
                     : "memory", "scc", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105");
    };
#undef BF_I_DPP
    // the zero prefix (56 samples x 2 frames = 28 quads per row) of this wave's two rows, in both halves: only the parked rows of the
    // power pass overwrite it, so a group restores it once, before its first half is staged
    auto wipe_prefix = [&]() {
        constexpr int PQ = LEAD >> 1;
        static_assert(2 * PQ <= kWave, "one lane per prefix quad of two rows");
        const int l = lane_id();
        if (l < 2 * PQ) {
            float* rows = lds + my_mic * G::kSlot + part * C * RS;
            float4* q = reinterpret_cast<float4*>(rows + (l < PQ ? 0 : RS)) + (l < PQ ? l : l - PQ);
            q[0] = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(reinterpret_cast<char*>(q) + kHalfBytes) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    BF_STAMP_DECL
    Staged2 st = fetch_next();

    for (int g0 = tile_begin; g0 < tile_end; g0 += kGroup) {
        f32x2 acc[DW][4];                                       // (frame 0, frame 1) of samples 2l, 2l+1, 128+2l, 128+2l+1
#pragma unroll
        for (int j = 0; j < DW; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[j][q] = f32x2{0.0f, 0.0f};

        BF_STAMP(7);
        __syncthreads();   // the previous group's parked rows have been summed
        BF_STAMP(1);
        wipe_prefix();
        stage(row0, st);
        st = fetch_next();                                      // half 1
        BF_STAMP(2);
        __syncthreads();
        BF_STAMP(3);

        const int dw0 = g0 + wave * DW;                         // wave-uniform
        const bool busy = dw0 < tile_end;
        const size_t grp = busy ? (size_t)(dw0 - a.dir_begin) / DW : 0;
        const int32_t* __restrict__ etg = dig + grp * M * DW;
        const float* __restrict__ htg = reinterpret_cast<const float*>(dig) + a.digest_h_off + grp * M * DW;
        int row_next = row1;                                    // where the next half is staged: halves alternate
        for (int h = 0; h < n_half; ++h) {
            // The priority ladder.  A SIMD issues by priority, then by age, so at one priority its four waves (w, w + 4, w + 8, w + 12:
            // measured) end every half as a staircase, the youngest sweeping the last stretch alone with nobody to fill the slots
            // its scalar work and LDS round trips leave.  Keyed to progress -- 3 from the barrier on (the staging included), 2, 1,
            // 0 at mics 2, 4, 6 -- a wave that is behind outranks one that is ahead and the four converge on the barrier
            // (the wait for the staged chunk 23.7 % -> 8.9 % of a wave's life, the launch -7.1 %).  One scalar
            // instruction where it changes, before a mic's first statement: never while the hard-wired quads are in flight.
            asm volatile("s_setprio 3");
            asm volatile(";BF_STAGE_BEGIN");                    // (;BF_STAGE_*: path markers for scripts/dev/pair2_instruction_budget.py, comments in the assembly)
            if (h + 1 < n_half) {
                stage(row_next, st);                            // into the half whose sweeps ended before the last barrier
                row_next = row0 + row1 - row_next;
                st = fetch_next();                              // staged an iteration from now: half h + 2, or the next group's first half
                BF_STAMP(2);
            }
            asm volatile(";BF_STAGE_END");
            if (busy) {
                // one table base per half: the eight mics' entries and weights are immediate offsets off it
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
                    pair2_first(acc, cur.e[0], cur.hp[0], lb);
                    request(E[K2], m + 2);      // after the first statement's wait, so that it does not sit on these loads
                    pair2_rest(acc, cur.e, cur.hp, lb);
                };
                using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
                static_assert(HC == 8, "eight mics, the three entry sets in rotation");
                mic(0, I0{}); mic(1, I1{});
                asm volatile("s_setprio 2");
                mic(2, I2{}); mic(3, I0{});
                asm volatile("s_setprio 1");
                mic(4, I1{}); mic(5, I2{});
                asm volatile("s_setprio 0");
                mic(6, I0{}); mic(7, I1{});
                __builtin_amdgcn_s_waitcnt(0xC07F);             // the entries requested past the half's end have landed (and are dropped)
            }
            BF_STAMP(0);       // sweep -> waiting for the others
            __syncthreads();   // half h is free, half h + 1 is staged
            BF_STAMP(h + 1 < n_half ? 3 : 4);
        }
        asm volatile("s_setprio 0");    // (a wave without directions of its own kept 3 from barrier to barrier, where it issues next to nothing)

        // ---- k-ordered mean power (pad_and_sum.c:120-128), both frames at once, one HALF of the samples at a time.  A frame's 128 rows
        // of 256 squares fill the LDS image the rows alias, but 256 rows of 128 do not: so the 16 waves park the squared means of samples
        // 0..127 of their directions for both frames (row 128 f + direction of the group, Geo<1>::kParkHalf floats apart), one (frame,
        // direction) per lane of waves 0..3 adds its row to a running sum, and a second round does the same for samples 128..N-1.  A
        // direction's additions stay strictly in k order; the chain of a round is 128 adds instead of a frame's 256, on four waves
        // instead of two.
        // (the whole pass once per way of dividing, behind the real branch on a.n_is_pow2 -- DESIGN.md 4.1: hipcc speculates the division
        //  sequence otherwise -- and not the divisions alone: where the two ways meet again hipcc moves all 64 values to other registers
        //  and spills.  For the same reason a round squares its own half: all 64 squares pinned before round 0 spill too)
        auto power_pass = [&](auto mul_c) __attribute__((always_inline)) {
        constexpr bool MUL = decltype(mul_c)::value;
        if constexpr (MUL) asm volatile(";BF_POWER_POW2"); else asm volatile(";BF_POWER_DIV");      // (;BF_POWER_*: markers for scripts/dev/pair2_instruction_budget.py, comments in the assembly)
        // (the wave's number behind an empty statement: what the pass derives from it -- row addresses, who sums, which frame -- is then
        //  computed here, a few scalar instructions per group, not hoisted out of the group loop into SGPRs the sweep has none of to spare)
        int wv = wave;
        asm volatile("" : "+s"(wv));
        float sum = 0.0f;               // of this lane's (frame, direction), carried from round 0 to round 1 (waves 0..3)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1) {
                __syncthreads();        // round 0's rows have been summed
                BF_STAMP(4);
            }
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
                // lane l holds samples 2l, 2l+1 of the half, one frame's two floats in two register pairs.  ds_write2_b32 stores them from
                // where they are (as a float2 they are moved together first), and each to a part of its own: a row is [64 even samples]
                // [64 odd samples], so that the lanes of either store cover 64 banks (side by side at 8 l: two lanes per bank, measured).
                // add_in_order_rolling reads the two parts back into k order.  The offsets, 8 bits of dwords, reach two rows.
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
            BF_STAMP(5);                // -> waiting
            __syncthreads();
            BF_STAMP(6);                // -> ordered sum (four waves; the others go on to the next barrier)
            if (wv < 2 * (kGroup / kWave)) {
                const int lane_o = lane_id();                 // (recomputed: keeps the per-lane row address out of the registers the sweep needs)
                const int g = (wv & 1) * kWave + lane_o;    // this lane's direction of the group; its parked row is wave * 64 + lane: frame 1's rows follow frame 0's
                const int d = g0 + g;
                if (d < tile_end && (wv < kGroup / kWave || two)) {
                    const unsigned row = (unsigned)(size_t)((__attribute__((address_space(3))) char*)lds) + (unsigned)(wv * kWave + lane_o) * (kParkHalf * 4u);
                    sum = add_in_order_rolling(row, r == 0 ? 32 : (N - 128) >> 2, sum);     // round 1 stops at N
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
    BF_STAMP(7);
    BF_STAMP_FLUSH;
}

}  // namespace copies

template <int ALGO>
hipError_t launch_pair_algo(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream)
{
    constexpr bool kLerp = ALGO == ALGO_LERP;           // das_pair_kernel (pad) / das_pair2_kernel (lerp: frames interleaved in the rows)
    using PG = std::conditional_t<kLerp, copies::Pair2Geo, copies::PairGeo>;
    if (plan.family != (kLerp ? DAS_PAIR_LERP : DAS_PAIR_PAD) || L.tab.digest_direct || plan.waves != copies::kWaves || plan.mic_chunk != PG::kMc ||
        plan.row_stride != PG::kRs || plan.lead != PG::kLead || (L.n_mics % 16) != 0)
        return hipErrorInvalidValue;
    auto kernel = [] { if constexpr (kLerp) return copies::das_pair2_kernel<ALGO>; else return copies::das_pair_kernel<ALGO>; }();
    static int pair_scratch = -1;
    const dim3 pair_grid((unsigned)plan.n_tiles * (unsigned)((frames + 1) / 2));
    return launch_with_lds(kernel, pair_grid, dim3((unsigned)plan.waves * kWave), plan.lds_bytes, stream, &pair_scratch, L.signals, L.images, L.mics,
                           L.tab.whole, L.tab.frac, reinterpret_cast<const float*>(L.tab.digest), make_args(L, plan));
}

}  // namespace

hipError_t launch_pair(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream)
{
    switch (L.algo) {
        case ALGO_PAD: return launch_pair_algo<ALGO_PAD>(L, plan, frames, stream);
        case ALGO_LERP: return launch_pair_algo<ALGO_LERP>(L, plan, frames, stream);
        default: return hipErrorInvalidValue;
    }
}

// Profiling build only: read and clear the phase totals of das_pair_kernel (16 counters; zeros in a production build).
hipError_t read_phase_stamps(unsigned long long* out16, bool clear)
{
#ifdef BF_STAMPS
    static unsigned long long all[64 * 16];
    hipError_t e = hipMemcpyFromSymbol(all, HIP_SYMBOL(copies::g_stamps), sizeof(all));
    if (e != hipSuccess) return e;
    for (int i = 0; i < 16; ++i) { out16[i] = 0; for (int r = 0; r < 64; ++r) out16[i] += all[16 * r + i]; }
    if (!clear) return e;
    for (int i = 0; i < 64 * 16; ++i) all[i] = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(copies::g_stamps), all, sizeof(all));
#else
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    (void)clear;
    return hipSuccess;
#endif
}

// Profiling build only: the per-wave rows beside the totals (16 wave indices x 8 counters; zeros in a production build).
hipError_t read_wave_stamps(unsigned long long* out128, bool clear)
{
#ifdef BF_STAMPS
    static unsigned long long all[64 * 128];
    hipError_t e = hipMemcpyFromSymbol(all, HIP_SYMBOL(copies::g_wave_stamps), sizeof(all));
    if (e != hipSuccess) return e;
    for (int i = 0; i < 128; ++i) { out128[i] = 0; for (int r = 0; r < 64; ++r) out128[i] += all[128 * r + i]; }
    // [6]: the recorded workgroups in which wave w ran on the SIMD of wave w & 3, [7]: the workgroups recorded (all 16 waves seen)
    static unsigned char simd[4096 * 16];
    e = hipMemcpyFromSymbol(simd, HIP_SYMBOL(copies::g_wave_simd), sizeof(simd));
    if (e != hipSuccess) return e;
    for (int g = 0; g < 4096; ++g) {
        const unsigned char* s = simd + 16 * g;
        bool whole = true;
        for (int w = 0; w < 16; ++w) whole = whole && (s[w] & 0x80);
        if (!whole) continue;
        for (int w = 0; w < 16; ++w) { out128[8 * w + 6] += s[w] == s[w & 3]; out128[8 * w + 7] += 1; }
    }
    if (!clear) return e;
    for (int i = 0; i < 64 * 128; ++i) all[i] = 0;
    for (int i = 0; i < 4096 * 16; ++i) simd[i] = 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(copies::g_wave_simd), simd, sizeof(simd));
    if (e != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(copies::g_wave_stamps), all, sizeof(all));
#else
    for (int i = 0; i < 128; ++i) out128[i] = 0;
    (void)clear;
    return hipSuccess;
#endif
}

}  // namespace bf
