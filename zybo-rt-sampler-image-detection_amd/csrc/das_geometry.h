// What the host planner (das_plan.cpp) and the delay-and-sum kernel units (das_kernels.hip, das_strided.hip, das_pair.hip, das_cells.hip) share, and nothing of the device:
// the compile-time geometry of every kernel family, what follows from a plan's family (family_traits, digest_layout), each stated once, and the
// per-family launchers launch_das chooses between.
// Not installed; das_device.h includes it, and the C-ABI layer for the family's traits.
#pragma once
#include "das_kernels.h"

#include <algorithm>

namespace bf {

namespace {

constexpr int kWave = 64;

// pad / lerp ("plain") against the three FIR flavours
constexpr bool is_plain(int algo) { return algo == ALGO_PAD || algo == ALGO_LERP; }
constexpr bool is_fir(int algo) { return algo == ALGO_HYBRID || algo == ALGO_FIR_NAIVE || algo == ALGO_FIR_VEC; }

// Entries of a grouped digest (digest_grouped_kernel): the launch's directions padded to whole groups of plan.dpw, times the mics.
inline long long grouped_entries_for_args(const DasLaunch& L, const DasPlan& plan)
{
    const long long groups = ((long long)(L.dir_end - L.dir_begin) + plan.dpw - 1) / plan.dpw;
    return groups * L.n_mics * plan.dpw;
}

namespace copies {

constexpr int kWaves = 16;       // waves per workgroup (8 for pad / lerp at N <= 256: two workgroups per CU cover each other's barriers)

// Shifted copies kept per staged array.  The sweep of pad / lerp re-reads rarely and reads 8-byte halves: one copy per
// delay mod 2 is enough (half the staging writes and half the LDS per mic).  The kernels that read at every step -- the
// 8-tap FIR flavours and the direction-outer (DIRECT) variant of pad / lerp -- need ds_read_b128: one copy per delay mod 4.
__host__ __device__ constexpr int copies_of(int algo, bool direct) { return ((algo == ALGO_PAD || algo == ALGO_LERP) && !direct) ? 2 : 4; }

// Geometry of the shifted-copies layout for a block of NSEG x 256 samples (N <= 256: 1, <= 512: 2, <= 1024: 4).
//   * a wave owns DW directions x NSEG segments of 256 samples (one aligned quad per lane per segment);
//   * compile-time row stride (RS > 0) when the largest delay fits kLead: the D / segment reads become immediate offsets.
template <int NSEG>
struct Geo {
    static constexpr int kDw = NSEG == 1 ? 8 : NSEG == 2 ? 8 : 4;   // directions per wave
    static constexpr int kBatch = 4 / NSEG;                          // mics whose reads are in flight together
    static constexpr int kLead = NSEG == 1 ? 56 : 64;                // zero prefix of the fixed-stride variant (56: the as-shipped array's delays, up to 47 samples, still fit; 32 lerp mics x 4 rows x 312 floats = 156 KiB)
    static constexpr int kRs = NSEG * 256 + kLead;                   // its row stride
    static constexpr int kPark = NSEG * 256 + 4;                     // floats per parked row of squares
    static constexpr int kParkHalf = 128 + 4;                        // ... of the kernels that park a row in two halves of 128 samples (das_pair2_kernel); 4 (mod 64) dwords like kPark
    static constexpr int kFirTail = 8;                               // 8-tap FIR rows: the reference's zero padding after the block
    static constexpr int kRsFir = kRs + kFirTail;
};

// das_pair_kernel (das_pair.hip)
struct PairGeo {
    static constexpr int kC = 2, kRs = Geo<1>::kRs, kLead = Geo<1>::kLead;
    static constexpr int kSlot = kC * kRs;               // floats per staged (mic, frame)
    static constexpr int kFoff = kSlot * 4;              // bytes from a frame-0 quad to the same quad of frame 1
    static constexpr int kMc = 16;                       // mics per LDS image (the digest's slot count) ...
    static constexpr int kHalf = 8;                      // ... swept and re-staged in halves of 8
};

// das_pair2_kernel (das_pair.hip)
struct Pair2Geo {
    static constexpr int kC = 2, kLead = Geo<1>::kLead, kRs = 2 * Geo<1>::kRs, kMc = 16, kHalf = 8;
    static constexpr int kSlot = 2 * kC * kRs;           // floats per staged mic (both frames): samples and differences
    static constexpr int kDoff = kC * kRs * 4;           // bytes from a sample quad to its difference quad
};

// das_pair2_cells_kernel (das_cells.hip): a mic is one row of 16-byte cells (s f0, s f1, D f0, D f1), one per sample, no shifted copies
struct CellGeo {
    static constexpr int kLead = Geo<1>::kLead, kCells = 256 + kLead;   // zero cells in front, cells per row
    static constexpr int kSlot = 4 * kCells;             // floats per staged mic (both frames, samples and differences)
#ifndef BF_CELLS_HC
#define BF_CELLS_HC 16                                   // (8: the measuring aid of das_cells.hip, never the shipped build)
#endif
    static constexpr int kHalf = BF_CELLS_HC, kMc = 2 * kHalf;   // mic slots of the LDS image (the digest's slot count: 32), swept and re-staged in halves of 16
};

// das_hybrid_pair_kernel (das_kernels.hip)
struct HybridGeo {
    static constexpr int kC = 2, kLead = Geo<1>::kLead, kRs = 2 * Geo<1>::kRsFir;   // floats per row: two frames interleaved
    static constexpr int kHalf = 16, kMc = 2 * kHalf;
    static constexpr int kSlot = kC * kRs;               // floats per staged mic (both frames)
};

// das_long_kernel (das_kernels.hip)
template <int ALGO, int NSEG>
struct LongGeo {
    static constexpr bool kLerp = ALGO == ALGO_LERP;
    static constexpr int kA = kLerp ? 2 : 1, kC = 2, kDw = Geo<NSEG>::kDw, kHalf = 16 / NSEG, kMc = 2 * kHalf;
    static constexpr int kPark = Geo<NSEG>::kPark;
};

}  // namespace copies

// What follows from a plan's family, stated once: the frames a workgroup carries; what bf_last_das_variant / bf_last_das_rows report (9 is
// the stream call's); the digest -- FLAT: [D][M] (digest_kernel), GROUPED: by the wave's directions (digest_grouped_kernel); whether the
// grouped digest takes a sweep order; whether a 16-wave launch whose digest counted a re-read at more than half of the shareable steps is
// handed over to DAS_COPIES_DIRECT (ensure_digest, beamformer_api.cpp).
enum DigestKind : int { DIGEST_NONE = 0, DIGEST_FLAT, DIGEST_GROUPED };
struct FamilyTraits { int frames_per_wg, variant, rows; DigestKind digest; bool sweep_order, reread_handover; };
constexpr FamilyTraits family_traits(DasFamily f)
{
    switch (f) {                      //      frames  variant  rows  digest     sweep order  hand-over
        case DAS_COPIES:        return {1, 2, 0, DIGEST_GROUPED, false, true};
        case DAS_COPIES_DIRECT: return {1, 3, 0, DIGEST_FLAT, false, false};
        case DAS_COPIES_FIR:    return {1, 4, 0, DIGEST_FLAT, false, false};      // (hybrid; the plain FIRs have no whole-sample table: no digest)
        case DAS_PAIR_PAD:      return {2, 5, 0, DIGEST_GROUPED, true, true};
        case DAS_PAIR_LERP:     return {2, 8, 1, DIGEST_GROUPED, true, true};
        case DAS_PAIR_CELLS:    return {2, 8, 2, DIGEST_GROUPED, true, true};
        case DAS_PAIR_FIR:      return {2, 7, 0, DIGEST_GROUPED, false, false};   // (the plain FIRs too: their taps regrouped)
        case DAS_LONG:          return {1, 6, 0, DIGEST_GROUPED, false, true};
        default:                return {1, 0, 0, DIGEST_NONE, false, false};      // DAS_STRIDED
    }
}
inline int wg_frames(DasFamily f, int frames) { return (frames + family_traits(f).frames_per_wg - 1) / family_traits(f).frames_per_wg; }   // frames (frame pairs) a column of the grid walks

// The digest of a launch (DeviceTables::digest, 4-byte elements).  Grouped: [entries offsets][entries lerp weights, or the hybrid pair kernel's
// packed guards: h_off][the sweep order, one entry per padded position: order_off | the FIR pair kernel's taps regrouped per 8 directions, 8 per
// entry: t_off]; the plain FIRs' pair digest is the taps alone.  A pad / lerp buffer also holds the [D][M] digest a hand-over would build in it.
// An entry is the LDS offset of slot m % slots, each `arrays` x `copies` rows of slot_stride floats with a sample `width` floats wide
// (CellGeo's for the cell rows, the plan's otherwise), looking back `bias` samples beyond the delay.
struct DigestLayout {
    DigestKind kind;
    size_t elements;                         // of the buffer (0: none)
    long long entries, h_off, t_off, order_off;
    int slots, arrays, slot_stride, lead, bias, copies, width;
};
inline DigestLayout digest_layout(const DasLaunch& L, const DasPlan& plan)
{
    using CG = copies::CellGeo;
    const FamilyTraits ft = family_traits(plan.family);
    const bool lerp = L.algo == ALGO_LERP, hybrid = L.algo == ALGO_HYBRID, cells = plan.family == DAS_PAIR_CELLS;
    DigestLayout d{};
    d.kind = (plan.family == DAS_COPIES_FIR && !hybrid) ? DIGEST_NONE : ft.digest;
    d.entries = grouped_entries_for_args(L, plan);
    const size_t flat = (size_t)L.n_dirs * (size_t)L.n_mics, e = (size_t)d.entries;
    if (plan.family == DAS_PAIR_FIR) {
        d.h_off = hybrid ? d.entries : 0; d.t_off = hybrid ? 2 * d.entries : 0;
        d.elements = hybrid ? std::max(flat, 10 * e) : 8 * e;
    } else if (is_plain(L.algo) && plan.family != DAS_STRIDED) {
        d.h_off = lerp ? d.entries : 0; d.order_off = ft.sweep_order ? (lerp ? 2 : 1) * d.entries : 0;
        d.elements = std::max((lerp ? 2 : 1) * e + (ft.sweep_order ? e / L.n_mics : 0), flat);
    } else if (d.kind == DIGEST_FLAT) {
        d.elements = flat;
    }
    // what the kernel looks back by beyond the whole-sample delay: lerp reads s[k - p - 1], hybrid starts its window at s[k - p - 1 - T/2] (T = 8)
    d.bias = lerp ? 1 : hybrid ? 5 : 0;
    d.slots = cells ? CG::kMc : plan.mic_chunk; d.slot_stride = cells ? CG::kSlot : plan.row_stride;
    d.lead = cells ? CG::kLead : plan.lead; d.copies = cells ? 1 : plan.copies;
    // rows of one staged mic in units of its shifted copies: samples and lerp's differences (inside the row for the long rows and the cells),
    // both frames of the pad pair kernel (the other pair kernels interleave them inside a row: a sample is 2 floats wide, a cell 4)
    const DasFamily f = plan.family;
    d.arrays = (f == DAS_PAIR_PAD || f == DAS_PAIR_LERP || ((f == DAS_COPIES || f == DAS_COPIES_DIRECT) && lerp)) ? 2 : 1;
    d.width = cells ? 4 : (f == DAS_PAIR_LERP || f == DAS_PAIR_FIR || (f == DAS_LONG && lerp)) ? 2 : 1;
    return d;
}

}  // namespace

// One launcher per kernel family, each defined beside its kernels.  launch_das (das_plan.cpp) switches on the plan's family and has checked
// what the families share (the digest is there, the FIR flavours have 8 taps); every launcher checks its own geometry against the plan.
hipError_t launch_strided(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);       // das_strided.hip: das_mimo_kernel<.., HIST = false>
hipError_t launch_copies(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);        // das_kernels.hip: das_copies_kernel
hipError_t launch_pair(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);          // das_pair.hip: das_pair_kernel (pad), das_pair2_kernel (lerp)
hipError_t launch_pair_cells(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);    // das_cells.hip: das_pair2_cells_kernel (lerp)
hipError_t launch_hybrid_pair(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);   // das_kernels.hip: das_hybrid_pair_kernel
hipError_t launch_long(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);          // das_kernels.hip: das_long_kernel

}  // namespace bf
