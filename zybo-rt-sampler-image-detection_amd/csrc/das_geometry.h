// What the host planner (das_plan.cpp) and the delay-and-sum kernel units (das_kernels.hip, das_strided.hip, das_pair.hip, das_cells.hip) share, and nothing of the device:
// the compile-time geometry of every kernel family, stated once, and the per-family launchers launch_das chooses between.
// Not installed; das_device.h includes it.
#pragma once
#include "das_kernels.h"

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

}  // namespace

// One launcher per kernel family, each defined beside its kernels.  launch_das (das_plan.cpp) picks the family and has checked what
// the families share (the digest is there, the FIR flavours have 8 taps); every launcher checks its own geometry against the plan.
hipError_t launch_strided(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);       // das_strided.hip: das_mimo_kernel<.., HIST = false>
hipError_t launch_copies(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);        // das_kernels.hip: das_copies_kernel
hipError_t launch_pair(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);          // das_pair.hip: das_pair_kernel (pad), das_pair2_kernel (lerp)
hipError_t launch_pair_cells(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);    // das_cells.hip: das_pair2_cells_kernel (lerp, plan.cells)
hipError_t launch_hybrid_pair(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);   // das_kernels.hip: das_hybrid_pair_kernel
hipError_t launch_long(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream);          // das_kernels.hip: das_long_kernel

}  // namespace bf
