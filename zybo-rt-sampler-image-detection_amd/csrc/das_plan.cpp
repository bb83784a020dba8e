// das_plan.cpp -- the host side of a delay-and-sum launch, no device code: plan_das / plan_stream_maps size the LDS image, the
// chunks and the grid, the digest_* functions size the digest, and launch_das picks the kernel family of a plan.  The kernels'
// geometry comes from das_geometry.h; das_kernels.hip says what each family is.
#include "das_geometry.h"

#include <algorithm>

namespace bf {

namespace {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The strided layout's LDS image, given the zero columns in front of (`lead`) and behind (`tail`) every row: one 1024-thread
// workgroup (16 waves) per CU owns the whole 160 KiB LDS:
//   [ mic rows of one frame (or one chunk of them) | per-wave power scratch: waves x pbw rows of 64*nc+4 floats ]
// When the frame's mic block does not fit beside the scratch, the mics are staged in chunks and every wave
// carries 4 directions' accumulators across the chunks.  false: one microphone row does not fit.
bool size_strided(DasPlan& p, int n_samples, int n_mics, int lead, int tail)
{
    const int nc = (n_samples + kWave - 1) / kWave;
    p.nc = nc <= 1 ? 1 : nc <= 2 ? 2 : nc <= 4 ? 4 : nc <= 8 ? 8 : 16;
    p.lead = lead;
    p.row_stride = p.lead + p.nc * kWave + tail;
    const size_t row_bytes = (size_t)p.row_stride * sizeof(float);
    const size_t lds_budget = 160 * 1024;
    p.waves = 16;
    p.srow = p.nc * kWave + 4;   // +4: keeps rows 16-byte aligned and 4 banks apart; column nc*64 holds the direction id
    p.pbw = p.nc <= 4 ? 4 : p.nc <= 8 ? 2 : 1;
    const size_t scratch_bytes = (size_t)p.waves * p.pbw * p.srow * sizeof(float);
    const size_t sig_budget = lds_budget - scratch_bytes - 16;
    if (row_bytes * (size_t)n_mics <= sig_budget) {
        p.mic_chunk = n_mics; p.n_chunks = 1; p.dpw = 1;
    } else {
        int mc = (int)(sig_budget / row_bytes);          // (fewer than n_mics: the block did not fit)
        if (mc < 1) return false;
        if (mc >= 4) mc &= ~3;
        p.mic_chunk = mc; p.n_chunks = (n_mics + mc - 1) / mc;
        p.dpw = 4;
    }
    p.scratch_off = round_up(p.mic_chunk * p.row_stride, 4);
    p.lds_bytes = (size_t)p.scratch_off * sizeof(float) + scratch_bytes;
    return true;
}

}  // namespace

int plan_das(const DasLaunch& L, int n_cus, DasPlan* plan, const char** why)
{
    static const char* kWhy[] = {"", "N_SAMPLES must be in [1, 1024]", "N_TAPS must be in [1, 64] (multiple of 8 for the vectorized FIR)",
                                 "one microphone row does not fit in LDS", "empty launch"};
    auto fail = [&](int i) { if (why) *why = kWhy[i]; return -i; };
    if (L.n_samples < 1 || L.n_samples > 1024) return fail(1);
    const bool fir = is_fir(L.algo);
    if (fir && (L.n_taps < 1 || L.n_taps > 64 || (L.algo == ALGO_FIR_VEC && (L.n_taps % 8) != 0))) return fail(2);
    if (L.n_mics < 1 || L.frames < 1 || L.dir_end <= L.dir_begin) return fail(4);

    DasPlan p{};
    p.nf = 1;
    p.frame_inner = 0;
    const int T = fir ? L.n_taps : 0;
    const int shift = (L.algo == ALGO_FIR_NAIVE || L.algo == ALGO_FIR_VEC) ? 0 : L.tab.max_whole;
    if (!size_strided(p, L.n_samples, L.n_mics, round_up(shift + 1 + T / 2, 4), round_up(T, 4))) return fail(3);
    // Layout: 2 = shifted copies for pad / lerp at 128 < N <= 1024 and for the 8-tap FIR flavours at 128 < N <= 256, 0 = strided
    // everywhere else.
    const bool plain = is_plain(L.algo);
    const bool copies_ok = plain ? p.nc >= 4 : (p.nc == 4 && L.n_taps == 8);
    p.layout = copies_ok ? 2 : 0;
    if (p.layout == 2) {
        const int nseg = p.nc / 4, arrays = (L.algo == ALGO_LERP) ? 2 : 1;
        const int fixed_lead = nseg == 1 ? copies::Geo<1>::kLead : copies::Geo<4>::kLead;   // Geo<2> == Geo<4> here
        const int dw = nseg == 4 ? copies::Geo<4>::kDw : copies::Geo<1>::kDw;               // Geo<2> == Geo<1> here
        // zero prefix: the furthest look-back is the delay (+1 for lerp, +1 + T/2 for hybrid, T/2 for the plain FIRs)
        const int back = L.algo == ALGO_HYBRID ? L.tab.max_whole + 1 + L.n_taps / 2 : fir ? L.n_taps / 2 : L.tab.max_whole + 1;
        p.lead = round_up(back + 1, 4);
        if (p.lead <= fixed_lead) p.lead = fixed_lead;   // compile-time row stride
        p.row_stride = p.lead + nseg * 256 + (fir ? copies::Geo<1>::kFirTail : 0);
        p.copies = copies::copies_of(L.algo, L.tab.digest_direct);
        const size_t slot_bytes = (size_t)arrays * p.copies * p.row_stride * sizeof(float);
        // a chunk: as many mics as fit beside nothing else in 156 KiB, at most 16 (one s_load of table entries) and at
        // most what the 16 waves stage in one go (one (mic, segment) pair each; two for pad with several segments)
        int stage_pairs = 16 * ((nseg > 1 && L.algo == ALGO_PAD) ? 2 : 1);
        // One 16-wave workgroup per CU with (nearly) the whole LDS.  pad / lerp at N <= 256 also come as 8-wave workgroups
        // (two per CU, 78 KiB each): twice the staging per direction, so only for grids too coarse to fill 16 waves' 128
        // directions (cfg1: 121 directions, 637K -> 961K frames/s).  (cfg2, 190 frames: 16 waves 80.0K, 8 waves 72.0K.)
        const int waves = (plain && nseg == 1 && (L.dir_end - L.dir_begin) < 256) ? 8 : copies::kWaves;
        const size_t budget = waves == 8 ? (size_t)78 * 1024 : (size_t)156 * 1024;
        if (plain && nseg == 1 && waves == copies::kWaves && !L.tab.digest_direct) stage_pairs = 32;
        int mc = (int)(budget / slot_bytes);
        if (mc > stage_pairs / nseg) mc = stage_pairs / nseg;
        mc = mc >= 32 ? 32 : mc >= 16 ? 16 : mc >= 8 ? 8 : mc >= 4 ? 4 : mc >= 2 ? 2 : mc;
        if (mc < 1) return fail(3);
        if (mc > L.n_mics) mc = L.n_mics;
        // Two frames per workgroup (das_pair_kernel) where its fixed geometry applies: the per-step scalar work is then shared
        // by both frames.
        p.nf = 1;
        if (plain && nseg == 1 && waves == copies::kWaves && !L.tab.digest_direct && p.lead == fixed_lead && (L.n_mics % 16) == 0 &&
            (L.n_samples % 4) == 0 && L.frames >= 2) {
            p.nf = 2;
            mc = 16;
            // frames interleaved in the rows (das_pair2_kernel) for lerp: 4 instead of 8 LDS reads per (re)load, +1.5 %; pad reads
            // half as much to begin with and measured 2 % slower that way
            if (L.algo == ALGO_LERP) {
                p.interleaved = 1;
                p.row_stride = 2 * copies::Geo<1>::kRs;         // the two frames of a mic share a row, sample by sample
                // whole halves of 16 mics, an even number of them: rows of 16-byte cells (das_pair2_cells_kernel), half the staging
                // stores per mic and half the barriers.  The plan's exported fields stay those of das_pair2_kernel's image, which
                // is the same 159,744 bytes.
                static_assert(copies::CellGeo::kMc * copies::CellGeo::kSlot <= copies::Pair2Geo::kMc * copies::Pair2Geo::kSlot, "one LDS image for both row layouts");
                p.cells = (L.n_mics % copies::CellGeo::kMc) == 0 && L.n_samples > 128 ? 1 : 0;
            }
        }
        // The hybrid beamformer's two-frame sweep (das_hybrid_pair_kernel) under the same conditions.
        if (fir && nseg == 1 && L.n_taps == 8 && waves == copies::kWaves && p.lead == fixed_lead && (L.n_mics % 16) == 0 &&
            (L.n_samples % 4) == 0 && L.frames >= 2) {
            p.nf = 2;
            mc = copies::HybridGeo::kMc;                        // 32 mic slots: two frames interleaved per row, two shifted copies
            p.copies = copies::HybridGeo::kC;
            p.row_stride = copies::HybridGeo::kRs;
            p.interleaved = 1;
        }
        const bool hybrid_pair = fir && p.nf == 2;
        // Long rows (2 / 4 segments): das_long_kernel where its LDS image -- two halves of 16 / nseg mics -- fits and the mic count is
        // a whole number of halves.
        p.long_rows = 0;
        if (plain && nseg > 1 && !L.tab.digest_direct) {
            const int half = 16 / nseg;
            if ((L.n_mics % half) == 0 && (L.n_samples % 4) == 0 && slot_bytes * (size_t)(2 * half) <= (size_t)160 * 1024) {
                p.long_rows = 1;
                mc = 2 * half;
                if (L.algo == ALGO_LERP) {                      // rows of (sample pair, difference pair) quads: two floats per sample, no separate difference rows
                    p.interleaved = 1;
                    p.row_stride *= 2;
                }
            }
        }
        p.mic_chunk = mc; p.n_chunks = (L.n_mics + mc - 1) / mc;
        p.waves = waves; p.dpw = dw; p.srow = nseg * 256 + 4;
        p.scratch_off = 0;
        const size_t buf = hybrid_pair ? (size_t)mc * copies::HybridGeo::kSlot * sizeof(float) : slot_bytes * (size_t)mc * (size_t)p.nf;
        const size_t wave_rows = (size_t)dw * p.srow * sizeof(float);          // the parked rows of one wave
        p.lds_bytes = buf > 2 * wave_rows ? buf : 2 * wave_rows;
        if (p.long_rows && p.lds_bytes < 8 * wave_rows) p.lds_bytes = 8 * wave_rows;             // eight waves park together (two rounds)
        if (nseg == 1 && p.lds_bytes < p.waves * wave_rows) p.lds_bytes = p.waves * wave_rows;   // N <= 256: the whole group parks at once
        int pw = (int)(p.lds_bytes / wave_rows);                                 // waves that park together (power of two)
        p.pbw = pw >= 16 ? 16 : pw >= 8 ? 8 : pw >= 4 ? 4 : 2;
        if (p.pbw > p.waves) p.pbw = p.waves;
    }

    // Tile size: enough workgroups to fill the chip a few times over, but as many directions per staged block
    // as possible.  A tile is a whole number of wave groups -- except for small launches (a single frame through the
    // host-pointer API), where latency matters: then every CU gets a tile, even if that leaves waves of a group idle.
    const int group = p.waves * p.dpw;
    const long long dirs = (long long)(L.dir_end - L.dir_begin);
    bool spread = false;   // no XCD affinity of the tiles (see below)
    const long long target_wgs = (long long)n_cus * 4;
    const long long wg_frames = p.nf == 2 ? (L.frames + 1) / 2 : L.frames;   // frames (frame pairs) a column of the grid walks
    long long td = (dirs * wg_frames + target_wgs - 1) / target_wgs;
    if (dirs * wg_frames < (long long)n_cus * group) {
        td = (dirs * wg_frames + n_cus - 1) / n_cus;
        td = round_up((int)(td < 1 ? 1 : td), p.dpw);
    } else {
        // A whole number of wave groups per tile, chosen by what the grid costs.  Workgroup ids go round-robin over the 8 XCDs.
        //   * Large tables: workgroup id -> (tile, frame) with the tile count padded to a multiple of 8 keeps
        //     tile % 8 == id % 8, so every XCD's L2 serves only its own tiles' table rows for all frames; XCD x then runs
        //     the tiles with tile % 8 == x on its 32 CUs and the launch takes  max_x ceil(tiles_x * frames / 32)  rounds of
        //     k groups.  (cfg2, 95 frame pairs, lerp: k = 2 or 5 -> 30 units, 122K frames/s; k = 4 -> 36, 106K; k = 8 -> 48,
        //     80K: measured.)
        //   * Tables that fit every XCD's L2 whole (a rank's direction shard of bench.py --gpus 4 / 8): no padding, every
        //     tile's workgroups spread over the XCDs, ceil(tiles * frames / CUs) rounds -- pinning 10 tiles to 8 XCDs left
        //     a rank of the 8-GPU shape at 63 % of the one-GPU rate.
        // Ties go to the first of 2, 3, .., 8, 1.
        const size_t table_bytes = (size_t)dirs * (size_t)L.n_mics * 4u * ((L.algo == ALGO_LERP ? 2u : 1u) + (fir ? (size_t)L.n_taps : 0u));
        spread = table_bytes <= ((size_t)3 << 20);
        // an XCD's share of the table beyond its L2: all frames of a tile back to back (tile_and_frame)
        p.frame_inner = (!spread && p.layout == 2 && table_bytes > ((size_t)16 << 20) && wg_frames > 1) ? 1 : 0;
        const int wg_per_cu = 1;
        const int xcds = 8, cus_per_xcd = (n_cus >= xcds ? n_cus / xcds : 1) * wg_per_cu;
        long long best_cost = -1;
        int best_k = 4;
        for (int i = 0; i < 8; ++i) {
            const int k = i < 7 ? i + 2 : 1;
            const long long tiles = (dirs + (long long)k * group - 1) / ((long long)k * group);
            const long long tiles_x = tiles / xcds + (tiles % xcds ? 1 : 0);        // the busiest XCD's share
            const long long slots = (long long)n_cus * wg_per_cu;
            const long long rounds = spread ? (tiles * wg_frames + slots - 1) / slots : (tiles_x * wg_frames + cus_per_xcd - 1) / cus_per_xcd;
            const long long cost = rounds * k;
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_k = k; }
        }
        td = (long long)best_k * group;
    }
    p.tile_dirs = (int)td;
    p.n_tiles = spread ? (int)((dirs + td - 1) / td) : round_up((int)((dirs + td - 1) / td), 8);
    *plan = p;
    if (why) *why = kWhy[0];
    return 0;
}

// Where the sweep order of a launch sits in its digest (behind the grouped entries and lerp's weights), 0 where the plan's kernel
// takes none: only the pad / lerp pair kernels do.
long long digest_order_offset(const DasLaunch& L, const DasPlan& plan)
{
    if (plan.layout != 2 || plan.nf != 2 || (L.algo != ALGO_PAD && L.algo != ALGO_LERP)) return 0;
    return (L.algo == ALGO_LERP ? 2 : 1) * grouped_entries_for_args(L, plan);
}

size_t digest_elements(const DasLaunch& L, const DasPlan& plan)
{
    if (plan.layout != 2) return 0;
    const size_t direct = (size_t)L.n_dirs * (size_t)L.n_mics;                 // the [D][M] layout of the DIRECT variant
    const size_t order = digest_order_offset(L, plan) != 0 ? (size_t)(grouped_entries_for_args(L, plan) / L.n_mics) : 0;   // one entry per (padded) position
    if (L.algo == ALGO_PAD) return std::max((size_t)grouped_entries_for_args(L, plan) + order, direct);
    if (L.algo == ALGO_LERP) return std::max((size_t)(2 * grouped_entries_for_args(L, plan)) + order, direct);    // offsets, then the lerp weights in the same order
    // the FIR pair kernel: offsets and packed guards (hybrid), then the taps regrouped per 8 directions
    if (L.algo == ALGO_HYBRID) return std::max((size_t)L.n_dirs * (size_t)L.n_mics, plan.nf == 2 ? (size_t)(10 * grouped_entries_for_args(L, plan)) : (size_t)0);
    if ((L.algo == ALGO_FIR_NAIVE || L.algo == ALGO_FIR_VEC) && plan.nf == 2) return (size_t)(8 * grouped_entries_for_args(L, plan));
    return 0;
}

// Steps of a launch over which the sweep can share reads at all (all but the first direction of every group).
long long digest_shareable_steps(const DasLaunch& L, const DasPlan& plan)
{
    return plan.dpw > 1 ? grouped_entries_for_args(L, plan) / plan.dpw * (plan.dpw - 1) : 0;
}

// The family of a plan: the strided kernels for layout 0, and for the shifted copies (layout 2: pad / lerp beyond 128 samples, the
// 8-tap FIR flavours at 128 < N <= 256) the two-frame kernels, the long rows, or the one-frame sweep, in this order.
hipError_t launch_das(const DasLaunch& L, const DasPlan& plan, hipStream_t stream)
{
    if (L.algo < 0 || L.algo >= ALGO_COUNT) return hipErrorInvalidValue;
    if (plan.nc != 1 && plan.nc != 2 && plan.nc != 4 && plan.nc != 8 && plan.nc != 16) return hipErrorInvalidValue;
    const bool fir = is_fir(L.algo);
    if (!fir && plan.nc >= 4) {
        if (plan.layout != 2) return hipErrorInvalidValue;   // pad / lerp beyond 128 samples: shifted copies only (plan_das gives them no other layout)
    } else if (!(plan.nc == 4 && plan.layout == 2)) {        // the 8-tap FIR flavours; other tap counts take the strided kernel
        return launch_strided(L, plan, L.frames, stream);
    }
    const int nseg = plan.nc / 4;
    const bool needs_digest = L.algo != ALGO_FIR_NAIVE && L.algo != ALGO_FIR_VEC;
    if (needs_digest && L.tab.digest == nullptr) return hipErrorInvalidValue;   // launch_digest first
    if (fir && L.n_taps != 8) return hipErrorInvalidValue;
    if (plan.nf == 2 && (fir || nseg == 1))
        return fir ? launch_hybrid_pair(L, plan, L.frames, stream) : plan.cells ? launch_pair_cells(L, plan, L.frames, stream) : launch_pair(L, plan, L.frames, stream);
    if (!fir && nseg > 1 && plan.long_rows) return launch_long(L, plan, L.frames, stream);
    return launch_copies(L, plan, L.frames, stream);
}

// ---- continuous-stream mode: planning (launch_stream_maps / launch_stream_beams: das_strided.hip) --------------------------

int stream_history(int algo, int max_whole)
{
    return algo == ALGO_PAD ? max_whole : algo == ALGO_LERP ? max_whole + 1 : -1;
}

// Tiles of a strided launch that has no table affinity to keep (the stream maps, the listed directions): whole wave groups, about four
// workgroups per CU; a launch too small for that gives every CU a tile.  With one chunk a tile stages its frame once, so more groups per
// tile save staging; with several chunks every group restages anyway.
static void tile_strided(DasPlan& p, long long dirs, int frames, int n_cus)
{
    const int group = p.waves * p.dpw;
    const long long work = dirs * frames;
    long long td;
    if (work < (long long)n_cus * group) {
        td = round_up((int)std::max<long long>(1, (work + n_cus - 1) / n_cus), p.dpw);
    } else {
        long long k = p.n_chunks > 1 ? 1 : work / ((long long)n_cus * 4 * group);
        k = std::min<long long>(std::max<long long>(k, 1), 8);
        td = k * group;
    }
    p.tile_dirs = (int)td;
    p.n_tiles = (int)((dirs + td - 1) / td);
}

// Maps in stream mode always take the strided layout (lane l owns samples l, l + 64, ..), whatever N: the sizing is plan_das's
// for that layout -- one 16-wave workgroup with the whole LDS, mic rows (or a chunk of them) beside the per-wave power scratch.
int plan_stream_maps(const DasLaunch& L, int n_cus, DasPlan* plan, const char** why)
{
    auto fail = [&](const char* msg) { if (why) *why = msg; return -1; };
    if (L.algo != ALGO_PAD && L.algo != ALGO_LERP) return fail("continuous mode exists for pad and lerp only");
    if (L.n_samples < 1 || L.n_samples > 1024) return fail("N_SAMPLES must be in [1, 1024]");
    if (L.n_mics < 1 || L.frames < 1 || L.dir_end <= L.dir_begin) return fail("empty launch");
    DasPlan p{};
    p.nf = 1;
    if (!size_strided(p, L.n_samples, L.n_mics, round_up(L.tab.max_whole + 1, 4), 0))      // lead >= the history of either flavour
        return fail("one microphone row does not fit in LDS");
    tile_strided(p, (long long)(L.dir_end - L.dir_begin), L.frames, n_cus);
    *plan = p;
    if (why) *why = "";
    return 0;
}

// The listed directions (das_select_kernel) take the strided layout too, whatever N and the algorithm: plan_das's rows for the
// window-local call (zero columns for the delay and the taps), plan_stream_maps's for the stream call; the LIST [0, L.dir_end) is tiled.
int plan_select(const DasLaunch& L, bool stream, int n_cus, DasPlan* plan, const char** why)
{
    auto fail = [&](const char* msg) { if (why) *why = msg; return -1; };
    if (stream ? !is_plain(L.algo) : (L.algo != ALGO_PAD && L.algo != ALGO_LERP && L.algo != ALGO_HYBRID && L.algo != ALGO_FIR_VEC))
        return fail(stream ? "continuous mode exists for pad and lerp only" : "no map at listed directions for this algorithm");
    if (L.n_samples < 1 || L.n_samples > 1024) return fail("N_SAMPLES must be in [1, 1024]");
    const bool fir = is_fir(L.algo);
    if (fir && (L.n_taps < 1 || L.n_taps > 64 || (L.algo == ALGO_FIR_VEC && (L.n_taps % 8) != 0)))
        return fail("N_TAPS must be in [1, 64] (multiple of 8 for the vectorized FIR)");
    if (L.n_mics < 1 || L.frames < 1 || L.dir_begin != 0 || L.dir_end < 1) return fail("empty launch");
    DasPlan p{};
    p.nf = 1;
    const int T = fir ? L.n_taps : 0;
    const int shift = L.algo == ALGO_FIR_VEC ? 0 : L.tab.max_whole;
    if (!size_strided(p, L.n_samples, L.n_mics, round_up(shift + 1 + T / 2, 4), round_up(T, 4))) return fail("one microphone row does not fit in LDS");
    if (p.dpw == 4 && L.algo == ALGO_HYBRID && p.nc == 16) p.dpw = 2;   // das_select_kernel<HYBRID, 16, 4> would spill (the value does not depend on dpw)
    tile_strided(p, L.dir_end, L.frames, n_cus);
    *plan = p;
    if (why) *why = "";
    return 0;
}

}  // namespace bf
