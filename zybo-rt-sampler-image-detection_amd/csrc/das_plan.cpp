// das_plan.cpp -- the host side of a delay-and-sum launch, no device code: plan_das picks the kernel family of a launch and sizes its
// LDS image, chunks and grid (plan_stream_maps / plan_select: the strided family's), and launch_das forwards a plan to its family's
// launcher.  The kernels' geometry, a family's traits and the digest's layout come from das_geometry.h; das_kernels.hip says what each family is.
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

// What the shifted-copies families share (pad / lerp at 128 < N <= 1024, the 8-tap FIR flavours at 128 < N <= 256; everything else is
// strided: !eligible), and what pick_family decides by.
struct CopiesShape {
    bool eligible;
    int nseg, fixed_lead;   // segments of 256 samples; the zero prefix of the compile-time row stride
    int lead, row_stride, copies, waves, dpw;
    size_t slot_bytes;      // one staged mic of the one-frame sweep: its arrays x copies rows ...
    int mic_chunk;          // ... and how many of them a chunk of that sweep holds (< 1: not one)
};

CopiesShape shape_copies(const DasLaunch& L, int nc)
{
    CopiesShape s{};
    const bool plain = is_plain(L.algo), fir = is_fir(L.algo);
    s.eligible = plain ? nc >= 4 : (nc == 4 && L.n_taps == 8);
    if (!s.eligible) return s;
    s.nseg = nc / 4;
    const int arrays = (L.algo == ALGO_LERP) ? 2 : 1;
    s.fixed_lead = s.nseg == 1 ? copies::Geo<1>::kLead : copies::Geo<4>::kLead;   // Geo<2> == Geo<4> here
    s.dpw = s.nseg == 4 ? copies::Geo<4>::kDw : copies::Geo<1>::kDw;              // Geo<2> == Geo<1> here
    // zero prefix: the furthest look-back is the delay (+1 for lerp, +1 + T/2 for hybrid, T/2 for the plain FIRs)
    const int back = L.algo == ALGO_HYBRID ? L.tab.max_whole + 1 + L.n_taps / 2 : fir ? L.n_taps / 2 : L.tab.max_whole + 1;
    s.lead = std::max(round_up(back + 1, 4), s.fixed_lead);   // (at least the compile-time row stride's)
    s.row_stride = s.lead + s.nseg * 256 + (fir ? copies::Geo<1>::kFirTail : 0);
    s.copies = copies::copies_of(L.algo, L.tab.digest_direct);
    s.slot_bytes = (size_t)arrays * s.copies * s.row_stride * sizeof(float);
    // One 16-wave workgroup per CU with (nearly) the whole LDS.  pad / lerp at N <= 256 also come as 8-wave workgroups
    // (two per CU, 78 KiB each): twice the staging per direction, so only for grids too coarse to fill 16 waves' 128
    // directions (cfg1: 121 directions, 637K -> 961K frames/s).  (cfg2, 190 frames: 16 waves 80.0K, 8 waves 72.0K.)
    s.waves = (plain && s.nseg == 1 && (L.dir_end - L.dir_begin) < 256) ? 8 : copies::kWaves;
    const size_t budget = s.waves == 8 ? (size_t)78 * 1024 : (size_t)156 * 1024;
    // a chunk: as many mics as fit beside nothing else in 156 KiB, at most 16 (one s_load of table entries) and at
    // most what the 16 waves stage in one go (one (mic, segment) pair each; two for pad with several segments)
    int stage_pairs = 16 * ((s.nseg > 1 && L.algo == ALGO_PAD) ? 2 : 1);
    if (plain && s.nseg == 1 && s.waves == copies::kWaves && !L.tab.digest_direct) stage_pairs = 32;
    const int mc = std::min((int)(budget / s.slot_bytes), stage_pairs / s.nseg);
    s.mic_chunk = std::min(mc >= 32 ? 32 : mc >= 16 ? 16 : mc >= 8 ? 8 : mc >= 4 ? 4 : mc >= 2 ? 2 : mc, L.n_mics);
    return s;
}

// The family of a launch: the one place it is decided (DasFamily, das_kernels.h).  The strided kernels where the shifted copies are not
// eligible, else the two-frame kernels, the long rows, or the one-frame sweep, in this order.
DasFamily pick_family(const DasLaunch& L, const CopiesShape& s)
{
    if (!s.eligible) return DAS_STRIDED;
    // Two frames per workgroup where the pair kernels' fixed geometry applies: the per-step scalar work is then shared by both frames.
    const bool pair = s.nseg == 1 && s.waves == copies::kWaves && s.lead == s.fixed_lead && (L.n_mics % 16) == 0 && (L.n_samples % 4) == 0 && L.frames >= 2;
    if (is_fir(L.algo)) return pair ? DAS_PAIR_FIR : DAS_COPIES_FIR;
    if (L.tab.digest_direct) return DAS_COPIES_DIRECT;
    if (pair) {
        // frames interleaved in the rows (das_pair2_kernel) for lerp: 4 instead of 8 LDS reads per (re)load, +1.5 %; pad reads
        // half as much to begin with and measured 2 % slower that way
        if (L.algo == ALGO_PAD) return DAS_PAIR_PAD;
        // whole halves of 16 mics, an even number of them: rows of 16-byte cells (das_pair2_cells_kernel), half the staging
        // stores per mic and half the barriers
        return (L.n_mics % copies::CellGeo::kMc) == 0 && L.n_samples > 128 ? DAS_PAIR_CELLS : DAS_PAIR_LERP;
    }
    // Long rows (2 / 4 segments): das_long_kernel where its LDS image -- two halves of 16 / nseg mics -- fits and the mic count is
    // a whole number of halves.
    const int half = 16 / s.nseg;
    if (s.nseg > 1 && (L.n_mics % half) == 0 && (L.n_samples % 4) == 0 && s.slot_bytes * (size_t)(2 * half) <= (size_t)160 * 1024) return DAS_LONG;
    return DAS_COPIES;
}

// The shifted-copies families' LDS image -- a family writes its rows (mic_chunk, row_stride, copies) once, in its row of the table, with
// the bytes of one mic slot -- and what the waves park in it.
void size_copies_family(DasPlan& p, const CopiesShape& s, const DasLaunch& L)
{
    using namespace copies;
    size_t image = 0;
    auto rows = [&](int mic_chunk, int row_stride, int ncopies, size_t slot_bytes) {
        p.mic_chunk = mic_chunk; p.row_stride = row_stride; p.copies = ncopies; image = slot_bytes * (size_t)mic_chunk;
    };
    // The cell rows' plan keeps das_pair2_kernel's exported fields: its image is the same 159,744 bytes.
    static_assert(CellGeo::kMc * CellGeo::kSlot <= Pair2Geo::kMc * Pair2Geo::kSlot, "one LDS image for both row layouts");
    switch (p.family) {
        case DAS_PAIR_PAD: rows(PairGeo::kMc, PairGeo::kRs, s.copies, 2 * s.slot_bytes); break;                                  // 16 mics, both frames
        case DAS_PAIR_LERP: case DAS_PAIR_CELLS: rows(Pair2Geo::kMc, Pair2Geo::kRs, s.copies, 2 * s.slot_bytes); break;          // the two frames of a mic share a row, sample by sample
        case DAS_PAIR_FIR: rows(HybridGeo::kMc, HybridGeo::kRs, HybridGeo::kC, HybridGeo::kSlot * sizeof(float)); break;         // 32 mic slots: two frames interleaved per row, two shifted copies
        // two halves of 16 / nseg mics; lerp: rows of (sample pair, difference pair) quads: two floats per sample, no separate difference rows
        case DAS_LONG: rows(2 * (16 / s.nseg), (L.algo == ALGO_LERP ? 2 : 1) * s.row_stride, s.copies, s.slot_bytes); break;
        default: rows(s.mic_chunk, s.row_stride, s.copies, s.slot_bytes); break;                                                  // DAS_COPIES, DAS_COPIES_DIRECT, DAS_COPIES_FIR: the one-frame sweep's chunk
    }
    p.lead = s.lead;
    p.n_chunks = (L.n_mics + p.mic_chunk - 1) / p.mic_chunk;
    p.waves = s.waves; p.dpw = s.dpw; p.srow = s.nseg * 256 + 4;
    p.scratch_off = 0;
    const size_t wave_rows = (size_t)p.dpw * p.srow * sizeof(float);          // the parked rows of one wave
    p.lds_bytes = std::max(image, 2 * wave_rows);
    if (p.family == DAS_LONG) p.lds_bytes = std::max(p.lds_bytes, 8 * wave_rows);            // eight waves park together (two rounds)
    if (s.nseg == 1) p.lds_bytes = std::max(p.lds_bytes, p.waves * wave_rows);               // N <= 256: the whole group parks at once
    const int pw = (int)(p.lds_bytes / wave_rows);                           // waves that park together (power of two)
    p.pbw = std::min(pw >= 16 ? 16 : pw >= 8 ? 8 : pw >= 4 ? 4 : 2, p.waves);
}

// Tile size: enough workgroups to fill the chip a few times over, but as many directions per staged block
// as possible.  A tile is a whole number of wave groups -- except for small launches (a single frame through the
// host-pointer API), where latency matters: then every CU gets a tile, even if that leaves waves of a group idle.
void choose_tiles(DasPlan& p, const DasLaunch& L, int n_cus)
{
    const int group = p.waves * p.dpw;
    const long long dirs = (long long)(L.dir_end - L.dir_begin);
    bool spread = false;   // no XCD affinity of the tiles (see below)
    const long long target_wgs = (long long)n_cus * 4;
    const long long cols = wg_frames(p.family, L.frames);   // frames (frame pairs) a column of the grid walks
    long long td = (dirs * cols + target_wgs - 1) / target_wgs;
    if (dirs * cols < (long long)n_cus * group) {
        td = (dirs * cols + n_cus - 1) / n_cus;
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
        const size_t table_bytes = (size_t)dirs * (size_t)L.n_mics * 4u * ((L.algo == ALGO_LERP ? 2u : 1u) + (is_fir(L.algo) ? (size_t)L.n_taps : 0u));
        spread = table_bytes <= ((size_t)3 << 20);
        // an XCD's share of the table beyond its L2: all frames of a tile back to back (tile_and_frame)
        p.frame_inner = (!spread && p.family != DAS_STRIDED && table_bytes > ((size_t)16 << 20) && cols > 1) ? 1 : 0;
        const int wg_per_cu = 1;
        const int xcds = 8, cus_per_xcd = (n_cus >= xcds ? n_cus / xcds : 1) * wg_per_cu;
        long long best_cost = -1;
        int best_k = 4;
        for (int i = 0; i < 8; ++i) {
            const int k = i < 7 ? i + 2 : 1;
            const long long tiles = (dirs + (long long)k * group - 1) / ((long long)k * group);
            const long long tiles_x = tiles / xcds + (tiles % xcds ? 1 : 0);        // the busiest XCD's share
            const long long slots = (long long)n_cus * wg_per_cu;
            const long long rounds = spread ? (tiles * cols + slots - 1) / slots : (tiles_x * cols + cus_per_xcd - 1) / cus_per_xcd;
            const long long cost = rounds * k;
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_k = k; }
        }
        td = (long long)best_k * group;
    }
    p.tile_dirs = (int)td;
    p.n_tiles = spread ? (int)((dirs + td - 1) / td) : round_up((int)((dirs + td - 1) / td), 8);
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
    const int T = fir ? L.n_taps : 0;
    const int shift = (L.algo == ALGO_FIR_NAIVE || L.algo == ALGO_FIR_VEC) ? 0 : L.tab.max_whole;
    if (!size_strided(p, L.n_samples, L.n_mics, round_up(shift + 1 + T / 2, 4), round_up(T, 4))) return fail(3);
    const CopiesShape s = shape_copies(L, p.nc);
    if (s.eligible && s.mic_chunk < 1) return fail(3);
    p.family = pick_family(L, s);
    if (p.family != DAS_STRIDED) size_copies_family(p, s, L);      // (strided: size_strided's)
    choose_tiles(p, L, n_cus);
    *plan = p;
    if (why) *why = kWhy[0];
    return 0;
}

long long digest_order_offset(const DasLaunch& L, const DasPlan& plan) { return digest_layout(L, plan).order_off; }
size_t digest_elements(const DasLaunch& L, const DasPlan& plan) { return digest_layout(L, plan).elements; }

// Steps of a launch over which the sweep can share reads at all (all but the first direction of every group).
long long digest_shareable_steps(const DasLaunch& L, const DasPlan& plan)
{
    return plan.dpw > 1 ? grouped_entries_for_args(L, plan) / plan.dpw * (plan.dpw - 1) : 0;
}

// Behind the checks the families share (a digest where the family takes one, 8 taps for the FIR flavours' shifted copies), one
// launcher per family; each checks its own geometry against the plan.
hipError_t launch_das(const DasLaunch& L, const DasPlan& plan, hipStream_t stream)
{
    if (L.algo < 0 || L.algo >= ALGO_COUNT) return hipErrorInvalidValue;
    if (plan.nc != 1 && plan.nc != 2 && plan.nc != 4 && plan.nc != 8 && plan.nc != 16) return hipErrorInvalidValue;
    if (plan.family == DAS_STRIDED) {
        if (is_plain(L.algo) && plan.nc >= 4) return hipErrorInvalidValue;   // pad / lerp beyond 128 samples: shifted copies only (plan_das gives them no other family)
        return launch_strided(L, plan, L.frames, stream);
    }
    if (plan.nc < 4 || (is_fir(L.algo) && (plan.nc != 4 || L.n_taps != 8))) return hipErrorInvalidValue;
    if (digest_layout(L, plan).kind != DIGEST_NONE && L.tab.digest == nullptr) return hipErrorInvalidValue;   // launch_digest first
    switch (plan.family) {
        case DAS_COPIES: case DAS_COPIES_DIRECT: case DAS_COPIES_FIR: return launch_copies(L, plan, L.frames, stream);
        case DAS_PAIR_PAD: case DAS_PAIR_LERP: return launch_pair(L, plan, L.frames, stream);
        case DAS_PAIR_CELLS: return launch_pair_cells(L, plan, L.frames, stream);
        case DAS_PAIR_FIR: return launch_hybrid_pair(L, plan, L.frames, stream);
        case DAS_LONG: return launch_long(L, plan, L.frames, stream);
        default: return hipErrorInvalidValue;
    }
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
    DasPlan p{};                                          // (family: DAS_STRIDED)
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
    DasPlan p{};                                          // (family: DAS_STRIDED)
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
