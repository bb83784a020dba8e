// Stand-alone driver of csrc/das_plan.cpp for tests/test_plan_families_host.py, which builds the two files (and nothing else) with
// -fsanitize=address,undefined on the host side: plan_das over a sweep of launches that reaches every kernel family, one text row each.
// usage: plan_table_main all | sub | none      (which rows are printed; the per-family counts always follow, as `# variant rows count` lines)
//   sub: digest_direct = 0, n_cus = 256, max_whole in {12, 56, 200} -- the launches tests/batched_cases.plan restates.
// A row: algo N n T frames dirs max_whole digest_direct n_cus : rc, and for an accepted launch the plan's numeric fields (nc lead row_stride
// mic_chunk n_chunks waves scratch_off srow pbw dpw frame_inner copies tile_dirs n_tiles lds_bytes), the bf_last_das_variant / bf_last_das_rows
// numbers of its family, digest_elements, digest_order_offset, digest_shareable_steps, the digest offsets make_args hands the kernel
// (h_off t_off) and the launcher launch_das reaches (0 strided, 1 copies, 2 pair, 3 cells, 4 FIR pair, 5 long rows; -1 refused).
#include <cstdio>
#include <cstring>

#include "das_device.h"

namespace bf {

// The six family launchers, in place of the kernel units: each records that launch_das reached it.
static int g_reached = -1;
hipError_t launch_strided(const DasLaunch&, const DasPlan&, int, hipStream_t) { g_reached = 0; return hipSuccess; }
hipError_t launch_copies(const DasLaunch&, const DasPlan&, int, hipStream_t) { g_reached = 1; return hipSuccess; }
hipError_t launch_pair(const DasLaunch&, const DasPlan&, int, hipStream_t) { g_reached = 2; return hipSuccess; }
hipError_t launch_pair_cells(const DasLaunch&, const DasPlan&, int, hipStream_t) { g_reached = 3; return hipSuccess; }
hipError_t launch_hybrid_pair(const DasLaunch&, const DasPlan&, int, hipStream_t) { g_reached = 4; return hipSuccess; }
hipError_t launch_long(const DasLaunch&, const DasPlan&, int, hipStream_t) { g_reached = 5; return hipSuccess; }

// What bf_last_das_variant / bf_last_das_rows report for a plan.
static void observed(const DasLaunch&, const DasPlan& plan, int* variant, int* rows)
{
    const FamilyTraits ft = family_traits(plan.family);
    *variant = ft.variant; *rows = ft.rows;
}

}  // namespace bf

int main(int argc, char** argv)
{
    const bool all = argc == 2 && !std::strcmp(argv[1], "all"), sub = argc == 2 && !std::strcmp(argv[1], "sub");
    if (!all && !sub && !(argc == 2 && !std::strcmp(argv[1], "none"))) { std::fprintf(stderr, "usage: %s all | sub | none\n", argv[0]); return 2; }
    static const int kN[] = {1, 63, 64, 65, 128, 129, 130, 200, 202, 256, 257, 300, 512, 513, 1000, 1024};
    static const int kMics[] = {1, 3, 4, 8, 12, 16, 24, 32, 40, 48, 64, 256};
    static const int kTaps[] = {1, 7, 8, 16, 64};
    static const int kFrames[] = {1, 2, 3, 190};
    static const int kDirs[] = {1, 7, 121, 255, 256, 10201, 130321};
    static const int kWhole[] = {0, 12, 47, 54, 55, 56, 95, 200, 1024};
    static const int kCus[] = {256, 64};
    static int32_t digest_stands_in;          // launch_das only asks whether a digest is there
    long long counts[10][3] = {}, refused = 0, total = 0;
    for (int algo = 0; algo < bf::ALGO_COUNT; ++algo)
    for (int N : kN)
    for (int n : kMics)
    for (int T : kTaps) {
        if (bf::is_plain(algo) && T != 8) continue;
        for (int frames : kFrames)
        for (int dirs : kDirs)
        for (int mw : kWhole)
        for (int direct = 0; direct < 2; ++direct)
        for (int n_cus : kCus) {
            bf::DasLaunch L{};
            L.algo = algo; L.n_mics = n; L.m_total = n; L.n_samples = N; L.n_taps = T; L.n_dirs = dirs;
            L.dir_begin = 0; L.dir_end = dirs; L.image_stride = dirs; L.image_origin = 0; L.frames = frames;
            L.tab.max_whole = mw < N ? mw : N;
            L.tab.digest_direct = direct != 0;
            L.tab.digest = &digest_stands_in;
            bf::DasPlan p{};
            const char* why = nullptr;
            const int rc = bf::plan_das(L, n_cus, &p, &why);
            ++total;
            const bool print = all || (sub && direct == 0 && n_cus == 256 && (mw == 12 || mw == 56 || mw == 200));
            if (print) std::printf("%d %d %d %d %d %d %d %d %d : %d", algo, N, n, T, frames, dirs, mw, direct, n_cus, rc);
            if (rc != 0) {
                ++refused;
                if (why == nullptr || !*why) { std::fprintf(stderr, "a refusal without a reason\n"); return 1; }
            } else {
                int variant = -1, rows = -1;
                bf::observed(L, p, &variant, &rows);
                if (variant < 0 || variant > 9 || rows < 0 || rows > 2) { std::fprintf(stderr, "variant %d rows %d\n", variant, rows); return 1; }
                ++counts[variant][rows];
                const bf::KArgs a = bf::make_args(L, p);
                bf::g_reached = -1;
                if (bf::launch_das(L, p, nullptr) != hipSuccess) bf::g_reached = -1;
                if (print)
                    std::printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d %d %zu %lld %lld %lld %lld %d", p.nc, p.lead, p.row_stride, p.mic_chunk, p.n_chunks,
                                p.waves, p.scratch_off, p.srow, p.pbw, p.dpw, p.frame_inner, p.copies, p.tile_dirs, p.n_tiles, p.lds_bytes, variant, rows,
                                bf::digest_elements(L, p), bf::digest_order_offset(L, p), bf::digest_shareable_steps(L, p), a.digest_h_off, a.digest_t_off,
                                bf::g_reached);
            }
            if (print) std::printf("\n");
        }
    }
    std::printf("# launches %lld refused %lld\n", total, refused);
    for (int v = 0; v < 10; ++v)
        for (int r = 0; r < 3; ++r)
            if (counts[v][r]) std::printf("# %d %d %lld\n", v, r, counts[v][r]);
    return 0;
}
