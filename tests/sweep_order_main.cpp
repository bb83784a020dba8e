// Stand-alone driver of csrc/sweep_order.cpp for tests/test_sweep_order_host.py, which builds the two files (and nothing else)
// with -fsanitize=address,undefined.  usage: sweep_order_main <table file> <order file>
// table file: int32 header {n_dirs, n_mics, dir_begin, dir_end, dpw}, then int32 [n_dirs][n_mics];
// order file: int32 [dir_end - dir_begin], then int32 {segments, reversed, identity}, then int64 {changes_identity, changes_order}.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sweep_order.h"

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <table file> <order file>\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    int32_t hdr[5];
    if (std::fread(hdr, sizeof(int32_t), 5, in) != 5) { std::fprintf(stderr, "short header\n"); return 2; }
    const int n_dirs = hdr[0], n_mics = hdr[1], dir_begin = hdr[2], dir_end = hdr[3], dpw = hdr[4];
    if (n_dirs < 1 || n_mics < 1 || dir_begin < 0 || dir_end > n_dirs || dir_begin >= dir_end) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> table((size_t)n_dirs * n_mics);            // exactly the table: a read past a row's or the range's end is caught
    if (std::fread(table.data(), sizeof(int32_t), table.size(), in) != table.size()) { std::fprintf(stderr, "short table\n"); return 2; }
    std::fclose(in);

    std::vector<int32_t> order((size_t)(dir_end - dir_begin));
    bf::SweepOrderStats st;
    if (bf::sweep_order(table.data() + (size_t)dir_begin * n_mics, n_mics, dir_end - dir_begin, n_mics, dir_begin, dpw, order.data(), &st) != 0) return 1;
    // the refusals: none of them may touch memory
    if (bf::sweep_order(nullptr, n_mics, 1, n_mics, 0, dpw, order.data(), nullptr) != -1 ||
        bf::sweep_order(table.data(), n_mics, 0, n_mics, 0, dpw, order.data(), nullptr) != -1 ||
        bf::sweep_order(table.data(), n_mics - 1, 1, n_mics, 0, dpw, order.data(), nullptr) != -1 ||
        bf::sweep_order(table.data(), n_mics, 1, n_mics, 0, 0, order.data(), nullptr) != -1)
        return 3;

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    const int32_t tail[3] = {st.segments, st.reversed, st.identity ? 1 : 0};
    const int64_t counts[2] = {st.changes_identity, st.changes_order};
    std::fwrite(order.data(), sizeof(int32_t), order.size(), out);
    std::fwrite(tail, sizeof(int32_t), 3, out);
    std::fwrite(counts, sizeof(int64_t), 2, out);
    return std::fclose(out) == 0 ? 0 : 2;
}
