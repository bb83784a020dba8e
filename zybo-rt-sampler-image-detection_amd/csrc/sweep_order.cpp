// sweep_order.cpp -- see sweep_order.h for the rule.  Pure host code: no HIP, no state.
#include "sweep_order.h"

#include <stddef.h>

#include <vector>

namespace bf {

namespace {

struct Rows {
    const int32_t* p;
    long long stride;
    int n_mics;
    int differ(int s, int t) const   // mics whose whole-sample delay differs between rows s and t
    {
        const int32_t* a = p + (long long)s * stride;
        const int32_t* b = p + (long long)t * stride;
        int c = 0;
        for (int m = 0; m < n_mics; ++m) c += a[m] != b[m];
        return c;
    }
};

}  // namespace

int sweep_order(const int32_t* rows, long long row_stride, int n_pos, int n_mics, int first_dir, int dpw, int32_t* order, SweepOrderStats* stats)
{
    if (rows == nullptr || order == nullptr || n_pos < 1 || n_mics < 1 || dpw < 1 || row_stride < n_mics) return -1;
    const Rows R{rows, row_stride, n_mics};
    SweepOrderStats st;

    // rules 1 and 2: the changes of every identity step, and the segments they cut
    std::vector<int> c((size_t)n_pos, 0);          // c[s]: step s -> s + 1 (c[n_pos - 1] unused)
    std::vector<int> seg_begin{0};
    for (int s = 0; s + 1 < n_pos; ++s) {
        c[s] = R.differ(s, s + 1);
        if (2 * (long long)c[s] > n_mics) seg_begin.push_back(s + 1);
        if ((s + 1) % dpw != 0) st.changes_identity += c[s];
    }
    seg_begin.push_back(n_pos);
    st.segments = (int)seg_begin.size() - 1;

    // rules 3 and 4: place the segments (as rows 0 .. n_pos - 1; first_dir is added at the end)
    std::vector<int> pos((size_t)n_pos);
    int placed = 0;
    for (int k = 0; k < st.segments; ++k) {
        const int a = seg_begin[k], b = seg_begin[k + 1];
        const bool rev = k > 0 && R.differ(pos[placed - 1], b - 1) < R.differ(pos[placed - 1], a);
        st.reversed += rev;
        for (int i = 0; i < b - a; ++i) pos[placed++] = rev ? b - 1 - i : a + i;
    }

    // rule 5: steps inside a segment are identity steps (c[] again); only the segment joints need two rows compared
    long long changes = 0;
    for (int s = 1; s < n_pos; ++s) {
        if (s % dpw == 0) continue;
        const int u = pos[s - 1], v = pos[s];
        changes += (v == u + 1) ? c[u] : (u == v + 1) ? c[v] : R.differ(u, v);
    }
    st.identity = !(changes < st.changes_identity);
    st.changes_order = st.identity ? st.changes_identity : changes;
    for (int s = 0; s < n_pos; ++s) order[s] = first_dir + (st.identity ? s : pos[s]);
    if (stats != nullptr) *stats = st;
    return 0;
}

}  // namespace bf
