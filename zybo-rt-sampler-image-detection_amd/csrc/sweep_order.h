// sweep_order.h -- the order in which the pad / lerp pair kernels sweep the directions of a launch.  Host only, no HIP.
//
// A wave of das_pair_kernel / das_pair2_kernel carries `dpw` consecutive POSITIONS of the launch and re-reads a microphone's
// quads whenever the whole-sample delay changes from one position to the next.  Results are per direction, so which direction
// sits at which position is free; this function chooses it from the table alone (the C-ABI knows no grid shape).
//
// Input: the whole-sample rows p[s][m] of the launch's range, s in [0, n_pos) (position s of the identity = flat direction
// first_dir + s), m in [0, n_mics); row s starts at rows + s * row_stride.
// Output: order[s] = flat direction swept at position s, a permutation of [first_dir, first_dir + n_pos).
//
// The rule:
//   1. c[s] = number of mics with p[s+1][m] != p[s][m], for s in [0, n_pos - 1).
//   2. A new segment starts at s + 1 wherever 2 * c[s] > n_mics (a grid's row end: most delays jump).
//   3. The first segment runs forward.
//   4. Every later segment [a, b) is placed forward (a, a+1, .., b-1) or reversed (b-1, .., a).  With L = the row placed last
//      so far, it is reversed if the number of mics with L[m] != p[b-1][m] is strictly smaller than the number with
//      L[m] != p[a][m].
//   5. changes(order) = number of (position s with s % dpw != 0, mic m) with p[order[s-1]][m] != p[order[s]][m] -- what the sweep
//      re-reads, counted inside runs of dpw positions from position 0 as the digest build counts them.  Unless the new order has
//      strictly fewer changes than the identity, the identity is returned.
// On a rectangular grid swept along its rows this is a serpentine; on a table without structure it is the identity.
#pragma once
#include <stdint.h>

namespace bf {

struct SweepOrderStats {
    long long changes_identity = 0;   // rule 5's count for the identity
    long long changes_order = 0;      // ... and for the order returned
    int segments = 0, reversed = 0;   // of the candidate order (also when the identity was returned in its place)
    bool identity = true;             // the order returned is the identity
};

// Returns 0, or -1 on a bad argument (null pointer, n_pos < 1, n_mics < 1, dpw < 1, row_stride < n_mics).
int sweep_order(const int32_t* rows, long long row_stride, int n_pos, int n_mics, int first_dir, int dpw, int32_t* order, SweepOrderStats* stats);

}  // namespace bf
