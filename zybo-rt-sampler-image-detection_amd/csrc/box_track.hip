// box_track.hip -- bf_track_boxes_device: SORT on the device, identity over time for the detector's boxes.
//
// Definition (include/beamformer_hip.h): per frame predict every track, IoU gains against the frame's detections, association (the
// pairs over the threshold where they are unambiguous, the assignment of maximal total gain otherwise), Kalman updates, births,
// report and retire.  The frame loop is sequential by definition, so the launch is ONE workgroup of kBoxTrackThreads lanes and the
// frames run in order inside it; the state buffer is read once and written once.
//
//   box_track_kernel : lane s of wave 0 owns slot s and keeps its track in registers from the first frame to the last.  Per frame:
//       rows      every lane validates ceil(max_boxes / lanes) consecutive rows; a workgroup prefix scan of the counts compacts the
//                 detections' boxes and row numbers into LDS in row order.
//       predict   wave 0, a lane per slot; the live slots' boxes go to LDS in slot order (a ballot gives a slot its row).
//       gains     a lane per detection (strided), a loop over the rows: the pair's gain, the detection's over-threshold count in a
//                 register, the row's by an LDS integer atomic, the row's (only) partner by a plain store.
//       associate the shortcut reads the partners; otherwise the shortest-augmenting-path assignment below.
//       update / birth / outputs   wave 0 again; births are serial over the detections left, lowest free slot by ballot.
//   assignment: potentials, per-column minima, predecessors and flags live in LDS; a gain is recomputed from the two boxes whenever
//       it is needed (five subtractions, two products, a division) instead of keeping a 64 x 1088 matrix.  One step of a row's
//       search relaxes all unused columns over all lanes, takes the minimum by (value, column) -- per lane, then across the wave
//       by shuffles, then across the waves through LDS; the order is total, so the result is the sequential scan's whatever the
//       split --, and applies delta to the potentials.  Two barriers per step; at most R (R + 1) / 2 steps for R rows.
// Every float32 operation is written once, in a helper both phases share, and the build contracts nothing, so a gain has the same
// bits wherever it is computed.  The kernel is bound by latency (barriers and dependent LDS reads), not by throughput.
#include <hip/hip_runtime.h>

#include <climits>

#include "das_kernels.h"

namespace bf {
namespace {

constexpr int kLanes = 64;
constexpr int kBoxTrackThreads = 256;
constexpr int kMaxWaves = kBoxTrackThreads / kLanes;
constexpr int kMaxCols = kBoxTrackMaxBoxes + kBoxTrackMaxSlots;
constexpr int kSlotWords = 20;
static_assert(kBoxTrackMaxSlots <= kLanes, "a lane of wave 0 per slot");
static_assert((kBoxTrackMaxBoxes + kBoxTrackThreads - 1) / kBoxTrackThreads <= 32, "a lane's rows fit a 32-bit mask");

struct BoxTrackShared {
    float4 dbox[kBoxTrackMaxBoxes];          // the detections' x1, y1, x2, y2 in row order
    int drow[kBoxTrackMaxBoxes];             // ... and their rows in d_boxes
    double minv[kMaxCols], V[kMaxCols];      // the assignment: per-column minima and potentials,
    double U[kBoxTrackMaxSlots];             //     per-row potentials,
    int way[kMaxCols], row_of[kMaxCols];     //     predecessor column, assigned row (-1 = none)
    unsigned char used[kMaxCols];
    unsigned char dtaken[kBoxTrackMaxBoxes]; // a slot took this detection
    float4 tbox[kBoxTrackMaxSlots];          // the live slots' predicted boxes, by row
    int rowcnt[kBoxTrackMaxSlots], rowhit[kBoxTrackMaxSlots], row_col[kBoxTrackMaxSlots];
    double part_val[kMaxWaves];
    int part_col[kMaxWaves];
    int scan[kMaxWaves];
    int n_rows, multi;
};

__device__ __forceinline__ float bt_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float bt_min(float a, float b) { return a < b ? a : b; }

// step 2 of the definition, d a detection and t a track's box
__device__ __forceinline__ float bt_gain(const float4 d, const float4 t)
{
    const float xx1 = bt_max(d.x, t.x), yy1 = bt_max(d.y, t.y), xx2 = bt_min(d.z, t.z), yy2 = bt_min(d.w, t.w);
    const float w = bt_max(0.0f, xx2 - xx1), h = bt_max(0.0f, yy2 - yy1);
    const float wh = w * h;
    const float o = wh / (((d.z - d.x) * (d.w - d.y) + (t.z - t.x) * (t.w - t.y)) - wh);
    return o > 0.0f ? o : 0.0f;
}

__device__ __forceinline__ float4 bt_state_box(float u, float v, float s, float r)
{
    const float w = sqrtf(s * r);
    const float h = s / w;
    const float hw = 0.5f * w, hh = 0.5f * h;
    return make_float4(u - hw, v - hh, u + hw, v + hh);
}

__device__ __forceinline__ float4 bt_measurement(const float4 d)
{
    const float w = d.z - d.x, h = d.w - d.y;
    return make_float4(d.x + 0.5f * w, d.y + 0.5f * h, w * h, w / h);
}

__device__ __forceinline__ bool bt_finite4(const float4 b) { return isfinite(b.x) && isfinite(b.y) && isfinite(b.z) && isfinite(b.w); }

struct Block { float p00, p01, p11; };

__device__ __forceinline__ void bt_predict(Block& p, float q0, float q1)
{
    const float a = p.p00 + p.p01, b = p.p01 + p.p11;
    p.p00 = (a + b) + q0;
    p.p01 = b;
    p.p11 = p.p11 + q1;
}

// the gains of a block measured in its first state with noise r, and its Joseph-form covariance
__device__ __forceinline__ void bt_update(Block& p, float r, float& k0, float& k1)
{
    const float S = p.p00 + r;
    k0 = p.p00 / S;
    k1 = p.p01 / S;
    const float m = 1.0f - k0;
    const float n00 = (m * m) * p.p00 + (k0 * k0) * r;
    const float t = p.p01 - k1 * p.p00;
    const float n01 = m * t + (k0 * k1) * r;
    const float kk = k1 * k1;
    const float n11 = ((p.p11 - (2.0f * k1) * p.p01) + kk * p.p00) + kk * r;
    p.p00 = n00; p.p01 = n01; p.p11 = n11;
}

__device__ __forceinline__ bool bt_less(double a, int ja, double b, int jb) { return a < b || (a == b && ja < jb); }

// The definition's ASSIGNMENT over sh.tbox[0 .. R) x sh.dbox[0 .. D) -> sh.row_col[0 .. R).  Every lane of the workgroup calls it.
__device__ void bt_assign(BoxTrackShared& sh, const int R, const int D)
{
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kLanes - 1), wave = tid / kLanes, waves = T / kLanes;
    const int C = D + R;
    for (int j = tid; j < C; j += T) { sh.V[j] = 0.0; sh.row_of[j] = -1; }
    if (tid < R) sh.U[tid] = 0.0;
    for (int i = 0; i < R; ++i) {
        for (int j = tid; j < C; j += T) { sh.minv[j] = INFINITY; sh.used[j] = 0; sh.way[j] = -1; }
        __syncthreads();
        int i0 = i, j0 = -1;
        for (;;) {
            const float4 t = sh.tbox[i0];
            const double ui0 = sh.U[i0];
            double bv = INFINITY;
            int bj = INT_MAX;
            for (int j = tid; j < C; j += T) {
                if (sh.used[j]) continue;
                const double cost = j < D ? -(double)bt_gain(sh.dbox[j], t) : 0.0;
                const double cur = (cost - ui0) - sh.V[j];
                double m = sh.minv[j];
                if (cur < m) { m = cur; sh.minv[j] = cur; sh.way[j] = j0; }
                if (bt_less(m, j, bv, bj)) { bv = m; bj = j; }
            }
            for (int off = kLanes / 2; off > 0; off >>= 1) {
                const double ov = __shfl_xor(bv, off, kLanes);
                const int oj = __shfl_xor(bj, off, kLanes);
                if (bt_less(ov, oj, bv, bj)) { bv = ov; bj = oj; }
            }
            if (lane == 0) { sh.part_val[wave] = bv; sh.part_col[wave] = bj; }
            __syncthreads();
            bv = sh.part_val[0]; bj = sh.part_col[0];
            for (int w = 1; w < waves; ++w) {
                const double ov = sh.part_val[w];
                const int oj = sh.part_col[w];
                if (bt_less(ov, oj, bv, bj)) { bv = ov; bj = oj; }
            }
            const double delta = bv;                     // (uniform: an unused column always exists, C > the used ones)
            const int j1 = bj;
            for (int j = tid; j < C; j += T) {
                if (sh.used[j]) {
                    const int r = sh.row_of[j];          // (the rows of distinct used columns are distinct, and none is i)
                    sh.U[r] = sh.U[r] + delta;
                    sh.V[j] = sh.V[j] - delta;
                } else {
                    sh.minv[j] = sh.minv[j] - delta;
                }
            }
            if (tid == 0) sh.U[i] = sh.U[i] + delta;
            if (j1 % T == tid) sh.used[j1] = 1;          // by the lane that owns the column, after it has treated it as unused
            __syncthreads();
            j0 = j1;
            const int r = sh.row_of[j0];
            if (r < 0) break;
            i0 = r;
        }
        if (tid == 0) {
            do {
                const int jp = sh.way[j0];
                sh.row_of[j0] = jp < 0 ? i : sh.row_of[jp];
                j0 = jp;
            } while (j0 >= 0);
        }
        __syncthreads();                                 // row_of is final for this row; way, minv, used may be reset
    }
    for (int j = tid; j < C; j += T) {
        const int r = sh.row_of[j];
        if (r >= 0) sh.row_col[r] = j;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kBoxTrackThreads) box_track_kernel(const float* __restrict__ boxes, const int* __restrict__ n_boxes, int frames, int max_boxes,
                                                                     float conf, int slots, float thr, int max_age, int min_hits, int* __restrict__ state,
                                                                     float* __restrict__ tracks, int* __restrict__ ids, int* __restrict__ match,
                                                                     float* __restrict__ live_out, int* __restrict__ counts)
{
    __shared__ BoxTrackShared sh;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kLanes - 1), wave = tid / kLanes, waves = T / kLanes;
    const bool mine = tid < slots;                       // (slots <= 64: the owners are lanes of wave 0)
    int* const sw = state + 4 + kSlotWords * tid;
    float* const sf = reinterpret_cast<float*>(sw);
    // wave 0's copy of the stream counters is the one that is stored
    int next_id = state[0], frame_count = state[1];
    int id = 0, tsu = 0, hits = 0, streak = 0;
    float u = 0.0f, v = 0.0f, s = 0.0f, r = 0.0f, du = 0.0f, dv = 0.0f, ds = 0.0f, c = 0.0f;
    Block A = {0.0f, 0.0f, 0.0f}, B = {0.0f, 0.0f, 0.0f};
    if (mine) {
        id = sw[0]; tsu = sw[1]; hits = sw[2]; streak = sw[3];
        u = sf[4]; v = sf[5]; s = sf[6]; r = sf[7]; du = sf[8]; dv = sf[9]; ds = sf[10];
        A.p00 = sf[11]; A.p01 = sf[12]; A.p11 = sf[13]; B.p00 = sf[14]; B.p01 = sf[15]; B.p11 = sf[16]; c = sf[17];
    }
    const int per = (max_boxes + T - 1) / T;             // rows per lane, consecutive
    for (int f = 0; f < frames; ++f) {
        const float* const rows = boxes + (size_t)f * max_boxes * 6;
        const int n = n_boxes ? min(max(n_boxes[f], 0), max_boxes) : max_boxes;
        // ---- rows: validate, scan, compact in row order
        unsigned valid = 0;
        const int j_lo = tid * per;
        for (int k = 0; k < per; ++k) {
            const int j = j_lo + k;
            if (j >= n) break;
            const float* const b = rows + (size_t)j * 6;
            const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3], sc = b[4];
            if (isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && isfinite(sc) && x2 > x1 && y2 > y1 && sc > conf) valid |= 1u << k;
        }
        const int cnt = __popc(valid);
        int incl = cnt;
        for (int off = 1; off < kLanes; off <<= 1) {
            const int o = __shfl_up(incl, off, kLanes);
            if (lane >= off) incl += o;
        }
        if (lane == kLanes - 1) sh.scan[wave] = incl;
        for (int j = tid; j < kBoxTrackMaxBoxes; j += T) sh.dtaken[j] = 0;
        if (tid < kBoxTrackMaxSlots) sh.rowcnt[tid] = 0;
        if (tid == 0) sh.multi = 0;
        __syncthreads();
        int D = 0, pos = incl - cnt;
        for (int w = 0; w < waves; ++w) {
            const int t = sh.scan[w];
            if (w < wave) pos += t;
            D += t;
        }
        for (int k = 0; k < per; ++k) {
            if (!((valid >> k) & 1u)) continue;
            const float* const b = rows + (size_t)(j_lo + k) * 6;
            sh.dbox[pos] = make_float4(b[0], b[1], b[2], b[3]);
            sh.drow[pos] = j_lo + k;
            ++pos;
        }
        const int ignored = n - D;
        // ---- 1. predict (wave 0)
        int born = 0, ended = 0, dropped = 0, my_row = 0;
        float4 pb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (wave == 0) {
            frame_count += 1;
            bool ends = false;
            if (id != 0) {
                if (ds + s <= 0.0f) ds = 0.0f;
                u = u + du;
                v = v + dv;
                s = s + ds;
                bt_predict(A, 1.0f, 0.01f);
                bt_predict(B, 1.0f, 1e-4f);
                c = c + 1.0f;
                if (tsu > 0) streak = 0;
                tsu += 1;
                pb = bt_state_box(u, v, s, r);
                if (!bt_finite4(pb)) { id = 0; ends = true; }
            }
            ended = __popcll(__ballot(ends));
            const unsigned long long alive = __ballot(id != 0);
            my_row = __popcll(alive & ((1ull << lane) - 1ull));
            if (id != 0) sh.tbox[my_row] = pb;
            if (lane == 0) sh.n_rows = __popcll(alive);
        }
        __syncthreads();                                 // dbox, drow, tbox, n_rows and the cleared flags are visible
        const int R = sh.n_rows;
        // ---- 2. gains and over-threshold counts, 3. association
        int took = -1;                                   // the detection (index into dbox) this lane's slot takes
        if (R > 0 && D > 0) {                            // (uniform)
            for (int j = tid; j < D; j += T) {
                const float4 d = sh.dbox[j];
                int cc = 0;
                for (int i = 0; i < R; ++i) {
                    if (bt_gain(d, sh.tbox[i]) > thr) {
                        ++cc;
                        atomicAdd(&sh.rowcnt[i], 1);
                        sh.rowhit[i] = j;                // (read only where the row's count is 1: a single writer)
                    }
                }
                if (cc > 1) sh.multi = 1;
            }
            __syncthreads();
            if (tid < R && sh.rowcnt[tid] > 1) sh.multi = 1;
            __syncthreads();
            if (sh.multi) {                              // (uniform)
                bt_assign(sh, R, D);
                if (wave == 0 && id != 0) {
                    const int col = sh.row_col[my_row];
                    if (col < D && !(bt_gain(sh.dbox[col], pb) < thr)) took = col;
                }
            } else if (wave == 0 && id != 0 && sh.rowcnt[my_row] == 1) {
                took = sh.rowhit[my_row];
            }
            if (took >= 0) sh.dtaken[took] = 1;
            __syncthreads();
        }
        if (wave == 0) {
            int mrow = -1;                               // the row of d_boxes behind `took`, or the one the slot is born from
            // ---- 4. update
            if (took >= 0) {
                mrow = sh.drow[took];
                const float4 z = bt_measurement(sh.dbox[took]);
                tsu = 0;
                hits += 1;
                streak += 1;
                float k0, k1;
                bt_update(A, 1.0f, k0, k1);
                float e = z.x - u;
                u = u + k0 * e;
                du = du + k1 * e;
                e = z.y - v;
                v = v + k0 * e;
                dv = dv + k1 * e;
                bt_update(B, 10.0f, k0, k1);
                e = z.z - s;
                s = s + k0 * e;
                ds = ds + k1 * e;
                const float S = c + 10.0f;
                const float k = c / S;
                e = z.w - r;
                r = r + k * e;
                const float m = 1.0f - k;
                c = (m * m) * c + (k * k) * 10.0f;
            }
            // ---- 5. birth: the detections left, in row order, each into the lowest free slot
            unsigned long long free_slots = __ballot(mine && id == 0);
            for (int base = 0; base < D; base += kLanes) {
                const int j = base + lane;
                unsigned long long avail = __ballot(j < D && !sh.dtaken[j]);
                for (; avail; avail &= avail - 1) {
                    if (!free_slots) { dropped += __popcll(avail); break; }
                    const int jj = base + __ffsll((long long)avail) - 1;
                    const int slot = __ffsll((long long)free_slots) - 1;
                    free_slots &= free_slots - 1;
                    next_id += 1;
                    born += 1;
                    if (lane == slot) {
                        const float4 z = bt_measurement(sh.dbox[jj]);
                        id = next_id; tsu = 0; hits = 0; streak = 0; mrow = sh.drow[jj];
                        u = z.x; v = z.y; s = z.z; r = z.w; du = 0.0f; dv = 0.0f; ds = 0.0f;
                        A.p00 = 10.0f; A.p01 = 0.0f; A.p11 = 1e4f; B = A; c = 10.0f;
                    }
                }
            }
            // ---- 6. report, then retire
            bool ends = false;
            if (mine) {
                const size_t o = (size_t)f * slots + lane;
                const bool live = id != 0;
                const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float4 sb = live ? bt_state_box(u, v, s, r) : zero;
                const bool reported = live && tsu < 1 && (streak >= min_hits || frame_count <= min_hits);
                const float4 tb = reported ? sb : zero;
                float* const tr = tracks + o * 6;
                tr[0] = tb.x; tr[1] = tb.y; tr[2] = tb.z; tr[3] = tb.w;
                tr[4] = reported ? rows[(size_t)mrow * 6 + 4] : 0.0f;
                tr[5] = reported ? rows[(size_t)mrow * 6 + 5] : 0.0f;
                if (ids) ids[o] = id;
                if (match) match[o] = live ? mrow : -1;
                if (live_out) { live_out[o * 4 + 0] = sb.x; live_out[o * 4 + 1] = sb.y; live_out[o * 4 + 2] = sb.z; live_out[o * 4 + 3] = sb.w; }
                ends = live && tsu > max_age;
                if (ends) id = 0;
            }
            ended += __popcll(__ballot(ends));
            if (counts && lane < 4) counts[(size_t)f * 4 + lane] = lane == 0 ? born : lane == 1 ? ended : lane == 2 ? dropped : ignored;
        }
        __syncthreads();                                 // every read of this frame's LDS is done before the next frame's rows land
    }
    if (tid == 0) { state[0] = next_id; state[1] = frame_count; state[2] = 0; state[3] = 0; }
    if (mine) {
        const bool live = id != 0;                       // a free slot is stored as zeros
        sw[0] = id; sw[1] = live ? tsu : 0; sw[2] = live ? hits : 0; sw[3] = live ? streak : 0;
        sf[4] = live ? u : 0.0f; sf[5] = live ? v : 0.0f; sf[6] = live ? s : 0.0f; sf[7] = live ? r : 0.0f;
        sf[8] = live ? du : 0.0f; sf[9] = live ? dv : 0.0f; sf[10] = live ? ds : 0.0f;
        sf[11] = live ? A.p00 : 0.0f; sf[12] = live ? A.p01 : 0.0f; sf[13] = live ? A.p11 : 0.0f;
        sf[14] = live ? B.p00 : 0.0f; sf[15] = live ? B.p01 : 0.0f; sf[16] = live ? B.p11 : 0.0f;
        sf[17] = live ? c : 0.0f; sw[18] = 0; sw[19] = 0;
    }
}

}  // namespace

hipError_t launch_track_boxes(const float* d_boxes, const int* d_n_boxes, int frames, int max_boxes, float conf, int slots, float iou_threshold, int max_age,
                              int min_hits, int* d_state, float* d_tracks, int* d_ids, int* d_match, float* d_live, int* d_counts, hipStream_t stream)
{
    if (frames < 1 || max_boxes < 1 || max_boxes > kBoxTrackMaxBoxes || slots < 1 || slots > kBoxTrackMaxSlots) return hipErrorInvalidValue;
    hipLaunchKernelGGL(box_track_kernel, dim3(1), dim3(kBoxTrackThreads), 0, stream, d_boxes, d_n_boxes, frames, max_boxes, conf, slots, iou_threshold, max_age,
                       min_hits, d_state, d_tracks, d_ids, d_match, d_live, d_counts);
    return hipGetLastError();
}

}  // namespace bf
