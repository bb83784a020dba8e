// Internal interface between the C-ABI layer (beamformer_api.cpp) and the gfx950 kernels (das_kernels.hip, das_strided.hip, das_pair.hip, das_cells.hip, planned by das_plan.cpp).
// Not installed; the public boundary is include/beamformer_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bf {

// Delay flavours of the reference's four beamformers (PC/src/algorithms/*.c).
enum Algo : int {
    ALGO_PAD = 0,        // pad_and_sum.c        integer shift
    ALGO_LERP = 1,       // lerp_and_sum.c       integer shift + linear interpolation
    ALGO_HYBRID = 2,     // hybrid_convolve_and_sum.c  integer shift + T-tap fractional FIR
    ALGO_FIR_NAIVE = 3,  // convolve_and_sum.c   T-tap FIR, sequential tap order (mimo_convolve_naive)
    ALGO_FIR_VEC = 4,    // convolve_and_sum.c   T-tap FIR, AVX2 lane/tree order  (mimo_convolve_vectorized)
    ALGO_COUNT = 5
};

// One steering-table set resident in HBM (what load_coefficients_* uploads).
struct DeviceTables {
    const int32_t* whole = nullptr;  // [D][M]      integer delays            (pad, lerp, hybrid)
    const float* frac = nullptr;     // [D][M]      h = 1 - frac              (lerp)
    const float* taps = nullptr;     // [D][M][T]   FIR taps                  (hybrid, fir)
    int max_whole = 0;               // max over the table, clamped to N (sizes the zero prefix in LDS)
    bool digest_direct = false;      // digest is in the [D][M] layout: run the direction-outer (DIRECT) kernel variant (plan_das sizes the chunk for its four copies)
    const int32_t* digest = nullptr; // LDS byte offsets for the shifted-copies layout (launch_digest): grouped by the wave's directions for pad / lerp
                                     // (+ the lerp weights in the same order), [D][M] for hybrid; null when not built
    long long digest_order_off = 0;  // grouped digest of the pad / lerp pair kernels: where its sweep order starts (4-byte elements); 0: position = direction
};

// Geometry of one launch.  Directions [dir_begin, dir_end) of every frame in [0, frames).
struct DasLaunch {
    const float* signals;    // [frames][m_total][N] device, mic-major (receiver.c:94-151 layout)
    float* images;           // [frames][image_stride] device; direction d lands at images[f*image_stride + d - image_origin]
    const int32_t* mics;     // [M] device copy of adaptive_array (row of `signals` for each active slot)
    DeviceTables tab;
    int algo;
    int n_mics;              // M  = n of the reference call
    int m_total;             // rows in one frame of `signals`
    int n_samples;           // N
    int n_taps;              // T
    int n_dirs;              // D  = MAX_RES_X * MAX_RES_Y
    int dir_begin, dir_end;  // shard of the direction grid handled by this launch
    int image_stride, image_origin;
    int frames;
};

// The kernel family of a batched delay-and-sum launch.  plan_das picks it, once (pick_family, das_plan.cpp); the launchers, the digest and
// the C-ABI read it.  What follows from a family -- frames per workgroup, digest, the numbers bf_last_das_variant / bf_last_das_rows
// report -- is family_traits' table (das_geometry.h).
enum DasFamily : int {
    DAS_STRIDED = 0,     // das_mimo_kernel: N <= 128; the FIR flavours with other than 8 taps or beyond 256 samples; stream maps, listed directions
    DAS_COPIES,          // das_copies_kernel: pad / lerp beyond 128 samples that no kernel below takes -- the one-frame sweep
    DAS_COPIES_DIRECT,   // das_copies_kernel<.., DIRECT>: pad / lerp on a table without structure (DeviceTables::digest_direct) -- direction-outer, four copies
    DAS_COPIES_FIR,      // das_copies_kernel: the 8-tap FIR flavours at 128 < N <= 256
    DAS_PAIR_PAD,        // das_pair_kernel: pad at N <= 256, the fixed row stride, a multiple of 16 mics, two or more frames -- two frames per workgroup
    DAS_PAIR_LERP,       // das_pair2_kernel: lerp under the same conditions -- both frames interleaved in the rows, sample by sample
    DAS_PAIR_CELLS,      // das_pair2_cells_kernel: ... and a multiple of 32 mics -- rows of 16-byte cells (mic_chunk, row_stride and lds_bytes stay das_pair2_kernel's)
    DAS_PAIR_FIR,        // das_hybrid_pair_kernel: the 8-tap FIR flavours under the pair conditions
    DAS_LONG,            // das_long_kernel: pad / lerp at 256 < N <= 1024 whose mics are whole halves of 16 / nseg -- LDS image in two halves
    DAS_FAMILY_COUNT
};

// Plan chosen on the host for a launch (exposed so tests can check LDS sizing without a GPU).
struct DasPlan {
    DasFamily family;
    int nc;          // 64-sample segments per row (N rounded up to 64*nc)
    int lead;        // zero floats in front of every LDS row
    int row_stride;  // floats per LDS row
    int mic_chunk;   // mics staged per pass
    int n_chunks;
    int waves;       // waves per workgroup
    int scratch_off; // float offset of the per-wave power scratch in LDS
    int srow;        // scratch row stride in floats (64*nc + 4)
    int pbw;         // scratch rows (finished directions) per wave
    int dpw;         // directions a wave carries across mic chunks
    int frame_inner; // workgroup id -> (tile, frame): 1 = an XCD runs all frames of a tile back to back (tables beyond the L2s)
    int copies;      // shifted copies per staged array (0: strided; 2: the sweeps of pad / lerp and the FIR pair kernel, 4: the one-frame FIR flavours and DAS_COPIES_DIRECT)
    int tile_dirs;   // directions per workgroup
    int n_tiles;     // padded to a multiple of 8 (XCD affinity: tile % 8 == workgroup id % 8) unless the launch's table fits every XCD's L2
    size_t lds_bytes;
};

// Returns 0 and fills `plan`, or a negative value when the shape is unsupported (message in `why`).
int plan_das(const DasLaunch& L, int n_cus, DasPlan* plan, const char** why);

// Build DeviceTables::digest for the layout `plan` describes (shifted-copies layout only).
size_t digest_elements(const DasLaunch& L, const DasPlan& plan);   // 4-byte elements the digest of this launch needs (0: none)
// The layout is digest_layout's (das_geometry.h): flat [D][M] or grouped, as the plan's family takes it.
// d_reload_count (grouped build, optional) receives the number of direction steps whose delay differs from the previous one's.
// order_off (grouped build; 0: none): the sweep order already stored at d_digest + order_off -- int32, one entry per position of the
// launch padded to whole groups of plan.dpw by repeating the last (digest_order_offset says where; sweep_order.h what) -- in which
// the digest is then grouped and its re-reads counted.
long long digest_order_offset(const DasLaunch& L, const DasPlan& plan);    // 0: the plan's kernel takes no order (all but the pad / lerp pair kernels)
hipError_t launch_digest(const DasLaunch& L, const DasPlan& plan, int32_t* d_digest, unsigned long long* d_reload_count, long long order_off, hipStream_t stream);
long long digest_shareable_steps(const DasLaunch& L, const DasPlan& plan);

// Enqueue on `stream`; no host synchronisation, no allocation (graph-capturable).
hipError_t launch_das(const DasLaunch& L, const DasPlan& plan, hipStream_t stream);

// One steered beam -> raw out[N] (miso_pad / miso_lerp / miso_convolve_*).  `row_offset` is the reference's flat
// table `offset` (d*M); `init_dev` (may be null) seeds the accumulators, which turns the launch into the
// single-signal helpers `out += delay(signal)` (pad_delay, lerp_delay, convolve_*_delay*).
hipError_t launch_miso(const DasLaunch& L, const DasPlan& plan, long long row_offset, const float* init_dev, float* out_dev,
                       hipStream_t stream);

// Steered beams of a batch (bf_miso_device): the same kernel with one workgroup per (frame, group of up to kMisoWaves beams),
// one wave per beam.  d_offsets int32 [L.frames][beams] (table offsets, checked in the kernel against `entries`), d_out float32
// [L.frames][beams][out_stride], d_status int32 [L.frames][beams] or null; gain 0 = raw beams.  `plan` is the one-direction,
// one-frame plan run_miso_host uses (LDS is per workgroup, so its chunk sizing holds for any wave count).
constexpr int kMisoWaves = 16;
hipError_t launch_miso_batch(const DasLaunch& L, const DasPlan& plan, const int32_t* d_offsets, int beams, long long entries, float gain,
                             float* d_out, int out_stride, int* d_status, hipStream_t stream);

// Continuous-stream mode (bf_das_stream_device / bf_miso_stream_device; pad and lerp): the samples a delay reaches before the start
// of frame f come from frame f - 1 of the launch, for frame 0 from d_prev (float32 [m_total][N], the frame that started `hop`
// samples earlier; null = silence).  stream_history: samples of history a table needs (max_whole for pad, max_whole + 1 for lerp,
// -1 for the other flavours); the launches want history <= hop <= N.
int stream_history(int algo, int max_whole);
// Maps: always the strided layout (das_mimo_kernel<.., HIST = true>); `plan` comes from plan_stream_maps, never from plan_das.
int plan_stream_maps(const DasLaunch& L, int n_cus, DasPlan* plan, const char** why);
hipError_t launch_stream_maps(const DasLaunch& L, const DasPlan& plan, const float* d_prev, int hop, hipStream_t stream);
// Beams (das_miso_kernel<.., HIST = true>): `plan` is the one-direction, one-frame plan launch_miso_batch takes.
hipError_t launch_stream_beams(const DasLaunch& L, const DasPlan& plan, const float* d_prev, int hop, const int32_t* d_offsets, int beams,
                               long long entries, float gain, float* d_out, int out_stride, int* d_status, hipStream_t stream);

// Map values at listed directions (bf_das_select_device / bf_das_select_stream_device; das_select_kernel): the mean power of the beam at
// every table offset of a device list, d_offsets int32 [L.frames][count] (per_frame != 0) or [count] for all frames, judged in the kernel
// as launch_miso_batch judges them (d_status int32 [L.frames][count] or null; a rejected entry's power is NaN).  The launch describes the
// LIST: L.dir_begin = 0, L.dir_end = count, L.images float32 [L.frames][L.image_stride] with list index b at column b, L.image_origin = 0.
// `plan` comes from plan_select: the strided layout at every N, tiles of the list.  stream = true sizes the rows for launch_select_stream
// (pad and lerp; d_prev / hop as launch_stream_maps), false for launch_select (pad, lerp, hybrid, the vectorized FIR).
int plan_select(const DasLaunch& L, bool stream, int n_cus, DasPlan* plan, const char** why);
hipError_t launch_select(const DasLaunch& L, const DasPlan& plan, const int32_t* d_offsets, int per_frame, long long entries, int* d_status, hipStream_t stream);
hipError_t launch_select_stream(const DasLaunch& L, const DasPlan& plan, const float* d_prev, int hop, const int32_t* d_offsets, int per_frame, long long entries,
                                int* d_status, hipStream_t stream);

// bf_remove_sources_device (remove_sources.hip; pad and lerp): d_residual = d_signals - c * (adjoint of the delay operator)(beams), rows of the frames
// named by d_row_slot int32 [m_total] (slot m of the adaptive array, or -1: the row is copied).  d_offsets / d_status / entries as
// launch_miso_batch; d_beams float32 [frames][beams][beam_stride], rows of rejected offsets never read.  d_residual may equal d_signals.
constexpr int kRemoveMaxBeams = 64;
hipError_t launch_remove_sources(int algo, const float* d_signals, float* d_residual, int m_total, int frames, int n_samples, int n_mics,
                                 const int32_t* d_row_slot, const DeviceTables& tab, long long entries, const int32_t* d_offsets, int beams,
                                 const float* d_beams, int beam_stride, float c, int* d_status, hipStream_t stream);

// FPGA protocol-v2 datagrams (one per sample instant) -> float32 [n_mics_out][n_samples] mic-major frame (receiver.c:94-151).
hipError_t launch_ingest(const void* d_packets, int packet_stride, int header_bytes, int n_samples, int n_mics_out, int stream_len,
                         int rows, int columns, float* d_frame, hipStream_t stream);
// A stream of datagrams -> float32 [frames][m_total][n_samples], frame f from datagrams [f*hop, f*hop + n_samples) (bf_ingest_stream_device):
// rows named by d_row_mask (m_total bytes, or null) and rows [n_mics_out, m_total) are zero; d_status int32 [frames][4] or null.
hipError_t launch_ingest_stream(const void* d_packets, int packet_stride, int n_samples, int stream_len, int n_mics_out, int rows, int columns,
                                int hop, int frames, int m_total, const unsigned char* d_row_mask, int protocol_ver, int n_arrays,
                                float* d_frames, int* d_status, hipStream_t stream);

// heat-map post-processing (PC/src/visual.py:143-188, 295-322, 450-452); see heatmap_kernels.hip
hipError_t launch_colorize(const float* d_power, int frames, int res_x, int res_y, float threshold, float amount, float exponent,
                           unsigned char* d_small, int* d_overlay, hipStream_t stream);
hipError_t launch_overlay(const unsigned char* d_small, int frames, int small_w, int small_h, int out_w, int out_h, unsigned char* d_prev,
                          const unsigned char* d_camera, unsigned char* d_out, float w_prev, float w_new, float w_cam, float w_heat,
                          hipStream_t stream);
// uint8 BGR frame [sh][sw][3] -> [oh][ow][3]: cv2.resize(INTER_LINEAR) to new_w x new_h at (top, left), the rest = value (heatmap_kernels.hip)
hipError_t launch_letterbox(const unsigned char* d_src, int sh, int sw, unsigned char* d_out, int oh, int ow, int new_h, int new_w, int top, int left, int value,
                            hipStream_t stream);
hipError_t launch_power_center(const float* d_power, int frames, int rows, int cols, float* d_centers, float* d_workspace, hipStream_t stream);
// d_offsets[f] = argmax_{j < n_dirs} d_power[f * image_stride + j] * offset_per_dir, np.argmax's rules (first maximum, first NaN)
hipError_t launch_peak_offsets(const float* d_power, int frames, int image_stride, int n_dirs, int offset_per_dir, int* d_offsets, hipStream_t stream);
// bf_peaks_device: the k loudest sources of every map that are the maximum of their (2 radius + 1)^2 window.  Maps that fit LDS take one
// workgroup per frame and no workspace; larger ones three launches over peaks_workspace_words(...) 8-byte words (0: none needed).
size_t peaks_workspace_words(int frames, int rows, int cols, int k);
hipError_t launch_peaks(const float* d_power, int frames, int image_stride, int rows, int cols, int radius, int k, float floor_rel, float floor_abs,
                        int offset_per_dir, int* d_offsets, float* d_values, int* d_counts, unsigned long long* d_workspace, size_t workspace_words,
                        hipStream_t stream);
// bf_track_sources_device: bf_peaks_device's [frames][k] offsets -> [frames][slots] offsets whose slot s is one source over time (greedy
// gated nearest neighbour + a constant-velocity Kalman filter per slot).  One launch of one wave; d_state (4 + 12 * slots words)
// carries the tracks from call to call.  k and slots at most kTrackMaxSlots; the four outputs after d_track_offsets may be null.
constexpr int kTrackMaxSlots = 64;
hipError_t launch_track_sources(const int* d_offsets, int frames, int k, int rows, int cols, int offset_per_dir, int slots, float gate2, int max_miss,
                                int min_hits, float q, float r, int* d_state, int* d_track_offsets, int* d_track_ids, float* d_track_pos, int* d_match,
                                int* d_counts, hipStream_t stream);
// bf_fuse_boxes_device: every detector box's footprint on the map -> its loudest cell, its centre cell and its rect; every source's
// best-scored box.  Maps of at most kFuseStageMax directions (60 KiB of LDS, two workgroups to a CU) are staged, larger ones read
// through L2.  One launch for the boxes, a second of one wave per frame when n_src > 0 or d_counts is given; n_src at most
// kFuseMaxSources; no workspace.
constexpr int kFuseMaxSources = 64;
constexpr int kFuseStageMax = 15360;
hipError_t launch_fuse_boxes(const float* d_power, int frames, int image_stride, int rows, int cols, int offset_per_dir, const float* d_boxes,
                             const int* d_box_counts, int max_boxes, int img_w, int img_h, float conf, const int* d_src_offsets, int n_src,
                             int* d_peak_offsets, float* d_peak_power, int* d_center_offsets, int* d_rects, int* d_src_box, int* d_counts, hipStream_t stream);

// bf_track_boxes_device (box_track.hip): the detector's [frames][max_boxes][6] rows -> [frames][slots][6] rows whose slot s is one object
// over time (SORT: a constant-velocity Kalman filter per box, IoU association by the optimal assignment, max_age / min_hits).  One
// launch of one workgroup; d_state (4 + 20 * slots words) carries the tracks from call to call; d_n_boxes and the four outputs after
// d_tracks may be null; no workspace.
constexpr int kBoxTrackMaxSlots = 64;
constexpr int kBoxTrackMaxBoxes = 1024;
hipError_t launch_track_boxes(const float* d_boxes, const int* d_n_boxes, int frames, int max_boxes, float conf, int slots, float iou_threshold, int max_age,
                              int min_hits, int* d_state, float* d_tracks, int* d_ids, int* d_match, float* d_live, int* d_counts, hipStream_t stream);

// bf_match_boxes_device (patch_match.hip): every box of d_boxes float32 [frames][max_boxes][box_stride] sought in image f of d_images uint8
// [frames][height][width][3] by the normalised cross-correlation of its patch of image f - 1 (d_prev for f = 0, null = none) -> the moved box,
// the score, the shift and a status per row.  One launch of frames * max_boxes workgroups, all of a CU's LDS to each; no workspace, no atomics.
constexpr int kMatchMaxPixels = 16384;
constexpr int kMatchMaxBoxes = 1024;
constexpr int kMatchMaxSide = 8192;
hipError_t launch_match_boxes(const unsigned char* d_images, const unsigned char* d_prev, int frames, int height, int width, const float* d_boxes, int box_stride,
                              const int* d_n_boxes, int max_boxes, int t_pct, int s_pct, float* d_moved, float* d_score, int* d_shift, int* d_status,
                              hipStream_t stream);
// bf_smooth_boxes_device (patch_match.hip): one frame of detector rows and the match results of the previous frame's kept boxes (d_state, 4 + 4 * slots
// words) -> the rows with the reference's hysteresis applied to their scores, and the new kept boxes in d_state.  One launch of one workgroup.
constexpr int kSmoothMaxSlots = 64;
hipError_t launch_smooth_boxes(const float* d_boxes, const int* d_n_boxes, int max_boxes, float conf_low, float conf_high, float iou_threshold, float corr_threshold,
                               int slots, const float* d_moved, const float* d_score, const int* d_status, int* d_state, float* d_out, int* d_boosted,
                               int* d_counts, hipStream_t stream);

// bf_band_filter_device (band_filter.hip): `bands` FIRs of n_taps taps (d_taps float32 [bands][n_taps]) on every row of d_signals float32
// [frames][rows][n_samples] -> d_out float32 [bands][frames][rows][n_samples].  The n_taps - 1 samples before a row come from the
// frame before it (`hop` samples earlier; d_prev float32 [rows][n_samples] for frame 0, null = silence), hop 0 = zeros for every frame.
// One launch; no workspace.  d_out must not overlap the inputs (frame f - 1 is read while frame f is written).
constexpr int kBandMaxBands = 16;
hipError_t launch_band_filter(const float* d_signals, int rows, int frames, int n_samples, int hop, const float* d_prev, const float* d_taps, int n_taps,
                              int bands, float* d_out, hipStream_t stream);

// bf_filter_sum_device (filter_sum.hip): `beams` filter-and-sum beams of the n microphone rows d_mics (int32, device) of d_signals float32
// [frames][m_total][n_samples]: d_taps float32 [beams][n][n_taps], one FIR per (beam, microphone), the filtered rows summed in
// microphone order -> d_out float32 [frames][beams][out_stride] (floats past n_samples of a row untouched).  hop / d_prev as
// launch_band_filter.  One launch; no workspace, no atomics.  d_out must not overlap the inputs.  n_cus: compute units of the device
// (a batch that leaves most of them idle splits its microphones over more waves).
constexpr int kFilterSumMaxBeams = 16;
hipError_t launch_filter_sum(const float* d_signals, int m_total, int frames, int n_samples, int hop, const float* d_prev, const int32_t* d_mics, int n,
                             const float* d_taps, int n_taps, int beams, float* d_out, int out_stride, int n_cus, hipStream_t stream);
// Waves of a filter-and-sum workgroup: 1, 2, 4, 8 or 16 pins them (the launch still halves what the LDS cannot hold), 0 gives the
// choice back to the launch.  Returns the previous value, -1 for any other argument.  The result does not depend on it.
int filter_sum_waves(int waves);

// bf_lcmv_design_device (lcmv_design.hip): null-steering taps for launch_filter_sum, designed in float64 from one row of slot offsets.
// d_tau float64 [dirs][n], d_offsets int32 [sources]; bins [bin_lo, bin_hi] of the n_taps-point grid, K of them -> d_gains float64
// [sources][K][n][2] (the intermediate, and an output), d_taps float32 [sources][n][n_taps], d_kept int32 [sources][K][sources], d_status
// int32 [sources].  Two launches (gains, then taps); no workspace, no atomics.  The outputs must not overlap the inputs or each other.
constexpr int kLcmvMaxSources = 8;
constexpr int kLcmvMaxTaps = 1024;
hipError_t launch_lcmv_design(const double* d_tau, int dirs, int n, const int32_t* d_offsets, int sources, int offset_per_dir, int n_taps, int bin_lo, int bin_hi,
                              double rho, double* d_gains, float* d_taps, int32_t* d_kept, int32_t* d_status, hipStream_t stream);
// Its second launch on its own: gains float64 [sources][K][n][2] and the status the gains stage wrote -> d_taps (a beam whose status is
// not 0 gets zeros).  bf_mvdr_design_device ends with it.
hipError_t launch_lcmv_taps(const double* d_gains, const int32_t* d_status, int sources, int n, int n_taps, int bin_lo, int K, float* d_taps, hipStream_t stream);

// bf_mvdr_design_device (mvdr_design.hip): adaptive taps for launch_filter_sum from the covariance of the frames themselves, float64.
// Snapshots of n_taps samples (segment q of frame f starts at seg_first + q seg_hop; d_window float64 [n_taps] or null) -> d_snap float64
// [frames * segs][K][n][2]; their covariance per bin -> d_cov float64 [K][n][n][2] (Hermitian bit for bit); the loaded matrix's Cholesky
// factor -> d_chol float64 [K][n][n][2]; one MVDR solve per source slot -> d_gains float64 [sources][K][n][2]; launch_lcmv_taps -> d_taps.
// d_fallback int32 [K]: 1 where the trace was not finite and > 0 and the identity stood in.  Four launches; no atomics, no workspace
// beyond these buffers, which must not overlap the inputs or each other.  d_mics: the n rows (int32, device).
constexpr int kMvdrMaxMics = 256;
hipError_t launch_mvdr_design(const float* d_signals, int m_total, int frames, int n_samples, const int32_t* d_mics, int n, int seg_first, int seg_hop, int segs,
                              const double* d_window, const double* d_tau, int dirs, const int32_t* d_offsets, int sources, int offset_per_dir, int n_taps,
                              int bin_lo, int bin_hi, double loading, double* d_snap, double* d_cov, double* d_chol, double* d_gains, float* d_taps,
                              int32_t* d_status, int32_t* d_fallback, hipStream_t stream);
// bf_mvdr_learn_device (mvdr_design.hip): the same design from a covariance that is device STATE.  d_acc float64 [K][n][n][2] (the weighted
// sum of X X^H, Hermitian bit for bit once written) and d_mass float64 [1] are read and written in place, all-zero bytes being the empty
// state; d_weights float64 [frames] or null (all 1): a frame is learned iff its weight is finite and > 0, and a learned frame multiplies
// the state by forget, in (0, 1], before it is added.  d_used int32 [2] = (frames learned, weights refused).  d_cov = d_acc / d_mass (0
// where the mass is not > 0); factor, solve and taps are launch_mvdr_design's launches.  frames == 0 re-aims: no snapshots (d_signals,
// d_window, d_weights, d_snap are not read), the state is untouched, three launches instead of four.
hipError_t launch_mvdr_learn(const float* d_signals, int m_total, int frames, int n_samples, const int32_t* d_mics, int n, int seg_first, int seg_hop, int segs,
                             const double* d_window, const double* d_weights, double forget, const double* d_tau, int dirs, const int32_t* d_offsets, int sources,
                             int offset_per_dir, int n_taps, int bin_lo, int bin_hi, double loading, double* d_acc, double* d_mass, int32_t* d_used,
                             double* d_snap, double* d_cov, double* d_chol, double* d_gains, float* d_taps, int32_t* d_status, int32_t* d_fallback,
                             hipStream_t stream);

// bf_resample_device (resample.hip): the rows of a window stream (d_in float32 [frames][rows][in_stride], the last hop samples of every
// window of n, hop 0 = whole windows; d_prev float32 [rows][in_stride], the window before, null = silence) converted by up / down through
// the polyphase table d_taps float32 [up][n_taps] -> d_out float32 [rows][out_stride] and / or d_pcm int16 [cap][rows], cap =
// resample_capacity(frames * len, up, down).  d_state int32 [4] carries (input index of the next output, phase, 0, 0) between calls;
// d_clip int32 [rows] is added to (PCM samples out of range), d_count int32 [2] = (count, status).  Two launches: the conversion, which
// only reads the state, then one thread that advances it.  No workspace.  The written ranges must not overlap the read ones.
constexpr int kResampleMaxPhases = 16384;
constexpr int kResampleMaxTaps = 128;
long long resample_capacity(long long samples_in, int up, int down);      // ceil(samples_in * up / down); -1 on bad arguments
hipError_t launch_resample(const float* d_in, int rows, int frames, int n, int in_stride, int hop, const float* d_prev, const float* d_taps, int up, int down,
                           int n_taps, int32_t* d_state, float gain, float* d_out, int out_stride, short* d_pcm, int32_t* d_clip, int32_t* d_count,
                           hipStream_t stream);

// bf_spectrogram_device (spectrogram.hip): the rows of a flat stream (d_in float32 [rows][in_stride], `len` new samples each, or d_len[0] of
// them, read on the device) as frames of n_win samples every `hop`, windowed, transformed at n_fft points, |.|^2, through the filterbank
// d_bank float32 [n_bands][n_fft / 2 + 1] (null: the power spectrum) over d_support int32 [n_bands][2] (null: whole rows), linear
// (scale == 0) or scale * log10f(max(., floor_)) -> d_out float32 [rows][out_frames][n_bands].  d_hist float32 [rows][n_win - 1] and
// d_state int32 [4] (start of the next frame, 0, 0, 0) carry between calls; d_count int32 [2] = (count, status).  Two launches: the
// transform, which only reads them, then one workgroup per row that advances them.  No workspace, no table: the twiddles are computed.
constexpr int kSpectrogramMinFft = 32;
constexpr int kSpectrogramMaxFft = 4096;
constexpr int kSpectrogramMaxBands = 4096;
long long spectrogram_capacity(long long len, int hop);      // ceil(len / hop); -1 on bad arguments
hipError_t launch_spectrogram(const float* d_in, int rows, int in_stride, int len, const int32_t* d_len, float* d_hist, int32_t* d_state, const float* d_window,
                              int n_win, int n_fft, int hop, const float* d_bank, const int32_t* d_support, int n_bands, float scale, float floor_,
                              float* d_out, int out_frames, int32_t* d_count, hipStream_t stream);

// bf_whiten_device (whiten.hip): every row of d_signals float32 [items][n_samples] (items = frames * rows; n_samples a power of two in
// [kWhitenMinN, kWhitenMaxN]) windowed by d_window float32 [n_samples] (null: rectangular), transformed, and per band b the bins
// [lo[b], hi[b]) (already clipped to [0, n_samples / 2 + 1], lo < hi) weighted by max(|X_k|, floor)^-beta[b] and transformed back ->
// d_out float32 [n_bands][items][n_samples], scaled by gain[b] / n_samples.  The bands travel in the launch's arguments.  One launch;
// no workspace, no table: the twiddles are computed.
constexpr int kWhitenMinN = 32;
constexpr int kWhitenMaxN = 4096;
constexpr int kWhitenMaxBands = 16;
struct WhitenBands {
    int lo[kWhitenMaxBands], hi[kWhitenMaxBands];
    float beta[kWhitenMaxBands], gain[kWhitenMaxBands];
};
hipError_t launch_whiten(const float* d_signals, long long items, int n_samples, const float* d_window, const WhitenBands& bands, int n_bands, float floor_rel,
                         float floor_abs, float* d_out, hipStream_t stream);

// bf_enhance_device (enhance.hip): the rows of a window stream (as launch_resample reads it) through analysis frames of n_fft samples every
// hop_s under d_win_a, a gain per (frame, bin) -- the decision-directed Wiener recursion over d_noise / d_prior float32 [rows][n_fft / 2 + 1],
// or d_gain_in float32 [rows][cap][n_fft / 2 + 1] -- and overlap-add synthesis under d_win_s -> d_out float32 [rows][out_stride], the stream
// delayed by n_fft.  d_hist float32 [rows][n_fft - 1], d_ola float32 [rows][n_fft] and d_state int32 [4] carry between calls; d_count int32
// [2] = (count, status); d_power_out / d_gain_out (null: not wanted) as d_gain_in.  Four launches: analysis, gains, synthesis, and the
// overlap-add that also writes the history, the partial sums and the state.  d_work: enhance_workspace floats.  The frame grid and its
// limits (kEnhanceMinFft, kEnhanceMaxFft, kEnhanceMaxOverlap): stream_grid.h.
long long enhance_workspace(int rows, long long samples, int n_fft, int hop_s);      // -1 on bad arguments
hipError_t launch_enhance(const float* d_in, int rows, int frames, int n, int in_stride, int hop, float* d_hist, float* d_ola, float* d_noise, float* d_prior,
                          int32_t* d_state, const float* d_win_a, const float* d_win_s, int n_fft, int hop_s, const float* d_gain_in, float alpha, float a_noise,
                          float g0, float g1, float g_min, int n_init, float* d_work, float* d_out, int out_stride, float* d_power_out, float* d_gain_out,
                          int32_t* d_count, hipStream_t stream);

// bf_postfilter_device (postfilter.hip): the multichannel (Zelinski / Simmer) post-filter gains of up to kPostfilterMaxSlots look directions,
// on bf_enhance_device's frame grid, from the n microphone rows d_mics of d_signals float32 [frames][m_total][n_samples] read as one stream
// each (the last hop, or n_samples, samples of every window behind d_hist float32 [n][n_fft - 1 + lag]).  d_offsets int32 [slots] names the
// directions (launch_lcmv_design's slot rule over d_tau float64 [dirs][n]); d_steer float32 [slots][n][n_fft / 2 + 1][2] is written per call.
// d_num / d_den float32 [slots][n_fft / 2 + 1] and d_state int32 [2 + slots] carry between calls; d_gains (and d_num_out / d_den_out, null:
// not wanted) float32 [slots][cap][n_fft / 2 + 1] as launch_enhance's d_gain_in; d_status int32 [slots]; d_count int32 [2] = (count, status).
// Four launches: steering, analysis + reduce, the recursion, and the carry that alone writes the history and the state.
// d_work: postfilter_workspace floats.
constexpr int kPostfilterMaxSlots = 8;
long long postfilter_workspace(int slots, long long samples, int n_fft, int hop_s);  // -1 on bad arguments
hipError_t launch_postfilter(const float* d_signals, int m_total, int frames, int n_samples, int hop, const int32_t* d_mics, int n, const double* d_tau, int dirs,
                             const int32_t* d_offsets, int slots, int offset_per_dir, float* d_hist, float* d_num, float* d_den, int32_t* d_state,
                             const float* d_window, int n_fft, int hop_s, int lag, int den_mode, float beta, float g_min, float* d_work, float* d_steer,
                             float* d_gains, float* d_num_out, float* d_den_out, int32_t* d_status, int32_t* d_count, hipStream_t stream);

// frequency-domain beamformers (freq_kernels.hip): steering phasors, DFT of the selected bins, and the MFMA complex GEMM
// with its three epilogues (phase-steer DAS power, covariance, MVDR quadratic form) plus the per-bin Cholesky inverse.
hipError_t launch_fd_steering(const double* d_tau, const double* d_freq, int n_dirs, int n_mics, int n_bins, float* d_are, float* d_aim, hipStream_t stream);
// Twiddle table of the MFMA DFT for (N, bin range): fd_twiddle_floats floats, built by launch_fd_twiddles.  launch_fd_dft
// without a table runs the plain one-workgroup-per-row kernel.
size_t fd_twiddle_floats(int n_samples, int n_bins);
hipError_t launch_fd_twiddles(int n_samples, int bin_lo, int n_bins, float* d_tw, hipStream_t stream);
hipError_t launch_fd_dft(const float* d_frames, const int32_t* d_mics, int m_total, int n_samples, int n_frames, int n_mics, int bin_lo, int n_bins,
                         const float* d_tw, float* xre_mf, float* xim_mf, float* xre_fm, float* xim_fm, hipStream_t stream);
// Workspace (floats) that lets the two bin-reducing GEMMs split the bins over several workgroup groups (optional: without
// it they run one group).  n_rows = frames for the delay-and-sum power, 1 for MVDR.
size_t fd_workspace_floats(int n_rows, int n_dirs, int n_bins);
hipError_t launch_fd_das_power(const float* xre_mf, const float* xim_mf, const float* are, const float* aim, int n_frames, int n_mics, int n_dirs,
                               int n_bins, float* d_power, float* d_work, size_t work_floats, hipStream_t stream);
hipError_t launch_fd_covariance(const float* xre_fm, const float* xim_fm, int n_frames, int n_mics, int n_bins, float* rre, float* rim, hipStream_t stream);
// Up to 128 mics: one in-LDS factorisation per bin, no workspace.  129..256 mics: two-by-two blocks of 128 (in-LDS kernel on
// the diagonal blocks, small strided MFMA GEMMs in between), needs fd_cholesky_workspace_floats(n_mics, n_bins) floats.
size_t fd_cholesky_workspace_floats(int n_mics, int n_bins);
hipError_t launch_fd_cholesky_inverse(const float* rre, const float* rim, int n_mics, int n_bins, float loading, float* lire_t, float* liim_t,
                                      int* d_status, float* d_work, size_t work_floats, hipStream_t stream);
hipError_t launch_fd_mvdr_power(const float* lire_t, const float* liim_t, const float* are, const float* aim, int n_mics, int n_dirs, int n_bins,
                                float* d_power, float* d_work, size_t work_floats, hipStream_t stream);

// Profiling build only (-DBF_STAMPS): phase totals of das_pair_kernel, see das_pair.hip (zeros in a production build).
hipError_t read_phase_stamps(unsigned long long* out16, bool clear);
hipError_t read_wave_stamps(unsigned long long* out128, bool clear);      // one row of 8 per wave index of the workgroup

// detector post-processing (nms_kernels.hip): YOLOv5 head decode + confidence filter, greedy NMS over score-sorted candidates
hipError_t launch_yolo_decode(const void* const raw[3], const int hs[3], const int ws[3], const int strides[3], const float* anchors,
                              int batch, int nc, int format, float conf_thres, float* d_boxes, float* d_scores, int* d_cls, hipStream_t stream);
// The detector's tensor kernels (conv_kernels.hip).  elem_bytes: 2 = float16, 4 = float32 activations / weights.
// out [B][H][W][ca + cb] = (nearest 2x upsampling of a [B][H/2][W/2][ca], b [B][H][W][cb]), NHWC
hipError_t launch_upsample_concat(const void* a, const void* b, void* out, int B, int H, int W, int ca, int cb, int elem_bytes, hipStream_t stream);
// SPPF pooling inside the concatenation buffer [B][H][W][4c]: channels [c, 4c) = the three cascaded 5x5 max pools of channels [0, c)
hipError_t launch_sppf_pool(void* buf, int B, int H, int W, int c, int elem_bytes, hipStream_t stream);
// uint8 BGR frames [pixels][3] -> RGB / 255 [pixels][cpad], channels 3.. zero
hipError_t launch_preprocess_bgr8(const void* frames, void* out, long long pixels, int cpad, int elem_bytes, hipStream_t stream);
// Convolution + bias + optional SiLU, NHWC in / out, weights [N][KH][KW][C] in rows padded to whole 64-byte stages.  C a power of two >= 4,
// KW * C a whole number of 16-byte chunks.  ldy: elements between consecutive output pixels (>= N: the output may be a channel slice of a
// wider buffer); res / ldr: optional residual added to the result.  x2 / c1 / ld1 / ld2 / up1: a 1x1 window over the virtual
// concatenation (x [.., c1) at pixel pitch ld1, optionally 2x-upsampled; x2 [c1, C) at pitch ld2) -- pass nullptr, C, C, 0, 0 otherwise.
int conv_dma_switch(int value);
int conv_f32_mode(int value);
int gemm_f32_mode(int value);
int conv_weight_row(int elem_bytes, int kh, int kw, int c);
hipError_t launch_conv2d_nhwc(int elem_bytes, const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int N, int KH, int KW,
                              int stride, int pad, int act, int ldy, const void* res, int ldr, const void* x2, int c1, int ld1, int ld2, int up1,
                              hipStream_t stream);
// The layer as launch_conv2d_nhwc is given it, without the pointers: which exist, and which are not 16-byte aligned.
enum { kConvMisalignedX = 1, kConvMisalignedW = 2, kConvMisalignedX2 = 4, kConvMisalignedY = 8, kConvMisalignedRes = 16 };
struct ConvLayer {
    int elem_bytes, B, H, W, C, N, KH, KW, stride, pad, ldy, ldr, c1, ld1, ld2, up1;
    bool has_res, has_x2;
    unsigned misaligned;
};
// What the launch does with it (plan_conv2d decides, launch_conv2d_nhwc only dispatches on the result).
enum { kConvRegStaged = 0, kConvDma = 1, kConvPatch = 2 };
struct ConvPlan {
    int elem_bytes, family;
    int bm, bn;              // output tile: pixels x channels per workgroup
    int cpr;                 // 16-byte chunks per staged row: 4 (64-byte rows) or 8 (128-byte rows, LDS-DMA only); 0 for the patch kernel
    int cat, split, fast_tap;   // the kernels' kCat, kSplit (LDS-DMA, float32) and ConvArgs::fast_tap (LDS-DMA, window path)
    int wide;                // 16-byte stores in the epilogue (ConvArgs::wide)
    long long grid_x, grid_y;
    int lds_bytes;           // dynamic LDS (the patch kernel; 0 otherwise)
    int row_env, tap_env, patch_env;   // $BF_CONV_ROW / $BF_CONV_TAP / $BF_CONV_PATCH as this process read them (0 / 1 / -1 when unset)
    int n_cus;
    // derived sizes the kernels' arguments are filled from
    int Ho, Wo, wld, c1;
    long long M;
    unsigned x_bytes, x2_bytes, w_bytes;
};
hipError_t plan_conv2d(const ConvLayer& layer, int dma_switch, int f32_mode, int n_cus, ConvPlan* plan);
bool last_conv2d_plan(ConvPlan* plan);      // the plan of this process's most recent convolution launch; false before the first
hipError_t launch_topk_candidates(const float* d_scores, const float* d_boxes, const int* d_cls, int batch, int total, int K, float* d_top_scores,
                                  float* d_top_boxes, int* d_top_cls, int* d_counts, hipStream_t stream);
hipError_t launch_nms(const float* d_boxes, const float* d_scores, const int* d_cls, const int* d_counts, int batch, int K, float iou_thres,
                      int max_det, unsigned long long* d_mask, float* d_out, int* d_out_count, hipStream_t stream);

}  // namespace bf
