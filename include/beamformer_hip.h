/*
 * beamformer_hip.h -- C-ABI of libbeamformer_hip.so, the MI355X (gfx950) drop-in for the reference's
 * CPU delay-and-sum path.
 *
 * PART 1 re-exports, with identical names, argument order and ownership rules, the plain-C symbols the
 * reference links into its Cython extensions (`beamformer` via PC/setup.py:22-23, `tests` via
 * PC/src/benchmark.pyx:28-55).  Each prototype cites the reference declaration it replaces.
 *
 * Differences a maintainer must know:
 *   - Sizes.  The reference bakes N_SAMPLES / MAX_RES_X / MAX_RES_Y / N_TAPS / N_MICROPHONES into config.h
 *     at build time.  Here they are run-time state: defaults are the as-shipped PC/src/config.json, replaced
 *     by bf_configure(...) or, on first use, by the JSON file named in $BF_CONFIG.
 *   - Errors.  Reference functions return void and never check anything.  These keep the void signatures;
 *     a failure (no GPU, bad size, HIP error) is printed to stderr, recorded for bf_last_error() and the
 *     output buffer is filled with NaN so it cannot pass for a result.  There is NO CPU fallback.
 *   - Process model.  The HIP context is created lazily by the first load_* / mimo_* call in the CALLING
 *     process (the reference forks its workers before loading tables: PC/src/main.pyx:172-181,707).
 *   - Tables are copied to the GPU by load_*; the caller's buffer may be freed afterwards (as in the
 *     reference, which malloc+memcpy's: PC/src/algorithms/pad_and_sum.c:147-151).
 *
 * PART 2 (bf_* names) is the extension surface: run-time configuration, device-resident / batched entry
 * points that take HIP device pointers and a stream (what bench.py and the multi-GPU path use), the steering
 * table generators of PC/src/directions.pyx, and error reporting.
 */
#ifndef BEAMFORMER_HIP_H
#define BEAMFORMER_HIP_H

#include <stdbool.h>   /* load(bool), as PC/src/api.h:4 */

#ifdef __cplusplus
extern "C" {
#endif

/* ===================================================================== PART 1: reference symbols */

/* ---- PC/src/algorithms/pad_and_sum.h:5-13 ---- */
void pad_delay(float *signal, float *out, int pos_pad);                                   /* :5  */
void miso_pad(float *signals, float *out, int *adaptive_array, int n, int offset);        /* :6  */
void miso_pad2(float *signals, float *out, int *adaptive_array, int n, int offset);       /* :7  */
void mimo_pad(float *signals, float *image, int *adaptive_array, int n);                  /* :8  */
void load_coefficients_pad(int *whole_samples, int n);                                    /* :10 */
void load_coefficients_pad2(int *whole_miso, int n);                                      /* :11 */
void unload_coefficients_pad(void);                                                       /* :12 */
void unload_coefficients_pad2(void);                                                      /* :13 */

/* ---- PC/src/algorithms/lerp_and_sum.h:4-12 ---- */
void lerp_delay(float *signal, float *out, float h, int pad);                             /* :4  */
void miso_lerp(float *signals, float *out, int *adaptive_array, int n, int offset);       /* :6  */
void mimo_lerp(float *signals, float *image, int *adaptive_array, int n);                 /* :8  */
void load_coefficients_lerp(float *delays, int n);                                        /* :10 */
void unload_coefficients_lerp(void);                                                      /* :12 */

/* ---- PC/src/algorithms/convolve_and_sum.h:4-22 (convolve_naive, :12, is declared but never defined there) ---- */
void convolve_delay_naive_add(float *signal, float *h, float *out);                       /* :4  */
void convolve_delay_vectorized(float *signal, float *h, float *out);                      /* :6  */
void convolve_delay_vectorized_add(float *signal, float *h, float *out);                  /* :8  */
void convolve_delay_naive(float *signal, float *out, float *h);                           /* :10 */
void mimo_convolve_naive(float *signals, float *image, int *adaptive_array, int n);       /* :14 */
void miso_convolve_vectorized(float *signals, float *out, int *adaptive_array, int n, int offset); /* :16 */
void mimo_convolve_vectorized(float *signals, float *image, int *adaptive_array, int n);  /* :18 */
void load_coefficients_convolve(float *h, int n);                                         /* :20 */
void unload_coefficients_convolve(void);                                                  /* :22 */

/* ---- PC/src/algorithms/hybrid_convolve_and_sum.h:4-12 ---- */
void convolve_hybrid_delay_add(float *signal, float *h, int pad, float *out);             /* :4  */
void miso_convolve_hybrid(float *signals, float *out, int *adaptive_array, int n, int offset); /* :6 */
void mimo_convolve_hybrid(float *signals, float *image, int *adaptive_array, int n);      /* :8  */
void load_coefficients_convolve_hybrid(float *h, int n);                                  /* :10 */
void unload_coefficients_convolve_hybrid(void);                                           /* :12 */

/* ---- PC/src/api.h:8-21, the shims that pair get_data() with an algorithm (PC/src/api.c:951-1104).
 * The UDP receiver / SysV ring buffer behind get_data() is out of scope; here get_data() copies the frame
 * most recently published with bf_publish_frame() (the hook a receiver process calls once per window). ---- */
void get_data(float *signals);                                                            /* api.h:7  */
void pad_mimo(float *image, int *adaptive_array, int n);                                  /* api.h:10 */
void lerp_mimo(float *image, int *adaptive_array, int n);                                 /* api.h:11 */
void convolve_mimo_naive(float *image, int *adaptive_array, int n);                       /* api.h:12 */
void convolve_mimo_vectorized(float *image, int *adaptive_array, int n);                  /* api.h:13 */
void mimo_truncated(float *image, int *adaptive_array, int n);                            /* api.h:16 */
void load_coefficients2(int *whole_samples, int n);                                       /* api.h:17 */
void miso_steer_listen(float *out, int *adaptive_array, int n, int steer_offset);         /* api.h:19 */

/* ---- PC/src/api.h:6-9,41-45: the process management around the path.  Exported so that the reference's main.pyx
 * (cdef extern block, PC/src/main.pyx:33-60) links against this library unchanged.  What they manage in the reference
 * -- the forked UDP receiver with its SysV ring buffer (api.c:874-939) and the forked PortAudio playback child
 * (api.c:491-543, 583-640) -- is live-hardware I/O outside the beamforming path:
 *   load            no receiver is forked: records an error and returns -1 (frames arrive through bf_publish_frame);
 *   stop_receiving  drops the published frame (get_data then reports "no frame published");
 *   signal_handler  no-op;
 *   load_miso       initialises the listen state exactly as miso_init_shared_memory does (api.c:461-489: n = 1,
 *                   adaptive_array all zero, steer_offset 0) and returns 0; no playback child is started --
 *                   bf_miso_listen_block below is the body of its loop;
 *   load_pa         the microphone set of the listening beam (api.c:553-567);
 *   steer           the flat table offset of the listening beam (api.c:576-581);
 *   stop_miso       clears the listen state. ---- */
int load(bool replay_mode);                                                               /* api.h:6  */
void stop_receiving(void);                                                                /* api.h:8  */
void signal_handler(void);                                                                /* api.h:9  */
int load_miso(void);                                                                      /* api.h:42 */
void load_pa(int *adaptive_array, int n);                                                 /* api.h:43 */
void stop_miso(void);                                                                     /* api.h:44 */
void steer(int offset);                                                                   /* api.h:45 */

/* ===================================================================== PART 2: extensions */

enum bf_algo {
    BF_PAD = 0,        /* mimo_pad                  */
    BF_LERP = 1,       /* mimo_lerp                 */
    BF_HYBRID = 2,     /* mimo_convolve_hybrid      */
    BF_FIR_NAIVE = 3,  /* mimo_convolve_naive       */
    BF_FIR_VEC = 4     /* mimo_convolve_vectorized  */
};

/* Run-time replacement of the config.h size macros (PC/src/config.json:3-11).  Returns 0, or -1 (see
 * bf_last_error).  Changing sizes drops every loaded table. */
int bf_configure(int n_microphones, int n_samples, int max_res_x, int max_res_y, int n_taps);
/* Same, reading the keys N_MICROPHONES, N_SAMPLES, MAX_RES_X, MAX_RES_Y, N_TAPS of section "general" from a
 * file laid out like PC/src/config.json. */
int bf_configure_from_json(const char *path);
/* Current sizes: out[0..4] = N_MICROPHONES, N_SAMPLES, MAX_RES_X, MAX_RES_Y, N_TAPS. */
void bf_get_config(int out[5]);

/* Last failure of any entry point on this thread's process ("" when none); bf_clear_error resets it. */
const char *bf_last_error(void);
void bf_clear_error(void);

/* 1 when a gfx9xx GPU is usable by this process, else 0 (never initialises a context as a side effect of
 * loading the library). */
int bf_gpu_available(void);
/* Kernel family of the last delay-and-sum launch: 0 strided, 1 retired (was quad + DPP), 2 shifted copies (sweep), 3 shifted copies
 * (direction-outer, chosen for tables without structure), 4 shifted copies (8-tap FIR), 5 shifted copies (sweep, two
 * frames per workgroup: batched launches of pad / lerp), 6 shifted copies for long blocks (256 < N_SAMPLES <= 1024: LDS image in
 * two halves, conflict-free lane mapping), 7 hybrid sweep with shared windows, two frames per workgroup (batched launches of the
 * 8-tap FIR flavours), 8 the two-frame sweep on frame-interleaved rows (batched lerp), 9 strided with the previous window's tail in
 * front of every row (bf_das_stream_device); -1 before the first launch. */
int bf_last_das_variant(void);
/* The row layout of the last delay-and-sum launch where the family comes in more than one: family 8 (two frames interleaved in the
 * rows) runs das_pair2_kernel on rows of sample pairs in two shifted copies (1), or, where the microphone count is a multiple of 32,
 * das_pair2_cells_kernel on rows of 16-byte cells (2).  0 for every other family and before the first launch. */
int bf_last_das_rows(void);
/* The digest the last delay-and-sum launch used (families 2, 3, 5, 8 of bf_last_das_variant: pad / lerp with 16 waves): *steps =
 * direction steps inside a wave's run over which the sweep could share its reads (7 of every 8 positions, times the microphones),
 * *changes = those of them at which the whole-sample delay changes, i.e. the sweep re-reads -- counted in the order the launch
 * sweeps (bf_sweep_order).  Returns 0, or -1 with both set to -1 / 0 when the last launch counted nothing. */
int bf_last_das_reloads(long long *changes, long long *steps);
/* The order in which a batched pad / lerp launch (families 5 and 8) over directions [dir_begin, dir_end) sweeps them: order_out[s]
 * = flat direction at position s, s in [0, dir_end - dir_begin).  A wave carries dpw (8) consecutive positions and re-reads a
 * microphone's samples wherever its whole-sample delay changes between two of them; the images do not depend on the order.
 * Host only: needs no GPU.  whole: int32 [n_dirs][n_mics] whole-sample delays (the pad table; floor of the lerp table).  The rule,
 * with p[s] = row dir_begin + s, M = n_mics:
 *   1. c[s] = number of mics with p[s+1][m] != p[s][m]
 *   2. a new segment starts at s + 1 wherever 2 * c[s] > M
 *   3. the first segment runs forward
 *   4. a later segment [a, b) is reversed if fewer mics differ between the row placed last and p[b-1] than between it and p[a]
 *   5. unless this order has strictly fewer changes inside runs of dpw positions (counted from position 0) than the identity,
 *      the identity is returned.
 * Returns 0, or -1 (bf_last_error) for a null pointer, a size below 1 or a range outside [0, n_dirs). */
int bf_sweep_order(const int *whole, int n_dirs, int n_mics, int dir_begin, int dir_end, int dpw, int *order_out);
/* Profiling builds only (hipcc -DBF_STAMPS, scripts/dev/phase_stamps.py): per-phase wave time of the batched pad / lerp kernel,
 * summed over all waves since the last clear: out16[0..7] = sweep, wait, staging, wait, wait, parking, wait, ordered power sum
 * (s_memtime ticks), out16[8] = waves counted.  All zero in the production build.  Returns 0 or -1. */
int bf_read_phase_stamps(unsigned long long *out16, int clear);
/* The same build's per-wave rows: out128[8 w + 0..7] for wave index w = 0..15 of the workgroup = its sweep ticks, its ticks waiting
 * for the staged chunk, the number of workgroups in which it ran on SIMD 0, 1, 2, 3 (HW_ID), and of the last launch's recorded
 * workgroups ([7]) those in which it ran on the SIMD of wave w & 3 ([6]).  All zero in the production build. */
int bf_read_wave_stamps(unsigned long long *out128, int clear);
/* Select the HIP device (default 0, or $BF_DEVICE) before the first load_* call. */
int bf_set_device(int device);

/* Frame hand-off for the api.h shims: copies n_microphones*n_samples floats (mic-major). */
void bf_publish_frame(const float *signals);
/* One trip of the reference's playback loop (miso_loop, PC/src/api.c:505-531): get_data(), miso_pad at the offset set by
 * steer() over the microphones set by load_pa(), then out[i] = out[i] / n * mic_gain (MIC_GAIN, config.json:62).
 * out = float32 [N_SAMPLES], host pointer.  Returns 0 or -1. */
int bf_miso_listen_block(float *out, float mic_gain);
/* The listen state as steer() / load_pa() left it: returns the steer offset, *n_out = microphone count. */
int bf_get_steer(int *n_out);

/* ---- device-resident, batched delay-and-sum (the throughput path) ----
 * d_signals : HIP device pointer, float32 [frames][m_total][N_SAMPLES], mic-major
 * d_images  : HIP device pointer, float32 [frames][image_stride]; direction d of the launched range is
 *             written to d_images[f*image_stride + d - dir_begin]
 * adaptive_array / n : HOST array of the active mic rows, as in the reference calls
 * [dir_begin, dir_end) : shard of the flat direction grid 0..MAX_RES_X*MAX_RES_Y handled by this call
 * stream    : hipStream_t (0 = null stream).  Enqueue only, graph-capturable -- except the FIRST call for a (table, launch
 *             geometry) pair, which builds that geometry's digest of the table and waits for it, and a call with a new
 *             adaptive array, which synchronises the device before replacing the uploaded copy.  Up to four geometries per
 *             table stay cached (one-frame and batched calls, direction shards), so alternating callers do not rebuild.
 * Returns 0 or -1. */
int bf_das_device(int algo, const float *d_signals, int m_total, float *d_images, int image_stride, int frames,
                  const int *adaptive_array, int n, int dir_begin, int dir_end, void *stream);

/* ---- device-resident, batched steered beams (the MISO counterpart of bf_das_device) ----
 * algo      : BF_PAD -> miso_pad, BF_LERP -> miso_lerp, BF_HYBRID -> miso_convolve_hybrid, BF_FIR_VEC -> miso_convolve_vectorized;
 *             BF_FIR_NAIVE is refused (the reference has no MISO form of it).  Uses the table the matching load_coefficients_*
 *             loaded -- the one bf_das_device reads, so one load serves maps and beams.
 * d_signals : HIP device pointer, float32 [frames][m_total][N_SAMPLES], mic-major, as bf_das_device (no dead-row masking here:
 *             bf_ingest_stream_device's row mask zeroes dead rows when it builds the frames)
 * adaptive_array / n : HOST array of the active mic rows, handled as bf_das_device handles it
 * d_offsets : HIP device pointer, int32 [frames][beams]: the `offset` argument of the matching miso_* call -- the flat table
 *             offset d * n, for BF_FIR_VEC the float offset d * n * N_TAPS into the tap table
 * mic_gain  : 0 -> raw beams, bit-identical to miso_* at that offset; any other finite value -> out[i] = (out[i] / (float)n) * mic_gain
 *             (two float32 roundings, as the reference's playback loop, api.c:519-523, and bf_miso_listen_block); not finite -> error
 * d_out     : HIP device pointer, float32 [frames][beams][out_stride], out_stride >= N_SAMPLES; floats [N_SAMPLES, out_stride) of
 *             every row are left untouched
 * d_status  : HIP device pointer, int32 [frames][beams], or NULL.  When given, every entry is written: 0 ok, 1 offset negative or
 *             past the loaded table (offset + n > entries; BF_FIR_VEC: offset + n * N_TAPS > entries, counted in floats),
 *             2 BF_FIR_VEC offset not a multiple of N_TAPS.  A rejected beam reads nothing from the table and its N_SAMPLES
 *             floats are NaN; the other beams of the call are unaffected.
 * stream    : hipStream_t (0 = null stream).  Enqueue only, no allocation after the first call -- except a call with a new
 *             adaptive array, which synchronises the device as bf_das_device does; graph-capturable after one warm-up call.
 *             Does not change bf_last_das_variant.
 * Returns 0, or -1 (see bf_last_error; nothing enqueued) for an unknown or refused algo, a null pointer (d_status excepted),
 * frames < 1, beams < 1, n < 1, out_stride < N_SAMPLES, an adaptive_array row outside [0, m_total), a mic_gain that is not finite,
 * no GPU, or a table that is not loaded.  The arguments are checked before device bring-up. */
int bf_miso_device(int algo, const float *d_signals, int m_total, int frames, const int *adaptive_array, int n,
                   const int *d_offsets, int beams, float mic_gain, float *d_out, int out_stride, int *d_status, void *stream);
/* d_offsets[f] = argmax_{0 <= j < n_dirs} d_power[f * image_stride + j] * offset_per_dir (device pointers, enqueue only): the
 * loudest direction of every map as a [frames][1] offset array for bf_miso_device (offset_per_dir = n, or n * N_TAPS for
 * BF_FIR_VEC).  Ties and NaN as np.argmax: the first of equal maxima wins, a NaN counts as the maximum (the first NaN wins).
 * Returns 0, or -1 for a null pointer, frames / n_dirs / offset_per_dir < 1, image_stride < n_dirs,
 * (n_dirs - 1) * offset_per_dir > INT_MAX, or no GPU. */
int bf_peak_offsets_device(const float *d_power, int frames, int image_stride, int n_dirs, int offset_per_dir,
                           int *d_offsets, void *stream);

/* ---- the K loudest separated sources of every map: maps -> [frames][k] offsets for bf_miso_device, one enqueue ----
 * bf_peak_offsets_device is a plain argmax: one source per frame.  The reference authors list the general case as open
 * (PC/TODO.md, "Peak detection"): their 2D convolution for local maxima "failed when the resolution went up", because neighbouring
 * pixels of one lobe each looked like a peak.  Here the neighbourhood scales with the grid: a direction is a source only if it is
 * the maximum of its whole (2*radius+1) x (2*radius+1) window.  The reference has nothing to compare with; the definition below
 * consists of comparisons and one float32 multiplication, so results are exact.
 *
 * d_power   : HIP device pointer, float32 [frames][image_stride]; the first rows*cols entries of a frame are the map in the library's
 *             own order d = x*cols + y (rows = MAX_RES_X, cols = MAX_RES_Y, as mimo_* write image[d]); the rest is never read.
 * Non-finite entries (NaN, +inf, -inf) are never sources and never suppress a neighbour: they compare as below everything.  They
 *             are counted in d_counts[f][2].
 * Order     : finite entries are totally ordered by (value descending, flat index d ascending); -0.0f equals 0.0f.  This is the tie
 *             rule of bf_peak_offsets_device.
 * Candidates: a finite entry (x, y) is a candidate iff no OTHER finite entry (x', y') of the grid with |x'-x| <= radius and
 *             |y'-y| <= radius comes before it in that order.  So any two candidates are more than `radius` apart in Chebyshev
 *             distance; a constant map has exactly one candidate, index 0; radius 0 makes every finite entry a candidate (a plain
 *             top-k); radius >= max(rows, cols) - 1 leaves at most one.
 * Threshold : top = the first entry of the order = the largest finite value of the frame (always a candidate);
 *             thr = fmaxf(floor_abs, floor_rel * top), the product one float32 multiplication.  Candidates with value >= thr are kept.
 * d_offsets : HIP device pointer, int32 [frames][k]: d * offset_per_dir of the kept candidates, in order; unfilled slots hold -1,
 *             which bf_miso_device rejects with status 1 and a NaN beam.
 * d_values  : HIP device pointer, float32 [frames][k], or NULL: the powers image[d] of those candidates; unfilled slots hold 0.0f.
 * d_counts  : HIP device pointer, int32 [frames][3], or NULL: [0] slots filled = min(k, [1]); [1] kept candidates in total (shows when
 *             k truncated the list); [2] non-finite entries of the frame.
 * Every entry of every output is written by every call.  A frame with no finite entry, or with floor_abs above its top, has no source.
 * The result does not depend on which of the two internal forms runs (one workgroup per frame where the map fits LDS -- up to 13632
 * directions --, three launches over tiles and a library-owned buffer above that) nor on the order workgroups run in.
 * stream    : hipStream_t (0 = null stream).  Enqueue only; the buffer of the tiled form grows on the first call of a larger shape
 *             and nothing is allocated after that: graph-capturable after one warm-up call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_power or d_offsets null; frames, rows, cols or
 * offset_per_dir < 1; k < 1 or k > BF_PEAKS_MAX_K; radius < 0; rows*cols not fitting an int or exceeding image_stride;
 * (rows*cols - 1) * offset_per_dir > INT_MAX; floor_rel not finite or outside [0, 1]; floor_abs not finite; no GPU.  All arguments are
 * checked before device bring-up. */
#define BF_PEAKS_MAX_K 64
int bf_peaks_device(const float *d_power, int frames, int image_stride, int rows, int cols, int radius, int k,
                    float floor_rel, float floor_abs, int offset_per_dir,
                    int *d_offsets, float *d_values, int *d_counts, void *stream);

/* ---- take beams back out of the frames: the subtraction step of a time-domain CLEAN loop (BF_PAD, BF_LERP) ----
 * Every map is a plain delay-and-sum map, so a source 10 dB below another one sits under the stronger one's main-lobe skirt and
 * sidelobes; the reference authors list this as open (PC/TODO.md, "Improved spatial filtering": "techniques for suppressing signals
 * from undesired directions").  Subtractive deconvolution answers it with what the library already has: take the loudest direction
 * of the map (bf_peaks_device), form its beam (bf_miso_device), project the beam back onto the microphones and subtract it from the
 * frames (this call), map the residual (bf_das_device), repeat.  The projection is the ADJOINT (transpose) of the delay operator,
 * not an inverse: the steering operator has no inverse (n microphones onto one beam), and with gain / n in front the adjoint is the
 * least-squares step for a source that dominates its beam -- for whole-sample delays it returns every microphone's share exactly.
 *
 * algo      : BF_PAD or BF_LERP; reads the table the matching load_coefficients_* loaded, the one bf_miso_device reads.
 * d_signals : HIP device pointer, float32 [frames][m_total][N_SAMPLES], mic-major, as bf_miso_device
 * adaptive_array / n : HOST array of the active mic rows, as bf_miso_device; here no row may be listed twice
 * d_offsets : HIP device pointer, int32 [frames][beams], table offsets as bf_miso_device takes them (d * n)
 * d_beams   : HIP device pointer, float32 [frames][beams][beam_stride], beam_stride >= N_SAMPLES: the RAW beams, as bf_miso_device
 *             writes them with mic_gain 0
 * gain      : the CLEAN loop gain, any finite value; c = gain / (float)n, one float32 division on the host
 * d_residual: HIP device pointer, float32 [frames][m_total][N_SAMPLES].  Every element is written; rows not named in adaptive_array
 *             are copied unchanged.  May be d_signals itself (every element depends on its own input element and the beams only);
 *             any other overlap of the two is not supported.
 * d_status  : HIP device pointer, int32 [frames][beams], or NULL; bf_miso_device's codes: 0 ok, 1 offset negative or past the loaded
 *             table (offset + n > entries).  A rejected beam subtracts nothing and its d_beams row is never read, so a -1 slot from
 *             bf_peaks_device, or the NaN beam bf_miso_device wrote for it, is harmless.
 *
 * Definition, float32, every operation rounded once and none contracted.  N = N_SAMPLES; p, h = the loaded table's entries at
 * offset_b + m (pad: p only); o_b = beam b of the frame; r_m = adaptive_array[m].  For every j in [0, N):
 *     acc = x[f][r_m][j]
 *     for b = 0 .. beams-1, accepted offsets only, in this order:
 *         pad :  a = (j + p < N) ? o_b[j + p] : 0
 *         lerp:  u = (j + p + 1 < N) ? o_b[j + p + 1] : 0
 *                v = (j >= 1 && j + p < N) ? o_b[j + p] : 0
 *                a = (1 - h) * u  +  h * v                   (sub, mul, mul, add)
 *         acc = acc - c * a                                  (mul, sub)
 *     residual[f][r_m][j] = acc
 * `a` is the transpose of the library's delay operators, miso_pad: out[p + i] += s[i] (i < N - p), miso_lerp: out[p + i + 1] +=
 * s[i] + h * (s[i + 1] - s[i]) (i < N - p - 1): sum_t beam(x)[t] * o[t] == sum_{m, j} x[m][j] * a_m[j] in exact arithmetic.  Table
 * entries at or beyond N give a = 0; NaN and infinities propagate.  The result does not depend on which internal path runs (16-byte
 * or 4-byte accesses, beams staged in LDS or read through L2).
 * stream    : hipStream_t (0 = null stream).  Enqueue only, no allocation after the first call -- except a call with a new
 *             adaptive array or m_total, which synchronises the device as bf_das_device does; graph-capturable after one warm-up
 *             call.  Does not change bf_last_das_variant.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: any algo but BF_PAD / BF_LERP; a null pointer (d_status
 * excepted); frames < 1; beams < 1 or > BF_REMOVE_MAX_BEAMS; n < 1; beam_stride < N_SAMPLES; an adaptive_array row outside
 * [0, m_total) or listed twice; a gain that is not finite; no GPU; a table that is not loaded.  All arguments are checked before
 * device bring-up; the table check needs the device the table lives on. */
#define BF_REMOVE_MAX_BEAMS 64
int bf_remove_sources_device(int algo, const float *d_signals, int m_total, int frames, const int *adaptive_array, int n,
                             const int *d_offsets, int beams, const float *d_beams, int beam_stride, float gain,
                             float *d_residual, int *d_status, void *stream);

/* ---- track map sources across frames: bf_peaks_device's [frames][k] offsets -> [frames][slots] offsets with identity over time ----
 * bf_peaks_device orders a frame's sources loudest first, so two talkers of similar level swap slots from window to window, a source
 * that drops out shifts everyone behind it up a slot, and a one-window false alarm takes a slot.  Joining slot b of every window
 * into one signal needs slot b to be the same source in every window.  The reference authors list this as open (PC/TODO.md,
 * "Tracking + Prediction") and wrote a constant-velocity Kalman filter for it (PC/src/kf.hpp) that nothing calls.  This call is that
 * filter, one per slot, with a gated greedy nearest-neighbour association in front of it and track birth / coasting / death around
 * it.  ONE deliberate difference from kf.hpp: a track starts at its first measurement (velocity 0, P = I), not at the origin.
 *
 * d_offsets : HIP device pointer, int32 [frames][k], as bf_peaks_device writes it: d * offset_per_dir or -1; k <= BF_PEAKS_MAX_K.  An
 *             entry is a DETECTION iff it is >= 0, a multiple of offset_per_dir, and d < rows*cols; anything else (an empty -1 slot
 *             included) is ignored and counted in d_counts[f][3].  A detection's position is zx = (float)(d / cols),
 *             zy = (float)(d % cols), the library's own order d = x*cols + y.
 * d_state   : HIP device pointer, bf_track_state_words(slots) = 4 + 12 * slots 32-bit words, read and written: the tracks carried from
 *             one call to the next.  All zero is a fresh stream (hipMemset it once).  Integer fields int32, the rest float32:
 *                 word 0                 next_id (ids start at 1 and are never reused)
 *                 words 1..3             0
 *                 words 4 + 12*s ..      slot s: id (0 = free), hits, misses, 0, x, vx, y, vy, p00, p01, p11, 0
 *             A free slot is written as twelve zeros.
 * d_track_offsets : HIP device pointer, int32 [frames][slots]: for a live slot with hits >= min_hits, (xi*cols + yi) * offset_per_dir
 *             with xi = clamp((int)rintf(x), 0, rows-1), yi = clamp((int)rintf(y), 0, cols-1) -- ready for bf_miso_device; every other
 *             slot holds -1, which bf_miso_device rejects with status 1 and a NaN beam.
 * d_track_ids : int32 [frames][slots], or NULL: the slot's id, 0 for a free slot; unconfirmed tracks (hits < min_hits) show theirs.
 * d_track_pos : float32 [frames][slots][4], or NULL: x, y, vx, vy; zeros for a free slot.
 * d_match   : int32 [frames][slots], or NULL: the column of d_offsets the slot took in this frame (a newborn track: the column it was
 *             born from); -1 when the slot is coasting or free.
 * d_counts  : int32 [frames][4], or NULL: tracks born, tracks ended, detections dropped because no slot was free, entries ignored.
 * Every entry of every given output is written by every call.
 *
 * Definition.  Frames in order f = 0 .. frames-1; float32, every operation rounded once and none contracted, plain division.
 * gate2 = gate * gate (one float32 multiplication on the host).  A slot is live iff its id != 0.  Per frame:
 *   1. Predict every live slot:   x = x + vx;  y = y + vy;
 *                                 a = p00 + p01;  b = p01 + p11;  p00 = (a + b) + q;  p01 = b;  p11 = p11 + q
 *      (A P A^T + Q of kf.hpp:88-89 for one axis: kf.hpp's A, Q, H, R never couple the axes and P starts as the identity, so all axes
 *      share one 2x2 covariance and the 6x6 form reduces to this.)
 *   2. Associate.  For live slot s and detection column j: dx = zx - x; dy = zy - y; cost = dx*dx + dy*dy (sub, sub, mul, mul, add);
 *      the pair is eligible iff cost <= gate2.  Repeat: among the eligible pairs whose slot and detection are both unassigned take the
 *      smallest by (cost, slot index, column) and assign it; stop when none is left.
 *   3. Update each assigned slot from its predicted state and its detection z (kf.hpp:92-98):
 *                                 S = p00 + r;  k0 = p00 / S;  k1 = p01 / S
 *                     per axis:   e = z - x;  x = x + k0*e;  v = v + k1*e
 *          from the old values:   p00 = p00 - k0*p00;  p01 = p01 - k0*p01;  p11 = p11 - k1*p01
 *                                 hits += 1;  misses = 0
 *   4. Coast each unassigned live slot: it keeps the prediction, misses += 1; if misses > max_miss the slot becomes free (counted as
 *      ended) and is available to step 5 of this same frame.
 *   5. Birth.  Each unassigned detection, in column order, takes the lowest free slot: next_id += 1; id = next_id; hits = 1;
 *      misses = 0; x = zx; y = zy; vx = vy = 0; p00 = 1; p01 = 0; p11 = 1; d_match gets its column.  With no free slot the detection
 *      is dropped and counted.
 *   6. Write the frame's outputs from the state as it now stands.
 * The clamp of step 6's rounding is done in float before the conversion, so a position outside the int range (or NaN -> 0) is defined.
 * One call over F frames equals two calls over F1 + F2 frames on the same d_state, bit for bit.  next_id wraps like an int32.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: one launch of one 64-lane wave (lane s owns slot s), no allocation, no
 *             synchronisation, no workspace; graph-capturable from the first call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_offsets, d_state or d_track_offsets null; frames < 1;
 * k < 1 or k > BF_PEAKS_MAX_K; slots < 1 or slots > BF_TRACK_MAX_SLOTS; rows, cols or offset_per_dir < 1; rows*cols not fitting an
 * int; (rows*cols - 1) * offset_per_dir > INT_MAX; gate not finite or < 0; max_miss < 0; min_hits < 1; q not finite or < 0; r not
 * finite or <= 0; no GPU.  All arguments are checked before device bring-up.
 * bf_track_state_words(slots) returns 4 + 12 * slots, or -1 for slots outside [1, BF_TRACK_MAX_SLOTS] (it records no error). */
#define BF_TRACK_MAX_SLOTS 64
int bf_track_state_words(int slots);
int bf_track_sources_device(const int *d_offsets, int frames, int k, int rows, int cols, int offset_per_dir,
                            int slots, float gate, int max_miss, int min_hits, float q, float r,
                            void *d_state, int *d_track_offsets, int *d_track_ids, float *d_track_pos,
                            int *d_match, int *d_counts, void *stream);

/* ---- detector boxes meet the acoustic map: what does a detected object sound like, which box is the talker of a track slot ----
 * The camera half of the device path ends in bf_nms_device's boxes, the acoustic half in bf_das_device's maps and the offsets of
 * bf_peaks_device / bf_track_sources_device; the reference relates the two in PC/sensorfusion/decider.py (focus_beam, :70-88: a
 * detection box steers the listening beam).  This call is that relation on the device: for every box the part of the map it covers
 * (its FOOTPRINT) and the loudest direction in it as a table offset bf_miso_device takes, and for every source the box it lies in.
 * focus_beam's own arithmetic is not reproduced: it maps the box centre linearly to an angle and indexes the grid as if it spanned
 * +-90 degrees (main.pyx:498-515), while the grid spans VIEW_ANGLE and is linear in tan(angle), so it does not point where the box is
 * drawn.  The footprint here is the nearest-cell inverse of the display path the library reproduces: direction (x, y) is painted at
 * small-image pixel [MAX_RES_Y-1-y][MAX_RES_X-1-x] (bf_heatmap_colorize_device), and the overlay stretches that image over the frame
 * with half-pixel centres (cv2.resize INTER_LINEAR, bf_heatmap_overlay_device).
 *
 * d_power   : HIP device pointer, float32 [frames][image_stride]; the first rows*cols entries of a frame are the map in the library's
 *             order d = x*cols + y, as bf_peaks_device reads it.
 * d_boxes   : HIP device pointer, float32 [frames][max_boxes][6] = x1, y1, x2, y2, score, cls, coordinates in pixels of the
 *             img_w x img_h frame the heat-map was overlaid on: what bf_nms_device writes.
 * d_box_counts : HIP device pointer, int32 [frames], or NULL.  When given, rows at or beyond clamp(count, 0, max_boxes) are not boxes;
 *             NULL: all rows are candidates.
 * conf      : a row is a BOX iff it is inside the count and score >= conf (a NaN score is not a box).  The decider uses 0.5.
 * d_src_offsets : HIP device pointer, int32 [frames][n_src], or NULL with n_src == 0: offsets as bf_peaks_device or
 *             bf_track_sources_device write them.  An entry is a SOURCE iff it is >= 0, a multiple of offset_per_dir, and
 *             d < rows*cols (the tracker's rule); its cell is (d / cols, d % cols).
 *
 * Footprint of a box.  float32, every operation rounded once and none contracted, then integers.  Horizontally:
 *     ua = ceilf(x1 - 0.5f);  ub = floorf(x2 - 0.5f)            the display columns whose centres lie inside the box
 *     ua = fmaxf(ua, 0);      ub = fminf(ub, (float)(img_w - 1))
 *     the axis is EMPTY if x1 or x2 is NaN or !(ua <= ub), decided in float before any conversion; the conversion to int then
 *     clamps to img_w - 1 (which matters only where (float)(img_w - 1) rounds up, above 2^24 pixels)
 *     c(u) = ((2u + 1) * rows) / (2 * img_w)                    64-bit integer division: the small-image column under display column u
 *     xa = rows-1 - c(ub);    xb = rows-1 - c(ua)
 * and the same with y1, y2, img_h, cols and r(v) = ((2v + 1) * cols) / (2 * img_h) for ya, yb.  The footprint is the cells
 * [xa, xb] x [ya, yb]; a box with an empty axis has none.
 *
 * d_peak_offsets : int32 [frames][max_boxes]: of the FINITE cells of the footprint the first in bf_peaks_device's order (value
 *             descending, flat index ascending, -0.0f == 0.0f), as d * offset_per_dir; -1 when the row is not a box, the box has no
 *             footprint, or no cell of it is finite.  bf_miso_device turns -1 into status 1 and a NaN beam.
 * d_peak_power : float32 [frames][max_boxes], or NULL: that cell's power; 0.0f wherever the offset is -1.
 * d_center_offsets : int32 [frames][max_boxes], or NULL: the cell under the box's midpoint (focus_beam's analogue):
 *             um = floorf((x1 + x2) * 0.5f), valid iff 0 <= um <= (float)(img_w - 1); vm likewise from y1, y2, img_h; the offset is
 *             ((rows-1 - c(um)) * cols + (cols-1 - r(vm))) * offset_per_dir; -1 for a row that is not a box or an invalid midpoint.
 * d_rects   : int32 [frames][max_boxes][4], or NULL: xa, xb, ya, yb; four -1 for a row that is not a box or an empty footprint.
 * d_src_box : int32 [frames][n_src]; required when n_src > 0, ignored when n_src == 0: the lowest row index of a box whose footprint
 *             contains the source's cell -- bf_nms_device's rows come in descending score order, so that is the best-scored box --,
 *             -1 when there is none or the entry is not a source.  Two sources may share a box.
 * d_counts  : int32 [frames][3], or NULL: boxes, boxes with a peak offset >= 0, sources with a box.
 * Every entry of every given output is written by every call.
 *
 * The result does not depend on which internal form reads the map (staged into LDS once per workgroup up to BF_FUSE_STAGE_MAX =
 * 15360 directions, 60 KiB, through L2 above that), on how a frame's rows are split over workgroups (32 rows each) or on the order
 * workgroups run in.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: one launch for the boxes, and one more of one wave per frame when
 *             n_src > 0 or d_counts is given; no allocation, no synchronisation, no workspace; graph-capturable from the first call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_power, d_boxes or d_peak_offsets null; frames, rows,
 * cols, offset_per_dir, max_boxes, img_w or img_h < 1; rows*cols not fitting an int or exceeding image_stride;
 * (rows*cols - 1) * offset_per_dir > INT_MAX; conf not finite; n_src < 0 or > BF_FUSE_MAX_SOURCES; n_src > 0 with d_src_offsets or
 * d_src_box null; no GPU.  All arguments are checked before device bring-up. */
#define BF_FUSE_MAX_SOURCES 64
#define BF_FUSE_STAGE_MAX 15360
int bf_fuse_boxes_device(const float *d_power, int frames, int image_stride, int rows, int cols, int offset_per_dir,
                         const float *d_boxes, const int *d_box_counts, int max_boxes, int img_w, int img_h, float conf,
                         const int *d_src_offsets, int n_src,
                         int *d_peak_offsets, float *d_peak_power, int *d_center_offsets, int *d_rects,
                         int *d_src_box, int *d_counts, void *stream);

/* ---- track detector boxes across frames: bf_nms_device's [frames][max_boxes][6] rows -> [frames][slots][6] rows with identity over time ----
 * bf_nms_device orders a frame's rows by score, so row b of one frame and row b of the next are not the same object, and a one-frame
 * false alarm takes a row.  The reference's running detector (image-detection/src/yolo_smooth_tracking.py,
 * process_video_track_boxes_only, :275-347) therefore hands every frame's detections to SORT (Bewley, Ge, Ott, Ramos, Upcroft,
 * "Simple online and realtime tracking", ICIP 2016): a constant-velocity Kalman filter per box, association by the assignment of
 * maximal total IoU, and max_age / min_hits birth and death; the tracked box is what PC/sensorfusion/decider.py steers the beam at.
 * This call is that tracker on the device, written from the paper and from the behaviour of the reference's call, one frame after
 * another on a carried state.  It is to boxes what bf_track_sources_device is to map sources.
 *
 * d_boxes   : HIP device pointer, float32 [frames][max_boxes][6] = x1, y1, x2, y2, score, cls: what bf_nms_device writes.
 * d_n_boxes : HIP device pointer, int32 [frames], or NULL.  n = clamp(d_n_boxes[f], 0, max_boxes); NULL: n = max_boxes.
 * conf      : row j is a DETECTION iff j < n, its four coordinates are finite, x2 > x1, y2 > y1, and its score is finite and
 *             > conf (strictly: the reference skips confl < conf, :304; its conf is 0.1).  Every other row below n is ignored and
 *             counted in d_counts[f][3].  The detections of a frame keep their row order.
 * slots     : tracks held at once, at most BF_BOX_TRACK_MAX_SLOTS.  iou_threshold, max_age, min_hits: SORT's (0.3, 1, 3).
 * d_state   : HIP device pointer, bf_box_track_state_words(slots) = 4 + 20 * slots 32-bit words, read and written: the tracks
 *             carried from one call to the next.  All zero is a fresh stream (hipMemset it once).  Integer fields int32, the rest
 *             float32 by their bits:
 *                 word 0                 next_id (ids start at 1 and are never reused; it wraps like an int32)
 *                 word 1                 frame_count
 *                 words 2..3             0
 *                 words 4 + 20*s ..      slot s: id (0 = free), time_since_update, hits, hit_streak,
 *                                        u, v, s, r, du, dv, ds       centre, area, aspect w/h, and the rates of the first three
 *                                        a00, a01, a11                the covariance of (u, du), which is also that of (v, dv)
 *                                        b00, b01, b11                the covariance of (s, ds)
 *                                        c                            the variance of r
 *                                        0, 0
 *             A free slot is written as twenty zeros.
 * d_tracks  : HIP device pointer, float32 [frames][slots][6]: a REPORTED slot (step 6) holds its state box, then the score and cls
 *             of the detection it took in this frame; every other slot six zeros.  The layout is d_boxes' own, so
 *             bf_fuse_boxes_device reads it with d_box_counts = NULL: a zero score is not a box for any conf > 0.
 * d_ids     : int32 [frames][slots], or NULL: the slot's id, 0 for a free slot; live tracks that are not reported show theirs.
 * d_match   : int32 [frames][slots], or NULL: the row of d_boxes the slot took in this frame or was born from; otherwise -1.
 * d_live    : float32 [frames][slots][4], or NULL: the state box of every live slot, coasting ones included; zeros for a free slot.
 *             This is what keeps a beam on an object through a missed detection.
 * d_counts  : int32 [frames][4], or NULL: tracks born, tracks ended, detections dropped because no slot was free, rows ignored.
 * Every entry of every given output is written by every call.
 *
 * The filter.  SORT's is a 7-state (u, v, s, r, du, dv, ds) / 4-measurement (u, v, s, r) Kalman filter with F = I plus the
 * couplings (u, du), (v, dv), (s, ds), H = the first four states, R = diag(1, 1, 10, 10), Q = diag(1, 1, 1, 1, .01, .01, .0001),
 * P0 = diag(10, 10, 10, 10, 1e4, 1e4, 1e4) and the Joseph-form covariance update.  None of these couples (u, du), (v, dv), (s, ds)
 * and r with one another, so P stays block diagonal for ever: one 2x2 block A for (u, du) and (v, dv) alike (q = (1, .01), r = 1),
 * one 2x2 block B for (s, ds) (q = (1, 1e-4), r = 10) and one scalar c for r (q = 1, r = 10) -- the reduction
 * bf_track_sources_device makes for kf.hpp.  For a block p = (p00, p01, p11) with process noise (q0, q1) and measurement noise r:
 *     PREDICT(p):  a = p00 + p01;  b = p01 + p11;  p00 = (a + b) + q0;  p01 = b;  p11 = p11 + q1
 *     UPDATE(p):   S = p00 + r;  k0 = p00 / S;  k1 = p01 / S;  m = 1 - k0;  then, from the old p00, p01, p11:
 *                  p00 = (m * m) * p00 + (k0 * k0) * r
 *                  t = p01 - k1 * p00;                    p01 = m * t + (k0 * k1) * r
 *                  kk = k1 * k1;                          p11 = ((p11 - (2 * k1) * p01) + kk * p00) + kk * r
 *                  a state pair (x, dx) measured as z:    e = z - x;  x = x + k0 * e;  dx = dx + k1 * e
 *     the scalar:  predict c = c + 1;   update S = c + 10;  k = c / S;  e = z - r;  r = r + k * e;  m = 1 - k;
 *                  c = (m * m) * c + (k * k) * 10
 *     BOX(state):  w = sqrtf(s * r);  h = s / w;  hw = 0.5f * w;  hh = 0.5f * h;  (u - hw, v - hh, u + hw, v + hh)
 *     Z(row):      w = x2 - x1;  h = y2 - y1;  z = (x1 + 0.5f * w, y1 + 0.5f * h, w * h, w / h)
 *
 * Definition.  Frames in order f = 0 .. frames-1.  float32, every operation rounded once and none contracted, plain division and a
 * correctly rounded sqrtf; max(a, b) = a > b ? a : b and min(a, b) = a < b ? a : b.  A slot is live iff its id != 0.  Per frame:
 *   1. frame_count += 1.  Every live slot: if ds + s <= 0 then ds = 0;  u = u + du;  v = v + dv;  s = s + ds;  PREDICT(A), PREDICT(B),
 *      c = c + 1;  if time_since_update > 0 then hit_streak = 0;  time_since_update += 1.  Its box is BOX(state); a slot whose box has
 *      a coordinate that is not finite becomes free (counted as ended) and is available to step 5 of this frame.
 *   2. Gain of (live slot with box t, detection d), in the order of SORT's iou_batch:
 *          xx1 = max(d.x1, t.x1);  yy1 = max(d.y1, t.y1);  xx2 = min(d.x2, t.x2);  yy2 = min(d.y2, t.y2)
 *          w = max(0, xx2 - xx1);  h = max(0, yy2 - yy1);  wh = w * h
 *          o = wh / (((d.x2 - d.x1) * (d.y2 - d.y1) + (t.x2 - t.x1) * (t.y2 - t.y1)) - wh);   g = o > 0 ? o : 0    (a NaN counts as 0)
 *   3. Associate.  With no live slot or no detection nothing is matched.  If no slot and no detection has more than one pair with
 *      g > iou_threshold, the matches are exactly the pairs with g > iou_threshold.  Otherwise the ASSIGNMENT below gives every live
 *      slot a column, and the slot is matched to it iff the column is a detection and not g < iou_threshold.  (A pair with
 *      g == iou_threshold is therefore kept by the assignment and not by the shortcut: the reference's own asymmetry.)
 *      ASSIGNMENT.  Rows i = 0 .. R-1: the live slots in slot order.  Columns j = 0 .. C-1, C = D + R: the D detections in row
 *      order, then one dummy per row.  cost(i, j) = -(double)g for a detection, 0.0 for a dummy.  float64 potentials U[i], V[j],
 *      all 0.0; row_of[j] = none.  For i = 0 .. R-1 in order:
 *          minv[j] = +inf, used[j] = false, way[j] = none for every j;  i0 = i;  j0 = none;  repeat:
 *              for every j not used:  cur = (cost(i0, j) - U[i0]) - V[j];  if cur < minv[j] then minv[j] = cur, way[j] = j0
 *              j1 = the lowest j not used whose minv[j] equals the minimum over the j not used;  delta = minv[j1]
 *              U[i] = U[i] + delta;  for every used j:  U[row_of[j]] = U[row_of[j]] + delta,  V[j] = V[j] - delta;
 *              for every j not used:  minv[j] = minv[j] - delta
 *              used[j1] = true;  j0 = j1;  stop if row_of[j0] is none, else i0 = row_of[j0]
 *          then walk back:  repeat { jp = way[j0];  row_of[j0] = (jp is none ? i : row_of[jp]);  j0 = jp } until j0 is none.
 *      Row i's column is the j with row_of[j] = i.  This is the shortest-augmenting-path method; it maximises the total gain, and
 *      the order above gives ties one answer.
 *   4. Every matched slot, from its predicted state and its detection's Z:  time_since_update = 0;  hits += 1;  hit_streak += 1;
 *      UPDATE(A) with (u, du) then (v, dv);  UPDATE(B) with (s, ds);  the scalar update of r.
 *   5. Birth.  Every detection no slot took, in row order, takes the lowest free slot:  next_id += 1;  id = next_id;
 *      time_since_update = hits = hit_streak = 0 (a track's first hit is its first update);  (u, v, s, r) = Z;  du = dv = ds = 0;
 *      A = B = (10, 0, 1e4);  c = 10.  With no free slot the detection is dropped and counted.
 *   6. Report, then retire.  The frame's outputs are written from the state as it now stands.  A live slot is REPORTED iff
 *      time_since_update < 1 and (hit_streak >= min_hits or frame_count <= min_hits); its box and d_live's are BOX(state).  Then a
 *      slot with time_since_update > max_age becomes free (counted as ended); it is free from the next frame on.
 * Three deliberate differences from the reference's call: (a) it deletes a track whose predicted box has a NaN but mis-indexes on an
 * infinity (sort.py masks rows with any invalid entry, yet lists only NaN rows for deletion); here either frees the slot.  (b) It
 * re-finds a track's confidence by scanning the detections for one with IoU > 0.5 (:319-324); d_tracks passes on the matched
 * detection's.  (c) When NO pair exceeds the threshold it still runs the assignment and can keep a pair with g == iou_threshold
 * exactly; here that frame takes the shortcut and matches nothing.
 * One call over F frames equals two calls over F1 + F2 frames on the same d_state, bit for bit; a graph replay advances the state
 * like any other call.  The result does not depend on the workgroup size the launch uses.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: one launch of one workgroup, no allocation, no synchronisation, no
 *             workspace; graph-capturable from the first call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_boxes, d_state or d_tracks null; frames < 1;
 * max_boxes < 1 or > BF_BOX_TRACK_MAX_BOXES; slots < 1 or > BF_BOX_TRACK_MAX_SLOTS; conf not finite; iou_threshold not finite or
 * outside [0, 1]; max_age < 0; min_hits < 0; no GPU.  All arguments are checked before device bring-up.
 * bf_box_track_state_words(slots) returns 4 + 20 * slots, or -1 for slots outside [1, BF_BOX_TRACK_MAX_SLOTS] (it records no error). */
#define BF_BOX_TRACK_MAX_SLOTS 64
#define BF_BOX_TRACK_MAX_BOXES 1024
int bf_box_track_state_words(int slots);
int bf_track_boxes_device(const float *d_boxes, const int *d_n_boxes, int frames, int max_boxes,
                          float conf, int slots, float iou_threshold, int max_age, int min_hits,
                          void *d_state, float *d_tracks, int *d_ids, int *d_match, float *d_live, int *d_counts, void *stream);

/* ---- follow boxes by the camera image: a box of the previous image re-found in the current one by template match ----
 * The reference's detector (image-detection/src/yolo_smooth_tracking.py, process_video, :87-143) trusts detections above confh = 0.7
 * and, in a frame that has none, keeps a low-score candidate only if a box of the previous frame can be re-found in the current
 * image: track_with_correlation (:59-69) takes the previous frame's patch around the box (extract_patch, scale 1.2), locates it with
 * cv2.matchTemplate(..., TM_CCOEFF_NORMED) inside the current frame's search area (scale 1.5) and reports the moved box and the
 * correlation.  bf_track_boxes_device bridges a missed detection by a Kalman prediction, which looks at no pixel; this call looks at
 * the pixels.  bf_smooth_boxes_device below is the hysteresis on top of it.
 *
 * d_images  : HIP device pointer, uint8 [frames][height][width][3], the camera batch.
 * d_prev    : HIP device pointer, uint8 [height][width][3], or NULL.  The previous image of frame f is image f - 1; for f = 0 it is d_prev.
 * d_boxes   : HIP device pointer, float32 [frames][max_boxes][box_stride], box_stride >= 4, x1, y1, x2, y2 first: a stride of 6 reads
 *             detector or tracker rows, a stride of 4 d_live and the smoother's state rows.  The boxes of frame f are positions in the
 *             previous image and are sought in image f.
 * d_n_boxes : HIP device pointer, int32 [frames], or NULL.  n = clamp(d_n_boxes[f], 0, max_boxes); NULL: n = max_boxes.
 * t_pct, s_pct : the template and search scales in percent (the reference's 1.2 and 1.5 are 120 and 150), 100 <= t_pct <= s_pct <= 400.
 * d_moved   : float32 [frames][max_boxes][4];  d_score : float32 [frames][max_boxes];  d_shift : int32 [frames][max_boxes][2], or NULL;
 * d_status  : int32 [frames][max_boxes].  Every entry of every given output is written by every call.
 *
 * Definition.  Integer arithmetic up to the last three float64 operations; `/` on integers truncates (every operand is >= 0 where it
 * matters).
 *   1. Row j of frame f is a BOX iff j < n, its four coordinates are finite and of magnitude < 2^20, and with ix = (int)x (truncation
 *      toward zero, the reference's map(int, box)) w = ix2 - ix1 >= 1 and h = iy2 - iy1 >= 1.  Otherwise status 1.
 *   2. PATCH(pct):  nw = w * pct / 100;  nh = h * pct / 100;  cx = ix1 + w / 2;  cy = iy1 + h / 2;  columns
 *      [max(0, cx - nw / 2), min(width, cx + nw / 2)), rows [max(0, cy - nh / 2), min(height, cy + nh / 2)): the reference's extract_patch
 *      (int(w * 1.2) == w * 120 / 100 and int(w * 1.5) == w * 150 / 100 for every w in 1..8192).
 *   3. The template is PATCH(t_pct) of the previous image: columns [ta, tb), rows [tc, td), tw = tb - ta, th = td - tc.  The search
 *      area is PATCH(s_pct) of image f: [sa, sb) x [sc, sd), sw, sh; it contains the template's rectangle because s_pct >= t_pct.  The
 *      zero displacement is dx0 = ta - sa, dy0 = tc - sc.  tw < 1 or th < 1 (the box is off the image): status 2.  Otherwise f = 0 with
 *      d_prev NULL: status 4.
 *   4. Decimation.  q = the smallest integer >= 1 with pw * ph <= BF_MATCH_MAX_PIXELS, pw = ceil(tw / q), ph = ceil(th / q);  P = pw * ph.
 *      Template samples are the pixels (ta + q i, tc + q j), i < pw, j < ph.  Window positions are dx = (dx0 mod q) + q u <= sw - tw
 *      and dy = (dy0 mod q) + q v <= sh - th, u, v >= 0: the zero displacement is always one of them.  Window samples are
 *      (sa + dx + q i, sc + dy + q j).
 *   5. Over the P samples and the three channels c, as exact integers:  S_T[c], S_I[c] the sums of the template and of the window,
 *      Q_T, Q_I the sums of squares over all channels, X the sum of the products.  Then
 *          N = P X - sum_c S_T[c] S_I[c];   A = P Q_T - sum_c S_T[c]^2;   B = P Q_I - sum_c S_I[c]^2
 *      which is TM_CCOEFF_NORMED as OpenCV publishes it (per-channel means) multiplied through by P.  X <= 16384 * 3 * 255^2 < 2^32
 *      and |N|, A, B < 2^46: exact in int64, and exactly convertible to float64.
 *   6. A == 0 (a flat template): status 3.  Otherwise the score of a position is r = B == 0 ? 0.0 : (double)N / sqrt((double)A * (double)B),
 *      the product, the correctly rounded square root and the correctly rounded division each rounded once.  The match is the
 *      position with the greatest r, the first one in (dy, dx) row-major order on ties (minMaxLoc's rule).
 *   7. Status 0:  shift = (dx - dx0, dy - dy0);  moved = (x1 + (float)shift_x, y1 + (float)shift_y, x2 + (float)shift_x,
 *      y2 + (float)shift_y), float32 additions;  score = (float)r.  Status 3: moved = the box unchanged, score 0, shift 0.  Status 1, 2,
 *      4: zeros.
 * Four deliberate differences from the reference's call: (a) it adds max_loc itself to the box; max_loc is measured from the search
 * area's corner, so its predicted box is offset by (dx0, dy0), about 0.15 of the box, even for a still object: here the shift is
 * measured from the zero displacement.  (b) Where the template is larger than the search area cv2 raises; here the clipping of both
 * patches to the image makes that impossible.  (c) Templates above BF_MATCH_MAX_PIXELS pixels are decimated, not refused.  (d) The
 * score is restated from the published formula rather than computed by cv2, as the heat-map's resize is.
 * One call over F frames equals F one-frame calls that pass the previous image as d_prev.  The result does not depend on how the
 * launch tiles the search area.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: one launch, no allocation, no synchronisation, no workspace;
 *             graph-capturable from the first call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_images, d_boxes, d_moved, d_score or d_status null;
 * frames < 1; height or width outside [1, BF_MATCH_MAX_SIDE]; max_boxes outside [1, BF_MATCH_MAX_BOXES]; box_stride < 4; t_pct < 100,
 * s_pct < t_pct or s_pct > 400; frames * max_boxes not fitting an int; no GPU.  All arguments are checked before device bring-up. */
#define BF_MATCH_MAX_PIXELS 16384      /* template pixels after decimation */
#define BF_MATCH_MAX_BOXES 1024
#define BF_MATCH_MAX_SIDE 8192
int bf_match_boxes_device(const unsigned char *d_images, const unsigned char *d_prev, int frames, int height, int width,
                          const float *d_boxes, int box_stride, const int *d_n_boxes, int max_boxes, int t_pct, int s_pct,
                          float *d_moved, float *d_score, int *d_shift, int *d_status, void *stream);

/* ---- the reference's confidence hysteresis (process_video, :100-143), one frame per call ----
 * d_boxes   : HIP device pointer, float32 [max_boxes][6] = x1, y1, x2, y2, score, cls: one frame of detector rows.
 * d_n_boxes : HIP device pointer, int32 [1], or NULL (n = max_boxes); clamped to [0, max_boxes].
 * d_state   : HIP device pointer, bf_smooth_state_words(slots) = 4 + 4 * slots 32-bit words, read and written: word 0 = the number m of
 *             previous boxes (int32), words 1..3 = 0, then `slots` rows of four float32, the previous frame's kept boxes (rows from m
 *             on are zeros).  All zero is a fresh stream.
 * d_moved, d_score, d_status : float32 [slots][4], float32 [slots], int32 [slots]: the results of bf_match_boxes_device run on d_state's
 *             rows (frames = 1, d_boxes = d_state + 4 words, box_stride = 4, d_n_boxes = d_state, max_boxes = slots).  Previous box p
 *             TAKES PART iff p < clamp(m, 0, slots) and d_status[p] == 0.
 * Definition.  A row j < n whose four coordinates are finite, with x2 > x1, y2 > y1 and a finite score, is VALID iff score > conf_high
 * and a CANDIDATE iff conf_low < score <= conf_high.
 *   If any row is valid:  d_out = the rows with every non-valid row's score set to 0; the kept rows are the valid ones.
 *   Otherwise:  a candidate is BOOSTED iff some previous box p that takes part has IoU(d_moved[p], candidate) > iou_threshold OR
 *   d_score[p] > corr_threshold; a boosted row's score becomes conf_high, every other row's 0; the kept rows are the boosted ones
 *   (the reference's >= confh).
 *   IoU is compute_iou (:26-37) in float32, every operation rounded once: iw = max(0, min(x2, x2g) - max(x1, x1g)), ih likewise,
 *   inter = iw * ih, union = ((x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g)) - inter, union > 0 ? inter / union : 0, max(0, v) = v > 0 ? v : 0.
 *   The first `slots` kept rows' boxes, in row order, become the state's rows and m their number; the kept rows beyond are counted.
 * The `OR d_score[p] > corr_threshold` arm is the reference's, and it is indiscriminate: one well-correlated previous box boosts EVERY
 * candidate of the frame, wherever the candidate lies.  A corr_threshold > 1 switches that arm off, so that overlap is required.
 * d_out     : float32 [max_boxes][6]: coordinates and class pass through unchanged (rows from n on included, with score 0).  A zero
 *             score is not a box to bf_track_boxes_device and bf_fuse_boxes_device, so d_out feeds both with d_n_boxes = NULL.
 * d_boosted : int32 [max_boxes], or NULL: 1 for a boosted row.  d_counts : int32 [4], or NULL: valid rows, candidates (boosted ones
 *             included), boosted rows, kept rows dropped for want of a slot.
 * stream    : enqueue only, one launch of one workgroup; graph-capturable from the first call.
 * Returns 0, or -1 for: d_boxes, d_moved, d_score, d_status, d_state or d_out null; max_boxes outside [1, BF_MATCH_MAX_BOXES]; slots
 * outside [1, BF_SMOOTH_MAX_SLOTS]; conf_low, conf_high, iou_threshold or corr_threshold not finite; no GPU.  All arguments are checked
 * before device bring-up.  bf_smooth_state_words(slots) returns 4 + 4 * slots, or -1 for slots outside that range (it records no error). */
#define BF_SMOOTH_MAX_SLOTS 64
int bf_smooth_state_words(int slots);
int bf_smooth_boxes_device(const float *d_boxes, const int *d_n_boxes, int max_boxes, float conf_low, float conf_high,
                           float iou_threshold, float corr_threshold, int slots, const float *d_moved, const float *d_score,
                           const int *d_status, void *d_state, float *d_out, int *d_boosted, int *d_counts, void *stream);

/* ---- continuous-stream mode of the device path (BF_PAD, BF_LERP): delays read the previous window ----
 * Every other entry point treats a window as if the world began at its first sample: a microphone delayed by p samples gives
 * nothing to the first p outputs (out[p + i] += s[i], zero prefix), as the reference does.  That is the first item of the reference
 * authors' own low-level future work (PC/TODO.md, "Padding -> read previous samples": the zero prefix "introduces clipping", "a
 * better solution is to read the last N samples of the previous signal", a ring buffer for it "has not been put in place").  Here
 * the samples a delay reaches before the start of frame f are taken from frame f - 1 of the batch, for f = 0 from d_prev.
 *
 * Definition.  N = N_SAMPLES; frames float32 [frames][m_total][N], mic-major, as bf_das_device takes them; `hop` = distance in samples
 * between the starts of consecutive frames (the hop of bf_ingest_stream_device).  For frame f, microphone row r:
 *     x_r(t) = frame f's own sample [r][t]          for 0 <= t < N
 *     x_r(t) = prev_f[r][hop + t]                   for t < 0
 * prev_f = frame f - 1 of the call for f >= 1; prev_0 = d_prev, float32 [m_total][N] on the device: the frame that started `hop`
 * samples before frame 0 (NULL: all zeros -- silence before the stream).  With p_m, h_m the loaded table's entries for (direction,
 * mic m) and r_m = adaptive_array[m], summed in mic order m = 0 .. n-1 starting from 0.0f, for EVERY t in [0, N):
 *     pad :  out[t] = sum_m x_{r_m}(t - p_m)
 *     lerp:  out[t] = sum_m fma(h_m, x_{r_m}(t - p_m) - x_{r_m}(t - p_m - 1), x_{r_m}(t - p_m - 1))
 * (the reference drops the i < 0 edge samples; this mode does not).  For t >= H both equal miso_pad / miso_lerp bit for bit.
 * With d_prev == NULL and silence as history, lerp gives h * s[0] at t = p where the reference gives 0: that follows from the
 * definition, the sample before the stream is 0, not absent.
 * A map entry is image[d] = (sum_t (out_d[t] / n)^2) / N, summed in t order in float32 with every square rounded before it is
 * added.  (bf_das_device sums in the same order, and where N_SAMPLES % 4 != 0 fuses square and add for the last N_SAMPLES % 4
 * samples, as the compiled reference does; this mode has no such reference and does not.)
 *
 * History: H = max_whole (pad) or max_whole + 1 (lerp), max_whole the largest whole-sample delay of the loaded table.  The calls
 * require H <= hop <= N_SAMPLES.  bf_stream_history returns H for BF_PAD / BF_LERP, -1 when that table is not loaded or for any
 * other algo (it records no error).
 *
 * bf_miso_stream_device: bf_miso_device's contract -- d_offsets, mic_gain, d_status codes, NaN beams for rejected offsets,
 * out_stride, adaptive_array -- with the two extra arguments.  bf_das_stream_device: bf_das_device's contract (direction shards,
 * image_stride, adaptive_array); maps in this mode always take the strided kernel layout (bf_last_das_variant 9; the beam call
 * leaves that value alone), no digest is built.  Both only enqueue and allocate nothing after the first call (a new adaptive
 * array synchronises the device, as in bf_das_device); graph-capturable after one warm-up call.  d_prev is read by the launch: keep
 * it alive and unchanged until the launch has run.
 * Return 0, or -1 (bf_last_error names the value; nothing enqueued) for: BF_HYBRID, BF_FIR_NAIVE, BF_FIR_VEC (they read ahead of
 * the window's end, which a causal stream cannot supply) or an unknown algo; hop < 1; hop > N_SAMPLES; H > hop; a table with
 * entries beyond N_SAMPLES (the loader clamps them, a stream cannot reach them); and everything bf_miso_device / bf_das_device
 * refuse.  All arguments are checked before device bring-up; the table checks need the device the table lives on. */
int bf_stream_history(int algo);
int bf_miso_stream_device(int algo, const float *d_signals, int m_total, int frames, int hop, const float *d_prev,
                          const int *adaptive_array, int n, const int *d_offsets, int beams, float mic_gain,
                          float *d_out, int out_stride, int *d_status, void *stream);
int bf_das_stream_device(int algo, const float *d_signals, int m_total, float *d_images, int image_stride, int frames, int hop,
                         const float *d_prev, const int *adaptive_array, int n, int dir_begin, int dir_end, void *stream);

/* ---- map values at listed directions: the power map evaluated at a device list of table offsets, one enqueue ----
 * Every consumer of a power map reads a few cells of it (bf_peaks_device's window maxima, a tracker's slots, the loudest cell under a
 * detector box), and bf_das_device / bf_das_stream_device give a cell's value only as part of a contiguous direction range.  These
 * two calls give the map at the directions a list names; the list lives on the device and may differ from frame to frame, so a
 * coarse scan, its peaks and a fine scan around them chain without a host round trip.
 *
 * Definition.  d_power[f][b] is the mean-power rule of the matching map call applied to the beam miso_* forms at offset d_offsets[f][b]
 * of frame f (bf_das_select_device: the beam of bf_miso_device with mic_gain 0; bf_das_select_stream_device: that of
 * bf_miso_stream_device, the definition above).  The rule: out[t] /= (float)n, the squares summed in t order in float32, the sum
 * / N_SAMPLES.  The window-local call fuses square and add for the last N_SAMPLES % 4 samples, as bf_das_device and the compiled
 * reference do; the stream call rounds every square, as bf_das_stream_device does.  So for an accepted offset d * n (BF_FIR_VEC:
 * d * n * N_TAPS) d_power[f][b] equals the float bf_das_device (bf_das_stream_device) writes for direction d of frame f BIT FOR BIT,
 * whichever kernel family bf_das_device chose.  The value does not depend on the list's order or length, on count or on frames.
 *
 * algo      : bf_das_select_device: BF_PAD, BF_LERP, BF_HYBRID, BF_FIR_VEC (bf_miso_device's set; BF_FIR_NAIVE is refused);
 *             bf_das_select_stream_device: BF_PAD, BF_LERP.  The table is the one the matching load_coefficients_* loaded.
 * d_signals / m_total / frames / adaptive_array / n : as bf_miso_device; hop / d_prev : as bf_miso_stream_device
 * d_offsets : HIP device pointer, int32 [frames][count] when per_frame != 0, [count] shared by all frames when per_frame == 0 (the
 *             lattice of a coarse scan).  Table offsets exactly as bf_miso_device takes them; unsorted lists and repeated entries are fine.
 * d_power   : HIP device pointer, float32 [frames][power_stride], power_stride >= count; floats [count, power_stride) of every row are
 *             left untouched.
 * d_status  : HIP device pointer, int32 [frames][count], or NULL.  When given, every entry is written with bf_miso_device's codes: 0 ok,
 *             1 offset negative or past the loaded table, 2 BF_FIR_VEC offset not a multiple of N_TAPS.  A rejected entry reads nothing
 *             from the table and its power is a quiet NaN (0x7fc00000); the other entries are unaffected.  bf_peaks_device's and the
 *             trackers' empty slots (-1) are such entries.
 * stream    : hipStream_t (0 = null stream).  Enqueue only, one launch, no atomics, no allocation after the first call -- except a
 *             call with a new adaptive array, which synchronises the device as bf_das_device does; graph-capturable after one warm-up
 *             call.  No digest is built.  Does not change bf_last_das_variant.
 * Return 0, or -1 (bf_last_error names the value; nothing enqueued) for: everything bf_miso_device refuses (the stream call:
 * everything bf_miso_stream_device refuses); count < 1; power_stride < count; d_offsets or d_power null; d_power or d_status
 * sharing a byte with d_signals, d_prev, d_offsets or each other.  All arguments are checked before device bring-up; the table checks
 * need the device the table lives on.
 * bf_plan_das_select: the launch geometry of such a call (no GPU needed), out[0..9] as bf_plan_das; stream_mode != 0 plans the
 * stream call.  The rows always take the strided layout, so n_chunks may differ from bf_plan_das's for the same sizes. */
int bf_das_select_device(int algo, const float *d_signals, int m_total, int frames, const int *adaptive_array, int n,
                         const int *d_offsets, int count, int per_frame, float *d_power, int power_stride, int *d_status, void *stream);
int bf_das_select_stream_device(int algo, const float *d_signals, int m_total, int frames, int hop, const float *d_prev,
                                const int *adaptive_array, int n, const int *d_offsets, int count, int per_frame,
                                float *d_power, int power_stride, int *d_status, void *stream);
int bf_plan_das_select(int algo, int n, int frames, int count, int max_whole, int stream_mode, int n_cus, long long out[10]);

/* The plans of the stream and listed-direction launches, for tests that have to know which kernel instantiation a shape reaches.
 * bf_plan_das_stream: the launch geometry bf_das_stream_device gives directions [dir_begin, dir_end) of `frames` frames (no GPU
 *   needed), out[0..9] as bf_plan_das.  It is the map planner's own answer, not bf_plan_das_select's with stream_mode != 0.
 *   -1 for out == NULL and for what the planner refuses (BF_HYBRID and the FIRs, an empty launch).
 * bf_last_strided_plan: what the most recent launch of this process among bf_das_stream_device, bf_das_select_device,
 *   bf_das_select_stream_device and bf_miso_stream_device dispatched on: out[0..9] the plan as above (for bf_miso_stream_device
 *   the one-beam plan of bf_plan_das(algo, n, 1, 0, 1, max_whole)), out[10] the kernel (0 das_mimo_kernel with history, 1 das_select_kernel,
 *   2 das_select_kernel with history, 3 das_miso_kernel with history), out[11] the algorithm.  The kernel's template arguments are
 *   (out[11], out[0], out[6]).  -1 for out == NULL and before the first such launch; a call that was refused leaves the record alone. */
int bf_plan_das_stream(int algo, int n, int frames, int dir_begin, int dir_end, int max_whole, int n_cus, long long out[10]);
int bf_last_strided_plan(long long out[12]);

/* ---- band selection on the time-domain path: one FIR per band on every row of a frame batch, continuous across windows ----
 * The time-domain maps and beams are broadband; delay-and-sum is linear, so ONE filter applied to every microphone row leaves all
 * inter-microphone delays intact: a band-limited map is bf_das_device on filtered frames, band-limited audio is the same filter on
 * the [frames][beams][N] output of bf_miso_device (far fewer rows than the microphones).
 * d_signals : HIP device pointer, float32 [frames][rows][N_SAMPLES] (N = N_SAMPLES); `rows` is whatever the caller has --
 *             the microphone rows of a frame batch, or frames x beams rows of beams (then frames = 1, or hop = 0).
 * d_taps    : HIP DEVICE pointer, float32 [bands][n_taps]: h[b][t].
 * d_out     : HIP device pointer, float32 [bands][frames][rows][N_SAMPLES].  Every element is written.
 * Definition (builder-defined; there is no band selection on the reference's time-domain path):
 *     out[b][f][r][j] = acc_T,   acc_0 = 0.0f,   acc_{t+1} = fmaf(h[b][t], x~_f[r][j - t], acc_t)   for t = 0 .. n_taps-1
 * in that order, one float32 rounding per step (a single-rounding fused multiply-add, libm's fmaf), where
 *     x~_f[r][i] = d_signals[f][r][i]                                 for 0 <= i < N
 *     x~_f[r][i] = d_signals[f-1][r][hop + i]                         for i < 0, hop > 0, f >= 1  (frame f - 1 of the call)
 *     x~_0[r][i] = d_prev[r][hop + i], or 0.0f when d_prev is NULL    for i < 0, hop > 0
 *     x~_f[r][i] = 0.0f                                               for i < 0, hop == 0         (independent windows)
 * `hop` is the distance in samples between the starts of consecutive frames and d_prev float32 [rows][N_SAMPLES] the unfiltered
 * window that began `hop` samples before frame 0: bf_miso_stream_device's convention.  With n_taps - 1 <= hop the outputs of
 * overlapping windows agree bit for bit where both exist (out[f][j] == out[f-1][j + hop]), so the filtered frames are again the
 * windows of one stream -- of the filtered stream -- and may be handed to bf_das_stream_device / bf_miso_stream_device with
 * the filtered previous window as their d_prev.
 * The result does not depend on the internal blocking (a lane owns four consecutive outputs, all bands share the LDS reads),
 * on the alignment of the pointers or on N % 4: every output's chain runs t = 0 .. n_taps-1 in order, taps past the last are
 * skipped, not multiplied by zero.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: one launch; no allocation, no workspace, no atomics, no
 *             synchronisation; graph-capturable from the first call.  d_prev and d_taps are read by the launch.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_signals, d_taps or d_out null; rows, frames, bands or
 * n_taps < 1; bands > BF_BAND_MAX_BANDS; n_taps > N_SAMPLES; hop < 0; hop > N_SAMPLES; hop > 0 with n_taps - 1 > hop; d_out's byte
 * range overlapping that of d_signals or d_prev (frame f - 1 is read while frame f is written); no GPU.  All arguments are
 * checked before device bring-up. */
#define BF_BAND_MAX_BANDS 16
int bf_band_filter_device(const float *d_signals, int rows, int frames, int hop, const float *d_prev,
                          const float *d_taps, int n_taps, int bands, float *d_out, void *stream);

/* ---- phase-transform (SRP-PHAT) frames: every in-band DFT bin of every row weighted by |X_k|^-beta, K bands in one launch ----
 * A power map weighs a frequency by how loud it is, so a loud narrow-band interferer owns it.  The phase transform gives every in-band
 * bin of every microphone unit magnitude and keeps its phase: each frequency votes once, by its inter-microphone delays.  The weighting
 * is per row and zero-phase, so it leaves every delay intact: a PHAT map is bf_das_device on whitened frames, and peaks, listed
 * directions and tracking work on it unchanged.  Whitened audio is noise-like: listen on the RAW frames at the offsets the map gave.
 * The windows are whitened independently of each other: there is no hop and no carried state.
 * d_signals : HIP device pointer, float32 [frames][rows][N_SAMPLES] (N = N_SAMPLES, a power of two in [32, 4096]; bf_configure
 *             itself stops at N_SAMPLES = 1024 today, so 2048 and 4096 cannot be reached and are not tested).
 * d_window  : HIP DEVICE pointer, float32 [N] (features.hann makes one), or NULL: a rectangular window.  With a rectangular window the
 *             leakage of strong low tones carries their phase into every bin; Hann is the sensible default.
 * bins      : HOST pointer, int32 [bands][2] = [lo_b, hi_b), clipped to [0, N / 2 + 1].
 * beta, gain: HOST pointers, float32 [bands].  bins, beta and gain are copied into the launch's arguments: a captured graph keeps them.
 * d_out     : HIP device pointer, float32 [bands][frames][rows][N].  Every element is written.
 * Definition (builder-defined; the reference has no such weighting).  For every row x of N samples:
 *     u[t] = d_window[t] * x[t]                       one float32 multiply; u = x without a window
 *     X_k  = sum_t u[t] exp(-2 pi i k t / N)          k = 0 .. N / 2
 *   and for band b, lo <= k < hi after clipping:
 *     rms_b   = sqrt(mean over lo <= k < hi of |X_k|^2)
 *     floor_b = max(floor_abs, floor_rel * rms_b)
 *     d_k     = max(|X_k|, floor_b)
 *     W_k     = X_k                  beta == 0        (no floor is formed)
 *     W_k     = X_k / d_k            beta == 1        (IEEE division of both components)
 *     W_k     = d_k^-beta X_k        otherwise
 *     W_k     = 0                    where d_k == 0 (beta > 0), and outside the band
 *     out[b][f][r][j] = gain_b / N * (Re W_0 + (-1)^j Re W_{N/2} + 2 Re sum over 0 < k < N / 2 of W_k exp(+2 pi i j k / N))
 *   Both transforms are radix-2 decimation-in-time FFTs in float32 with twiddles rounded once from double; their rounding is not part of
 *   the definition (tests/whiten_np.py derives the tolerance: norm-wise, eta = 5 sqrt 2 per pass), these promises are:
 *   - a row's N outputs depend only on that row's N samples, the window and that band's scalars -- not on rows, on frames, on the row's
 *     position, on the other rows, on the other bands of the call or on the alignment of any pointer: band b of a K-band call equals
 *     the single-band call, bit for bit;
 *   - a row of zeros gives N outputs equal to 0 for every beta (ingest zeroes the dead microphones' rows; they stay silent);
 *   - with floor_abs == 0, multiplying a row by 2^e leaves a beta == 1 output bit for bit unchanged and multiplies a beta == 0 output
 *     by 2^e exactly, while nothing overflows or goes subnormal: the map does not depend on a microphone's gain;
 *   - a non-finite sample affects only its own (frame, row).
 * stream    : hipStream_t (0 = null stream).  Enqueue only: one launch (a workgroup per (frame, row), walking when there are more than
 *             2048; one wave up to N = 512, four above; 4.5 N + 8 floats of LDS); no allocation, no workspace, no atomics, no
 *             synchronisation; graph-capturable from the first call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_signals, bins, beta, gain or d_out null; rows, frames or
 * bands < 1; bands > BF_WHITEN_MAX_BANDS; N_SAMPLES not a power of two in [32, 4096]; a band with lo >= hi after clipping; a beta not
 * finite or outside [0, 1]; a gain not finite; floor_rel or floor_abs negative or not finite; d_out's byte range sharing a byte with
 * d_signals or d_window; no GPU.  All arguments are checked before device bring-up. */
#define BF_WHITEN_MAX_BANDS 16
int bf_whiten_device(const float *d_signals, int rows, int frames, const float *d_window,
                     const int *bins, const float *beta, const float *gain, int bands,
                     float floor_rel, float floor_abs, float *d_out, void *stream);

/* ---- filter-and-sum beams: one FIR per (beam, microphone), then a sum over the microphones ----
 * Every beam of bf_miso_device / bf_miso_stream_device is delay-and-sum: one whole-sample or lerp delay per microphone from the loaded
 * table, which has no gain control over any direction but its own.  Any FIXED beamformer -- null steering (LCMV), superdirective, MVDR
 * weights frozen over a batch -- is a filter-and-sum: this call takes the filters as taps and leaves their design to the caller
 * (filtersum.design_lcmv is one).  The loaded tables play no part.
 * d_signals : HIP device pointer, float32 [frames][m_total][N_SAMPLES] (N = N_SAMPLES), as bf_miso_device takes it.
 * adaptive_array / n : HOST array of the active rows, as in bf_miso_device: cached on the device, a new array synchronises the
 *             device once.
 * d_taps    : HIP DEVICE pointer, float32 [beams][n][n_taps]: g[b][m][t] is tap t of active microphone m (row r_m = adaptive_array[m])
 *             for beam b.
 * d_out     : HIP device pointer, float32 [frames][beams][out_stride], out_stride >= N_SAMPLES.  Floats past N_SAMPLES in a row are
 *             left untouched, every other element is written.
 * hop, d_prev : bf_band_filter_device's convention.  d_prev is float32 [m_total][N_SAMPLES] or NULL, and
 *     x~_f[r][i] = d_signals[f][r][i]                                 for 0 <= i < N
 *     x~_f[r][i] = d_signals[f-1][r][hop + i]                         for i < 0, hop > 0, f >= 1  (frame f - 1 of the call)
 *     x~_0[r][i] = d_prev[r][hop + i], or 0.0f when d_prev is NULL    for i < 0, hop > 0
 *     x~_f[r][i] = 0.0f                                               for i < 0, hop == 0         (independent windows)
 * Definition, in float32, nothing contracted except the written fmaf (single rounding, libm's fmaf):
 *     c_m[j]       = acc_T,  acc_0 = 0.0f,  acc_{t+1} = fmaf(g[b][m][t], x~_f[r_m][j - t], acc_t)   t = 0 .. n_taps-1, in that order
 *     out[f][b][j] = s_n,    s_0 = 0.0f,    s_{m+1} = s_m + c_m[j]                                   m = 0 .. n-1, in that order
 * A tap past the last is skipped, never multiplied by zero.  Two consequences:
 *   - with g[b][m][t] = (t == p_m) and finite samples, hop == 0 gives miso_pad / bf_miso_device(BF_PAD, mic_gain 0) at the delay
 *     row p bit for bit (a delta chain hands the sample through unchanged, and both sums start at +0.0f in microphone order);
 *   - with hop > 0 and max p_m + 1 <= n_taps <= hop + 1 the same taps give bf_miso_stream_device(BF_PAD) bit for bit.
 * With n_taps - 1 <= hop the outputs of overlapping windows agree bit for bit where both exist (out[f][b][j] == out[f-1][b][j + hop]).
 * The result does not depend on the internal blocking (a workgroup takes 256 outputs of one beam and deals the microphones round
 * its waves; a lane owns four consecutive outputs), on which wave computes which microphone (the c_m are parked and added by one
 * owner in microphone order, never accumulated where they are computed), on the alignment of the pointers, on N % 4 or on the
 * number of beams launched together.  bf_filter_sum_waves(1 | 2 | 4 | 8 | 16) pins the waves of a workgroup for measurements (0: the
 * launch decides, the default; returns the previous value, -1 for another argument): the result is the same for each.  It is a
 * process-global measurement switch, not a tuning interface: it changes the launch shape of every later call, captures included.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: one launch; no allocation after the first call, no workspace, no atomics;
 *             a new adaptive array synchronises the device; graph-capturable after one warm-up call, as bf_miso_device.  d_prev and
 *             d_taps are read by the launch.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_signals, adaptive_array, d_taps or d_out null; frames, n,
 * beams or n_taps < 1; beams > BF_FILTER_SUM_MAX_BEAMS; n_taps > N_SAMPLES; hop < 0; hop > N_SAMPLES; hop > 0 with n_taps - 1 > hop;
 * out_stride < N_SAMPLES; an adaptive_array row outside [0, m_total); d_out's byte range (its first float to the last one written)
 * overlapping that of d_signals, d_prev or d_taps; no GPU.  All arguments are checked before device bring-up. */
#define BF_FILTER_SUM_MAX_BEAMS 16
int bf_filter_sum_device(const float *d_signals, int m_total, int frames, int hop, const float *d_prev,
                         const int *adaptive_array, int n, const float *d_taps, int n_taps, int beams,
                         float *d_out, int out_stride, void *stream);
int bf_filter_sum_waves(int waves);

/* ---- null-steering taps designed on the device: one row of slot offsets -> the [beams][n][n_taps] taps bf_filter_sum_device reads ----
 * bf_peaks_device / bf_track_sources_device leave their offsets on the device and bf_filter_sum_device reads its taps there; this
 * call is the link between them, so tracker -> designer -> filter-and-sum beams is one stream of launches (and one captured graph)
 * with no host round trip when a source moves.  The design is filtersum.design_lcmv's, in float64 throughout (LCMV for spatially
 * white noise, by frequency sampling); filtersum.design_slots is its host statement with the slot semantics below.  The loaded
 * tables and the configured sizes play no part.
 * d_tau     : HIP device pointer, float64 [dirs][n]: calculate_delays() reshaped, uploaded once by the caller.  Microphone m LEADS
 *             by tau[d][m] samples (design_lcmv's convention).
 * d_offsets : HIP device pointer, int32 [sources]: one row of what bf_peaks_device or bf_track_sources_device writes.  Slot i is a
 *             SOURCE iff its entry is >= 0, a multiple of offset_per_dir and entry / offset_per_dir < dirs (the tracker's rule, as in
 *             bf_fuse_boxes_device); its direction is entry / offset_per_dir.
 * Beam i belongs to slot i; slots are NOT compacted, a tracker slot keeps its beam.  The look direction of beam i is slot i's, its
 * nulls are every OTHER slot that is a source, tried in slot order.  A slot that is not a source gets all-zero taps (a silent beam),
 * d_status[i] = 1, zero gains and zero kept entries; a designed slot gets d_status[i] = 0.
 * bin_lo .. bin_hi (inclusive) are the in-band bins k of the n_taps-point grid (T = n_taps), K = bin_hi - bin_lo + 1 of them; the host
 * computes them (filtersum.band_bins), no frequency is compared on the device.  For every beam i and in-band bin k:
 *     w = 2 pi k / T,   c_d[m] = e^{+jw tau[d][m]}
 *     a null is DROPPED at the bin iff |c^H c'| / n > rho against the look vector or against a null already kept at that bin
 *     C = [c_look, kept nulls],  f = (e^{-jw(T-1)/2}, 0, ..),  u = C (C^H C)^{-1} conj(f),  G_k[m] = conj(u[m])
 * the minimum-norm gains with H(w, look) = e^{-jw(T-1)/2} and H(w, kept null) = 0, and
 *     g[i][m][t] = (1/T) sum_k s_k Re(G_k[m] e^{+j 2 pi k t / T})   over the in-band bins, in ascending k,
 *     s_k = 1 for k = 0 and for k = T/2 with T even, 2 otherwise    (NumPy's irfft: the real part of a DC or Nyquist gain is kept)
 * rounded once to float32.  Everything before that rounding is float64; sines and cosines are the device library's, the p x p
 * system (p <= sources) is solved by a Cholesky factorisation, so gains agree with a host design to roundoff times the condition
 * of C^H C, not bit for bit.  rho = 1 with two slots on one direction keeps a null the look vector cannot be told from: C^H C is
 * singular and that beam's gains and taps are not finite; nothing else is affected.
 * d_gains   : float64 [sources][K][n][2], (re, im) of G_k[m].  Required: it is the call's intermediate (the second launch reads
 *             it) and an output a caller can inspect; because of it the call needs no workspace and allocates nothing.
 * d_taps    : float32 [sources][n][n_taps], bf_filter_sum_device's layout for beams = sources.
 * d_kept    : int32 [sources][K][sources]: 1 iff slot j is a kept null of beam i at that bin; the diagonal, slots that are no source
 *             and dropped nulls are 0.
 * d_status  : int32 [sources].
 * Every entry of every output is written by every call.  The result does not depend on the number of slots designed together
 * (slots behind the last source change nothing) and is the same bits from call to call.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: two launches (gains, then taps); no allocation, no synchronisation, no
 *             atomics; graph-capturable from the first call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: any pointer null; dirs, n, sources, offset_per_dir or
 * n_taps < 1; sources > BF_LCMV_MAX_SOURCES; sources > n (more constraints than microphones make C^H C singular); n_taps >
 * BF_LCMV_MAX_TAPS; a bin range outside 0 <= bin_lo <= bin_hi <= n_taps / 2; rho not in (0, 1] (NaN included); the byte range of an
 * output overlapping that of an input or of another output; no GPU.  All arguments are checked before device bring-up. */
#define BF_LCMV_MAX_SOURCES 8
#define BF_LCMV_MAX_TAPS 1024
int bf_lcmv_design_device(const double *d_tau, int dirs, int n, const int *d_offsets, int sources, int offset_per_dir,
                          int n_taps, int bin_lo, int bin_hi, double rho,
                          double *d_gains, float *d_taps, int *d_kept, int *d_status, void *stream);

/* ---- adaptive (MVDR) taps designed on the device: the frames' own covariance -> the [beams][n][n_taps] taps bf_filter_sum_device reads ----
 * bf_lcmv_design_device is geometry-only: a beam nulls a direction some slot names.  A talker under another one's main-lobe skirt, a
 * reflection, a fan never get a slot.  This call designs the taps from the data: frames already on the device go in, the sample
 * covariance of short segments of them is formed per bin, and every source slot gets the minimum-variance gains with unit response
 * in its own direction (MVDR, one constraint per beam; the other slots are NOT hard nulls here).  filtersum.design_mvdr_slots is the
 * host statement.  Everything before the taps' rounding to float32 is float64.  The loaded tables play no part.
 * d_signals, m_total, adaptive_array, n : as bf_filter_sum_device (float32 [frames][m_total][N_SAMPLES]; HOST array of the n active rows
 *             r_m, cached on the device, a new array synchronises the device once).  n <= BF_MVDR_MAX_MICS.
 * d_tau, dirs, d_offsets, sources, offset_per_dir, the slot rule, bin_lo .. bin_hi and T = n_taps : as bf_lcmv_design_device.
 *             K = bin_hi - bin_lo + 1, P = frames * segs.
 * Snapshots.  p = f * segs + q; segment q starts at sample s = seg_first + q * seg_hop of window f; for k = bin_lo + kk
 *     X_p[kk][m] = sum_t win[t] * (double)x_f[r_m][s + t] * e^{-j 2 pi ((k t) mod T) / T},   t = 0 .. T-1 in ascending order
 *   with cos / sin(2 pi r / T) from a sincospi table indexed by the integer (k t) mod T.  win = d_window, float64 [T], NULL = all ones.
 * Covariance.  R_k[a][b] = (1/P) sum_p X_p[a] conj(X_p[b]), one sequential chain per entry in ascending p, divided by P once;
 *   computed for a >= b and mirrored: d_cov is EXACTLY Hermitian, its diagonal's imaginary part is exactly zero.
 * Loading.  tr_k = sum_a R_k[a][a] in ascending a.  Finite and > 0: R'_k = R_k + (loading * tr_k / n) I, d_fallback[kk] = 0.  Otherwise
 *   (silence, NaN or Inf samples): R'_k = I, d_fallback[kk] = 1, and the gains below are the no-null design's, c conj(f0) / n.
 * Factor and solve.  R'_k = L L^H (Cholesky; an entry's subtractions run in ascending column order).  With w = 2 pi k / T, for every
 *   source slot i and its look vector c[m] = e^{+jw tau[d_i][m]}:
 *     y = L^{-1} c,  z = L^{-H} y,  den = sum_m |y_m|^2 (ascending m),  u = z conj(f0) / den,  f0 = e^{-jw(T-1)/2},  G_k[m] = conj(u[m])
 *   which is u = R'^{-1} c conj(f0) / (c^H R'^{-1} c): H(w, look) = f0.  All slots share one factorisation per bin.  A loading so small
 *   that R'_k is not numerically positive definite leaves that bin's gains (and the taps) not finite; nothing else is affected.
 * Taps.  bf_lcmv_design_device's second stage on these gains (the same launch).  A slot that is no source gets zero taps, zero gains
 *   and d_status 1; a designed slot d_status 0.
 * Known limit: with the look talker in the frames at the interferer's level and any steering mismatch, sample-covariance MVDR cancels
 * part of the look signal too (self-cancellation); the T-sample snapshot is a narrowband model and delays here reach 15 samples.
 * Learn the covariance from frames in which the look talker is weak, or raise the loading.
 * d_snap    : float64 [P][K][n][2].   d_cov, d_chol : float64 [K][n][n][2]; d_chol's lower triangle is L, its strict upper is 0.
 * d_gains   : float64 [sources][K][n][2].   d_taps : float32 [sources][n][n_taps].   d_status : int32 [sources].   d_fallback : int32 [K].
 * All seven are outputs a caller can inspect and the call's only workspace.  Every entry of every one is written by every call; the
 * bits are the same from call to call and do not depend on the number of slots designed together.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: four launches (snapshots, covariance, factor and solve, taps); no
 *             allocation after the first call, no atomics; a new adaptive array synchronises the device; graph-capturable after one
 *             warm-up call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: any pointer except d_window null; frames, n, segs, seg_hop,
 * dirs, sources, offset_per_dir or n_taps < 1; seg_first < 0; seg_first + (segs - 1) * seg_hop + n_taps > N_SAMPLES; n >
 * BF_MVDR_MAX_MICS; sources > BF_LCMV_MAX_SOURCES; n_taps > BF_LCMV_MAX_TAPS; a bin range outside 0 <= bin_lo <= bin_hi <= n_taps / 2;
 * loading not finite or <= 0; an adaptive_array row outside [0, m_total); the byte range of an output overlapping that of an input
 * or of another output; no GPU.  All arguments are checked before device bring-up. */
#define BF_MVDR_MAX_MICS 256
int bf_mvdr_design_device(const float *d_signals, int m_total, int frames, const int *adaptive_array, int n,
                          int seg_first, int seg_hop, int segs, const double *d_window,
                          const double *d_tau, int dirs, const int *d_offsets, int sources, int offset_per_dir,
                          int n_taps, int bin_lo, int bin_hi, double loading,
                          double *d_snap, double *d_cov, double *d_chol, double *d_gains,
                          float *d_taps, int *d_status, int *d_fallback, void *stream);

/* ---- the same taps from a covariance that is CARRIED, WEIGHTED and FORGOTTEN: bf_mvdr_design_device with its covariance as device state ----
 * bf_mvdr_design_device learns from every frame of one batch and drops what it learned.  Here the weighted sum of X X^H is state on the
 * device that carries from call to call, every frame has a weight read on the device (0 for a frame in which the look talker speaks:
 * no self-cancellation from it), and a forgetting factor sets how long old frames count.  filtersum.mvdr_learn followed by
 * filtersum.design_mvdr_learned is the host statement.  Every argument not named here means what it means in bf_mvdr_design_device.
 * State, read and written in place:  d_acc float64 [K][n][n][2], the weighted sum per bin;  d_mass float64 [1], the weights' sum times
 *   segs.  All-zero bytes are the empty state: the caller zeroes both to start a stream.  One state belongs to one (adaptive array,
 *   n_taps, bin range, window, segment layout); nothing records them.
 * d_weights : float64 [frames] on the device, NULL = all 1.0.  Frame f is LEARNED iff w_f is finite and > 0.  +-0.0 is skipped
 *   silently; a NaN, an Inf or a negative weight is skipped and counted.  d_used int32 [2] = (frames learned, weights refused); every
 *   call writes it.
 * forget : lambda in (0, 1], applied once per LEARNED frame; a skipped frame leaves the state untouched bit for bit.  Forgetting counts
 *   what was learned, not the time that passed: a long stretch of look-talker speech does not decay the state to 0 / 0.
 * The chains.  One per entry a >= b, starting at the stored d_acc[kk][a][b]; frames in ascending f; for a learned frame
 *     acc = forget * acc (both parts),   then for q = 0 .. segs-1:  acc = acc + w_f * t,   t = (ar*br + ai*bi, ai*br - ar*bi)
 *   with X_p[a] = (ar, ai), X_p[b] = (br, bi), p = f * segs + q: bf_mvdr_design_device's term; nothing is contracted.  And
 *     mass = forget * mass + w_f * (double)segs   over the same frames in the same order.
 *   After the last frame acc goes back to d_acc, its conjugate to the mirror, +0.0 to the diagonal's imaginary part (a call that learns
 *   no frame does not write d_acc at all), and d_cov = acc / mass where mass > 0, otherwise d_cov = 0: every bin then falls back
 *   (d_fallback 1, the beam without nulls).  With d_acc and d_mass zero, weights NULL or all 1.0 and forget 1 the chains are
 *   bf_mvdr_design_device's operations and all seven of its outputs come out byte for byte.
 * Loading, factor, solve, taps: bf_mvdr_design_device's launches on this d_cov.  d_snap is written for every frame, learned or not.
 * frames == 0 is the RE-AIM: new taps for the offsets given now from the state as it stands.  d_signals, d_weights, d_window and d_snap
 *   may be NULL (they are not touched), adaptive_array is still checked, the state is untouched, d_used = (0, 0).
 * stream : enqueue only: four launches (snapshots and the mass, accumulation, factor and solve, taps), three for the re-aim; no
 *   allocation after the first call, no atomics, the same bits from call to call on the same state and inputs; graph-capturable after one
 *   warm-up call.  A REPLAY ADVANCES THE STATE like any other call: a graph that learns, replayed twice on the same frames, has learned
 *   them twice.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued, the state untouched) for bf_mvdr_design_device's refusals with
 * frames < 0 in place of frames < 1, and: forget outside (0, 1] or NaN; d_acc, d_mass or d_used null; with frames > 0, d_signals or
 * d_snap null; the byte range of d_acc, d_mass, d_used or another output overlapping that of an input (d_weights among them) or of
 * another output.  All arguments are checked before device bring-up. */
int bf_mvdr_learn_device(const float *d_signals, int m_total, int frames, const int *adaptive_array, int n,
                         int seg_first, int seg_hop, int segs, const double *d_window,
                         const double *d_weights, double forget,
                         const double *d_tau, int dirs, const int *d_offsets, int sources, int offset_per_dir,
                         int n_taps, int bin_lo, int bin_hi, double loading,
                         double *d_acc, double *d_mass, int *d_used,
                         double *d_snap, double *d_cov, double *d_chol, double *d_gains,
                         float *d_taps, int *d_status, int *d_fallback, void *stream);

/* ---- the output stage: rational sample-rate conversion on the device, beams at a sound card's rate ----
 * Every listening path ends in float32 rows at the array's own rate (48828 Hz, an FPGA clock divider's by-product), which no sound card,
 * codec or file format takes.  This call converts the rows of a window stream by up / down (48828 -> 48000 Hz is 4000 / 4069) with a
 * polyphase FIR, continuous across windows and across calls, to float32 and / or interleaved 16-bit PCM.  Its phase lives on the device,
 * so a captured graph keeps converting correctly when it is replayed.  The configured sizes (bf_configure) and the loaded tables play no
 * part: the window length is the argument n.
 * d_in      : HIP device pointer, float32 [frames][rows][in_stride], in_stride >= n: what bf_miso_device / bf_miso_stream_device /
 *             bf_filter_sum_device write ([frames][beams][N_SAMPLES]).  A flat stream is frames = 1, hop = 0, n = its length.
 * d_prev    : HIP device pointer, float32 [rows][in_stride], or NULL: the last window of the call before.
 * d_taps    : HIP DEVICE pointer, float32 [up][n_taps]: h[p][t], tap t of phase p (audio_out.design_resampler makes one).
 * d_state   : HIP device pointer, int32 [4], read and written: it carries from call to call.  All zeros: the start of a stream.
 * Definition (builder-defined; the reference has no rate conversion).  Let len = hop > 0 ? hop : n, first = n - len, S = frames * len,
 * L = up, M = down, T = n_taps.
 *   Stream.  The call's input stream of row r is
 *       x[s] = d_in[s / len][r][first + s % len]                        for 0 <= s < S
 *       x[s] = d_prev[r][n + s], or 0.0f when d_prev is NULL            for -(T-1) <= s < 0
 *     -- the last `hop` samples of every window, the samples CarriedBeams.audio joins, behind the end of the window before.
 *   State.  d_state[0] = o >= 0 is the input index, relative to this call's x[0], of the next output; d_state[1] = phi, 0 <= phi < L,
 *     its phase.  d_state[2..3] are reserved and written 0.
 *   Outputs.  For k = 0, 1, .. with a_k = phi + k * M (64-bit): i_k = o + a_k / L, p_k = a_k % L.  Output k exists while i_k < S:
 *       count = o < S ? ceil(((S - o) * L - phi) / M) : 0
 *       y[r][k] = acc_T,   acc_0 = 0.0f,   acc_{t+1} = fmaf(h[p_k][t], x[i_k - t], acc_t)   for t = 0 .. T-1
 *     in that order, one float32 rounding per step (a single-rounding fused multiply-add, libm's fmaf).  Subnormals are kept.
 *   Gain.  v = y * gain, one float32 multiply.
 *   Float output.  d_out float32 [rows][out_stride]: d_out[r][k] = v for k < count, 0.0f for count <= k < cap with
 *     cap = bf_resample_capacity(S, L, M) = ceil(S * L / M) >= count; elements past cap are left untouched.
 *   PCM output.  d_pcm int16, interleaved [cap][rows]: d_pcm[k * rows + r] = clamp(rintf(v * 32768.0f), -32768, 32767), ties to even; a NaN
 *     gives 0; slots count <= k < cap get 0.  A sample is CLIPPED if v is NaN or the rounded value left the range (1.0f gives 32767 and
 *     is clipped, -1.0f gives -32768 and is not).  d_clip int32 [rows]: d_clip[r] is INCREASED by the row's clipped samples -- a meter
 *     that accumulates over calls; the caller zeroes it.  (Integer atomic adds: a sum of integers does not depend on the order.)
 *   Either of d_out and d_pcm may be NULL, not both; d_clip may be NULL, and is not touched by a call without d_pcm.
 *   New state.  With A = phi + count * M: o' = o + A / L - S, phi' = A % L (for o >= S: count = 0, o' = o - S, phi' = phi).
 *   d_count int32 [2] = (count, status).  A state with o < 0 or phi outside [0, L) gives status = 1, count = 0 and all-zero outputs
 *     (slots [0, cap)); the state and d_clip are left as they were.  Otherwise status = 0.
 * Two calls on F1 and F - F1 windows, the second with the first's state and last window, give the outputs of one call on F windows bit
 * for bit.  The result does not depend on the internal blocking (a workgroup takes a run of consecutive outputs of one row and stages
 * their contiguous input span in LDS), on the alignment of the pointers, on T % 4 or on out_stride: taps past the last are skipped,
 * not multiplied by zero.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: two launches -- the conversion, which only reads d_state, then one thread
 *             that writes d_state and d_count; no allocation, no workspace, no synchronisation; graph-capturable from the first call,
 *             and a replay advances the state like any other call.  Nothing else is carried on the device: the sample history is the
 *             caller's previous window.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_in, d_taps, d_state or d_count null; d_out and d_pcm both
 * null; rows, frames, n, up, down or n_taps < 1; up > BF_RESAMPLE_MAX_PHASES; n_taps > BF_RESAMPLE_MAX_TAPS; up * n_taps > 1 << 20;
 * down > 64 * up; hop < 0; hop > n; in_stride < n; n_taps - 1 > len (the history must be stream samples); frames * len > INT_MAX / 2;
 * cap > INT_MAX; d_out given with out_stride < cap; gain not finite; a written range (d_out, d_pcm, d_clip, d_state, d_count; each
 * from its first element to the last one touched) sharing a byte with a read range (d_in, d_prev, d_taps) or with another written
 * one; no GPU.  All arguments are checked before device bring-up.
 * bf_resample_capacity: ceil(samples_in * up / down), the slots a call on samples_in stream samples fills; -1 for samples_in < 0, up or
 * down < 1, or a product past 64 bits.  No GPU needed. */
#define BF_RESAMPLE_MAX_PHASES 16384
#define BF_RESAMPLE_MAX_TAPS   128
long long bf_resample_capacity(long long samples_in, int up, int down);
int bf_resample_device(const float *d_in, int rows, int frames, int n, int in_stride, int hop, const float *d_prev,
                       const float *d_taps, int up, int down, int n_taps, int *d_state, float gain,
                       float *d_out, int out_stride, short *d_pcm, int *d_clip, int *d_count, void *stream);

/* ---- spectral frames of beam audio: windowed STFT power through a filterbank, linear or on a log scale, on the device ----
 * What an audio model reads (log-mel frames) and what a user watching a beam wants (its spectrum, its band levels), computed from a
 * continuous float32 stream such as bf_resample_device's d_out, frame after frame across calls: the samples a frame still needs and
 * the position of the next frame live on the device, so a captured graph keeps framing correctly when it is replayed.  The configured
 * sizes (bf_configure) and the loaded tables play no part.
 * d_in      : HIP device pointer, float32 [rows][in_stride], in_stride >= len: the next `len` samples of every row's stream.
 * d_len     : HIP device pointer, int32 [1], or NULL: how many of the `len` samples are there, read on the device -- what
 *             bf_resample_device leaves in its d_count[0], so the two calls chain inside one graph although the count differs from push
 *             to push.
 * d_hist    : HIP device pointer, float32 [rows][n_win - 1], read and written: the samples before x[0].  The caller zeroes it at the
 *             start of a stream.
 * d_state   : HIP device pointer, int32 [4], read and written.  All zeros: the start of a stream (the first frame starts at the first
 *             sample).
 * d_window  : HIP DEVICE pointer, float32 [n_win] (features.hann makes one).
 * d_bank    : HIP DEVICE pointer, float32 [n_bands][n_fft / 2 + 1], or NULL: the power spectrum itself, n_bands == n_fft / 2 + 1.
 * d_support : HIP DEVICE pointer, int32 [n_bands][2] = [lo_b, hi_b), or NULL: whole rows.  (features.design_mel and design_bands make
 *             both.)  A range is clipped to [0, n_fft / 2 + 1]; lo_b >= hi_b is an empty band.
 * Definition (builder-defined; the reference has no spectral frames).  Let H = n_win - 1.
 *   Stream.  L = len when d_len is NULL, else min(max(d_len[0], 0), len).  Row r's samples are
 *       x[s] = d_in[r][s]                    for 0 <= s < L
 *       x[s] = d_hist[r][H + s]              for -H <= s < 0
 *   State.  d_state[0] = s0 >= -H is the start of the next frame relative to x[0]; d_state[1..3] are reserved and written 0.
 *   Frames.  Frame j starts at s_j = s0 + j * hop_s and exists while s_j + n_win <= L:
 *       count = s0 + n_win <= L ? (L - n_win - s0) / hop_s + 1 : 0            (64-bit; count <= cap)
 *   Values, float32 throughout:
 *       u[t] = d_window[t] * x[s_j + t] for t < n_win, one multiply; u[t] = 0 for n_win <= t < n_fft
 *       X_k  = sum_t u[t] exp(-2 pi i k t / n_fft),  k = 0 .. n_fft / 2
 *       P_k  = re(X_k)^2 + im(X_k)^2
 *       E_b  = sum over lo_b <= k < hi_b of d_bank[b][k] * P_k, in ascending k from 0.0f, product and sum each rounded;
 *              weights outside the support are not read; E_k = P_k without a bank
 *       out  = E_b where scale == 0, else scale * log10f(E_b < floor_ ? floor_ : E_b)   (1: the usual log-mel input; 10: dB; a NaN
 *              stays a NaN)
 *     The transform is a radix-2 decimation-in-time FFT with computed twiddles; its rounding is not part of the definition, these
 *     promises are: a frame's values depend only on its own n_win samples, the window, the bank and the scalars -- not on rows, on
 *     the other rows, on the frame's index j, on the alignment of any pointer, or on how the stream was cut into calls.  Two calls on
 *     L1 and L - L1 samples, the second with the first's d_hist and d_state, give the frames of one call on L samples bit for bit, and
 *     the counts add up.  A non-finite sample affects only the frames that contain it.
 *   Outputs.  d_out float32 [rows][out_frames][n_bands]: frames j < count; frames count <= j < cap are written 0.0f, with cap =
 *     bf_spectrogram_capacity(len, hop_s) = ceil(len / hop_s); frames past cap are left untouched.
 *   d_count int32 [2] = (count, status).  A state with s0 < -H gives status = 1, count = 0 and zeros in the frames [0, cap); the state
 *     and the history are left as they were.  Otherwise status = 0.
 *   New state.  s0' = s0 + count * hop_s - L (hop_s > n_win skips samples: s0' may be positive), and d_hist' = the last H samples of
 *     d_hist || x[0 .. L) (L < H shifts the history inside itself).
 * stream    : hipStream_t (0 = null stream).  Enqueue only: two launches -- the transform (a workgroup per frame; one wave up to n_fft =
 *             512, four above), which only reads d_state, d_hist and d_len, then a workgroup per row that writes d_hist, d_state and
 *             d_count (len == 0: that one alone); no allocation, no workspace, no table, no synchronisation, no atomics on floats;
 *             graph-capturable from the first call, and a replay advances the state like any other call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_in, d_hist, d_state, d_window, d_out or d_count null;
 * rows < 1; len < 0; in_stride < len; n_fft not a power of two in [32, 4096]; n_win < 1 or > n_fft; hop_s < 1; n_bands < 1 or >
 * BF_SPECTROGRAM_MAX_BANDS; d_bank null with n_bands != n_fft / 2 + 1; out_frames < cap; scale not finite; scale != 0 with floor_ not
 * finite or <= 0; a written range (d_out, d_hist, d_state, d_count; each from its first element to the last one touched) sharing a
 * byte with a read range (d_in, d_len, d_window, d_bank, d_support) or with another written one; no GPU.  All arguments are checked
 * before device bring-up.
 * bf_spectrogram_capacity: ceil(len / hop_s), the most frames one call on len samples can complete; -1 for len < 0 or hop_s < 1.  No
 * GPU needed. */
#define BF_SPECTROGRAM_MAX_BANDS 4096
long long bf_spectrogram_capacity(long long len, int hop_s);
int bf_spectrogram_device(const float *d_in, int rows, int in_stride, int len, const int *d_len,
                          float *d_hist, int *d_state,
                          const float *d_window, int n_win, int n_fft, int hop_s,
                          const float *d_bank, const int *d_support, int n_bands,
                          float scale, float floor_,
                          float *d_out, int out_frames, int *d_count, void *stream);

/* ---- noise suppression of beam audio: STFT analysis, a gain per (frame, bin), overlap-add synthesis, on the device ----
 * A beam carries the noise that arrives from its look direction and the sensors' own (a 64-microphone delay-and-sum beam has a white-
 * noise gain of about -24.7 dB, the adaptive designs less, and nothing below a few kHz is attenuated spatially on a 14 cm aperture).
 * This call is the single-channel spectral post-filter behind the beamformer: frames of the stream are transformed, every bin is
 * multiplied by a gain in [g_min, 1] -- a decision-directed Wiener rule over a recursively tracked noise spectrum, or gains the caller
 * supplies (a model's mask, say) -- and the frames are transformed back and overlap-added into an audio stream again, continuous
 * across windows and calls with all state on the device.  The configured sizes (bf_configure) and the loaded tables play no part.
 * d_in      : HIP device pointer, float32 [frames][rows][in_stride], in_stride >= n: as bf_resample_device reads it.  A flat stream is
 *             frames = 1, hop = 0, n = its length.
 * d_hist    : HIP device pointer, float32 [rows][n_fft - 1], read and written: the samples before x[0].
 * d_ola     : HIP device pointer, float32 [rows][n_fft], read and written: the partial sums of y for the n_fft positions before x[0].
 * d_noise   : HIP device pointer, float32 [rows][n_fft / 2 + 1], read and written: lam, the tracked noise power of every bin.
 * d_prior   : HIP device pointer, float32 [rows][n_fft / 2 + 1], read and written: G^2 P of the bin's last frame.
 * d_state   : HIP device pointer, int32 [4], read and written.  The caller zeroes d_hist, d_ola, d_noise, d_prior and d_state at the
 *             start of a stream.  d_noise and d_prior may be NULL where d_gain_in is given.
 * d_win_a, d_win_s : HIP DEVICE pointers, float32 [n_fft]: the analysis and the synthesis window (enhance.design_cola makes a pair
 *             whose products overlap-add to 1).
 * d_gain_in : HIP DEVICE pointer, float32 [rows][cap][n_fft / 2 + 1], or NULL: the caller's gains, frame i of the call in slot i.
 * d_work    : HIP device pointer, bf_enhance_workspace(rows, S, n_fft, hop_s) floats, written; its contents carry nothing.
 * Definition (builder-defined; the reference has no post-filter).  Let len = hop > 0 ? hop : n, S = frames * len, H = n_fft - 1,
 * B = n_fft / 2 + 1, cap = (hop_s - 1 + S) / hop_s.
 *   Stream.  x[s] = d_in[s / len][r][n - len + s % len]     for 0 <= s < S        (bf_resample_device's stream)
 *            x[s] = d_hist[r][H + s]                        for -H <= s < 0
 *   State.  d_state[0] = c, 0 <= c < hop_s: the stream samples since the last frame end.  d_state[1] = seen >= 0: the frames the noise
 *     tracker has seen, saturating at n_init.  d_state[2..3] are reserved and written 0.
 *   Frames.  count = (c + S) / hop_s.  Frame i < count ends at e_i = (i + 1) * hop_s - c - 1 and covers x[e_i - H .. e_i]: the first
 *     frames of a stream reach into the zeroed history, so every stream sample is covered by n_fft / hop_s frames; there is no fade-in.
 *   Analysis, float32:  u[t] = d_win_a[t] * x[e_i - H + t], one multiply;  X_k = sum_t u[t] exp(-2 pi i k t / n_fft), k = 0 .. n_fft / 2;
 *     P_k = re * re + im * im, two products and one add, each rounded.
 *   Gains.  With d_gain_in: G = d_gain_in[r][i][k]; d_noise, d_prior and seen are neither read nor written.  Otherwise, per (row, bin)
 *     over the call's frames in ascending order, with s = min(seen + i, n_init) for frame i (one counter for all bins), lam = d_noise,
 *     prior = d_prior, every operation one float32 operation in the order written, divisions IEEE-rounded, fmaf with one rounding,
 *     subnormals kept, max(a, b) = a < b ? b : a and min(a, b) = a > b ? b : a:
 *       if P is not finite:  G = NaN; lam and prior stay as they are (the frame comes out non-finite)
 *       else
 *         if s < n_init:  lam = (s == 0) ? P : lam + (P - lam) / (float)(s + 1)          -- the stream's first frames are taken as noise
 *         else:           g = P / max(lam, FLT_MIN);  p = min(max((g - g0) / (g1 - g0), 0), 1)
 *                         a = a_noise + (1 - a_noise) * p;  lam = fmaf(1 - a, P - lam, lam)
 *         den = max(lam, FLT_MIN);  gam = P / den
 *         xi  = fmaf(alpha, min(prior / den, FLT_MAX), (1 - alpha) * max(gam - 1, 0))    -- the clamp keeps alpha = 0 times an
 *                                                                                           overflowed ratio at 0
 *         G   = max(1 - 1 / (1 + xi), g_min)                                              -- 1, not NaN, at xi = inf
 *         prior = (G * G) * P
 *     1 - alpha, 1 - a_noise and g1 - g0 are float32 differences.  No operation of the else branch yields a NaN from finite P, lam >= 0
 *     and prior >= 0.  New state: seen' = min(seen + count, n_init); d_noise and d_prior hold lam and prior behind the last frame.
 *   Synthesis.  Y_k = G * X_k (one multiply per component; the imaginary parts of Y_0 and Y_{n_fft/2} are taken as 0);
 *     v[t] = (d_win_s[t] * (1.0f / n_fft)) * z[t] with z the unnormalised inverse real transform of Y.  The enhanced stream is
 *       y[t] = the sum over the frames covering t of v_frame[t - start], added in ascending frame order starting from 0.0f,
 *     and d_ola[r][j] carries that partial sum for position j - n_fft over the frames of earlier calls.
 *   Both transforms are radix-2 decimation-in-time FFTs with twiddles rounded once from double; their rounding is not part of the
 *     definition (tests/enhance_np.py derives the tolerance), these promises are: a frame's values depend only on its own n_fft
 *     samples, the windows, its gains and the scalars -- not on rows, on the other rows, on the frame's index in the call, on the
 *     alignment of any pointer, or on how the stream was cut into calls.  Two calls on F1 and F - F1 windows, the second with the
 *     first's state, give d_out and all state of one call on F windows bit for bit.  A row of zeros gives zeros.  A non-finite sample
 *     makes non-finite at most the outputs at the positions its covering frames span; d_noise and d_prior stay finite.
 *   Output.  d_out float32 [rows][out_stride]: d_out[r][s] = y[s - n_fft] for 0 <= s < S: a call on S samples emits exactly S samples,
 *     whatever c is; the stream is delayed by n_fft samples (a position is emitted once every frame that covers it has ended), and the
 *     first n_fft samples of a stream hold the zeros of d_ola plus what the first frames, which reach into the zeroed history, put in
 *     front of the stream: rounding at G = 1, the spread of the gains otherwise.  Elements past S are left untouched.
 *   Observables.  d_power_out and d_gain_out, float32 [rows][cap][B], either may be NULL: P and G of the frames i < count, 0.0f in the
 *     slots count <= i < cap.
 *   New state.  c' = (c + S) % hop_s; d_hist' = the last H samples of d_hist || x[0 .. S); d_ola'[j] = the partial sum of position
 *     S - n_fft + j.
 *   d_count int32 [2] = (count, status).  A state with c outside [0, hop_s) or seen < 0 gives status = 1, count = 0, zeros in
 *     d_out[r][0 .. S) and in the observables; d_hist, d_ola, d_noise, d_prior and d_state are left as they were.  Otherwise status = 0.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: four launches -- analysis (a workgroup per frame; one wave up to n_fft =
 *             512, four above), the gain recursion (a thread per (row, bin), which reads and then writes its own d_noise / d_prior
 *             element), synthesis into d_work, and the overlap-add, which alone writes d_hist, d_ola, d_state and d_count; no
 *             allocation, no synchronisation, no atomics on floats; graph-capturable from the first call, and a replay advances the
 *             stream like any other call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: d_in, d_hist, d_ola, d_state, d_win_a, d_win_s, d_work, d_out
 * or d_count null; d_noise or d_prior null without d_gain_in; rows, frames or n < 1; hop < 0; hop > n; in_stride < n; n_fft not a power
 * of two in [32, 4096]; hop_s < 1, not a divisor of n_fft, or n_fft / hop_s > BF_ENHANCE_MAX_OVERLAP; S > INT_MAX / 2; out_stride < S;
 * without d_gain_in: alpha or a_noise not finite or outside [0, 1), g0 not finite or < 0, g1 not finite or <= g0, g_min not finite or
 * outside [0, 1], n_init < 1; a written range (d_out, d_work, d_power_out, d_gain_out, d_hist, d_ola, d_noise, d_prior, d_state, d_count;
 * each from its first element to the last one touched) sharing a byte with a read range (d_in, d_win_a, d_win_s, d_gain_in) or with
 * another written one; no GPU.  All arguments are checked before device bring-up.
 * bf_enhance_workspace: the floats of d_work for a call on `samples` stream samples per row, 4 + rows * cap * (4 * B + n_fft); -1 for
 * rows < 1, samples < 1 or > INT_MAX / 2, or n_fft / hop_s outside the rules above.  No GPU needed. */
#define BF_ENHANCE_MAX_OVERLAP 8
long long bf_enhance_workspace(int rows, long long samples, int n_fft, int hop_s);
int bf_enhance_device(const float *d_in, int rows, int frames, int n, int in_stride, int hop,
                      float *d_hist, float *d_ola, float *d_noise, float *d_prior, int *d_state,
                      const float *d_win_a, const float *d_win_s, int n_fft, int hop_s,
                      const float *d_gain_in,
                      float alpha, float a_noise, float g0, float g1, float g_min, int n_init,
                      float *d_work, float *d_out, int out_stride,
                      float *d_power_out, float *d_gain_out, int *d_count, void *stream);

/* ---- multichannel post-filter gains: the Wiener gain of a steered beam read from the microphones' coherence, on the device ----
 * bf_enhance_device on its own sees only the beam and has to guess the noise from the beam's history.  The microphones carry what one
 * channel lacks: behind the steering to the look direction the target is coherent across them and sensor or diffuse noise is not.  The
 * multichannel post-filter (Zelinski 1988; Simmer's variant; Simmer, Bitzer & Marro, "Post-filtering techniques", 2001) reads the Wiener
 * gain from that, per frame and bin, with no noise history, no learning stretch and no stationarity assumption.  With n microphones the
 * cross-spectral sum over all n (n - 1) / 2 pairs is  sum_{i<j} Re(Z_i conj Z_j) = (|sum Z_i|^2 - sum |Z_i|^2) / 2 : no pair loop.  This
 * call makes the gains bf_enhance_device takes as d_gain_in, on its frame grid, for the slots a tracker names, without a host round trip.
 * The configured sizes (bf_configure) and the loaded tables play no part.
 * d_signals : HIP device pointer, float32 [frames][m_total][n_samples].
 * adaptive_array, n : as bf_filter_sum_device (HOST array of the n active rows r_m, cached on the device; a new array synchronises the
 *             device once).  2 <= n <= BF_MVDR_MAX_MICS.
 * d_tau, dirs, d_offsets, slots, offset_per_dir : as bf_lcmv_design_device (float64 [dirs][n], microphone m LEADS by tau[d][m]; ONE row
 *             of `slots` int32 entries).  A slot is a source iff its entry is >= 0, a multiple of offset_per_dir and entry /
 *             offset_per_dir < dirs.
 * d_hist    : HIP device pointer, float32 [n][H], H = n_fft - 1 + lag, read and written: the microphones' samples before x[0].
 * d_num, d_den : HIP device pointers, float32 [slots][K], K = n_fft / 2 + 1, read and written: the smoothed numerator N and denominator D.
 * d_state   : HIP device pointer, int32 [2 + slots] = (c, 0, seen_0 .. seen_{slots-1}), read and written.  The caller zeroes d_hist and
 *             d_state at the start of a stream (d_num and d_den are not read before a slot's first finite frame).
 * d_window  : HIP DEVICE pointer, float32 [n_fft]: the analysis window (the Enhancer's win_a).
 * d_work    : HIP device pointer, bf_postfilter_workspace(slots, S, n_fft, hop_s) floats, written; its contents carry nothing.
 * Definition (builder-defined; the reference has no post-filter).  Let len = hop > 0 ? hop : n_samples, S = frames * len,
 * cap = (hop_s - 1 + S) / hop_s.
 *   Stream, per microphone m (bf_enhance_device's convention, a row of the frames as one stream):
 *            x_m[s] = d_signals[s / len][r_m][n_samples - len + s % len]     for 0 <= s < S
 *            x_m[s] = d_hist[m][H + s]                                       for -H <= s < 0
 *   State.  0 <= c < hop_s: the stream samples since the last frame end.  seen_b in {0, 1}: whether slot b has had a finite frame since
 *     it last became a source.  d_state[1] is reserved and written 0.
 *   Frames.  count = (c + S) / hop_s (the Enhancer's formulas).  Frame i < count ends at e_i = (i + 1) * hop_s - c - 1 - lag and covers
 *     x[e_i - (n_fft - 1) .. e_i].  lag >= 0 reads the microphones that many samples late, so that the grid lines up with a beam that is
 *     itself late by lag (a FilterSumListener's (T - 1) / 2); lag = 0 is for delay-and-sum beams.
 *   Analysis, float32:  u[t] = d_window[t] * x_m[e_i - (n_fft - 1) + t], one multiply;  X_{m,k} = sum_t u[t] exp(-2 pi i k t / n_fft);
 *     q_{m,k} = re * re + im * im.
 *   Steering, computed per call (a moving tracker slot costs device memory only).  For a source slot b with direction d:
 *     sincospi(2.0 * k * tau[d][m] / n_fft) in double gives a_{b,m,k} = (cos, -sin), rounded once to float32: the conjugate of the
 *     designers' c[m]; it aligns a microphone that LEADS by tau.  d_steer float32 [slots][n][K][2] holds them (zeros for a slot that is
 *     no source): an output the caller may inspect, and the analysis launch's input.  Z = a X: four multiplies and two adds.
 *   Per (slot, frame, bin), float32:  Y = sum_m Z_m, Q = sum_m q_m; the order of the microphone sums is fixed by (n, n_fft) alone and is
 *     not part of the definition.   |Y|^2 = re * re + im * im;
 *       num = (|Y|^2 - Q) / (n (n - 1))           -- twice the mean over the pairs of Re(Z_i conj Z_j), halved by the pair count's 2
 *       den = Q / n             for den_mode 0    (Zelinski: the microphones' mean power)
 *       den = |Y|^2 / n^2       for den_mode 1    (Simmer: the beam's power)
 *   Recursion, per (slot, bin) over the call's frames in ascending order, every operation one float32 operation in the order written,
 *     the division IEEE-rounded, fmaf with one rounding, max(a, b) = a < b ? b : a and min(a, b) = a > b ? b : a.  A frame is finite for
 *     slot b iff num and den are finite in every one of its K bins.
 *       if the frame is not finite for the slot:  G = NaN in every bin; N, D and seen_b stay as they were
 *       else if seen_b == 0:                      N = num; D = den; seen_b = 1
 *       else:                                     N = fmaf(beta, N - num, num); D = fmaf(beta, D - den, den)
 *       G = D > 0 ? min(max(max(N, 0) / D, g_min), 1) : g_min
 *     A slot that is no source gets G = 0.0f in every frame slot of the call, zeros in the observables, d_status[b] = 1 and seen_b' = 0;
 *     its d_num / d_den are left alone, and when it becomes a source again it starts fresh.  A source slot gets d_status[b] = 0.
 *   Outputs.  d_gains float32 [slots][cap][K], exactly d_gain_in's layout for rows = slots: G of the frames i < count, 0.0f in the slots
 *     count <= i < cap.  d_num_out and d_den_out, the same shape, either may be NULL: the raw num and den.  d_count int32 [2] =
 *     (count, status).  A state with c outside [0, hop_s) or a seen outside {0, 1} gives status = 1, count = 0 and zeros in d_gains and the
 *     observables; d_hist, d_num, d_den and d_state are left as they were.  Otherwise status = 0.
 *   New state.  c' = (c + S) % hop_s; d_hist' = the last H samples of d_hist || x[0 .. S).
 *   The transform is bf_enhance_device's (radix-2, twiddles rounded once from double); its rounding is not part of the definition
 *     (tests/postfilter_np.py derives the tolerance), these promises are: a frame's gains depend only on its own n_fft samples of the n
 *     rows, the window, the steering, the scalars and the carried N and D -- not on m_total, on which rows of d_signals the microphones
 *     occupy, on `slots` (slots behind the last change nothing), on the frame's index, on the alignment of any pointer, or on how the
 *     stream was cut into calls.  Two calls on F1 and F - F1 windows, the second with the first's state, give one call's outputs and
 *     state bit for bit.  All-zero rows give G = g_min and finite state.  A non-finite sample makes NaN only the gains of the frames
 *     that cover it and leaves d_num and d_den finite.
 * stream    : hipStream_t (0 = null stream).  Enqueue only: four launches -- steering, analysis + reduce (a workgroup per frame walks
 *             the microphones: four waves with a microphone each up to n_fft = 512, one microphone per workgroup above), the recursion
 *             (a thread per (slot, bin), which reads and then writes its own d_num / d_den element), and the carry, which alone writes
 *             d_hist, d_state and d_count; no allocation after the first call (the cached adaptive array), no synchronisation unless the
 *             adaptive array changed, no atomics on floats; graph-capturable, and a replay advances the stream like any other call.
 * Returns 0, or -1 (bf_last_error names the value; nothing enqueued) for: a null pointer other than d_num_out and d_den_out; frames or
 * n_samples < 1; hop < 0 or hop > n_samples; n < 2 or n > BF_MVDR_MAX_MICS; a row outside [0, m_total); slots < 1 or slots >
 * BF_POSTFILTER_MAX_SLOTS; dirs or offset_per_dir < 1; n_fft not a power of two in [32, 4096]; hop_s < 1, not a divisor of n_fft, or
 * n_fft / hop_s > BF_ENHANCE_MAX_OVERLAP; lag < 0 or lag > n_fft; den_mode not 0 or 1; beta not finite or outside [0, 1); g_min not finite
 * or outside [0, 1]; S > INT_MAX / 2; a written range (d_gains, d_num_out, d_den_out, d_steer, d_work, d_status, d_count, d_hist, d_num,
 * d_den, d_state; each from its first element to the last one touched) sharing a byte with a read range (d_signals, d_tau, d_offsets,
 * d_window) or with another written one; no GPU.  All arguments are checked before device bring-up.
 * bf_postfilter_workspace: the floats of d_work for a call on `samples` stream samples, 16 + slots * cap * (1 + 2 * K); -1 for slots
 * outside 1 .. BF_POSTFILTER_MAX_SLOTS, samples < 1 or > INT_MAX / 2, or n_fft / hop_s outside the rules above.  No GPU needed. */
#define BF_POSTFILTER_MAX_SLOTS 8          /* = BF_LCMV_MAX_SOURCES */
long long bf_postfilter_workspace(int slots, long long samples, int n_fft, int hop_s);
int bf_postfilter_device(const float *d_signals, int m_total, int frames, int n_samples, int hop,
                         const int *adaptive_array, int n,
                         const double *d_tau, int dirs, const int *d_offsets, int slots, int offset_per_dir,
                         float *d_hist, float *d_num, float *d_den, int *d_state,
                         const float *d_window, int n_fft, int hop_s, int lag,
                         int den_mode, float beta, float g_min,
                         float *d_work, float *d_steer,
                         float *d_gains, float *d_num_out, float *d_den_out, int *d_status, int *d_count, void *stream);

/* ---- ingest: FPGA protocol-v2 datagrams -> the mic-major float32 frame the beamformers read (PC/src/receiver.c:94-151,
 * `receive_and_write_to_buffer`).  `packets` holds N_SAMPLES datagrams back to back, each
 * { u16 frequency; i8 n_arrays; i8 protocol_ver; i32 counter; i32 stream[N_MICROPHONES]; } (receiver.h:51-59).
 * Writes n_arrays*rows*columns mic rows of N_SAMPLES floats; rows/columns are the 8 x 8 tile of config.json:7-8.
 * bf_ingest takes host pointers (copies both ways); bf_ingest_device takes HIP device pointers and only enqueues.
 * The one element the reference reads past the end of the datagram (last array, last row, x = 0) is defined as 0. */
int bf_ingest(const void *packets, int n_arrays, int rows, int columns, float *frame);
int bf_ingest_device(const void *d_packets, int n_arrays, int rows, int columns, float *d_frame, void *stream);

/* ---- batched stream ingest: a stream of datagrams -> a batch of frames in one enqueue (the front door of the device path) ----
 * d_packets  : HIP device pointer, 4-byte aligned: n_datagrams datagrams back to back, each 8 + 4*N_MICROPHONES bytes laid out as
 *              `msg` above (receiver.h:51-59).  Frame f is built from datagrams [f*hop, f*hop + N_SAMPLES); hop < N_SAMPLES gives
 *              overlapping windows, hop > N_SAMPLES skips datagrams.
 * n_arrays / rows / columns : as bf_ingest_device (rows x columns is the 8 x 8 tile of config.json:7-8)
 * m_total    : rows of every output frame, >= n_arrays*rows*columns (what bf_das_device / bf_miso_device take as m_total)
 * d_row_mask : HIP device pointer, m_total bytes, or NULL for no mask.  A non-zero byte zeroes that row of every frame, as get_data
 *              zeroes its dead microphones (api.c:830-859; bf_default_disabled_mics below lists them).
 * protocol_ver : the version byte every header is expected to carry (FPGA_PROTOCOL_VERSION, config.json)
 * d_frames   : HIP device pointer, 4-byte aligned, float32 [frames][m_total][N_SAMPLES], mic-major.  EVERY element is written:
 *              rows s < n_arrays*rows*columns hold the reference's conversion in its serpentine order (receiver.c:122-145), value
 *              (float)v * 2^-24, bit-identical to bf_ingest_device on the frame's slice of the stream; masked rows and rows
 *              [n_arrays*rows*columns, m_total) are zero.  The one element the reference reads past the end of the datagram (all
 *              arrays present, last row, x = 0) is 0 here too: in a stream that address is the next datagram's header, and it is
 *              never read as data.
 * d_status   : HIP device pointer, int32 [frames][4], or NULL.  When given, every entry is written by every call (the caller clears
 *              nothing) and no entry depends on the order workgroups run in.  For frame f, over its N_SAMPLES datagrams:
 *                [0] datagrams whose protocol_ver byte differs from `protocol_ver`   (receive_header_data's check, receiver.c:224-239)
 *                [1] datagrams whose n_arrays byte differs from `n_arrays`           (same; both bytes are compared as unsigned values)
 *                [2] t in [1, N_SAMPLES) with counter[t] - counter[t-1] != 1 in wrapping int32 arithmetic -- counted inside the frame
 *                    only: a jump between the last datagram of one frame and the first of the next is in neither frame's count
 *                [3] the counter of the frame's first datagram
 *              [2] and [3] are an extension: the reference stores `counter` and never interprets it.  A non-zero entry changes
 *              nothing about d_frames; what to do with such a frame is the caller's decision.
 * stream     : hipStream_t (0 = null stream).  Enqueue only: no allocation, no synchronisation, graph-capturable from the first call.
 *              The fast form of the kernel (8-byte datagram reads, 16-byte stores) needs d_packets 8-byte aligned with N_MICROPHONES even
 *              and 64 % columns == 0, and d_frames 16-byte aligned with N_SAMPLES a multiple of 4; other shapes give the same result
 *              through narrower accesses.
 * Returns 0, or -1 (see bf_last_error, which names the failing value; nothing enqueued) for a null d_packets or d_frames, frames < 1,
 * hop < 1, n_arrays / rows / columns < 1, n_arrays*rows*columns > N_MICROPHONES or > m_total, (frames - 1)*hop + N_SAMPLES >
 * n_datagrams, a d_packets or d_frames that is not 4-byte aligned, more workgroups than one launch holds, or no GPU.  The arguments
 * are checked before device bring-up. */
int bf_ingest_stream_device(const void *d_packets, long long n_datagrams, int n_arrays, int rows, int columns,
                            int hop, int frames, int m_total, const unsigned char *d_row_mask, int protocol_ver,
                            float *d_frames, int *d_status, void *stream);
/* get_data's 122 dead rows (api.c:835-851), strictly increasing -- the list the get_data shim here applies: returns the count, fills
 * out[0..count) when out is not NULL. */
int bf_default_disabled_mics(int *out);

/* bf_jet_lut: visual.py:26-49 generate_color_map("jet") -- the colour table the colourise kernel uses, uint8 [256][3]. */
void bf_jet_lut(unsigned char *out768);

/* ---- heat-map post-processing on the device (PC/src/visual.py; display side of the path) ----
 * bf_heatmap_colorize_device: visual.py:143-185 -- d_power float32 [frames][MAX_RES_X*MAX_RES_Y] -> d_small uint8
 *   [frames][MAX_RES_Y][MAX_RES_X][3] (reversed-jet colours, flipped as the reference indexes it) and should_overlay flags.
 *   Reference defaults: threshold 1e-7, amount 0.5, exponent 5.  should_overlay follows NumPy's `np.max(image) > threshold`: a frame that
 *   contains a NaN has a NaN maximum, so it comes out blank with flag 0 (visual.py:156-162) and leaves its neighbours in the batch alone.
 * bf_heatmap_overlay_device: cv2.resize(INTER_LINEAR) to out_w x out_h (:186), res = w_prev*prev + w_new*new (:450, 0.5/0.5;
 *   d_prev uint8 [out_h][out_w][3] is the carried state, updated in place), then onto the camera frames
 *   w_cam*frame + w_heat*res (:452, 0.9/0.9) when d_camera is not NULL.  d_out uint8 [frames][out_h][out_w][3].
 * bf_power_center_device: find_power_center (:295-322) -> d_centers float32 [frames][2] = (center_x, center_y);
 *   d_workspace float32 [frames][MAX_RES_X*MAX_RES_Y].
 * All take HIP device pointers and a stream and only enqueue. */
int bf_heatmap_colorize_device(const float *d_power, int frames, float threshold, float amount, float exponent,
                               unsigned char *d_small, int *d_should_overlay, void *stream);
int bf_heatmap_overlay_device(const unsigned char *d_small, int frames, int out_w, int out_h, unsigned char *d_prev,
                              const unsigned char *d_camera, unsigned char *d_out, float w_prev, float w_new, float w_cam,
                              float w_heat, void *stream);
int bf_power_center_device(const float *d_power, int frames, float *d_centers, float *d_workspace, void *stream);

/* ---- frequency-domain beamformers (device pointers, enqueue only) ----
 * Delay-and-sum by phase steering: PC/application/realtime_scripts/beam_forming_algorithm.py:30-70 with the steering
 * phasors of calc_phase_shift_cartesian.py:37-50.  MVDR has no counterpart in the reference (builder-defined, see
 * DESIGN.md).  n_bins rFFT bins starting at bin_lo; planes are float32, complex values as separate re / im arrays.
 *   bf_fd_steering_device   a[k][m][d] = exp(-j 2 pi freq[k] tau[d][m])   (tau seconds, float64 [D][M]; freq Hz, float64 [K])
 *   bf_fd_dft_device        rfft of every active mic row of every frame -> X as [K][M][F] and as [K][F][M]
 *   bf_fd_das_power_device  P[f][d] = sum_k | sum_m X[k][m][f] a[k][m][d] |^2                                    -> float32 [F][D]
 *   bf_fd_covariance_device R[k] = (1/F) sum_f x x^H                                                              -> [K][M][M]
 *   bf_fd_cholesky_inverse_device  R += loading*tr(R)/M*I = L L^H;  writes inverse(L) transposed [K][col][row];  M <= 256 (two blocks of 128 above 128);
 *                           d_status int32 [K] (zeroed by the caller) receives the first column j (as j+1) whose pivot was not positive
 *   bf_fd_mvdr_power_device P[d] = sum_k 1 / || inverse(L_k) a[k][:, d] ||^2                                     -> float32 [D]
 *                           d_lire_t / d_liim_t are the planes bf_fd_cholesky_inverse_device writes, [K][col][row] of a LOWER-TRIANGULAR inverse: entries with
 *                           col > row are taken to be zero and whole 32 x 32 blocks of them are not multiplied at all
 *   bf_fd_gemm_f32_mode     how the two bin-reducing GEMMs (bf_fd_das_power_device, bf_fd_mvdr_power_device) multiply: 0 = v_mfma_f32_32x32x2_f32,
 *                           1 = exact three-way bfloat16 split of the float32 operands, six part products per product on v_mfma_f32_32x32x16_bf16,
 *                           float32 accumulation (float32 accuracy: tests/test_freqdomain.py holds both modes to the same bounds).  mode < 0 only
 *                           asks; returns the previous setting ($BF_GEMM_F32=native|split sets the initial one)  */
int bf_fd_gemm_f32_mode(int mode);
int bf_fd_steering_device(const double *d_tau, const double *d_freq, int n_dirs, int n_mics, int n_bins, float *d_are, float *d_aim, void *stream);
int bf_fd_dft_device(const float *d_frames, int m_total, int frames, const int *adaptive_array, int n, int bin_lo, int n_bins,
                     float *d_xre_mf, float *d_xim_mf, float *d_xre_fm, float *d_xim_fm, void *stream);
int bf_fd_das_power_device(const float *d_xre_mf, const float *d_xim_mf, const float *d_are, const float *d_aim, int frames, int n_mics,
                           int n_dirs, int n_bins, float *d_power, void *stream);
int bf_fd_covariance_device(const float *d_xre_fm, const float *d_xim_fm, int frames, int n_mics, int n_bins, float *d_rre, float *d_rim, void *stream);
int bf_fd_cholesky_inverse_device(const float *d_rre, const float *d_rim, int n_mics, int n_bins, float loading, float *d_lire_t, float *d_liim_t,
                                  int *d_status, void *stream);
int bf_fd_mvdr_power_device(const float *d_lire_t, const float *d_liim_t, const float *d_are, const float *d_aim, int n_mics, int n_dirs,
                            int n_bins, float *d_power, void *stream);

/* ---- detector post-processing (device pointers, enqueue only).  The reference obtains boxes from
 * ultralytics.YOLO(...).predict (image-detection/src/yolo_smooth_tracking.py:9-23); these are the published YOLOv5 head
 * decode and non-maximum suppression it performs internally.
 *   bf_yolo_decode_device: raw[l] = head output of level l, [batch][3*(5+nc)][h[l]][w[l]] (format bit 0: float16 maps, else float32;
 *       bit 1: the maps are NHWC, [batch][h][w][3*(5+nc)] -- the channels_last memory the detect convolutions write);
 *       anchors float32 [3][3][2] (pixels, HOST pointer); writes xyxy boxes [batch][T][4], scores [batch][T] (obj*cls, or -1
 *       when under conf_thres) and class ids [batch][T], T = 3 * sum(h*w).
 *   bf_nms_device: boxes / scores / cls of the K best candidates per image, already sorted by descending score, counts[b] valid
 *       entries; d_mask workspace uint64 [batch][K][ceil(K/64)]; writes up to max_det rows [x1,y1,x2,y2,score,cls] per image
 *       and the number kept.  K <= 4096. */
int bf_yolo_decode_device(const void *const raw[3], const int h[3], const int w[3], const int strides[3], const float *anchors, int batch, int nc,
                          int format, float conf_thres, float *d_boxes, float *d_scores, int *d_cls, void *stream);
/*   bf_topk_candidates_device: the k (<= 1024) best-scoring boxes of every image in descending score order (ties: lower box index
 *       first) -- d_top_scores [batch][k], d_top_boxes [batch][k][4], d_top_cls [batch][k], d_counts [batch] = entries with a
 *       positive score (decode marks rejected boxes with -1).  The order in full: scores compare as floats, so +0.0 and -0.0 tie
 *       (lower index first); a NaN of either sign and any payload ranks below every number, -inf included, and among NaNs the
 *       lower index comes first.  The first min(k, total) slots are copies of the selected entries bit for bit (a -0.0 or a NaN
 *       payload comes out as it went in); slots past min(k, total) hold score -1, a zero box and class 0.  d_boxes and d_top_boxes
 *       are read and written as 16-byte vectors and must be 16-byte aligned (not checked).
 *       One workgroup per image: radix select, ordered tie admission, bitonic sort in LDS.  This is the candidate list
 *       bf_nms_device walks. */
int bf_topk_candidates_device(const float *d_scores, const float *d_boxes, const int *d_cls, int batch, int total, int k, float *d_top_scores,
                              float *d_top_boxes, int *d_top_cls, int *d_counts, void *stream);
/*   bf_upsample_concat_device: the head's torch.cat((nn.Upsample(2, "nearest")(a), b), 1) in one pass -- a float16 NHWC [batch][h/2][w/2][ca],
 *       b [batch][h][w][cb], out [batch][h][w][ca + cb]; h, w even, ca, cb multiples of 8. */
int bf_upsample_concat_device(const void *d_a, const void *d_b, void *d_out, int batch, int h, int w, int ca, int cb, void *stream);
/*   bf_sppf_pool_device: the SPPF block's pooling inside its concatenation buffer, float16 NHWC [batch][h][w][4*c]: channels [c, 2c),
 *       [2c, 3c), [3c, 4c) become the 5x5 / stride 1 / pad 2 max pool of channels [0, c) applied once, twice and three times
 *       (nn.MaxPool2d(5, 1, 2) cascaded; exact).  c a multiple of 8, h * w <= 2048. */
int bf_sppf_pool_device(void *d_buf, int batch, int h, int w, int c, void *stream);
/*   bf_preprocess_bgr8_device: camera frames uint8 [batch][h][w][3] BGR (as OpenCV delivers them, main.pyx:632) -> the network's input,
 *       float16 NHWC [batch][h][w][cpad], RGB / 255 in channels 0..2, zeros above (cpad = 4: what the stem convolution reads). */
int bf_preprocess_bgr8_device(const void *d_frames, void *d_out, int batch, int h, int w, int cpad, void *stream);
/*   bf_conv2d_nhwc_f16_device: the detector's convolutions (the network behind ultralytics.YOLO, yolo_smooth_tracking.py:9-23) as an
 *       implicit GEMM on the f16 matrix cores: y[b][ho][wo][n] = act(bias[n] + sum x[b][ho*stride-pad+i][wo*stride-pad+j][c] * w[n][i][j][c]),
 *       x float16 NHWC [batch][h][w][c]; w float16 [n][kh][kw][c], every output channel's kh*kw*c values followed by zeros up to a
 *       multiple of 64 = whole 128-byte stages (bf_conv2d_weight_row(kh, kw, c) halfs per row); bias float32 [n] or NULL; y float16 NHWC
 *       [batch][(h+2*pad-kh)/stride+1][(w+2*pad-kw)/stride+1][n]; silu != 0 applies x*sigmoid(x) (f32 accumulation throughout).
 *       c a power of two >= 4 with kw * c a multiple of 8 (pad a 3-channel image with one zero channel; 4 channels need even
 *       stride, pad and width). */
int bf_conv2d_weight_row(int kh, int kw, int c);
/*   bf_conv2d_use_dma_kernel: the convolution entry points have two kernels behind them -- operand tiles staged by LDS-DMA (the default wherever
 *       every operand tensor is smaller than 2 GiB) or through registers.  enable = 1 / 0 selects (2: as 1, and the stem's patch kernel in either precision), < 0 only asks; returns the previous setting
 *       ($BF_CONV_DMA=0 sets the initial one).  Results of the two are bit-identical (same products, same summation order). */
int bf_conv2d_use_dma_kernel(int enable);
/*   bf_conv2d_f32_mode: how the float32 LDS-DMA convolution kernels multiply.  0 = the float32 matrix instruction on the operands as they are
 *       (v_mfma_f32_32x32x2_f32); 1 = every operand value split exactly into three bfloat16 parts and the product accumulated (in float32) from the
 *       six part products that matter (v_mfma_f32_32x32x16_bf16): float32 accuracy -- measured against float64 in tests/test_detector.py -- at
 *       2.67 x the matrix rate.  Differences from the float32 instruction: the summation order, an infinite operand gives NaN (inf - inf in the split)
 *       where the instruction gives an infinity, and operands below 2^-118 lose their low parts to bfloat16's exponent range (float32's own
 *       subnormal neighbourhood).  mode < 0 only asks; returns the previous setting ($BF_CONV_F32=native|split sets the initial one). */
int bf_conv2d_f32_mode(int mode);
int bf_conv2d_nhwc_f16_device(const void *d_x, const void *d_w, const float *d_bias, void *d_y, int batch, int h, int w, int c, int n, int kh, int kw,
                              int stride, int pad, int silu, void *stream);
/*   bf_conv2d_nhwc_f16_into_device: the same, writing into a channel slice of a wider NHWC buffer -- d_y points at the slice's first
 *       channel of pixel 0, ldy = halfs between consecutive pixels of that buffer (the network's torch.cat of convolution outputs
 *       becomes free) -- and optionally adding a residual tensor (d_res, row stride ldr; NULL for none) to the rounded result the
 *       way two float16 tensors are added (the bottlenecks' x + cv2(cv1(x))). */
int bf_conv2d_nhwc_f16_into_device(const void *d_x, const void *d_w, const float *d_bias, void *d_y, int ldy, const void *d_res, int ldr, int batch, int h,
                                   int w, int c, int n, int kh, int kw, int stride, int pad, int silu, void *stream);
/*   float32 forms of the detector's tensor kernels -- the precision ultralytics' predict runs at by default
 *       (yolo_smooth_tracking.py:13-23 passes no half=): the same kernels on float32 NHWC tensors, the convolution's products exact and its sums in f32 in either
 *       float32 mode (bf_conv2d_f32_mode above: three-way bfloat16 operand split on v_mfma_f32_32x32x16_bf16, the default, or v_mfma_f32_32x32x2_f32),
 *       SiLU as x / (1 + expf(-x)).
 *       Weight rows are padded to a multiple of 32 floats (bf_conv2d_weight_row_f32); c a power of two >= 4. */
int bf_conv2d_weight_row_f32(int kh, int kw, int c);
int bf_conv2d_nhwc_f32_device(const void *d_x, const void *d_w, const float *d_bias, void *d_y, int batch, int h, int w, int c, int n, int kh, int kw,
                              int stride, int pad, int silu, void *stream);
int bf_conv2d_nhwc_f32_into_device(const void *d_x, const void *d_w, const float *d_bias, void *d_y, int ldy, const void *d_res, int ldr, int batch, int h,
                                   int w, int c, int n, int kh, int kw, int stride, int pad, int silu, void *stream);
int bf_upsample_concat_f32_device(const void *d_a, const void *d_b, void *d_out, int batch, int h, int w, int ca, int cb, void *stream);
int bf_sppf_pool_f32_device(void *d_buf, int batch, int h, int w, int c, void *stream);
int bf_preprocess_bgr8_f32_device(const void *d_frames, void *d_out, int batch, int h, int w, int cpad, void *stream);
/*   bf_conv1x1_cat_nhwc_{f16,f32}_device: a 1x1 convolution (+ bias, SiLU, slice output, residual as above) whose input is a VIRTUAL
 *       concatenation, so that the network's torch.cat((a, b), 1) and torch.cat((upsample(a), b), 1) in front of a 1x1 layer cost no
 *       pass of their own: channels [0, c1) of pixel (b, y, x) are read from d_x1 (ld1 elements between consecutive pixels: a dense
 *       tensor or a channel slice of a wider NHWC buffer; up1 != 0: d_x1 is [batch][h/2][w/2] and pixel (y/2, x/2) is read =
 *       nn.Upsample(2, "nearest")), channels [c1, c) from d_x2 (pitch ld2; may be NULL when c1 == c).  c1, ld1, ld2 whole 16-byte
 *       chunks, pointers 16-byte aligned.  d_w: [n][c] rows as bf_conv2d_weight_row(_f32)(1, 1, c). */
int bf_conv1x1_cat_nhwc_f16_device(const void *d_x1, int ld1, int c1, int up1, const void *d_x2, int ld2, const void *d_w, const float *d_bias, void *d_y,
                                   int ldy, const void *d_res, int ldr, int batch, int h, int w, int c, int n, int silu, void *stream);
int bf_conv1x1_cat_nhwc_f32_device(const void *d_x1, int ld1, int c1, int up1, const void *d_x2, int ld2, const void *d_w, const float *d_bias, void *d_y,
                                   int ldy, const void *d_res, int ldr, int batch, int h, int w, int c, int n, int silu, void *stream);
/*   bf_plan_conv2d: what a convolution call like the above would launch (no GPU needed).  The layer as the entry points take it: elem_bytes 2 (float16) or
 *       4 (float32); batch, h, w, c, n, kh, kw, stride, pad; ldy; has_res != 0 and ldr for a residual; the sources as bf_conv1x1_cat_nhwc_* names them
 *       (c1, ld1, up1, has_x2 != 0, ld2 -- c1 = ld1 = c, up1 = has_x2 = 0 for the one dense source of bf_conv2d_nhwc_*); misaligned: bit 0 / 1 / 2 / 3 / 4 set
 *       when d_x / d_w / d_x2 / d_y / d_res is NOT 16-byte aligned (0: all are).  use_dma_kernel / f32_mode: the two process switches above as a setter
 *       would store them, < 0 = as they stand now; n_cus: compute units of the device (<= 0: 256).
 *       out[0..15] = elem_bytes, family (0 register-staged, 1 LDS-DMA, 2 patch kernel), tile pixels (bm), tile channels (bn), 16-byte chunks per staged
 *       row (4 or 8; 0 for the patch kernel), virtual concatenation (every 1x1 / stride 1 / unpadded layer), bfloat16 split, fast window taps, 16-byte
 *       store epilogue, grid x, grid y, dynamic LDS bytes (the patch kernel; 0 otherwise), $BF_CONV_ROW / $BF_CONV_TAP / $BF_CONV_PATCH as the
 *       process read them at its first plan (0 / 1 / -1 when unset), n_cus.  Returns 0, or -1 with bf_last_error for a layer the entry points refuse
 *       (out untouched).
 *   bf_last_conv2d_plan: the same array as the most recent convolution launch of this process dispatched on it (-1 before the first). */
int bf_plan_conv2d(int elem_bytes, int batch, int h, int w, int c, int n, int kh, int kw, int stride, int pad, int ldy, int has_res, int ldr, int c1, int ld1,
                   int up1, int has_x2, int ld2, int misaligned, int use_dma_kernel, int f32_mode, int n_cus, long long out[16]);
int bf_last_conv2d_plan(long long out[16]);
/*   bf_letterbox_bgr8_device: what ultralytics' predict does to a frame before the network (yolo_smooth_tracking.py:13-23): d_frame uint8 [h][w][3]
 *       resized with cv2.resize(INTER_LINEAR) semantics (8-bit fixed-point bilinear, half-pixel centres) to new_w x new_h and placed at (top, left) of
 *       d_out uint8 [out_h][out_w][3], whose other pixels get the border value (114 in ultralytics).  new_h == h and new_w == w copies. */
int bf_letterbox_bgr8_device(const unsigned char *d_frame, int h, int w, unsigned char *d_out, int out_h, int out_w, int new_h, int new_w, int top, int left,
                             int value, void *stream);
int bf_nms_device(const float *d_boxes, const float *d_scores, const int *d_cls, const int *d_counts, int batch, int k, float iou_thres, int max_det,
                  unsigned long long *d_mask, float *d_out, int *d_out_count, void *stream);

/* Launch geometry the planner picks for a call like the above (no GPU needed): out[0..9] = nc, lead,
 * row_stride, mic_chunk, n_chunks, waves, dpw, tile_dirs, n_tiles, lds_bytes.  Returns 0 or -1. */
int bf_plan_das(int algo, int n, int frames, int dir_begin, int dir_end, int max_whole, int n_cus, long long out[10]);

/* Copies of the tables as resident on the GPU after load_coefficients_lerp / _convolve_hybrid (the reference
 * keeps them in file-scope globals: lerp_and_sum.c:33-34, hybrid_convolve_and_sum.c:40-41). */
int bf_get_lerp_tables(int *whole, float *h, int n);
/* The whole-sample table as resident after load_coefficients_pad (entries beyond N_SAMPLES clamped to it), n = entries loaded. */
int bf_get_pad_table(int *whole, int n);
int bf_get_hybrid_tables(int *whole, float *taps, int n);

/* ---- steering tables: PC/src/directions.pyx, bit-exact, host C++ (float64 with the float32-typed
 * constants of config.pxd:14-23) ---- */
typedef struct bf_geometry {
    int rows, columns;          /* ROWS, COLUMNS                    config.json:7-8   */
    int arrays;                 /* _ACTIVE_MICS (8x8 tiles)         directions.pyx:16 */
    int skip_n_mics;            /* SKIP_N_MICS                      config.json:20    */
    float sample_rate;          /* SAMPLE_RATE                      config.json:16    */
    float propagation_speed;    /* PROPAGATION_SPEED                config.json:21    */
    float element_distance;     /* ELEMENT_DISTANCE                 config.json:17    */
    float view_angle;           /* VIEW_ANGLE                       config.json:13    */
    float z;                    /* Z                                config.json:11    */
} bf_geometry;
void bf_default_geometry(bf_geometry *g);                                   /* as-shipped config.json values */
/* directions.pyx:35-87; `unused`/`n_unused` = contents of unused_mics.npy (already offset), may be NULL/0.
 * Writes up to rows*columns*arrays sorted indices, returns how many. */
int bf_active_microphones(const bf_geometry *g, const int *unused, int n_unused, int *active_out);
/* directions.pyx:17-32; r_prime_out = float64 [2][n_active]. Returns n_active. */
int bf_calc_r_prime(const bf_geometry *g, const int *unused, int n_unused, double *r_prime_out);
/* directions.pyx:90-124; delays_out = float64 [max_res_x][max_res_y][n_active]. Returns n_active or -1. */
int bf_calculate_delays(const bf_geometry *g, int max_res_x, int max_res_y, const int *unused, int n_unused, double *delays_out);
/* directions.pyx:189-205 / :207-226; taps_out = float64[8] / float32[n_taps]. */
void bf_get_h(double frac, double *taps_out);
void bf_get_h2(double delay, int n_taps, float *taps_out);
/* The Python loops over those two (directions.pyx:240-243, :272-275) as one call: float32 [n][8] / [n][n_taps]. */
void bf_get_h_batch(const double *frac, long long n, float *taps_out);
void bf_get_h2_batch(const double *delay, long long n, int n_taps, float *taps_out);

#ifdef __cplusplus
}
#endif
#endif /* BEAMFORMER_HIP_H */
