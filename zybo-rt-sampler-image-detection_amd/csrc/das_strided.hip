// das_strided.hip -- the strided delay-and-sum kernels (lane l owns samples l, l+64, ...): maps (das_mimo_kernel), steered beams
// (das_miso_kernel) and the map at listed directions (das_select_kernel), each with a `bool HIST` for the continuous-stream mode.
// das_kernels.hip has the overview.
#include "das_device.h"

namespace bf {

namespace {

// First 64-entry block of a table row, requested one work item ahead (pad / lerp): lane m holds entry m.
struct RowHead {
    int p = 0;
    float h = 0.0f;
    bool valid = false;   // wave-uniform
};

template <int ALGO>
__device__ __forceinline__ RowHead request_row_head(const int32_t* __restrict__ whole, const float* __restrict__ frac, size_t row, int mc, int lane)
{
    RowHead r;
    if constexpr (ALGO == ALGO_PAD || ALGO == ALGO_LERP) {
        r.p = (lane < mc) ? whole[row + lane] : 0;
        if constexpr (ALGO == ALGO_LERP) r.h = (lane < mc) ? frac[row + lane] : 0.0f;
        r.valid = true;
    }
    return r;
}

// Accumulate mics [m0, m0+mc) of the table row starting at flat entry `row_base` (= d*M for direction d)
// into acc[NC] (lane l holds samples l + 64 c).  HIST (the continuous-stream kernels): the columns in front of a staged row hold
// the samples that precede the window instead of zeros, so lerp's i >= 0 guard is not applied (pad has none).
template <int ALGO, int NC, bool HIST = false>
__device__ __forceinline__ void accumulate(float (&acc)[NC], const float* lds, const KArgs& a, const int32_t* __restrict__ whole,
                                           const float* __restrict__ frac, const float* __restrict__ taps, size_t row_base, int m0,
                                           int mc, int lane, const RowHead head = RowHead())
{
    const size_t row = row_base + m0;
    const int rs = a.row_stride;

    // pad / lerp: the table row of a direction is fetched 64 mics at a time with ONE coalesced vector load (lane m
    // holds entry m; the next block is requested before the current one is consumed) and the wave-uniform entry of
    // each mic is then read out of that register with v_readlane.  Scalar loads would need no VALU slot, but
    // every new row misses the scalar cache and s_load shares the LDS wait counter, so their latency sat fully
    // exposed in front of every group of LDS reads (measured: 14 instead of 9 cycles per (direction, mic) per CU).
    if constexpr (ALGO == ALGO_PAD || ALGO == ALGO_LERP) {
        const int32_t* __restrict__ wrow = whole + row;
        const float* __restrict__ hrow = frac + row;
        int vp = head.p;
        float vh = head.h;
        if (!head.valid) {
            vp = (lane < mc) ? wrow[lane] : 0;
            if constexpr (ALGO == ALGO_LERP) vh = (lane < mc) ? hrow[lane] : 0.0f;
        }
        for (int b0 = 0; b0 < mc; b0 += kWave) {
            const int bn = min(kWave, mc - b0);
            int vp_next = 0;
            float vh_next = 0.0f;
            if (b0 + kWave < mc) {   // wave-uniform
                vp_next = (b0 + kWave + lane < mc) ? wrow[b0 + kWave + lane] : 0;
                if constexpr (ALGO == ALGO_LERP) vh_next = (b0 + kWave + lane < mc) ? hrow[b0 + kWave + lane] : 0.0f;
            }
            // (v_readlane is a convergent operation: the compiler will not unroll a runtime-trip loop around it, so the
            //  blocks of 8 / 4 mics are spelled out and a scalar remainder loop follows)
            auto pad_one = [&](int u) {
                // pad_and_sum.c:41-47,54-70   out[p + i] += s[i]
                const int p = __builtin_amdgcn_readlane(vp, u);
                const float* r = lds + (b0 + u) * rs + (a.lead - p) + lane;
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c] += r[c * kWave];
            };
            auto lerp_one = [&](int u) {
                // lerp_and_sum.c:50-56,67-92  out[p + i + 1] += s[i] + h * (s[i+1] - s[i]),  0 <= i < N - p - 1
                const int p = __builtin_amdgcn_readlane(vp, u);
                const float h = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vh), u));
                const float* r = lds + (b0 + u) * rs + (a.lead - p - 1) + lane;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float s0 = r[c * kWave];
                    const float s1 = r[c * kWave + 1];
                    float v = __fmaf_rn(h, s1 - s0, s0);      // gcc contracts s0 + h*(s1-s0) into one fma
                    if constexpr (!HIST) {
                        if (c * kWave <= p) v = (lane + c * kWave > p) ? v : 0.0f;   // i >= 0 only (wave-uniform guard)
                    }
                    acc[c] += v;
                }
            };
            int u = 0;
            if constexpr (ALGO == ALGO_PAD) {
                constexpr int kU = NC <= 4 ? 8 : 4;
                for (; u + kU <= bn; u += kU) {
#pragma unroll
                    for (int i = 0; i < kU; ++i) pad_one(u + i);
                }
                for (; u < bn; ++u) pad_one(u);
            } else {
                constexpr int kU = NC <= 4 ? 4 : 2;
                for (; u + kU <= bn; u += kU) {
#pragma unroll
                    for (int i = 0; i < kU; ++i) lerp_one(u + i);
                }
                for (; u < bn; ++u) lerp_one(u);
            }
            vp = vp_next;
            vh = vh_next;
        }
    } else if constexpr (ALGO == ALGO_HYBRID) {
        // hybrid_convolve_and_sum.c:51-64  out[p + i + 1] += h[t] * padded[i + t], t = 0..T-1 in order
        const int T = a.n_taps;
        const int32_t* __restrict__ wrow = whole + row;
        const float* __restrict__ trow = taps + row * T;
        for (int ms = 0; ms < mc; ++ms) {
            const int p = wrow[ms];
            const float* __restrict__ h = trow + ms * T;
            const float* r = lds + ms * rs + (a.lead - p - 1 - T / 2) + lane;
            if (T == 8) {   // the reference's N_TAPS: taps in scalar registers, tap loop unrolled
                const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float* x = r + c * kWave;
                    float o = acc[c];
                    o = __fmaf_rn(h0, x[0], o); o = __fmaf_rn(h1, x[1], o); o = __fmaf_rn(h2, x[2], o); o = __fmaf_rn(h3, x[3], o);
                    o = __fmaf_rn(h4, x[4], o); o = __fmaf_rn(h5, x[5], o); o = __fmaf_rn(h6, x[6], o); o = __fmaf_rn(h7, x[7], o);
                    acc[c] = (c * kWave <= p && !(lane + c * kWave > p)) ? acc[c] : o;   // samples with i < 0 receive nothing
                }
                continue;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float o = acc[c];
                if (c * kWave <= p) {
                    // this segment contains samples with i < 0: they must not receive anything
                    const bool live = lane + c * kWave > p;
                    for (int t = 0; t < T; ++t) o = live ? __fmaf_rn(h[t], r[c * kWave + t], o) : o;
                } else {
                    for (int t = 0; t < T; ++t) o = __fmaf_rn(h[t], r[c * kWave + t], o);
                }
                acc[c] = o;
            }
        }
    } else if constexpr (ALGO == ALGO_FIR_NAIVE) {
        // convolve_and_sum.c:197-211  out[i] += h[t] * padded[i + t], t in order (fma chain into out)
        const int T = a.n_taps;
        const float* __restrict__ trow = taps + row * T;
        for (int ms = 0; ms < mc; ++ms) {
            const float* __restrict__ h = trow + ms * T;
            const float* r = lds + ms * rs + (a.lead - T / 2) + lane;
            if (T == 8) {
                const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float* x = r + c * kWave;
                    float o = acc[c];
                    o = __fmaf_rn(h0, x[0], o); o = __fmaf_rn(h1, x[1], o); o = __fmaf_rn(h2, x[2], o); o = __fmaf_rn(h3, x[3], o);
                    o = __fmaf_rn(h4, x[4], o); o = __fmaf_rn(h5, x[5], o); o = __fmaf_rn(h6, x[6], o); o = __fmaf_rn(h7, x[7], o);
                    acc[c] = o;
                }
                continue;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float o = acc[c];
                for (int t = 0; t < T; ++t) o = __fmaf_rn(h[t], r[c * kWave + t], o);
                acc[c] = o;
            }
        }
    } else {  // ALGO_FIR_VEC
        // convolve_and_sum.c:158-192 + sum8 :132-153: 8 independent fma lanes over tap blocks, fixed tree, out +=
        const int T = a.n_taps;
        const float* __restrict__ trow = taps + row * T;
        for (int ms = 0; ms < mc; ++ms) {
            const float* __restrict__ h = trow + ms * T;
            const float* r = lds + ms * rs + (a.lead - T / 2) + lane;
            if (T == 8) {   // one AVX block: the eight fma lanes start from 0, i.e. they are plain products
                const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float* x = r + c * kWave;
                    const float q0 = x[0] * h0 + x[4] * h4, q1 = x[1] * h1 + x[5] * h5, q2 = x[2] * h2 + x[6] * h6, q3 = x[3] * h3 + x[7] * h7;
                    acc[c] += (q0 + q2) + (q1 + q3);
                }
                continue;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f, l4 = 0.f, l5 = 0.f, l6 = 0.f, l7 = 0.f;
                for (int t = 0; t < T; t += 8) {
                    const float* x = r + c * kWave + t;
                    l0 = __fmaf_rn(x[0], h[t + 0], l0); l1 = __fmaf_rn(x[1], h[t + 1], l1);
                    l2 = __fmaf_rn(x[2], h[t + 2], l2); l3 = __fmaf_rn(x[3], h[t + 3], l3);
                    l4 = __fmaf_rn(x[4], h[t + 4], l4); l5 = __fmaf_rn(x[5], h[t + 5], l5);
                    l6 = __fmaf_rn(x[6], h[t + 6], l6); l7 = __fmaf_rn(x[7], h[t + 7], l7);
                }
                const float q0 = l0 + l4, q1 = l1 + l5, q2 = l2 + l6, q3 = l3 + l7;
                const float d0 = q0 + q2, d1 = q1 + q3;
                acc[c] += d0 + d1;
            }
        }
    }
}

// ---- continuous-stream mode (bf_das_stream_device / bf_miso_stream_device / bf_das_select_stream_device): HIST = true ------------
// The kernels below with one change: the `hist` columns in front of every staged row, [lead - hist, lead), hold the samples that
// precede the window -- row[hop - hist, hop) of the previous frame (frame f - 1 of the launch; `prev0` for frame 0, zeros when that
// is null) -- instead of zeros, and accumulate<.., HIST = true> drops lerp's i >= 0 guard.  A delayed read lead - p (- 1) + k then
// finds x(k - p) for every k in [0, N): the first p outputs of a window are no longer sums over a growing subset of the
// microphones.  hist = max_whole (pad) or max_whole + 1 (lerp); the host checks hist <= hop <= N and hist <= lead
// (stream_launch_ok), so the slice lies inside the previous frame's row and inside the row's lead.  The slice starts at an arbitrary
// sample (hop - hist), so it is copied with plain dword loads; it is hist / N of the row's bytes.
__device__ __forceinline__ void stage_chunk_stream(float* lds, const KArgs& a, const int32_t* __restrict__ mics, const float* __restrict__ frame,
                                                   const float* __restrict__ prev, int hop, int hist, int m0, int mc, int wave, int nwaves, int lane)
{
    stage_chunk(lds, a, mics, frame, m0, mc, wave, nwaves, lane);
    for (int r = wave; r < mc; r += nwaves) {
        float* dst = lds + r * a.row_stride + (a.lead - hist);
        if (prev != nullptr) {   // (workgroup-uniform)
            const float* src = prev + (size_t)mics[m0 + r] * a.n_samples + (hop - hist);
            for (int i = lane; i < hist; i += kWave) dst[i] = src[i];
        } else {
            for (int i = lane; i < hist; i += kWave) dst[i] = 0.0f;
        }
    }
}

// Maps: a workgroup owns one frame and one tile of the directions [a.dir_begin, a.dir_end).  HIST = false is the window-local map
// (prev0 / hop / hist unused, the reference's tail rule for the mean power), HIST = true the continuous-stream map.
template <int ALGO, int NC, int DPW, bool HIST>
__global__ void __launch_bounds__(1024) das_mimo_kernel(BF_TABLE_PARAMS, KArgs a, const float* __restrict__ prev0, int hop, int hist)
{
    static_assert(!HIST || ALGO == ALGO_PAD || ALGO == ALGO_LERP, "the FIR flavours read ahead of the window's end");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = (int)(blockDim.x >> 6);
    const int tile = (int)(blockIdx.x % (unsigned)a.n_tiles);
    const int frame = (int)(blockIdx.x / (unsigned)a.n_tiles);
    const int tile_begin = a.dir_begin + tile * a.tile_dirs;
    if (tile_begin >= a.dir_end) return;  // padding tile (n_tiles is rounded up to a multiple of 8)
    const int tile_end = min(tile_begin + a.tile_dirs, a.dir_end);

    // zero the whole LDS image once: the lead / tail columns (HIST: the columns in front of the history and behind the samples) and
    // the unused rows stay zero for the kernel's lifetime
    {
        const int total4 = (a.mic_chunk * a.row_stride) >> 2;
        float4* z = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < total4; i += blockDim.x) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    const size_t frame_floats = (size_t)a.m_total * a.n_samples;
    const float* __restrict__ frame_sig = signals + (size_t)frame * frame_floats;
    const float* __restrict__ prev_sig = frame > 0 ? frame_sig - frame_floats : prev0;
    float* __restrict__ img = images + (size_t)frame * a.image_stride;
    const int group = nwaves * DPW;
    float* scratch = lds + a.scratch_off + wave * (a.pbw * a.srow);
    int filled = 0;   // wave-uniform

    // Work items of this wave, in order: for g0 / for chunk / for j.  The table-row head of item i+1 is requested
    // (vector load, its own wait counter) before item i is computed, so its HBM/L2 latency hides behind ~64 mics of work.
    auto item_dir = [&](int g0_, int j_) { return g0_ + j_ * nwaves + wave; };
    RowHead head;
    if (item_dir(tile_begin, 0) < tile_end)
        head = request_row_head<ALGO>(whole, frac, (size_t)item_dir(tile_begin, 0) * a.n_mics, min(a.mic_chunk, a.n_mics), lane);

    for (int g0 = tile_begin; g0 < tile_end; g0 += group) {
        float acc[DPW][NC];
#pragma unroll
        for (int j = 0; j < DPW; ++j)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[j][c] = 0.0f;

        for (int ch = 0; ch < a.n_chunks; ++ch) {
            const int m0 = ch * a.mic_chunk;
            const int mc = min(a.mic_chunk, a.n_mics - m0);
            if (a.n_chunks > 1 || g0 == tile_begin) {
                if (a.n_chunks > 1 && (ch > 0 || g0 != tile_begin)) __syncthreads();  // previous readers done
                if constexpr (HIST) stage_chunk_stream(lds, a, mics, frame_sig, prev_sig, hop, hist, m0, mc, wave, nwaves, lane);   // the history is refilled with every chunk
                else stage_chunk(lds, a, mics, frame_sig, m0, mc, wave, nwaves, lane);
                __syncthreads();
            }
#pragma unroll
            for (int j = 0; j < DPW; ++j) {
                const int d = g0 + j * nwaves + wave;  // wave-uniform
                // successor of (g0, ch, j)
                int ng0 = g0, nch = ch, nj = j + 1;
                if (nj == DPW) { nj = 0; nch = ch + 1; if (nch == a.n_chunks) { nch = 0; ng0 = g0 + group; } }
                const int nd = item_dir(ng0, nj);
                const RowHead cur = head;
                head = RowHead();
                if (nd < tile_end) {
                    const int nm0 = nch * a.mic_chunk;
                    head = request_row_head<ALGO>(whole, frac, (size_t)nd * a.n_mics + nm0, min(a.mic_chunk, a.n_mics - nm0), lane);
                }
                if (d < tile_end) accumulate<ALGO, NC, HIST>(acc[j], lds, a, whole, frac, taps, (size_t)d * a.n_mics, m0, mc, lane, cur);
            }
        }
#pragma unroll
        for (int j = 0; j < DPW; ++j) {
            const int d = g0 + j * nwaves + wave;
            if (d < tile_end) {
                park_squares<NC, !HIST>(acc[j], scratch + filled * a.srow, a, d, lane);
                if (++filled == a.pbw) { flush_powers<!HIST>(scratch, filled, img, a, lane); filled = 0; }
            }
        }
    }
    if (filled > 0) flush_powers<!HIST>(scratch, filled, img, a, lane);
}

// Steered beams, raw out[N] (miso_pad / miso_lerp / miso_convolve_*, pad_and_sum.c:54-70 ...).  Workgroup id = frame * groups +
// group: the workgroup's W = blockDim / 64 waves stage each microphone chunk of ITS frame together (the frame is read from HBM
// once per workgroup, not once per beam) and wave w then accumulates beam group * W + w out of the shared rows, in the
// reference's mic order, so every beam is the one-direction result bit for bit.
//   host path (bf::launch_miso): offsets == nullptr, one frame, one beam, offset a.miso_row, `miso_init` optionally seeds the
//                                 accumulators (the single-signal helpers), out = miso_out[0..N)
//   device path (launch_miso_batch): offsets [frames][beams] are table offsets (FIR_VEC: in floats, d * n * T), checked here
//                                 against `entries` (status 1: outside the table, 2: FIR_VEC offset not a multiple of T);
//                                 a rejected beam reads no table entry and its N samples are NaN.  gain != 0 scales the
//                                 beam as api.c:519-523 does, (out / n) * gain, two float32 roundings.
//   stream path (launch_stream_beams): HIST = true, the device path with the history staged in front of every row; it has
//                                 neither a.miso_row nor `miso_init`, and `offsets` is never null.
template <int ALGO, int NC, bool HIST>
__global__ void __launch_bounds__(1024) das_miso_kernel(BF_TABLE_PARAMS, const float* __restrict__ miso_init, float* __restrict__ miso_out, KArgs a,
                                                        const int32_t* __restrict__ offsets, int beams, int* __restrict__ status,
                                                        long long entries, float gain, int out_stride, const float* __restrict__ prev0, int hop, int hist)
{
    static_assert(!HIST || ALGO == ALGO_PAD || ALGO == ALGO_LERP, "the FIR flavours read ahead of the window's end");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = (int)(blockDim.x >> 6);
    const int groups = (beams + nwaves - 1) / nwaves;
    const int frame = (int)(blockIdx.x / (unsigned)groups);
    const int beam = (int)(blockIdx.x % (unsigned)groups) * nwaves + wave;   // wave-uniform
    const bool live = beam < beams;                                           // the last group may be partial
    const size_t slot = (size_t)frame * beams + beam;

    // This wave's table row (wave-uniform) and its verdict.  judge_offset's rule (below), written out in 64 bits as these kernels
    // always had it: taken from judge_offset (32-bit, or with the width as a template argument) the same rule compiles to other
    // code -- in all 35 instantiations, or in the five of FIR_VEC -- and this text keeps each of them, instruction for instruction,
    // what it was as two kernels (profiles/strided_fold_isa_equal.txt).
    long long row = HIST ? 0 : a.miso_row;
    int verdict = 0;
    if ((HIST || offsets != nullptr) && live) {
        const long long off = __builtin_amdgcn_readfirstlane(offsets[slot]);
        const long long per = ALGO == ALGO_FIR_VEC ? a.n_taps : 1;
        if (off < 0 || off + (long long)a.n_mics * per > entries) verdict = 1;
        else if (ALGO == ALGO_FIR_VEC && off % per != 0) verdict = 2;
        row = off / per;
    }
    const bool run = live && verdict == 0;

    // zero the whole LDS image once, as das_mimo_kernel does
    {
        const int total4 = (a.mic_chunk * a.row_stride) >> 2;
        float4* z = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < total4; i += blockDim.x) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const size_t frame_floats = (size_t)a.m_total * a.n_samples;
    const float* __restrict__ frame_sig = signals + (size_t)frame * frame_floats;
    const float* __restrict__ prev_sig = frame > 0 ? frame_sig - frame_floats : prev0;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        acc[c] = (!HIST && miso_init != nullptr && lane + c * kWave < a.n_samples) ? miso_init[lane + c * kWave] : 0.0f;
    for (int ch = 0; ch < a.n_chunks; ++ch) {
        const int m0 = ch * a.mic_chunk;
        const int mc = min(a.mic_chunk, a.n_mics - m0);
        if (ch > 0) __syncthreads();
        if constexpr (HIST) stage_chunk_stream(lds, a, mics, frame_sig, prev_sig, hop, hist, m0, mc, wave, nwaves, lane);
        else stage_chunk(lds, a, mics, frame_sig, m0, mc, wave, nwaves, lane);
        __syncthreads();
        if (run) accumulate<ALGO, NC, HIST>(acc, lds, a, whole, frac, taps, (size_t)row, m0, mc, lane);
    }
    if (!live) return;
    if (status != nullptr && lane == 0) status[slot] = verdict;
    float* __restrict__ out = miso_out + slot * (size_t)out_stride;
    const float nan = __int_as_float(0x7fc00000);
    const float fn = (float)a.n_mics;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float v = acc[c];
        if (gain != 0.0f) v = (v / fn) * gain;   // true division: a reciprocal multiply differs unless n is a power of two
        if (lane + c * kWave < a.n_samples) out[lane + c * kWave] = run ? v : nan;
    }
}

// ---- map values at listed directions (bf_das_select_device / bf_das_select_stream_device) ---------------------------------
// das_mimo_kernel<.., HIST> with one indirection: a workgroup owns one frame and one tile of the LIST [a.dir_begin, a.dir_end) =
// [0, count), and the table row of list index b is offsets[b] -- read wave-uniformly and judged as das_miso_kernel judges a beam's
// offset (judge_offset: 1 outside the table, 2 a FIR_VEC offset that is no multiple of T).  A rejected entry reads nothing
// from the table and its power is a quiet NaN.  park_squares carries the list index where the map kernels carry the
// direction, so flush_powers writes out[frame][b]; a value is one wave's sum in microphone order and one lane's in sample order,
// whatever the tiling, DPW and the wave count are.
// Prefetch: the entries of a wave's NEXT group are requested when the current group starts (a group later they cost no wait), and
// the table-row head of item i + 1 before item i is computed, as in das_mimo_kernel.
struct ListedRow {
    long long row = 0;   // table row start, in entries (FIR_VEC: in rows of T floats)
    int verdict = 0;     // 1: outside the table, 2: FIR_VEC offset not a multiple of T
};

template <int ALGO>
__device__ __forceinline__ ListedRow judge_offset(int raw, const KArgs& a, long long entries)
{
    ListedRow r;
    const int off = __builtin_amdgcn_readfirstlane(raw);
    const int per = ALGO == ALGO_FIR_VEC ? a.n_taps : 1;
    if (off < 0 || (long long)off + (long long)a.n_mics * per > entries) r.verdict = 1;
    else if (ALGO == ALGO_FIR_VEC && off % per != 0) r.verdict = 2;
    r.row = off / per;
    return r;
}

template <int ALGO, int NC, int DPW, bool HIST>
__global__ void __launch_bounds__(1024) das_select_kernel(BF_TABLE_PARAMS, KArgs a, const int32_t* __restrict__ offsets, int per_frame,
                                                          int* __restrict__ status, long long entries, const float* __restrict__ prev0, int hop, int hist)
{
    static_assert(!HIST || ALGO == ALGO_PAD || ALGO == ALGO_LERP, "the FIR flavours read ahead of the window's end");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = (int)(blockDim.x >> 6);
    const int tile = (int)(blockIdx.x % (unsigned)a.n_tiles);
    const int frame = (int)(blockIdx.x / (unsigned)a.n_tiles);
    const int count = a.dir_end;
    const int tile_begin = tile * a.tile_dirs;
    if (tile_begin >= count) return;
    const int tile_end = min(tile_begin + a.tile_dirs, count);

    {
        const int total4 = (a.mic_chunk * a.row_stride) >> 2;
        float4* z = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < total4; i += blockDim.x) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    const size_t frame_floats = (size_t)a.m_total * a.n_samples;
    const float* __restrict__ frame_sig = signals + (size_t)frame * frame_floats;
    const float* __restrict__ prev_sig = frame > 0 ? frame_sig - frame_floats : prev0;
    const int32_t* __restrict__ list = offsets + (per_frame ? (size_t)frame * count : 0);
    float* __restrict__ out = images + (size_t)frame * a.image_stride;
    int* __restrict__ verdicts = status != nullptr ? status + (size_t)frame * count : nullptr;
    const int group = nwaves * DPW;
    float* scratch = lds + a.scratch_off + wave * (a.pbw * a.srow);
    int filled = 0;   // wave-uniform

    auto item_index = [&](int g0_, int j_) { return g0_ + j_ * nwaves + wave; };
    auto request_entries = [&](int g0_, int (&raw)[DPW]) {   // every lane loads the same word: the value comes back through readfirstlane
#pragma unroll
        for (int j = 0; j < DPW; ++j) raw[j] = item_index(g0_, j) < tile_end ? list[item_index(g0_, j)] : -1;
    };
    auto head_of = [&](const ListedRow& r, int m0) {
        return r.verdict == 0 ? request_row_head<ALGO>(whole, frac, (size_t)r.row + m0, min(a.mic_chunk, a.n_mics - m0), lane) : RowHead();
    };

    int raw[DPW];
    request_entries(tile_begin, raw);
    ListedRow rows[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) rows[j] = judge_offset<ALGO>(raw[j], a, entries);
    RowHead head;
    if (item_index(tile_begin, 0) < tile_end) head = head_of(rows[0], 0);

    for (int g0 = tile_begin; g0 < tile_end; g0 += group) {
        request_entries(g0 + group, raw);
        float acc[DPW][NC];
#pragma unroll
        for (int j = 0; j < DPW; ++j)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[j][c] = 0.0f;

        for (int ch = 0; ch < a.n_chunks; ++ch) {
            const int m0 = ch * a.mic_chunk;
            const int mc = min(a.mic_chunk, a.n_mics - m0);
            if (a.n_chunks > 1 || g0 == tile_begin) {
                if (a.n_chunks > 1 && (ch > 0 || g0 != tile_begin)) __syncthreads();  // previous readers done
                if constexpr (HIST) stage_chunk_stream(lds, a, mics, frame_sig, prev_sig, hop, hist, m0, mc, wave, nwaves, lane);
                else stage_chunk(lds, a, mics, frame_sig, m0, mc, wave, nwaves, lane);
                __syncthreads();
            }
#pragma unroll
            for (int j = 0; j < DPW; ++j) {
                const int b = item_index(g0, j);  // wave-uniform
                // successor of (g0, ch, j): the next entry of this group, its first entry at the next chunk, or the next group's first
                const bool last = j + 1 == DPW && ch + 1 == a.n_chunks;
                const int nj = j + 1 == DPW ? 0 : j + 1;
                const int nm0 = j + 1 == DPW ? (last ? 0 : m0 + a.mic_chunk) : m0;
                const RowHead cur = head;
                head = RowHead();
                if (item_index(last ? g0 + group : g0, nj) < tile_end) head = head_of(last ? judge_offset<ALGO>(raw[0], a, entries) : rows[nj], nm0);
                if (b < tile_end && rows[j].verdict == 0)
                    accumulate<ALGO, NC, HIST>(acc[j], lds, a, whole, frac, taps, (size_t)rows[j].row, m0, mc, lane, cur);
            }
        }
#pragma unroll
        for (int j = 0; j < DPW; ++j) {
            const int b = item_index(g0, j);
            if (b >= tile_end) continue;
            if (verdicts != nullptr && lane == 0) verdicts[b] = rows[j].verdict;
            if (rows[j].verdict != 0) {
                if (lane == 0) out[b] = __int_as_float(0x7fc00000);
                continue;
            }
            park_squares<NC, !HIST>(acc[j], scratch + filled * a.srow, a, b, lane);
            if (++filled == a.pbw) { flush_powers<!HIST>(scratch, filled, out, a, lane); filled = 0; }
        }
#pragma unroll
        for (int j = 0; j < DPW; ++j) rows[j] = judge_offset<ALGO>(raw[j], a, entries);
    }
    if (filled > 0) flush_powers<!HIST>(scratch, filled, out, a, lane);
}

// plan.nc as a template argument: f(std::integral_constant<int, NC>()).
template <typename F>
hipError_t dispatch_nc(int nc, F f)
{
    switch (nc) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        default: return hipErrorInvalidValue;
    }
}

// The history the table needs (*hist) and whether a continuous-stream launch can supply it: pad or lerp, hist <= hop <= N, and rows
// whose lead holds it.
bool stream_launch_ok(const DasLaunch& L, const DasPlan& plan, int hop, int* hist)
{
    *hist = stream_history(L.algo, L.tab.max_whole);
    return *hist >= 0 && hop >= *hist && hop <= L.n_samples && plan.lead >= *hist;
}

// das_mimo_kernel<ALGO, nc, dpw, HIST> of a plan_das (strided layout) or plan_stream_maps plan; d_prev / hop / hist are for HIST.
template <int ALGO, bool HIST>
hipError_t launch_mimo_algo(const DasLaunch& L, const DasPlan& plan, int frames, const float* d_prev, int hop, int hist, hipStream_t stream)
{
    const KArgs a = make_args(L, plan);
    auto go = [&](auto kernel) -> hipError_t {
        return launch_with_lds(kernel, dim3((unsigned)plan.n_tiles * (unsigned)frames), dim3((unsigned)plan.waves * kWave), plan.lds_bytes, stream, nullptr,
                               L.signals, L.images, L.mics, L.tab.whole, L.tab.frac, L.tab.taps, a, d_prev, hop, hist);
    };
    return dispatch_nc(plan.nc, [&](auto nc) -> hipError_t {
        constexpr int NC = decltype(nc)::value;
        if constexpr (!HIST && !is_fir(ALGO) && NC >= 4) {
            return hipErrorInvalidValue;                    // pad / lerp beyond 128 samples: shifted copies only (plan_das gives them no other layout)
        } else {
            if (plan.dpw == 1) return go(das_mimo_kernel<ALGO, NC, 1, HIST>);
            if (plan.dpw == 4) return go(das_mimo_kernel<ALGO, NC, 4, HIST>);
            return hipErrorInvalidValue;
        }
    });
}

// The beams of one das_miso_kernel launch (MisoBatch{} = the host path: one frame, one beam at KArgs::miso_row, one wave).
// prev / hop / hist are the stream path's.
struct MisoBatch {
    const int32_t* offsets = nullptr;
    int frames = 1, beams = 1, waves = 1;
    int* status = nullptr;
    long long entries = 0;
    float gain = 0.0f;
    int out_stride = 0;
    const float* prev = nullptr;
    int hop = 0, hist = 0;
};

template <int ALGO, bool HIST = false>
hipError_t launch_miso_algo(const DasLaunch& L, const KArgs& a, const DasPlan& plan, const float* init_dev, float* out_dev, const MisoBatch& B,
                            hipStream_t stream)
{
    const unsigned groups = (unsigned)((B.beams + B.waves - 1) / B.waves);
    const int out_stride = B.out_stride > 0 ? B.out_stride : L.n_samples;
    return dispatch_nc(plan.nc, [&](auto nc) -> hipError_t {
        return launch_with_lds(das_miso_kernel<ALGO, decltype(nc)::value, HIST>, dim3((unsigned)B.frames * groups), dim3((unsigned)B.waves * kWave), plan.lds_bytes,
                               stream, nullptr, L.signals, L.images, L.mics, L.tab.whole, L.tab.frac, L.tab.taps, init_dev, out_dev, a, B.offsets, B.beams,
                               B.status, B.entries, B.gain, out_stride, B.prev, B.hop, B.hist);
    });
}

hipError_t launch_miso_any(const DasLaunch& L, const DasPlan& plan, long long row_offset, const float* init_dev, float* out_dev, const MisoBatch& B,
                           hipStream_t stream)
{
    KArgs a = make_args(L, plan);
    a.miso_row = row_offset;
    switch (L.algo) {
        case ALGO_PAD: return launch_miso_algo<ALGO_PAD>(L, a, plan, init_dev, out_dev, B, stream);
        case ALGO_LERP: return launch_miso_algo<ALGO_LERP>(L, a, plan, init_dev, out_dev, B, stream);
        case ALGO_HYBRID: return launch_miso_algo<ALGO_HYBRID>(L, a, plan, init_dev, out_dev, B, stream);
        case ALGO_FIR_NAIVE: return launch_miso_algo<ALGO_FIR_NAIVE>(L, a, plan, init_dev, out_dev, B, stream);
        case ALGO_FIR_VEC: return launch_miso_algo<ALGO_FIR_VEC>(L, a, plan, init_dev, out_dev, B, stream);
        default: return hipErrorInvalidValue;
    }
}

// The device path's batch (launch_miso_batch, launch_stream_beams); false: a batch neither launches.
bool make_batch(const DasLaunch& L, const int32_t* d_offsets, int beams, long long entries, float gain, int out_stride, int* d_status, MisoBatch* B)
{
    B->offsets = d_offsets; B->frames = L.frames; B->beams = beams; B->waves = std::min(beams, kMisoWaves);
    B->status = d_status; B->entries = entries; B->gain = gain; B->out_stride = out_stride;
    return L.frames >= 1 && beams >= 1 && out_stride >= L.n_samples;
}

// das_select_kernel<ALGO, nc, dpw, HIST> of a plan_select plan; `hist` is 0 for the window-local call.
template <int ALGO, bool HIST>
hipError_t launch_select_algo(const DasLaunch& L, const DasPlan& plan, const float* d_prev, int hop, int hist, const int32_t* d_offsets, int per_frame,
                              long long entries, int* d_status, hipStream_t stream)
{
    const KArgs a = make_args(L, plan);
    auto go = [&](auto kernel) -> hipError_t {
        return launch_with_lds(kernel, dim3((unsigned)plan.n_tiles * (unsigned)L.frames), dim3((unsigned)plan.waves * kWave), plan.lds_bytes, stream, nullptr,
                               L.signals, L.images, L.mics, L.tab.whole, L.tab.frac, L.tab.taps, a, d_offsets, per_frame, d_status, entries, d_prev, hop, hist);
    };
    return dispatch_nc(plan.nc, [&](auto nc) -> hipError_t {
        constexpr int NC = decltype(nc)::value;
        if (plan.dpw == 1) return go(das_select_kernel<ALGO, NC, 1, HIST>);
        if constexpr (ALGO == ALGO_HYBRID && NC == 16) {   // four directions' accumulators of 16 segments beside the taps would spill: plan_select gives two
            if (plan.dpw == 2) return go(das_select_kernel<ALGO, NC, 2, HIST>);
        } else {
            if (plan.dpw == 4) return go(das_select_kernel<ALGO, NC, 4, HIST>);
        }
        return hipErrorInvalidValue;
    });
}

bool select_launch_ok(const DasLaunch& L, const DasPlan& plan, const int32_t* d_offsets)
{
    return L.frames >= 1 && L.dir_begin == 0 && L.dir_end >= 1 && L.image_origin == 0 && L.image_stride >= L.dir_end && d_offsets != nullptr &&
           L.images != nullptr && plan.family == DAS_STRIDED;
}

}  // namespace

hipError_t launch_strided(const DasLaunch& L, const DasPlan& plan, int frames, hipStream_t stream)
{
    switch (L.algo) {
        case ALGO_PAD: return launch_mimo_algo<ALGO_PAD, false>(L, plan, frames, nullptr, 0, 0, stream);
        case ALGO_LERP: return launch_mimo_algo<ALGO_LERP, false>(L, plan, frames, nullptr, 0, 0, stream);
        case ALGO_HYBRID: return launch_mimo_algo<ALGO_HYBRID, false>(L, plan, frames, nullptr, 0, 0, stream);
        case ALGO_FIR_NAIVE: return launch_mimo_algo<ALGO_FIR_NAIVE, false>(L, plan, frames, nullptr, 0, 0, stream);
        case ALGO_FIR_VEC: return launch_mimo_algo<ALGO_FIR_VEC, false>(L, plan, frames, nullptr, 0, 0, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_stream_maps(const DasLaunch& L, const DasPlan& plan, const float* d_prev, int hop, hipStream_t stream)
{
    int hist;
    if (!stream_launch_ok(L, plan, hop, &hist) || plan.family != DAS_STRIDED) return hipErrorInvalidValue;
    if (L.algo == ALGO_PAD) return launch_mimo_algo<ALGO_PAD, true>(L, plan, L.frames, d_prev, hop, hist, stream);
    return launch_mimo_algo<ALGO_LERP, true>(L, plan, L.frames, d_prev, hop, hist, stream);
}

hipError_t launch_miso(const DasLaunch& L, const DasPlan& plan, long long row_offset, const float* init_dev, float* out_dev,
                       hipStream_t stream)
{
    return launch_miso_any(L, plan, row_offset, init_dev, out_dev, MisoBatch{}, stream);
}

hipError_t launch_miso_batch(const DasLaunch& L, const DasPlan& plan, const int32_t* d_offsets, int beams, long long entries, float gain,
                             float* d_out, int out_stride, int* d_status, hipStream_t stream)
{
    MisoBatch B;
    if (!make_batch(L, d_offsets, beams, entries, gain, out_stride, d_status, &B)) return hipErrorInvalidValue;
    return launch_miso_any(L, plan, 0, nullptr, d_out, B, stream);
}

hipError_t launch_stream_beams(const DasLaunch& L, const DasPlan& plan, const float* d_prev, int hop, const int32_t* d_offsets, int beams,
                               long long entries, float gain, float* d_out, int out_stride, int* d_status, hipStream_t stream)
{
    MisoBatch B;
    if (!stream_launch_ok(L, plan, hop, &B.hist) || !make_batch(L, d_offsets, beams, entries, gain, out_stride, d_status, &B) || d_offsets == nullptr)
        return hipErrorInvalidValue;
    B.prev = d_prev; B.hop = hop;
    const KArgs a = make_args(L, plan);
    if (L.algo == ALGO_PAD) return launch_miso_algo<ALGO_PAD, true>(L, a, plan, nullptr, d_out, B, stream);
    return launch_miso_algo<ALGO_LERP, true>(L, a, plan, nullptr, d_out, B, stream);
}

hipError_t launch_select(const DasLaunch& L, const DasPlan& plan, const int32_t* d_offsets, int per_frame, long long entries, int* d_status, hipStream_t stream)
{
    if (!select_launch_ok(L, plan, d_offsets)) return hipErrorInvalidValue;
    switch (L.algo) {
        case ALGO_PAD: return launch_select_algo<ALGO_PAD, false>(L, plan, nullptr, 0, 0, d_offsets, per_frame, entries, d_status, stream);
        case ALGO_LERP: return launch_select_algo<ALGO_LERP, false>(L, plan, nullptr, 0, 0, d_offsets, per_frame, entries, d_status, stream);
        case ALGO_HYBRID: return launch_select_algo<ALGO_HYBRID, false>(L, plan, nullptr, 0, 0, d_offsets, per_frame, entries, d_status, stream);
        case ALGO_FIR_VEC: return launch_select_algo<ALGO_FIR_VEC, false>(L, plan, nullptr, 0, 0, d_offsets, per_frame, entries, d_status, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_select_stream(const DasLaunch& L, const DasPlan& plan, const float* d_prev, int hop, const int32_t* d_offsets, int per_frame, long long entries,
                                int* d_status, hipStream_t stream)
{
    int hist;
    if (!stream_launch_ok(L, plan, hop, &hist) || !select_launch_ok(L, plan, d_offsets)) return hipErrorInvalidValue;
    if (L.algo == ALGO_PAD) return launch_select_algo<ALGO_PAD, true>(L, plan, d_prev, hop, hist, d_offsets, per_frame, entries, d_status, stream);
    return launch_select_algo<ALGO_LERP, true>(L, plan, d_prev, hop, hist, d_offsets, per_frame, entries, d_status, stream);
}

}  // namespace bf
