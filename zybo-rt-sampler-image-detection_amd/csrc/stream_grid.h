// stream_grid.h -- what the stages on a continuous stream (resample.hip, spectrogram.hip, enhance.hip, postfilter.hip) share besides the
// transform (lds_fft.h): the window stream, the STFT frame grid and the history carry, each stated once, device and host side.
//
// The window stream.  A call brings `frames` windows, float32 [frames][rows][stride], of n samples each; every window adds its last
// len = hop ? hop : n samples to the stream of its row, so a call adds S = frames * len samples (<= kMaxStream: stream_len) and
//     x_r[s] = in[((s / len) * rows + r) * stride + (n - len) + s % len]                           0 <= s < S
// (WindowStream, stream_at).  A stage whose frames reach back before the call keeps the last H samples of the stream so far per row,
// hist [H], and reads x[s] = hist[H + s] for -H <= s < 0 (stream_or_history).
//
// The carry.  Behind a call the history is the last H samples of hist || x[0 .. S): new[j] = j + S < H ? hist[j + S] : x[j + S - H].
// With S < H it shifts inside itself, so a workgroup stages the whole row in LDS (carry_stage), the caller places the barrier, and only
// then is any of it written (carry_write).  One thread of one workgroup writes the stage's state and (count, status) = (count, 0), or
// (0, 1) and nothing else where the state is corrupt (report).
//
// The frame grid (enhance.hip; postfilter.hip walks the same one): frames of n_fft samples, a power of two in [kEnhanceMinFft,
// kEnhanceMaxFft], every hop_s samples, hop_s dividing n_fft into 1 .. kEnhanceMaxOverlap frames a sample (frame_grid_ok).  With
// c = d_state[0], 0 <= c < hop_s, the stream samples since the last frame end, a call on S samples completes
//     count = (c + S) / hop_s frames, in cap = ceil(S / hop_s) slots (frame_cap), and leaves c' = (c + S) % hop_s;
// frame i covers x[start .. start + n_fft), start = (i + 1) hop_s - c - lag - n_fft >= -(n_fft - 1 + lag) (frame_start; lag: a stage
// that reads its rows that many samples late), and is staged for lds_fft.h's passes as u = window * x at the bit-reversed index
// (stage_windowed).  Every launch derives (c, count, ok) from d_state (frame_grid) except the last one of a call, the only one that
// writes d_state: it reads them from four ints in front of d_work, (c, count, valid, 0), which an earlier launch left there
// (grid_header_write, grid_header_read).
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

#include "lds_fft.h"

namespace bf {

constexpr int kEnhanceMinFft = 32;
constexpr int kEnhanceMaxFft = 4096;
constexpr int kEnhanceMaxOverlap = 8;           // n_fft / hop_s
constexpr int kGridHeader = 4;                  // ints in front of d_work: (c, count, valid, 0)
constexpr int kMaxStream = 0x7fffffff / 2;      // samples a call may add to the stream

// ---------------------------------------------------------------- host side

struct StreamLen {
    int len;
    long long S;
    bool fits;                                  // S is within the range the kernels' int arithmetic was written for
};

inline StreamLen stream_len(int frames, int hop, int n)
{
    const int len = hop > 0 ? hop : n;
    return {len, (long long)frames * len, (long long)frames * len <= kMaxStream};
}

inline long long frame_cap(long long S, int hop_s) { return (S + hop_s - 1) / hop_s; }

inline bool frame_grid_ok(long long samples, int n_fft, int hop_s)
{
    return samples >= 1 && samples <= kMaxStream && n_fft >= kEnhanceMinFft && n_fft <= kEnhanceMaxFft && fft_log2(n_fft) >= 0 && hop_s >= 1 && hop_s <= n_fft &&
           n_fft % hop_s == 0 && n_fft / hop_s <= kEnhanceMaxOverlap;
}

// ---------------------------------------------------------------- device side

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= FLT_MAX; }

struct WindowStream {
    const float* in;
    int rows, stride, first, len;               // first = n - len: where a window's stream samples begin
};

__device__ __forceinline__ WindowStream window_stream(const float* in, int rows, int n, int stride, int len) { return {in, rows, stride, n - len, len}; }

// x_r[s], s >= 0.  Index: the caller's integer type for stream positions.
template <typename Index>
__device__ __forceinline__ float stream_at(const WindowStream& w, int r, Index s)
{
    const Index f = s / w.len;
    return w.in[((size_t)f * w.rows + r) * w.stride + w.first + (s - f * w.len)];
}

// x_r[s], -H <= s: hist_r is the row's carried history.
template <typename Index>
__device__ __forceinline__ float stream_or_history(const WindowStream& w, int r, const float* hist_r, int H, Index s)
{
    return s < 0 ? hist_r[H + s] : stream_at(w, r, s);
}

// The row's new history into `stage` [H]; sample(s) = x[s], 0 <= s < S.  A barrier, then carry_write.
template <typename Sample>
__device__ __forceinline__ void carry_stage(float* __restrict__ stage, const float* __restrict__ hist_r, int H, int S, int lane, int lanes, Sample sample)
{
    for (int j = lane; j < H; j += lanes) {
        const long long p = (long long)j + S;   // of hist || x[0 .. S), whose last H samples are kept
        stage[j] = p < H ? hist_r[p] : sample(p - H);
    }
}

__device__ __forceinline__ void carry_write(float* __restrict__ hist_r, const float* __restrict__ stage, int H, int lane, int lanes)
{
    for (int j = lane; j < H; j += lanes) hist_r[j] = stage[j];
}

__device__ __forceinline__ void report(int* __restrict__ count_status, bool ok, int count)
{
    count_status[0] = ok ? count : 0;
    count_status[1] = ok ? 0 : 1;
}

struct FrameGrid {
    int c, count;
    bool ok;
};

__device__ __forceinline__ bool frame_phase_ok(int c, int hop_s) { return c >= 0 && c < hop_s; }

// c = d_state[0]; ok: frame_phase_ok, and the stage's own condition on the rest of its state on top.
__device__ __forceinline__ FrameGrid frame_grid(int c, bool ok, int S, int hop_s) { return {c, ok ? (int)(((long long)c + S) / hop_s) : 0, ok}; }

template <typename Index = long long>
__device__ __forceinline__ Index frame_start(int i, int hop_s, int c, int n_fft, int lag = 0) { return ((Index)i + 1) * hop_s - c - lag - n_fft; }

__device__ __forceinline__ void grid_header_write(int* __restrict__ header, const FrameGrid& g)
{
    header[0] = g.c;
    header[1] = g.count;
    header[2] = g.ok ? 1 : 0;
    header[3] = 0;
}

__device__ __forceinline__ FrameGrid grid_header_read(const int* __restrict__ header) { return {header[0], header[1], header[2] != 0}; }

// u[t] = window[t] * sample(t), t < n_fft, into re at the bit-reversed index; im = 0.
template <typename Sample>
__device__ __forceinline__ void stage_windowed(float* re, float* im, const float* __restrict__ window, int n_fft, int log2n, int lane, int lanes, Sample sample)
{
    for (int t = lane; t < n_fft; t += lanes) {
        const int rev = fft_rev(t, log2n);
        re[rev] = window[t] * sample(t);
        im[rev] = 0.0f;
    }
}

}  // namespace bf
