// ingest_kernel.hip -- FPGA protocol-v2 datagrams -> float32 mic-major frames (the hot path's input layout): ingest_kernel, one frame
// per launch (bf_ingest / bf_ingest_device), and ingest_stream_kernel further down, a stream of datagrams -> a batch of frames in one
// launch (bf_ingest_stream_device).
//
// Reference: PC/src/receiver.c:94-151 (`receive_and_write_to_buffer`) / `receive_to_buffer`: one datagram per sample
// instant, `msg { u16 frequency; i8 n_arrays; i8 protocol_ver; i32 counter; i32 stream[N_MICROPHONES]; }`
// (PC/src/receiver.h:51-59); for array n, row y, column x the output mic index runs s = 0,1,2,... and reads
//     stream[n*ROWS*COLUMNS + y*COLUMNS + x]               on even rows,
//     stream[n*ROWS*COLUMNS + y*COLUMNS + COLUMNS - x]     on odd rows (serpentine wiring; note the reference's
//                                                          off-by-one: x = 0 reads the first element of the NEXT row),
// converts `(float)((double)v / NORM_FACTOR)` with NORM_FACTOR = 2^24, and writes data[s*N_SAMPLES + step].
// (float)((double)v / 2^24) == (float)v * 2^-24 exactly: int32 -> float rounds to nearest-even once, the scaling is a
// power of two -- so v_cvt_f32_i32 + v_mul_f32 reproduces it bit for bit.
// ingest_kernel is a 64 x 64 transpose through LDS: datagram-major reads and mic-major writes are both coalesced.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bf {

namespace {

__global__ void __launch_bounds__(256) ingest_kernel(const unsigned char* __restrict__ packets, int packet_stride, int header_bytes,
                                                     int n_samples, int n_mics_out, int stream_len, int rows, int columns,
                                                     float scale, float* __restrict__ frame)
{
    __shared__ float tile[64][65];
    const int s0 = blockIdx.x * 64;      // first output mic of the tile
    const int t0 = blockIdx.y * 64;      // first sample of the tile
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int per = rows * columns;
    // read: thread tx -> mic s0+tx (coalesced within a datagram up to the serpentine permutation), 16 datagrams per pass
    {
        const int s = s0 + tx;
        int idx = -1;
        if (s < n_mics_out) {
            const int n = s / per, rem = s - n * per, y = rem / columns, x = rem - y * columns;
            const int row = n * per + y * columns;
            idx = (y & 1) ? row + columns - x : row + x;
            if (idx >= stream_len) idx = -1;     // the reference reads one int past the datagram here; we define it as 0
        }
        for (int r = ty; r < 64; r += 4) {
            const int t = t0 + r;
            float v = 0.0f;
            if (idx >= 0 && t < n_samples) {
                const int32_t raw = *reinterpret_cast<const int32_t*>(packets + (size_t)t * packet_stride + header_bytes + 4 * (size_t)idx);
                v = (float)raw * scale;
            }
            tile[r][tx] = v;
        }
    }
    __syncthreads();
    // write: thread tx -> sample t0+tx of mic s0+r (coalesced along the sample axis)
    for (int r = ty; r < 64; r += 4) {
        const int s = s0 + r, t = t0 + tx;
        if (s < n_mics_out && t < n_samples) frame[(size_t)s * n_samples + t] = tile[tx][r];
    }
}

// ---------------------------------------------------------------- batched stream ingest (bf_ingest_stream_device)
//
// T datagrams back to back -> float32 [F][m_total][N_SAMPLES]; frame f is built from datagrams [f*hop, f*hop + N_SAMPLES), so frames
// overlap when hop < N_SAMPLES.  One launch covers every frame: a workgroup owns one (frame, 64 samples, 64 output rows) tile, and F
// further workgroups (only when a status array is given) write the header report of one frame each.
//
// Tile work.  `src` holds, per output row of the tile, the stream index the reference's serpentine order reads -- or -1 for a row
// that comes out as zero: a row the mask names, a row at or past n_mics_out, and the one index the reference reads past the end of the
// datagram.  In a stream that address is the next datagram's header; it is never loaded.
//   read, pair form (datagram base 8-byte aligned, N_MICROPHONES even, 64 % columns == 0): every tile starts on a row of the array and
//     its rows read stream indices [s0, s0 + 64] only.  Lane k of a half-wave loads the dwords s0 + 2k, s0 + 2k + 1 of one datagram as
//     8 bytes -- the widest access the 8-byte header in front of every datagram leaves aligned -- so a wave-instruction fetches two
//     whole 256-byte runs; index s0 + 64 (x = 0 of an odd last row) is one more dword per datagram.  LDS keeps the raw integers by
//     stream index, raw[sample][index - s0]; the serpentine permutation happens on the LDS read.
//   read, general form (any alignment and tile shape): lane -> output row, one dword at src[row], as ingest_kernel reads; raw[sample][row].
//   write: 8 lanes cover 32 consecutive samples of a row with 16 bytes each (N_SAMPLES a multiple of 4 and a 16-byte aligned output;
//     scalar stores otherwise), 8 rows per wave-instruction.
//   LDS banks (row pitch 65 dwords).  Pair-form stores: the 32 lanes of a group write dwords 2k of one row, a 2-way overlap, which a
//     ds_write_b32 absorbs.  Loads of the write phase: a group of 32 lanes reads raw[4q + i][col(r)] for q = 0..7 and four consecutive
//     rows r of the array; 4q * 65 = 4q (mod 32) and the four columns are consecutive stream indices on even and on odd rows alike,
//     so the 32 banks are all different.
// Workgroup order.  With hop < N_SAMPLES neighbouring frames read the same datagrams.  Workgroups with the same blockIdx % 8 share an
// XCD and its L2, so the work list (frame-major) is cut into eight contiguous runs, one per blockIdx % 8: overlapping frames are
// worked on by the same XCD at about the same time.  Placement is a matter of speed only; every workgroup is independent.
// Header report.  One workgroup per frame counts over that frame's N_SAMPLES headers and writes all four entries, so the caller clears
// nothing and no entry depends on the order workgroups run in.  The header bytes are compared as unsigned values.
constexpr int kStreamTile = 64;
constexpr int kStreamPitch = 65;
enum { STREAM_PAIRS = 1, STREAM_WIDE = 2 };

__global__ void __launch_bounds__(256) ingest_stream_kernel(const unsigned char* __restrict__ packets, int packet_stride, int n_samples, int stream_len,
                                                            int n_mics_out, int rows, int columns, int hop, int m_total, int tiles_s, int tiles_m,
                                                            int n_tiles, int n_items, const unsigned char* __restrict__ row_mask, int protocol_ver,
                                                            int n_arrays, int flags, float scale, float* __restrict__ out, int* __restrict__ status)
{
    __shared__ int32_t raw[kStreamTile][kStreamPitch];
    __shared__ int src[kStreamTile];
    __shared__ int counts[3];
    const int tid = threadIdx.x;
    // blockIdx % 8 names the XCD group, blockIdx / 8 the position inside that group's run of the work list
    const int item = (int)(blockIdx.x & 7u) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    if (item >= n_items) return;

    if (item >= n_tiles) {                 // header report of frame f
        const int f = item - n_tiles;
        if (tid < 3) counts[tid] = 0;
        __syncthreads();
        const unsigned char* base = packets + (size_t)f * hop * packet_stride;
        int bad_ver = 0, bad_arrays = 0, jumps = 0;
        for (int t = tid; t < n_samples; t += 256) {
            const uint32_t* h = reinterpret_cast<const uint32_t*>(base + (size_t)t * packet_stride);
            const uint32_t word = h[0], counter = h[1];                  // { u16 frequency; i8 n_arrays; i8 protocol_ver; } { i32 counter; }
            bad_arrays += ((word >> 16) & 0xffu) != (uint32_t)n_arrays;
            bad_ver += (word >> 24) != (uint32_t)protocol_ver;
            if (t > 0) jumps += counter - reinterpret_cast<const uint32_t*>(base + (size_t)(t - 1) * packet_stride)[1] != 1u;
        }
        if (bad_ver) atomicAdd(&counts[0], bad_ver);
        if (bad_arrays) atomicAdd(&counts[1], bad_arrays);
        if (jumps) atomicAdd(&counts[2], jumps);
        __syncthreads();
        if (tid < 3) status[4 * (size_t)f + tid] = counts[tid];
        if (tid == 3) status[4 * (size_t)f + 3] = reinterpret_cast<const int32_t*>(base)[1];
        return;
    }

    const int per_frame = tiles_s * tiles_m;
    const int f = item / per_frame, rem = item - f * per_frame;
    const int ts = rem / tiles_m, tm = rem - ts * tiles_m;
    const int s0 = tm * kStreamTile, t0 = ts * kStreamTile;
    const bool pairs = flags & STREAM_PAIRS, wide = flags & STREAM_WIDE;
    if (tid < kStreamTile) {
        const int s = s0 + tid;
        int idx = -1;
        if (s < n_mics_out && !(row_mask && row_mask[s])) {
            const int per = rows * columns;
            const int n = s / per, r2 = s - n * per, y = r2 / columns, x = r2 - y * columns;
            const int row = n * per + y * columns;
            idx = (y & 1) ? row + columns - x : row + x;
            if (idx >= stream_len) idx = -1;     // past the datagram: 0, as the oracle and ingest_kernel define it
        }
        src[tid] = idx;
    }
    __syncthreads();
    if (s0 < n_mics_out) {                 // (a tile of padding rows only reads nothing)
        const unsigned char* base = packets + ((size_t)f * hop + t0) * packet_stride + 8;
        if (pairs) {
            const int k = tid & 31, j = s0 + 2 * k;
            int2 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = (tid >> 5) + 8 * i;
                v[i] = make_int2(0, 0);
                if (j < stream_len && t0 + r < n_samples) v[i] = *reinterpret_cast<const int2*>(base + (size_t)r * packet_stride + 4 * (size_t)j);
            }
            int32_t last = 0;
            if (tid < kStreamTile && s0 + kStreamTile < stream_len && t0 + tid < n_samples)
                last = *reinterpret_cast<const int32_t*>(base + (size_t)tid * packet_stride + 4 * (size_t)(s0 + kStreamTile));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = (tid >> 5) + 8 * i;
                raw[r][2 * k] = v[i].x;
                raw[r][2 * k + 1] = v[i].y;
            }
            if (tid < kStreamTile) raw[tid][kStreamTile] = last;
        } else {
            const int idx = src[tid & 63];
            int32_t v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = (tid >> 6) + 4 * i;
                v[i] = 0;
                if (idx >= 0 && t0 + r < n_samples) v[i] = *reinterpret_cast<const int32_t*>(base + (size_t)r * packet_stride + 4 * (size_t)idx);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) raw[(tid >> 6) + 4 * i][tid & 63] = v[i];
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int pm = 0; pm < 2; ++pm) {
        const int sl = wave * 8 + (lane >> 3) + 32 * pm, s = s0 + sl;
        if (s >= m_total) continue;
        const int idx = src[sl];
        const int col = idx < 0 ? -1 : (pairs ? idx - s0 : sl);
        float* row_out = out + ((size_t)f * m_total + s) * n_samples;
#pragma unroll
        for (int pq = 0; pq < 2; ++pq) {
            const int tq = 4 * ((lane & 7) + 8 * pq), t = t0 + tq;
            if (t >= n_samples) continue;
            float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (col >= 0) {
                o.x = (float)raw[tq][col] * scale;
                o.y = (float)raw[tq + 1][col] * scale;
                o.z = (float)raw[tq + 2][col] * scale;
                o.w = (float)raw[tq + 3][col] * scale;
            }
            if (wide) {
                *reinterpret_cast<float4*>(row_out + t) = o;
            } else {
                row_out[t] = o.x;
                if (t + 1 < n_samples) row_out[t + 1] = o.y;
                if (t + 2 < n_samples) row_out[t + 2] = o.z;
                if (t + 3 < n_samples) row_out[t + 3] = o.w;
            }
        }
    }
}

}  // namespace

hipError_t launch_ingest(const void* d_packets, int packet_stride, int header_bytes, int n_samples, int n_mics_out, int stream_len,
                         int rows, int columns, float* d_frame, hipStream_t stream)
{
    const dim3 grid((unsigned)((n_mics_out + 63) / 64), (unsigned)((n_samples + 63) / 64));
    hipLaunchKernelGGL(ingest_kernel, grid, dim3(256), 0, stream, static_cast<const unsigned char*>(d_packets), packet_stride, header_bytes,
                       n_samples, n_mics_out, stream_len, rows, columns, 1.0f / 16777216.0f, d_frame);
    return hipGetLastError();
}

hipError_t launch_ingest_stream(const void* d_packets, int packet_stride, int n_samples, int stream_len, int n_mics_out, int rows, int columns,
                                int hop, int frames, int m_total, const unsigned char* d_row_mask, int protocol_ver, int n_arrays,
                                float* d_frames, int* d_status, hipStream_t stream)
{
    const int tiles_s = (n_samples + kStreamTile - 1) / kStreamTile, tiles_m = (m_total + kStreamTile - 1) / kStreamTile;
    const long long n_tiles = (long long)frames * tiles_s * tiles_m, n_items = n_tiles + (d_status ? frames : 0);
    if (n_items > 0x7fffff00ll) return hipErrorInvalidConfiguration;
    int flags = 0;
    if ((reinterpret_cast<uintptr_t>(d_packets) & 7) == 0 && (stream_len & 1) == 0 && kStreamTile % columns == 0) flags |= STREAM_PAIRS;
    if ((reinterpret_cast<uintptr_t>(d_frames) & 15) == 0 && (n_samples & 3) == 0) flags |= STREAM_WIDE;
    const unsigned grid = (unsigned)((n_items + 7) / 8) * 8u;
    hipLaunchKernelGGL(ingest_stream_kernel, dim3(grid), dim3(256), 0, stream, static_cast<const unsigned char*>(d_packets), packet_stride, n_samples,
                       stream_len, n_mics_out, rows, columns, hop, m_total, tiles_s, tiles_m, (int)n_tiles, (int)n_items, d_row_mask, protocol_ver,
                       n_arrays, flags, 1.0f / 16777216.0f, d_frames, d_status);
    return hipGetLastError();
}

}  // namespace bf
