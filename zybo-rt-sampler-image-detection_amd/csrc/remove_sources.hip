// remove_sources.hip -- bf_remove_sources_device's kernel and launcher for gfx950 (MI355X, CDNA4, wave64): the adjoint of the pad / lerp
// delay operator, applied to beams and subtracted from the frames.  Not a delay-and-sum map kernel: of the delay-and-sum units it
// shares the wave size and the table types only (das_geometry.h).
#include "das_geometry.h"

#include <algorithm>
#include <type_traits>

namespace bf {

// ---- bf_remove_sources_device: subtract beams, projected back onto the microphones, from the frames -------------------------
// residual[f][r_m][j] = x[f][r_m][j] - sum_b c * a_b[j], a_b = the transpose (adjoint) of the delay operator of miso_pad / miso_lerp
// applied to beam b of frame f (include/beamformer_hip.h has the definition, tests/separate_np.py restates it).  Every operation is
// one float32 operation in the stated order, so the result does not depend on the path taken here:
//   VEC     16-byte loads and stores of the frames (N a multiple of 4, both pointers 16-byte aligned), else one dword per access
//   STAGED  the frame's accepted beams are copied into LDS once per workgroup, else every read goes to L2.  The LDS image of a beam is
//           de-interleaved by four -- sample t sits at (t & 3) * S + (t >> 2) -- so that the lanes of a wave, which own consecutive
//           quads of a row and therefore read samples four apart, hit consecutive banks; S = 8 (mod 32) keeps the staging stores,
//           which write consecutive t, off each other's banks as well.
// Workgroup id = frame * groups + group; the group's rows are dealt to the four waves, one row per wave at a time, lane l owning
// quads l, l + 64, ..  Lane b of a wave holds (p, h) of beam b for the row in hand (beams <= 64 = one wave), read out with
// v_readlane as the beam loop goes along.  Rows not named in the adaptive array (row_slot < 0) are copied, or skipped in place.
struct RemoveArgs {
    int m_total, n_mics, n_samples, beams, beam_stride, rows_per, groups, lds_s, inplace;
    long long entries;
    float c;
};

constexpr int kRemoveThreads = 256;
constexpr int kRemoveStageFloats = 8192;   // 32 KiB of staged beams per workgroup at most: five workgroups share a CU's LDS

inline int remove_lds_s(int n_samples)
{
    const int q = (n_samples + 3) / 4;
    return q + ((8 - q % 32) + 32) % 32;
}

template <int ALGO, bool VEC, bool STAGED>
__global__ void __launch_bounds__(kRemoveThreads) remove_sources_kernel(const float* x, float* res, const int32_t* __restrict__ row_slot,
                                                                        const int32_t* __restrict__ whole, const float* __restrict__ frac,
                                                                        const int32_t* __restrict__ offsets, const float* __restrict__ beams_g,
                                                                        int* __restrict__ status, RemoveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    int* s_off = reinterpret_cast<int*>(lds_raw);          // [kRemoveMaxBeams] accepted offsets, -1 = rejected
    float* lds = lds_raw + kRemoveMaxBeams;                // the staged beams
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = kRemoveThreads / kWave;
    const int frame = (int)(blockIdx.x / (unsigned)a.groups);
    const int group = (int)(blockIdx.x % (unsigned)a.groups);
    const int N = a.n_samples;
    const int Q = (N + 3) >> 2;

    // the frame's offsets and their verdicts (bf_miso_device's rule); the frame's first group reports them
    if ((int)threadIdx.x < a.beams) {
        const long long off = offsets[(size_t)frame * a.beams + threadIdx.x];
        const int verdict = (off < 0 || off + (long long)a.n_mics > a.entries) ? 1 : 0;
        s_off[threadIdx.x] = verdict ? -1 : (int)off;
        if (group == 0 && status != nullptr) status[(size_t)frame * a.beams + threadIdx.x] = verdict;
    }
    __syncthreads();
    const float* __restrict__ frame_beams = beams_g + (size_t)frame * a.beams * a.beam_stride;
    if (STAGED) {
        for (int b = 0; b < a.beams; ++b) {
            if (s_off[b] < 0) continue;                     // a rejected beam's row is never read
            const float* __restrict__ src = frame_beams + (size_t)b * a.beam_stride;
            float* dst = lds + b * 4 * a.lds_s;
            for (int t = threadIdx.x; t < N; t += kRemoveThreads) dst[(t & 3) * a.lds_s + (t >> 2)] = src[t];
        }
        __syncthreads();
    }
    const int my_off = lane < a.beams ? s_off[lane] : -1;
    const unsigned long long accepted = __ballot(my_off >= 0);

    const int row_end = min(a.m_total, (group + 1) * a.rows_per);
    for (int row = group * a.rows_per + wave; row < row_end; row += nwaves) {
        const int slot = __builtin_amdgcn_readfirstlane(row_slot[row]);
        const size_t base = ((size_t)frame * a.m_total + row) * N;
        if (slot < 0 && a.inplace) continue;
        int p_l = 0;
        float h_l = 0.0f;
        if (slot >= 0 && my_off >= 0) {
            p_l = whole[(size_t)my_off + slot];
            if (ALGO == ALGO_LERP) h_l = frac[(size_t)my_off + slot];
        }
        for (int q0 = 0; q0 < Q; q0 += kWave) {
            const int q = q0 + lane;
            const int j0 = q << 2;
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (VEC) {
                if (q < Q) {
                    const float4 v = *reinterpret_cast<const float4*>(x + base + j0);
                    acc[0] = v.x; acc[1] = v.y; acc[2] = v.z; acc[3] = v.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j0 + i < N) acc[i] = x[base + j0 + i];
            }
            if (slot >= 0) {
                for (unsigned long long todo = accepted; todo != 0; todo &= todo - 1) {
                    const int b = __builtin_ctzll(todo);     // wave-uniform, ascending: the definition's order
                    const int p = __builtin_amdgcn_readlane(p_l, b);
                    const float h = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h_l), b));
                    const int t0 = j0 + p;                   // p <= N (the loaders clamp), j0 < 1024 + 4
                    constexpr int W = ALGO == ALGO_LERP ? 5 : 4;
                    float w[W];
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        const int t = t0 + k;
                        float v = 0.0f;
                        if (t < N) v = STAGED ? lds[b * 4 * a.lds_s + (t & 3) * a.lds_s + (t >> 2)] : frame_beams[(size_t)b * a.beam_stride + t];
                        w[k] = v;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float ab;
                        if (ALGO == ALGO_LERP) {
                            const float u = w[i + 1];                       // o[j + p + 1], 0 at and past N
                            const float v = (j0 + i >= 1) ? w[i] : 0.0f;    // o[j + p], 0 at and past N and for j = 0
                            ab = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, h), u), __fmul_rn(h, v));
                        } else {
                            ab = w[i];
                        }
                        acc[i] = __fsub_rn(acc[i], __fmul_rn(a.c, ab));
                    }
                }
            }
            if (VEC) {
                if (q < Q) *reinterpret_cast<float4*>(res + base + j0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j0 + i < N) res[base + j0 + i] = acc[i];
            }
        }
    }
}

hipError_t launch_remove_sources(int algo, const float* d_signals, float* d_residual, int m_total, int frames, int n_samples, int n_mics,
                                 const int32_t* d_row_slot, const DeviceTables& tab, long long entries, const int32_t* d_offsets, int beams,
                                 const float* d_beams, int beam_stride, float c, int* d_status, hipStream_t stream)
{
    if ((algo != ALGO_PAD && algo != ALGO_LERP) || frames < 1 || m_total < 1 || n_mics < 1 || beams < 1 || beams > kRemoveMaxBeams ||
        n_samples < 1 || n_samples > 1024 || beam_stride < n_samples || tab.whole == nullptr || (algo == ALGO_LERP && tab.frac == nullptr))
        return hipErrorInvalidValue;
    RemoveArgs a{};
    a.m_total = m_total; a.n_mics = n_mics; a.n_samples = n_samples; a.beams = beams; a.beam_stride = beam_stride;
    a.entries = entries; a.c = c; a.inplace = d_signals == d_residual;
    a.lds_s = remove_lds_s(n_samples);
    // about 2048 workgroups in all, each with at least one row per wave where the frame has that many
    const int want = std::max(1, (2048 + frames - 1) / frames);
    a.rows_per = std::max(std::min(m_total, kRemoveThreads / kWave), (m_total + want - 1) / want);
    a.groups = (m_total + a.rows_per - 1) / a.rows_per;
    const bool staged = beams * 4 * a.lds_s <= kRemoveStageFloats;
    const size_t lds_bytes = ((size_t)kRemoveMaxBeams + (staged ? (size_t)beams * 4 * a.lds_s : 0)) * sizeof(float);
    const bool vec = (n_samples & 3) == 0 && ((reinterpret_cast<uintptr_t>(d_signals) | reinterpret_cast<uintptr_t>(d_residual)) & 15) == 0;
    auto go = [&](auto kernel) -> hipError_t {
        hipLaunchKernelGGL(kernel, dim3((unsigned)frames * (unsigned)a.groups), dim3(kRemoveThreads), lds_bytes, stream, d_signals, d_residual,
                           d_row_slot, tab.whole, tab.frac, d_offsets, d_beams, d_status, a);
        return hipGetLastError();
    };
    auto by_path = [&](auto al) -> hipError_t {
        constexpr int A = decltype(al)::value;
        if (vec) return staged ? go(remove_sources_kernel<A, true, true>) : go(remove_sources_kernel<A, true, false>);
        return staged ? go(remove_sources_kernel<A, false, true>) : go(remove_sources_kernel<A, false, false>);
    };
    return algo == ALGO_PAD ? by_path(std::integral_constant<int, ALGO_PAD>()) : by_path(std::integral_constant<int, ALGO_LERP>());
}

}  // namespace bf
