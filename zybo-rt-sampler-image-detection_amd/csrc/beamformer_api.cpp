// beamformer_api.cpp -- the C-ABI of include/beamformer_hip.h: process-global state, table upload, launch glue.
//
// Mirrors the reference's process model: one table set per process, loaded once before the frame loop
// (PC/src/main.pyx:172-181), single-threaded callers.  Everything numerical runs in das_kernels.hip, das_strided.hip and das_pair.hip; this
// file only validates, copies and enqueues.  There is no CPU compute path: when no GPU is usable every entry
// point reports an error and poisons its output with NaN.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/beamformer_hip.h"
#include "das_geometry.h"      // (das_kernels.h, and what follows from a plan's family)
#include "stream_grid.h"
#include "sweep_order.h"

namespace {

using bf::Algo;

struct Sizes {
    int n_microphones = 256, n_samples = 256, res_x = 57, res_y = 32, n_taps = 8;  // PC/src/config.json:3-11
    int dirs() const { return res_x * res_y; }
};

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        // slack: the scalar-table kernels fetch 16 entries (or 4 mics x 8 taps) at a time and may run past the last row
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T) + 256);
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Everything a digest (bf::launch_digest) depends on; compared field by field.  The family says what the geometry fields do not: the
// row layout the offsets address, and whether the digest is grouped in the table's own sweep order (bf::family_traits).
struct DigestKey {
    bool valid = false;
    int family = 0, mic_chunk = 0, row_stride = 0, lead = 0, algo = 0, dpw = 0, dir_begin = 0, dir_end = 0, n_mics = 0;
    bool operator==(const DigestKey& o) const
    {
        return valid && o.valid && family == o.family && mic_chunk == o.mic_chunk && row_stride == o.row_stride && lead == o.lead && algo == o.algo &&
               dpw == o.dpw && dir_begin == o.dir_begin && dir_end == o.dir_end && n_mics == o.n_mics;
    }
};

// Page-locked host staging buffer (the host-pointer entry points copy through it: DMA straight from / to pinned memory
// instead of the runtime's own staging of pageable memory).
struct PinnedBuf {
    float* p = nullptr;
    size_t cap = 0;   // floats
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(float), hipHostMallocDefault);
        if (e == hipSuccess) cap = n;
        return e;
    }
};

// One loaded coefficient set (what a load_coefficients_* call leaves behind).
struct TableSet {
    bool loaded = false;
    int entries = 0;      // n of the load call = D * M
    int max_whole = 0;
    int clamped = 0;      // entries beyond N_SAMPLES that the loader clamped to it (the continuous-stream calls refuse such a table)
    DevBuf<int32_t> whole;
    DevBuf<float> frac;
    DevBuf<float> taps;
    // Digests of this table (shifted-copies layouts: LDS offsets per (direction, mic), see bf::launch_digest), one per launch
    // geometry that has been used -- one-frame and batched calls, the direction shards of several ranks -- so that alternating
    // callers do not rebuild (and re-synchronise) on every call, and a digest that an earlier launch on another stream may still
    // be reading is never overwritten in place: a slot is reused only after a device-wide synchronisation.
    struct DigestSlot {
        DevBuf<int32_t> buf;
        DigestKey key;            // what the digest was built for
        bool direct = false;      // ... in the [D][M] layout of the direction-outer kernel variant (table without structure)
        long long order_off = 0;  // where the digest keeps its sweep order (0: none -- the rule gave the identity, or the kernel takes no order)
        long long changes = -1, steps = 0;   // grouped build: direction steps that change a delay, of the steps that could share (-1: not counted)
        unsigned long long used = 0;
    };
    static constexpr int kDigestSlots = 4;
    DigestSlot digests[kDigestSlots];
    unsigned long long digest_clock = 0;
    void invalidate_digests() { for (auto& d : digests) d.key = DigestKey{}; }   // (buffers stay allocated; keys never match again)
    // What every loader ends with, once its uploads have succeeded: new table values, so any digest built from the old ones is stale.
    void commit(int n, int mx, int cl = 0)
    {
        loaded = true; entries = n; max_whole = mx; clamped = cl;
        invalidate_digests();
    }
    bf::DeviceTables device() const
    {
        bf::DeviceTables d;
        d.whole = whole.p; d.frac = frac.p; d.taps = taps.p; d.max_whole = max_whole;
        return d;
    }
    void drop()
    {
        loaded = false; entries = 0; max_whole = 0; clamped = 0;
        whole.release(); frac.release(); taps.release();
        for (auto& d : digests) { d.buf.release(); d.key = DigestKey{}; d.direct = false; d.order_off = 0; d.changes = -1; d.steps = 0; d.used = 0; }
    }
};

enum Slot { SLOT_PAD = 0, SLOT_LERP, SLOT_FIR, SLOT_HYBRID, SLOT_TRUNC, SLOT_COUNT };

struct State {
    std::mutex mu;
    Sizes sz;
    bool sizes_from_env_done = false;
    int device = -1;
    bool device_ready = false;
    int n_cus = 256;
    hipStream_t stream = nullptr;
    TableSet tab[SLOT_COUNT];
    std::vector<int> pad2_host;          // load_coefficients_pad2: per-mic delays (pad_and_sum.c:153-157)
    TableSet pad2_row;                   // miso_pad2: those delays for the call's microphones, a private one-row table in slot order
    TableSet delay_tab;                  // the single-signal helpers: a one-entry table (run_delay_host)
    // scratch for the host-pointer entry points
    DevBuf<float> d_frame, d_image, d_out, d_init;
    DevBuf<int32_t> d_mics;
    DevBuf<unsigned char> d_packets;     // bf_ingest: the caller's datagrams, staged
    DevBuf<unsigned long long> d_counter;  // digest build: direction steps that change the delay
    PinnedBuf h_frame, h_image;          // host-pointer mimo_*: pinned staging of the frame in / the image out
    DevBuf<float> fd_work;               // partial planes of the bin-reducing GEMMs (bf::fd_workspace_floats)
    DevBuf<float> fd_chol_work;          // blocks of the 129..256-mic Cholesky / inverse (bf::fd_cholesky_workspace_floats)
    DevBuf<float> fd_tw;                 // twiddles of the MFMA DFT for (N, bin_lo, n_bins) = fd_tw_key
    DevBuf<unsigned long long> peaks_work;  // row-pass results and per-tile lists of bf_peaks_device's tiled form (bf::peaks_workspace_words)
    long long fd_tw_key = -1;
    std::vector<int> mics_host;          // what d_mics currently holds
    DevBuf<int32_t> d_row_slot;          // bf_remove_sources_device: frame row -> slot of the adaptive array, -1 = not listed
    std::vector<int32_t> row_slot_host;  // what d_row_slot currently holds
    std::vector<float> published;        // bf_publish_frame / get_data
    std::vector<int> disabled_mics;      // get_data's dead-microphone rows
    bool disabled_default = true;
    int steer_offset = 0;                // steer(): flat table offset of the listening beam (api.c:576-581)
    std::vector<int> listen_mics;        // load_pa(): microphones of the listening beam (api.c:553-567); empty before load_miso / load_pa
    int last_variant = -1;               // bf_last_das_variant
    int last_rows = 0;                   // bf_last_das_rows
    long long last_changes = -1, last_steps = 0;   // bf_last_das_reloads
    long long last_strided[12] = {0};    // bf_last_strided_plan: the plan, the kernel and the algorithm of the most recent strided stream / select launch
    bool last_strided_set = false;
    std::string err;
};

State& S()
{
    static State s;
    return s;
}

void set_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    S().err = buf;
    fprintf(stderr, "[beamformer_hip] error: %s\n", buf);
}

void poison(float* out, size_t n)
{
    if (!out) return;
    for (size_t i = 0; i < n; ++i) out[i] = std::numeric_limits<float>::quiet_NaN();
}

#define HIP_OK(expr)                                                                          \
    ([&]() -> bool {                                                                          \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) { set_error("%s -> %s", #expr, hipGetErrorString(e__)); return false; } \
        return true;                                                                          \
    }())
// ... as an entry point's return value.  The call stays spelled at the call site: the message names what failed.
#define HIP_RC(expr) (HIP_OK(expr) ? 0 : -1)

hipStream_t as_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// ---- the checks the entry points share.  Each names the entry point (`who`) in its message, sets the error and returns false.
struct NamedPtr { const void* p; const char* name; };
bool need_ptrs(const char* who, std::initializer_list<NamedPtr> ptrs)   // refuses the first null one, in the order given
{
    for (const NamedPtr& a : ptrs)
        if (!a.p) { set_error("%s: %s is null", who, a.name); return false; }
    return true;
}

bool need_min(const char* who, const char* name, int v, int lo)
{
    if (v < lo) { set_error("%s: %s = %d < %d", who, name, v, lo); return false; }
    return true;
}

bool need_max(const char* who, const char* name, int v, int hi)
{
    if (v > hi) { set_error("%s: %s = %d > %d", who, name, v, hi); return false; }
    return true;
}

// (a bound that has a name of its own: a stride under N_SAMPLES, say)
bool need_min(const char* who, const char* name, int v, const char* bound, int lo)
{
    if (v < lo) { set_error("%s: %s = %d < %s = %d", who, name, v, bound, lo); return false; }
    return true;
}

// (a transform length)
bool need_pow2(const char* who, const char* name, int v, int lo, int hi)
{
    if (v < lo || v > hi || (v & (v - 1)) != 0) { set_error("%s: %s = %d is not a power of two in [%d, %d]", who, name, v, lo, hi); return false; }
    return true;
}

enum Finite { FINITE, FINITE_GE0, FINITE_GT0 };
bool need_finite(const char* who, const char* name, float v, Finite range = FINITE)
{
    static const char* wording[] = {"is not finite", "is not finite and >= 0", "is not finite and > 0"};
    if (!std::isfinite(v) || (range == FINITE_GE0 && v < 0.0f) || (range == FINITE_GT0 && !(v > 0.0f))) {
        set_error("%s: %s = %g %s", who, name, (double)v, wording[range]);
        return false;
    }
    return true;
}

// Every entry of the adaptive array names a row of the caller's frames.
bool need_rows(const char* who, const int* adaptive_array, int n, int m_total)
{
    for (int i = 0; i < n; ++i)
        if (adaptive_array[i] < 0 || adaptive_array[i] >= m_total) {
            set_error("%s: adaptive_array[%d] = %d is not a row of frames with m_total = %d rows", who, i, adaptive_array[i], m_total);
            return false;
        }
    return true;
}

// The geometry of a rows x cols map, in two parts because the entry points check other arguments in between: the three sizes ...
bool need_map_dims(const char* who, int rows, int cols, int offset_per_dir)
{
    return need_min(who, "rows", rows, 1) && need_min(who, "cols", cols, 1) && need_min(who, "offset_per_dir", offset_per_dir, 1);
}

// ... and a map of `count` directions (named `what` in the messages: "rows * cols", "n_dirs") whose flat table offsets d * offset_per_dir are
// ints, and which fits the image stride where the call has one (null: no such clause).
bool need_map(const char* who, const char* what, long long count, int offset_per_dir, const int* image_stride)
{
    const long long int_max = std::numeric_limits<int>::max();
    if (count > int_max) { set_error("%s: %s = %lld does not fit an int", who, what, count); return false; }
    if (image_stride && count > *image_stride) { set_error("%s: image_stride = %d < %s = %lld", who, *image_stride, what, count); return false; }
    if ((count - 1) * offset_per_dir > int_max) {
        set_error("%s: (%s - 1) * offset_per_dir = %lld does not fit an int offset", who, what, (count - 1) * offset_per_dir);
        return false;
    }
    return true;
}

// The shard [dir_begin, dir_end) of n_dirs directions, and room for it in every image.
bool need_dir_range(const char* who, int dir_begin, int dir_end, int n_dirs, int image_stride)
{
    if (dir_begin < 0 || dir_end > n_dirs || dir_begin >= dir_end) { set_error("%s: bad direction range [%d,%d) of %d", who, dir_begin, dir_end, n_dirs); return false; }
    if (image_stride < dir_end - dir_begin) { set_error("%s: image_stride %d < %d directions", who, image_stride, dir_end - dir_begin); return false; }
    return true;
}

// A window may continue the one before it by `hop` samples, and no further than its own length.
bool need_hop_max(const char* who, int hop, int N, const char* window = "N_SAMPLES")   // (window: what the call names its window length)
{
    if (hop > N) { set_error("%s: hop = %d > %s = %d (the windows would leave gaps in the stream)", who, hop, window, N); return false; }
    return true;
}

// A FIR of n_taps over such windows: it fits one, hop = 0 means unrelated windows, and a continued window has the n_taps - 1 samples of history
// in the one before it.  `subject` opens the last sentence ("the filter needs", "the filters need").
bool need_fir_window(const char* who, int n_taps, int hop, int N, const char* subject)
{
    if (n_taps > N) { set_error("%s: n_taps = %d > N_SAMPLES = %d", who, n_taps, N); return false; }
    if (!need_min(who, "hop", hop, 0) || !need_hop_max(who, hop, N)) return false;
    if (hop > 0 && n_taps - 1 > hop) {
        set_error("%s: %s n_taps - 1 = %d samples of history but hop = %d (continuous mode wants n_taps - 1 <= hop)", who, subject, n_taps - 1, hop);
        return false;
    }
    return true;
}

// The stream a call's windows add to (stream_grid.h); `window`: what the call names its window length.
bool need_stream_len(const char* who, const bf::StreamLen& sl, int hop, const char* window)
{
    if (!sl.fits) { set_error("%s: frames * %s = %lld > %d", who, hop > 0 ? "hop" : window, sl.S, bf::kMaxStream); return false; }
    return true;
}

// The STFT frame grid (stream_grid.h).
bool need_frame_grid(const char* who, int n_fft, int hop_s)
{
    static_assert(BF_ENHANCE_MAX_OVERLAP == bf::kEnhanceMaxOverlap, "the header's limit is the kernel's");
    if (!need_pow2(who, "n_fft", n_fft, bf::kEnhanceMinFft, bf::kEnhanceMaxFft) || !need_min(who, "hop_s", hop_s, 1)) return false;
    if (hop_s > n_fft || n_fft % hop_s != 0 || n_fft / hop_s > BF_ENHANCE_MAX_OVERLAP) {
        set_error("%s: hop_s = %d does not divide n_fft = %d into 1 .. %d frames a sample", who, hop_s, n_fft, BF_ENHANCE_MAX_OVERLAP);
        return false;
    }
    return true;
}

// The band [bin_lo, bin_hi] of an n_taps-point grid.
bool need_bins(const char* who, int bin_lo, int bin_hi, int n_taps)
{
    if (bin_lo < 0 || bin_hi < bin_lo || bin_hi > n_taps / 2) {
        set_error("%s: bins [%d, %d] are not within 0 <= bin_lo <= bin_hi <= n_taps / 2 = %d", who, bin_lo, bin_hi, n_taps / 2);
        return false;
    }
    return true;
}

// The bytes an argument covers.  Sizes saturate: four ints and N_SAMPLES can pass 2^64.
using u64 = unsigned long long;
constexpr u64 kTop = std::numeric_limits<u64>::max();
u64 sat_mul(u64 a, u64 b) { return b && a > kTop / b ? kTop : a * b; }
u64 sat_add(u64 a, u64 b) { return b > kTop - a ? kTop : a + b; }

struct Span { const void* p; u64 bytes; const char* name; const char* note = ""; };   // (note: why this one must not be written, behind its name)

// The first `n_outputs` spans are written.  Refuses the first pair (a, b), a an output and a < b, that shares a byte; an optional argument that
// was not given (null) is skipped.
bool need_disjoint(const char* who, std::initializer_list<Span> spans, int n_outputs)
{
    const Span* s = spans.begin();
    const int count = (int)spans.size();
    for (int a = 0; a < n_outputs; ++a)
        for (int b = a + 1; b < count; ++b) {
            if (!s[a].p || !s[b].p) continue;
            const u64 a0 = reinterpret_cast<uintptr_t>(s[a].p), b0 = reinterpret_cast<uintptr_t>(s[b].p);
            if (a0 < sat_add(b0, s[b].bytes) && b0 < sat_add(a0, s[a].bytes)) {
                set_error("%s: %s overlaps %s%s", who, s[a].name, s[b].name, s[b].note);
                return false;
            }
        }
    return true;
}

// Calls that exist for BF_PAD and BF_LERP only; `reason` says why the other algorithms are refused (`with_number` adds the algo's value).
bool need_pad_or_lerp(const char* who, int algo, bool with_number, const char* reason)
{
    if (algo == bf::ALGO_PAD || algo == bf::ALGO_LERP) return true;
    if (algo == bf::ALGO_HYBRID || algo == bf::ALGO_FIR_NAIVE || algo == bf::ALGO_FIR_VEC) {
        static const char* name[] = {"BF_PAD", "BF_LERP", "BF_HYBRID", "BF_FIR_NAIVE", "BF_FIR_VEC"};
        char number[16] = "";
        if (with_number) snprintf(number, sizeof(number), " (%d)", algo);
        set_error("%s: algo %s%s %s", who, name[algo], number, reason);
    } else {
        set_error("%s: unknown algo %d", who, algo);
    }
    return false;
}

// The host-pointer calls (one 64 KB frame in, one 40 KB map out) end in a wait for the stream.  hipStreamSynchronize may block or yield, depending on the
// scheduling policy the runtime picks for the box (CPU count, other devices): the same call measured 58 us on one box and 206 us on another.  A call this
// short is polled first -- hipStreamQuery in a spin for up to 2 ms -- and only then handed to the blocking wait.
static hipError_t sync_short(hipStream_t stream)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(stream);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    return hipStreamSynchronize(stream);
}

// ---- config.json reader: "KEY": number, anywhere in the file (keys are unique in PC/src/config.json)
bool json_number(const std::string& text, const char* key, double* out)
{
    const std::string pat = std::string("\"") + key + "\"";
    size_t pos = text.find(pat);
    if (pos == std::string::npos) return false;
    pos = text.find(':', pos + pat.size());
    if (pos == std::string::npos) return false;
    const char* s = text.c_str() + pos + 1;
    char* end = nullptr;
    const double v = strtod(s, &end);
    if (end == s) return false;
    *out = v;
    return true;
}

bool apply_sizes(int mics, int n, int x, int y, int t)
{
    if (mics < 1 || n < 1 || x < 1 || y < 1 || t < 1 || (long long)x * y > (1 << 24)) {
        set_error("bf_configure: invalid sizes N_MICROPHONES=%d N_SAMPLES=%d MAX_RES_X=%d MAX_RES_Y=%d N_TAPS=%d", mics, n, x, y, t);
        return false;
    }
    if (n > 1024) { set_error("bf_configure: N_SAMPLES=%d > 1024 is not supported by the gfx950 kernels", n); return false; }
    State& s = S();
    const Sizes old = s.sz;
    s.sz.n_microphones = mics; s.sz.n_samples = n; s.sz.res_x = x; s.sz.res_y = y; s.sz.n_taps = t;
    if (old.n_samples != n || old.res_x != x || old.res_y != y || old.n_taps != t)
        for (auto& t2 : s.tab) t2.drop();
    s.published.clear();
    return true;
}

bool configure_from_json(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("cannot open config file %s", path); return false; }
    std::string text;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
    fclose(f);
    Sizes z = S().sz;
    double v;
    if (json_number(text, "N_MICROPHONES", &v)) z.n_microphones = (int)v;
    if (json_number(text, "N_SAMPLES", &v)) z.n_samples = (int)v;
    if (json_number(text, "MAX_RES_X", &v)) z.res_x = (int)v;
    if (json_number(text, "MAX_RES_Y", &v)) z.res_y = (int)v;
    if (json_number(text, "N_TAPS", &v)) z.n_taps = (int)v;
    return apply_sizes(z.n_microphones, z.n_samples, z.res_x, z.res_y, z.n_taps);
}

void sizes_from_env_once()
{
    State& s = S();
    if (s.sizes_from_env_done) return;
    s.sizes_from_env_done = true;
    if (const char* p = getenv("BF_CONFIG")) (void)configure_from_json(p);
}

// How an entry point that reads the sizes begins: the process lock for the length of the call, then $BF_CONFIG on the first one.
struct Entered {
    State& s = S();
    std::lock_guard<std::mutex> lock{s.mu};
    Entered() { sizes_from_env_once(); }
};

// Lazy, per-process HIP bring-up (never at library load: callers fork first).
bool ensure_device()
{
    State& s = S();
    sizes_from_env_once();
    if (s.device_ready) return true;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1) {
        set_error("no usable HIP device (%s); this library has no CPU fallback", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return false;
    }
    int dev = s.device;
    if (dev < 0) { const char* p = getenv("BF_DEVICE"); dev = p ? atoi(p) : 0; }
    if (dev >= count) { set_error("HIP device %d requested but only %d present", dev, count); return false; }
    if (!HIP_OK(hipSetDevice(dev))) return false;
    hipDeviceProp_t prop;
    if (!HIP_OK(hipGetDeviceProperties(&prop, dev))) return false;
    if (strncmp(prop.gcnArchName, "gfx9", 4) != 0) {
        set_error("device %d is %s; this build carries gfx950 code only", dev, prop.gcnArchName);
        return false;
    }
    s.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (!HIP_OK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking))) return false;
    s.device = dev;
    s.device_ready = true;
    return true;
}

template <typename T>
bool upload(DevBuf<T>& dst, const T* src, size_t n)
{
    if (!HIP_OK(dst.reserve(n))) return false;
    return HIP_OK(hipMemcpy(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice));
}

bool upload_mics(const int* adaptive, int n, int* max_row)
{
    State& s = S();
    int mx = -1;
    for (int i = 0; i < n; ++i) {
        if (adaptive[i] < 0) { set_error("adaptive_array[%d] = %d is negative", i, adaptive[i]); return false; }
        mx = std::max(mx, adaptive[i]);
    }
    *max_row = mx;
    if ((int)s.mics_host.size() == n && std::equal(adaptive, adaptive + n, s.mics_host.begin()) && s.d_mics.p) return true;
    // a new adaptive array: launches already enqueued on the caller's (non-blocking) streams may still read the old copy
    if (s.d_mics.p && !HIP_OK(hipDeviceSynchronize())) return false;
    if (!upload(s.d_mics, adaptive, (size_t)n)) return false;
    s.mics_host.assign(adaptive, adaptive + n);
    return true;
}

int slot_of(int algo)
{
    switch (algo) {
        case bf::ALGO_PAD: return SLOT_PAD;
        case bf::ALGO_LERP: return SLOT_LERP;
        case bf::ALGO_HYBRID: return SLOT_HYBRID;
        case bf::ALGO_FIR_NAIVE:
        case bf::ALGO_FIR_VEC: return SLOT_FIR;
        default: return -1;
    }
}

const char* loader_name(int slot)
{
    static const char* n[] = {"load_coefficients_pad", "load_coefficients_lerp", "load_coefficients_convolve",
                              "load_coefficients_convolve_hybrid", "load_coefficients2"};
    return n[slot];
}

// Fill the launch descriptor shared by every entry point.  `n` = active mics, table must hold D*n entries.
bool describe(int algo, int slot, int n, bf::DasLaunch* L)
{
    State& s = S();
    const TableSet& t = s.tab[slot];
    if (!t.loaded) { set_error("%s has not been called", loader_name(slot)); return false; }
    const int D = s.sz.dirs();
    const bool fir = (slot == SLOT_FIR);
    const long long want = (long long)D * n * (fir ? s.sz.n_taps : 1);
    if (n < 1 || want != t.entries) {
        set_error("%s loaded %d coefficients but MAX_RES_X*MAX_RES_Y*n%s = %d*%d*%d%s = %lld", loader_name(slot), t.entries,
                  fir ? "*N_TAPS" : "", s.sz.res_x, s.sz.res_y, n, fir ? "*T" : "", want);
        return false;
    }
    L->algo = algo;
    L->tab = t.device();
    L->n_mics = n; L->n_samples = s.sz.n_samples; L->n_taps = s.sz.n_taps; L->n_dirs = D;
    L->dir_begin = 0; L->dir_end = D; L->image_stride = D; L->image_origin = 0; L->frames = 1;
    L->mics = s.d_mics.p;
    return true;
}

bool plan_or_error(const bf::DasLaunch& L, bf::DasPlan* plan)
{
    const char* why = "";
    if (bf::plan_das(L, S().n_cus, plan, &why) != 0) { set_error("unsupported shape: %s", why); return false; }
    return true;
}

// One beam of one frame: the launch every MISO path plans with (the batched and the stream calls raise L->frames afterwards), so
// that all of them reach the kernel instantiation the host-pointer miso_* call reaches.  The adaptive array is already uploaded.
bool plan_one_beam(int algo, const TableSet& t, int n, int m_total, const float* d_signals, bf::DasLaunch* L, bf::DasPlan* plan)
{
    State& s = S();
    *L = bf::DasLaunch{};
    L->algo = algo;
    L->tab = t.device();
    L->n_mics = n; L->m_total = m_total; L->n_samples = s.sz.n_samples; L->n_taps = s.sz.n_taps; L->n_dirs = 1;
    L->dir_begin = 0; L->dir_end = 1; L->image_stride = 1; L->image_origin = 0; L->frames = 1;
    L->signals = d_signals; L->images = nullptr; L->mics = s.d_mics.p;
    return plan_or_error(*L, plan);
}

// out[0..9] of the plan exports (bf_plan_das, bf_plan_das_select, bf_plan_das_stream, bf_last_strided_plan).
void export_plan(const bf::DasPlan& p, long long* out)
{
    out[0] = p.nc; out[1] = p.lead; out[2] = p.row_stride; out[3] = p.mic_chunk; out[4] = p.n_chunks;
    out[5] = p.waves; out[6] = p.dpw; out[7] = p.tile_dirs; out[8] = p.n_tiles; out[9] = (long long)p.lds_bytes;
}

// bf_last_strided_plan's record of a launch that was enqueued: kernel 0 = das_mimo_kernel with history, 1 = das_select_kernel, 2 = das_select_kernel with
// history, 3 = das_miso_kernel with history.
enum StridedKernel { STRIDED_STREAM_MAP = 0, STRIDED_SELECT, STRIDED_SELECT_HIST, STRIDED_STREAM_BEAM };
int launched_strided(hipError_t e, const char* call, StridedKernel kernel, int algo, const bf::DasPlan& plan)
{
    if (e != hipSuccess) { set_error("%s -> %s", call, hipGetErrorString(e)); return -1; }
    State& s = S();
    export_plan(plan, s.last_strided);
    s.last_strided[10] = kernel; s.last_strided[11] = algo;
    s.last_strided_set = true;
    return 0;
}
#define STRIDED_RC(kernel, algo, plan, expr) launched_strided((expr), #expr, kernel, algo, plan)

// The sweep order of a launch (bf::sweep_order on the whole-sample rows of its direction range, fetched once), stored at d_order
// padded to whole groups by repeating the last entry.  *stored = false when the rule gave the identity: nothing is written then.
bool store_sweep_order(const bf::DasLaunch& L, const bf::DasPlan& plan, int32_t* d_order, bool* stored)
{
    const int n_pos = L.dir_end - L.dir_begin;
    const size_t padded = ((size_t)n_pos + plan.dpw - 1) / plan.dpw * plan.dpw;
    std::vector<int32_t> rows((size_t)n_pos * L.n_mics), order(padded);
    if (!HIP_OK(hipMemcpy(rows.data(), L.tab.whole + (size_t)L.dir_begin * L.n_mics, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost))) return false;
    bf::SweepOrderStats st;
    if (bf::sweep_order(rows.data(), L.n_mics, n_pos, L.n_mics, L.dir_begin, plan.dpw, order.data(), &st) != 0) {
        set_error("sweep order: bad launch geometry");
        return false;
    }
    *stored = !st.identity;
    if (st.identity) return true;
    for (size_t i = (size_t)n_pos; i < padded; ++i) order[i] = order[(size_t)n_pos - 1];
    return HIP_OK(hipMemcpy(d_order, order.data(), padded * sizeof(int32_t), hipMemcpyHostToDevice));
}

// The families that take a digest: make sure the table set carries one built for this plan.  A slot whose table went to the
// direction-outer family replans the launch (L.tab.digest_direct, `plan`).
bool attach_digest(TableSet& t, bf::DasLaunch& L, bf::DasPlan& plan, hipStream_t stream)
{
    // everything the digest depends on: the plan's family and geometry, the algorithm and (grouped layouts) the direction range
    const bf::DigestLayout lay = bf::digest_layout(L, plan);
    const DigestKey key{true, plan.family, plan.mic_chunk, plan.row_stride, plan.lead, L.algo, plan.dpw, L.dir_begin, L.dir_end, L.n_mics};
    TableSet::DigestSlot* slot = nullptr;
    for (auto& d : t.digests)
        if (d.buf.p && d.key == key) slot = &d;
    if (slot == nullptr) {
        State& s = S();
        // an unused slot, else the least recently used one -- which launches still in flight on other streams may be reading
        TableSet::DigestSlot* victim = &t.digests[0];
        for (auto& d : t.digests) {
            if (!d.buf.p || !d.key.valid) { victim = &d; break; }
            if (d.used < victim->used) victim = &d;
        }
        if (victim->buf.p && !HIP_OK(hipDeviceSynchronize())) return false;
        victim->key = DigestKey{};
        if (!HIP_OK(victim->buf.reserve(lay.elements)) || !HIP_OK(s.d_counter.reserve(1))) return false;
        victim->direct = false;
        victim->order_off = 0; victim->changes = -1; victim->steps = 0;
        if (lay.order_off != 0) {                               // (the plan's kernel stores by an order table)
            bool stored = false;
            if (!store_sweep_order(L, plan, victim->buf.p + lay.order_off, &stored)) return false;
            if (stored) victim->order_off = lay.order_off;
        }
        const bool grouped = lay.kind == bf::DIGEST_GROUPED;
        if (grouped && !HIP_OK(hipMemsetAsync(s.d_counter.p, 0, sizeof(unsigned long long), stream))) return false;
        if (!HIP_OK(bf::launch_digest(L, plan, victim->buf.p, grouped ? s.d_counter.p : nullptr, victim->order_off, stream))) return false;
        // once per (table, geometry): wait, so that a later launch on ANOTHER stream cannot overtake the digest's construction
        if (!HIP_OK(hipStreamSynchronize(stream))) return false;
        if (bf::family_traits(plan.family).reread_handover && plan.waves == 16) {      // (the direction-outer variant exists for 16 waves only)
            // A table without structure (more than half of the direction steps change the delay, counted in sweep order) defeats the
            // sweep: use the direction-outer kernel variant and its [D][M] digest instead.
            unsigned long long reloads = 0;
            if (!HIP_OK(hipMemcpy(&reloads, s.d_counter.p, sizeof(reloads), hipMemcpyDeviceToHost))) return false;
            const long long steps = bf::digest_shareable_steps(L, plan);
            victim->changes = (long long)reloads; victim->steps = steps;
            if (steps > 0 && 2 * (long long)reloads > steps) {
                L.tab.digest_direct = true;
                if (!plan_or_error(L, &plan)) return false;     // that variant reads at every step: four shifted copies, its own chunk size
                if (!HIP_OK(bf::launch_digest(L, plan, victim->buf.p, nullptr, 0, stream)) || !HIP_OK(hipStreamSynchronize(stream))) return false;
                victim->direct = true;
                victim->order_off = 0;                          // (that variant walks [D][M] in flat order)
            }
        }
        victim->key = key;                                      // (the key is the sweep plan's: what the caller's planning yields next time)
        slot = victim;
    } else if (slot->direct) {
        L.tab.digest_direct = true;
        if (!plan_or_error(L, &plan)) return false;
    }
    slot->used = ++t.digest_clock;
    L.tab.digest_direct = slot->direct;
    L.tab.digest = slot->buf.p;
    L.tab.digest_order_off = slot->order_off;
    S().last_changes = slot->changes; S().last_steps = slot->steps;
    return true;
}

// What a batched launch needs beyond its plan: its digest, where its family takes one, and the record of the family it ends up with.
bool ensure_digest(TableSet& t, bf::DasLaunch& L, bf::DasPlan& plan, hipStream_t stream)
{
    S().last_changes = -1; S().last_steps = 0;
    const bool ok = bf::digest_layout(L, plan).kind == bf::DIGEST_NONE || attach_digest(t, L, plan, stream);
    const bf::FamilyTraits ft = bf::family_traits(plan.family);      // (attach_digest may have replanned the launch direction-outer)
    S().last_variant = ft.variant; S().last_rows = ft.rows;
    return ok;
}

// mimo_* with host pointers: one frame in, one image out (PC/src/algorithms/pad_and_sum.c:100-143 and twins).
void run_mimo_host(int algo, int slot, const float* signals, float* image, const int* adaptive, int n)
{
    Entered in;
    State& s = in.s;
    const size_t D = (size_t)s.sz.dirs();
    if (!signals || !image || !adaptive) { set_error("null argument"); poison(image, image ? D : 0); return; }
    bool ok = ensure_device();
    bf::DasLaunch L{};
    bf::DasPlan plan{};
    int max_row = 0;
    ok = ok && upload_mics(adaptive, n, &max_row);
    ok = ok && describe(algo, slot, n, &L);
    if (ok) {
        const size_t rows = (size_t)max_row + 1;
        L.m_total = (int)rows;
        const size_t frame_floats = rows * s.sz.n_samples;
        ok = HIP_OK(s.d_frame.reserve(frame_floats)) && HIP_OK(s.d_image.reserve(D)) && HIP_OK(s.h_frame.reserve(frame_floats)) && HIP_OK(s.h_image.reserve(D));
        if (ok) std::memcpy(s.h_frame.p, signals, frame_floats * sizeof(float));
        ok = ok && HIP_OK(hipMemcpyAsync(s.d_frame.p, s.h_frame.p, frame_floats * sizeof(float), hipMemcpyHostToDevice, s.stream));
        L.signals = s.d_frame.p; L.images = s.d_image.p; L.mics = s.d_mics.p;
        ok = ok && plan_or_error(L, &plan);
        ok = ok && ensure_digest(s.tab[slot], L, plan, s.stream);
        ok = ok && HIP_OK(bf::launch_das(L, plan, s.stream));
        ok = ok && HIP_OK(hipMemcpyAsync(s.h_image.p, s.d_image.p, D * sizeof(float), hipMemcpyDeviceToHost, s.stream));
        ok = ok && HIP_OK(sync_short(s.stream));
        if (ok) std::memcpy(image, s.h_image.p, D * sizeof(float));
    }
    if (!ok) poison(image, D);
}

// miso_*: one direction (table offset), raw out[N] (pad_and_sum.c:54-70 and twins).
void run_miso_host(int algo, const TableSet& t, const char* loader, bool fir, const float* signals, float* out,
                   const int* adaptive, int n, long long row_offset, const float* init)
{
    State& s = S();
    sizes_from_env_once();
    const size_t N = (size_t)s.sz.n_samples;
    if (!signals || !out || !adaptive) { set_error("null argument"); poison(out, out ? N : 0); return; }
    bool ok = ensure_device();
    bf::DasLaunch L{};
    bf::DasPlan plan{};
    int max_row = 0;
    ok = ok && upload_mics(adaptive, n, &max_row);
    if (ok) {
        if (!t.loaded) { set_error("%s has not been called", loader); ok = false; }
        const long long per = fir ? s.sz.n_taps : 1;
        if (ok && (row_offset < 0 || (row_offset + n) * per > t.entries)) {
            set_error("offset %lld + n %d exceeds the %d loaded coefficients", row_offset, n, t.entries);
            ok = false;
        }
    }
    if (ok) {
        const size_t rows = (size_t)max_row + 1;
        ok = HIP_OK(s.d_frame.reserve(rows * N)) && HIP_OK(s.d_out.reserve(N));
        ok = ok && HIP_OK(hipMemcpyAsync(s.d_frame.p, signals, rows * N * sizeof(float), hipMemcpyHostToDevice, s.stream));
        if (ok && init) {
            ok = HIP_OK(s.d_init.reserve(N)) && HIP_OK(hipMemcpyAsync(s.d_init.p, init, N * sizeof(float), hipMemcpyHostToDevice, s.stream));
        }
        ok = ok && plan_one_beam(algo, t, n, (int)rows, s.d_frame.p, &L, &plan);
        ok = ok && HIP_OK(bf::launch_miso(L, plan, row_offset, init ? s.d_init.p : nullptr, s.d_out.p, s.stream));
        ok = ok && HIP_OK(hipMemcpyAsync(out, s.d_out.p, N * sizeof(float), hipMemcpyDeviceToHost, s.stream));
        ok = ok && HIP_OK(sync_short(s.stream));
    }
    if (!ok) poison(out, N);
}

// The single-signal helpers (pad_delay, lerp_delay, convolve_*_delay*): out (+)= delayed(signal).  Run as a
// one-mic, one-entry-table MISO launch with `out` as the initial accumulator.
void run_delay_host(int algo, const float* signal, float* out, bool accumulate, int whole, float h, const float* taps)
{
    Entered in;
    State& s = in.s;
    const size_t N = (size_t)s.sz.n_samples;
    if (!signal || !out) { set_error("null argument"); poison(out, out ? N : 0); return; }
    bool ok = ensure_device();
    if (ok && (whole < 0)) { set_error("negative delay %d", whole); ok = false; }
    bf::DasLaunch L{};
    bf::DasPlan plan{};
    const int zero = 0;
    int max_row = 0;
    ok = ok && upload_mics(&zero, 1, &max_row);
    TableSet& t = s.delay_tab;
    if (ok) {
        const int w = std::min(whole, s.sz.n_samples);
        ok = upload(t.whole, &w, 1) && upload(t.frac, &h, 1);
        if (ok && taps) ok = upload(t.taps, taps, (size_t)s.sz.n_taps);
        t.max_whole = w;
    }
    if (ok) {
        ok = HIP_OK(s.d_frame.reserve(N)) && HIP_OK(s.d_out.reserve(N)) && HIP_OK(s.d_init.reserve(N));
        ok = ok && HIP_OK(hipMemcpyAsync(s.d_frame.p, signal, N * sizeof(float), hipMemcpyHostToDevice, s.stream));
        if (ok && accumulate) ok = HIP_OK(hipMemcpyAsync(s.d_init.p, out, N * sizeof(float), hipMemcpyHostToDevice, s.stream));
        ok = ok && plan_one_beam(algo, t, 1, 1, s.d_frame.p, &L, &plan);
        ok = ok && HIP_OK(bf::launch_miso(L, plan, 0, accumulate ? s.d_init.p : nullptr, s.d_out.p, s.stream));
        ok = ok && HIP_OK(hipMemcpyAsync(out, s.d_out.p, N * sizeof(float), hipMemcpyDeviceToHost, s.stream));
        ok = ok && HIP_OK(sync_short(s.stream));
    }
    if (!ok) poison(out, N);
}

// Integer table sanity shared by the loaders: no negative delays; values beyond N contribute nothing, so they
// are clamped to N (keeps the LDS zero prefix bounded).
bool sanitize_whole(std::vector<int32_t>& w, int n_samples, int* max_whole, const char* who, int* clamped = nullptr)
{
    int mx = 0, cl = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        if (w[i] < 0) { set_error("%s: negative delay %d at index %zu (the reference would write out of bounds)", who, w[i], i); return false; }
        if (w[i] > n_samples) { w[i] = n_samples; ++cl; }
        mx = std::max(mx, w[i]);
    }
    *max_whole = mx;
    if (clamped) *clamped = cl;
    return true;
}

bool load_whole_only(int slot, const int* whole, int n, const char* who)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    if (!whole || n < 1) { set_error("%s: null or empty table", who); return false; }
    if (!ensure_device()) return false;
    std::vector<int32_t> w(whole, whole + n);
    TableSet& t = s.tab[slot];
    int mx = 0, cl = 0;
    if (!sanitize_whole(w, s.sz.n_samples, &mx, who, &cl)) return false;
    if (!upload(t.whole, w.data(), w.size())) return false;
    t.commit(n, mx, cl);
    return true;
}

// hybrid_convolve_and_sum.c:124-157 (note its own pi constant and epsilon placement)
void hybrid_taps(float* h, double delay, int T)
{
    const double PI = 3.14159265359, eps = 1e-9;
    const double tau = 0.5 - delay + eps;
    double sum = 0.0;
    for (int i = 0; i < T; ++i) {
        double v = (double)i - ((double)T - 1.0) / 2.0 - tau;
        v = std::sin(v * PI) / (v * PI);
        const double n = (double)(i * 2 - T + 1);
        const double w = 0.42 + 0.5 * std::cos(PI * n / ((double)(T - 1)) + eps) + 0.08 * std::cos(2.0 * PI * n / ((double)(T - 1) + eps));
        v *= w;
        sum += v;
        h[i] = (float)v;
    }
    for (int i = 0; i < T; ++i) h[i] /= (float)sum;
}

template <typename F>
void parallel_for(size_t n, F body)
{
    unsigned hw = std::thread::hardware_concurrency();
    size_t workers = std::min<size_t>(hw ? hw : 1, 16);
    if (n < 65536 || workers < 2) { body(0, n); return; }
    std::vector<std::thread> pool;
    const size_t step = (n + workers - 1) / workers;
    for (size_t w = 0; w < workers; ++w) {
        const size_t lo = w * step, hi = std::min(n, lo + step);
        if (lo < hi) pool.emplace_back([=] { body(lo, hi); });
    }
    for (auto& th : pool) th.join();
}

}  // namespace

// ============================================================================================== C-ABI
extern "C" {

// ---------------------------------------------------------------- configuration / errors

int bf_configure(int n_microphones, int n_samples, int max_res_x, int max_res_y, int n_taps)
{
    std::lock_guard<std::mutex> lock(S().mu);
    S().sizes_from_env_done = true;  // an explicit call wins over $BF_CONFIG
    return apply_sizes(n_microphones, n_samples, max_res_x, max_res_y, n_taps) ? 0 : -1;
}

int bf_configure_from_json(const char* path)
{
    std::lock_guard<std::mutex> lock(S().mu);
    S().sizes_from_env_done = true;
    return (path && configure_from_json(path)) ? 0 : -1;
}

void bf_get_config(int out[5])
{
    Entered in;
    const Sizes& z = in.s.sz;
    out[0] = z.n_microphones; out[1] = z.n_samples; out[2] = z.res_x; out[3] = z.res_y; out[4] = z.n_taps;
}

const char* bf_last_error(void) { return S().err.c_str(); }
void bf_clear_error(void) { S().err.clear(); }

// Which kernel family the last delay-and-sum launch used, -1 before the first one (the values are listed at its declaration in
// include/beamformer_hip.h).  For tests and tuning.
int bf_last_das_variant(void) { return S().last_variant; }
int bf_last_das_rows(void) { return S().last_rows; }

int bf_last_das_reloads(long long* changes, long long* steps)
{
    if (!need_ptrs("bf_last_das_reloads", {{changes, "changes"}, {steps, "steps"}})) return -1;
    *changes = S().last_changes; *steps = S().last_steps;
    if (S().last_changes < 0) { set_error("bf_last_das_reloads: the last launch used no digest whose re-reads were counted"); return -1; }
    return 0;
}

int bf_sweep_order(const int* whole, int n_dirs, int n_mics, int dir_begin, int dir_end, int dpw, int* order_out)
{
    if (!need_ptrs("bf_sweep_order", {{whole, "whole"}, {order_out, "order_out"}})) return -1;
    if (n_dirs < 1 || n_mics < 1 || dpw < 1 || dir_begin < 0 || dir_end > n_dirs || dir_begin >= dir_end) {
        set_error("bf_sweep_order: want n_dirs, n_mics, dpw >= 1 and 0 <= dir_begin < dir_end <= n_dirs (got %d, %d, %d, [%d, %d))", n_dirs, n_mics, dpw,
                  dir_begin, dir_end);
        return -1;
    }
    static_assert(sizeof(int) == sizeof(int32_t), "the C-ABI's int tables are int32");
    return bf::sweep_order(reinterpret_cast<const int32_t*>(whole) + (size_t)dir_begin * n_mics, n_mics, dir_end - dir_begin, n_mics, dir_begin, dpw,
                           reinterpret_cast<int32_t*>(order_out), nullptr);
}
int bf_read_phase_stamps(unsigned long long* out16, int clear)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!out16 || !ensure_device()) return -1;
    return HIP_OK(hipDeviceSynchronize()) && HIP_OK(bf::read_phase_stamps(out16, clear != 0)) ? 0 : -1;
}
int bf_read_wave_stamps(unsigned long long* out128, int clear)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!out128 || !ensure_device()) return -1;
    return HIP_OK(hipDeviceSynchronize()) && HIP_OK(bf::read_wave_stamps(out128, clear != 0)) ? 0 : -1;
}

int bf_gpu_available(void)
{
    int count = 0;
    return (hipGetDeviceCount(&count) == hipSuccess && count > 0) ? 1 : 0;
}

int bf_set_device(int device)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (S().device_ready && device != S().device) { set_error("bf_set_device: device %d already in use", S().device); return -1; }
    S().device = device;
    return 0;
}

// ---------------------------------------------------------------- pad

void load_coefficients_pad(int* whole_samples, int n) { (void)load_whole_only(SLOT_PAD, whole_samples, n, "load_coefficients_pad"); }
void unload_coefficients_pad(void) { std::lock_guard<std::mutex> lock(S().mu); S().tab[SLOT_PAD].drop(); }

void load_coefficients_pad2(int* whole_miso, int n)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!whole_miso || n < 1) { set_error("load_coefficients_pad2: null or empty table"); return; }
    S().pad2_host.assign(whole_miso, whole_miso + n);
}
void unload_coefficients_pad2(void) { std::lock_guard<std::mutex> lock(S().mu); S().pad2_host.clear(); }

void mimo_pad(float* signals, float* image, int* adaptive_array, int n) { run_mimo_host(bf::ALGO_PAD, SLOT_PAD, signals, image, adaptive_array, n); }

void miso_pad(float* signals, float* out, int* adaptive_array, int n, int offset)
{
    std::lock_guard<std::mutex> lock(S().mu);
    run_miso_host(bf::ALGO_PAD, S().tab[SLOT_PAD], loader_name(SLOT_PAD), false, signals, out, adaptive_array, n, offset, nullptr);
}

void miso_pad2(float* signals, float* out, int* adaptive_array, int n, int offset)
{
    // pad_and_sum.c:77-92: delay looked up by MICROPHONE id in the pad2 table; `offset` is unused there too.
    (void)offset;
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    const size_t N = (size_t)s.sz.n_samples;
    if (!adaptive_array || n < 1) { set_error("miso_pad2: null or empty adaptive_array"); poison(out, N); return; }
    std::vector<int32_t> row((size_t)n);
    for (int m = 0; m < n; ++m) {
        const int mic = adaptive_array[m];
        if (mic < 0 || mic >= (int)s.pad2_host.size()) { set_error("miso_pad2: mic %d outside the %zu-entry pad2 table", mic, s.pad2_host.size()); poison(out, N); return; }
        row[(size_t)m] = s.pad2_host[(size_t)mic];
    }
    if (!ensure_device()) { poison(out, N); return; }
    int mx = 0;
    if (!sanitize_whole(row, s.sz.n_samples, &mx, "miso_pad2") || !upload(s.pad2_row.whole, row.data(), row.size())) { poison(out, N); return; }
    s.pad2_row.commit(n, mx);
    run_miso_host(bf::ALGO_PAD, s.pad2_row, "load_coefficients_pad2", false, signals, out, adaptive_array, n, 0, nullptr);
}

void pad_delay(float* signal, float* out, int pos_pad) { run_delay_host(bf::ALGO_PAD, signal, out, true, pos_pad, 0.f, nullptr); }

// ---------------------------------------------------------------- lerp

void load_coefficients_lerp(float* delays, int n)
{
    // lerp_and_sum.c:139-153: frac = modf((double)delay, &ip); h = 1.0 - (float)frac (rounded to float); whole = (int)ip
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    if (!delays || n < 1) { set_error("load_coefficients_lerp: null or empty table"); return; }
    if (!ensure_device()) return;
    std::vector<int32_t> w((size_t)n);
    std::vector<float> h((size_t)n);
    for (int i = 0; i < n; ++i) {
        double ip;
        const float frac = (float)std::modf((double)delays[i], &ip);
        h[(size_t)i] = (float)(1.0 - (double)frac);
        w[(size_t)i] = (int)ip;
    }
    TableSet& t = s.tab[SLOT_LERP];
    int mx = 0, cl = 0;
    if (!sanitize_whole(w, s.sz.n_samples, &mx, "load_coefficients_lerp", &cl)) return;
    if (!upload(t.whole, w.data(), w.size()) || !upload(t.frac, h.data(), h.size())) return;
    t.commit(n, mx, cl);
}
void unload_coefficients_lerp(void) { std::lock_guard<std::mutex> lock(S().mu); S().tab[SLOT_LERP].drop(); }

void mimo_lerp(float* signals, float* image, int* adaptive_array, int n) { run_mimo_host(bf::ALGO_LERP, SLOT_LERP, signals, image, adaptive_array, n); }
void miso_lerp(float* signals, float* out, int* adaptive_array, int n, int offset)
{
    std::lock_guard<std::mutex> lock(S().mu);
    run_miso_host(bf::ALGO_LERP, S().tab[SLOT_LERP], loader_name(SLOT_LERP), false, signals, out, adaptive_array, n, offset, nullptr);
}
void lerp_delay(float* signal, float* out, float h, int pad) { run_delay_host(bf::ALGO_LERP, signal, out, true, pad, h, nullptr); }

int bf_get_lerp_tables(int* whole, float* h, int n)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    const TableSet& t = s.tab[SLOT_LERP];
    if (!t.loaded || n != t.entries) { set_error("bf_get_lerp_tables: %d requested, %d loaded", n, t.loaded ? t.entries : 0); return -1; }
    bool ok = HIP_OK(hipMemcpy(whole, t.whole.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    ok = ok && HIP_OK(hipMemcpy(h, t.frac.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return ok ? 0 : -1;
}

int bf_get_pad_table(int* whole, int n)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    const TableSet& t = s.tab[SLOT_PAD];
    if (!whole) { set_error("bf_get_pad_table: whole is null"); return -1; }
    if (!t.loaded || n != t.entries) { set_error("bf_get_pad_table: %d requested, %d loaded", n, t.loaded ? t.entries : 0); return -1; }
    return HIP_RC(hipMemcpy(whole, t.whole.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------- convolve (full FIR)

void load_coefficients_convolve(float* h, int n)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    if (!h || n < 1) { set_error("load_coefficients_convolve: null or empty table"); return; }
    if (!ensure_device()) return;
    TableSet& t = s.tab[SLOT_FIR];
    if (!upload(t.taps, h, (size_t)n)) return;
    t.commit(n, 0);
}
void unload_coefficients_convolve(void) { std::lock_guard<std::mutex> lock(S().mu); S().tab[SLOT_FIR].drop(); }

void mimo_convolve_naive(float* signals, float* image, int* adaptive_array, int n) { run_mimo_host(bf::ALGO_FIR_NAIVE, SLOT_FIR, signals, image, adaptive_array, n); }
void mimo_convolve_vectorized(float* signals, float* image, int* adaptive_array, int n) { run_mimo_host(bf::ALGO_FIR_VEC, SLOT_FIR, signals, image, adaptive_array, n); }

void miso_convolve_vectorized(float* signals, float* out, int* adaptive_array, int n, int offset)
{
    // convolve_and_sum.c:276-292: offset counts taps (d * n * N_TAPS)
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    const int T = s.sz.n_taps;
    if (offset % T != 0) { set_error("miso_convolve_vectorized: offset %d is not a multiple of N_TAPS=%d", offset, T); poison(out, (size_t)s.sz.n_samples); return; }
    run_miso_host(bf::ALGO_FIR_VEC, s.tab[SLOT_FIR], loader_name(SLOT_FIR), true, signals, out, adaptive_array, n, offset / T, nullptr);
}

void convolve_delay_naive_add(float* signal, float* h, float* out) { run_delay_host(bf::ALGO_FIR_NAIVE, signal, out, true, 0, 0.f, h); }
void convolve_delay_naive(float* signal, float* out, float* h) { run_delay_host(bf::ALGO_FIR_NAIVE, signal, out, true, 0, 0.f, h); }
void convolve_delay_vectorized(float* signal, float* h, float* out) { run_delay_host(bf::ALGO_FIR_NAIVE, signal, out, false, 0, 0.f, h); }
void convolve_delay_vectorized_add(float* signal, float* h, float* out) { run_delay_host(bf::ALGO_FIR_VEC, signal, out, true, 0, 0.f, h); }

// ---------------------------------------------------------------- hybrid

void load_coefficients_convolve_hybrid(float* delays, int n)
{
    // hybrid_convolve_and_sum.c:161-180
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    if (!delays || n < 1) { set_error("load_coefficients_convolve_hybrid: null or empty table"); return; }
    if (!ensure_device()) return;
    const int T = s.sz.n_taps;
    std::vector<int32_t> w((size_t)n);
    std::vector<float> taps((size_t)n * T);
    parallel_for((size_t)n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            double ip;
            const double fraction = 1.0 - std::modf((double)delays[i], &ip);
            w[i] = (int)ip;
            hybrid_taps(taps.data() + i * T, fraction, T);
        }
    });
    TableSet& t = s.tab[SLOT_HYBRID];
    int mx = 0;
    if (!sanitize_whole(w, s.sz.n_samples, &mx, "load_coefficients_convolve_hybrid")) return;
    if (!upload(t.whole, w.data(), w.size()) || !upload(t.taps, taps.data(), taps.size())) return;
    t.commit(n, mx);
}
void unload_coefficients_convolve_hybrid(void) { std::lock_guard<std::mutex> lock(S().mu); S().tab[SLOT_HYBRID].drop(); }

void mimo_convolve_hybrid(float* signals, float* image, int* adaptive_array, int n) { run_mimo_host(bf::ALGO_HYBRID, SLOT_HYBRID, signals, image, adaptive_array, n); }
void miso_convolve_hybrid(float* signals, float* out, int* adaptive_array, int n, int offset)
{
    std::lock_guard<std::mutex> lock(S().mu);
    run_miso_host(bf::ALGO_HYBRID, S().tab[SLOT_HYBRID], loader_name(SLOT_HYBRID), false, signals, out, adaptive_array, n, offset, nullptr);
}
void convolve_hybrid_delay_add(float* signal, float* h, int pad, float* out) { run_delay_host(bf::ALGO_HYBRID, signal, out, true, pad, 0.f, h); }

int bf_get_hybrid_tables(int* whole, float* taps, int n)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    const TableSet& t = s.tab[SLOT_HYBRID];
    if (!t.loaded || n != t.entries) { set_error("bf_get_hybrid_tables: %d requested, %d loaded", n, t.loaded ? t.entries : 0); return -1; }
    bool ok = HIP_OK(hipMemcpy(whole, t.whole.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    ok = ok && HIP_OK(hipMemcpy(taps, t.taps.p, (size_t)n * s.sz.n_taps * sizeof(float), hipMemcpyDeviceToHost));
    return ok ? 0 : -1;
}

// ---------------------------------------------------------------- api.h shims

void bf_publish_frame(const float* signals)
{
    Entered in;
    const size_t n = (size_t)in.s.sz.n_microphones * in.s.sz.n_samples;
    if (!signals) { set_error("bf_publish_frame: null frame"); return; }
    in.s.published.assign(signals, signals + n);
}

// PC/src/api.c:835-856 zeroes the rows of the 122 microphones that are dead on the authors' arrays (get_data; bf_default_disabled_mics).
static const short kDeadMics[] = {0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30,
    31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64,
    83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 93, 94, 95, 96, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111,
    112, 135, 137, 143, 145, 146, 147, 148, 149, 150, 151, 152, 153, 154, 159, 160, 162, 163, 164, 165, 166, 167, 169, 175,
    184, 192, 193, 194, 195, 196, 197, 198, 199, 200, 201};

static bool copy_published(float* out, bool mask_dead)
{
    State& s = S();
    sizes_from_env_once();
    const size_t n = (size_t)s.sz.n_microphones * s.sz.n_samples;
    if (s.published.size() != n) { set_error("get_data: no frame published (call bf_publish_frame first)"); poison(out, n); return false; }
    std::memcpy(out, s.published.data(), n * sizeof(float));
    if (mask_dead) {
        if (s.disabled_default) {
            s.disabled_mics.assign(kDeadMics, kDeadMics + sizeof(kDeadMics) / sizeof(kDeadMics[0]));
            s.disabled_default = false;
        }
        for (int mic : s.disabled_mics)
            if (mic >= 0 && mic < s.sz.n_microphones) std::memset(out + (size_t)mic * s.sz.n_samples, 0, (size_t)s.sz.n_samples * sizeof(float));
    }
    return true;
}

void get_data(float* signals)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (signals) (void)copy_published(signals, true);
}

// The published frame as the api.h calls take it: get_data's copy, with the dead-microphone mask or (mimo_truncated) without.
// Empty after a refusal.
static std::vector<float> published_frame(bool mask_dead)
{
    std::vector<float> frame((size_t)S().sz.n_microphones * S().sz.n_samples);
    if (!copy_published(frame.data(), mask_dead)) frame.clear();
    return frame;
}

static void shim(int algo, int slot, float* image, int* adaptive_array, int n, bool mask_dead)
{
    std::vector<float> frame;
    {
        Entered in;
        frame = published_frame(mask_dead);
        if (frame.empty()) { poison(image, (size_t)in.s.sz.dirs()); return; }
    }
    run_mimo_host(algo, slot, frame.data(), image, adaptive_array, n);
}

void pad_mimo(float* image, int* adaptive_array, int n) { shim(bf::ALGO_PAD, SLOT_PAD, image, adaptive_array, n, true); }
void lerp_mimo(float* image, int* adaptive_array, int n) { shim(bf::ALGO_LERP, SLOT_LERP, image, adaptive_array, n, true); }
void convolve_mimo_naive(float* image, int* adaptive_array, int n) { shim(bf::ALGO_FIR_NAIVE, SLOT_FIR, image, adaptive_array, n, true); }
void convolve_mimo_vectorized(float* image, int* adaptive_array, int n) { shim(bf::ALGO_FIR_VEC, SLOT_FIR, image, adaptive_array, n, true); }

void load_coefficients2(int* whole_samples, int n) { (void)load_whole_only(SLOT_TRUNC, whole_samples, n, "load_coefficients2"); }
// api.c:1077-1087 copies the ring buffer WITHOUT the dead-microphone mask, then runs the pad algorithm
void mimo_truncated(float* image, int* adaptive_array, int n) { shim(bf::ALGO_PAD, SLOT_TRUNC, image, adaptive_array, n, false); }

void miso_steer_listen(float* out, int* adaptive_array, int n, int steer_offset)
{
    Entered in;
    State& s = in.s;
    std::vector<float> frame = published_frame(true);
    if (frame.empty()) { poison(out, (size_t)s.sz.n_samples); return; }
    run_miso_host(bf::ALGO_PAD, s.tab[SLOT_PAD], loader_name(SLOT_PAD), false, frame.data(), out, adaptive_array, n, steer_offset, nullptr);
}

// ---- api.h:6-9,41-45: process management around the path.  The receiver / playback children are live-hardware I/O and
// out of scope; what these keep is the STATE the path reads (listening offset, listening microphones).

int load(bool replay_mode)
{
    (void)replay_mode;
    std::lock_guard<std::mutex> lock(S().mu);
    set_error("load: the UDP receiver process (PC/src/api.c:874-939) is out of scope of this library; hand frames over with bf_publish_frame");
    return -1;
}

void stop_receiving(void)
{
    std::lock_guard<std::mutex> lock(S().mu);
    S().published.clear();
}

void signal_handler(void) {}

int load_miso(void)
{
    // miso_init_shared_memory (api.c:461-489) + the steer(0) that opens miso_loop (api.c:493): n = 1, adaptive_array all zero
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    s.listen_mics.assign(1, 0);
    s.steer_offset = 0;
    return 0;
}

void load_pa(int* adaptive_array, int n)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    if (!adaptive_array || n < 1) { set_error("load_pa: null or empty adaptive_array"); return; }
    s.listen_mics.assign(adaptive_array, adaptive_array + n);
}

void stop_miso(void)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    s.listen_mics.clear();
    s.steer_offset = 0;
}

void steer(int offset)
{
    std::lock_guard<std::mutex> lock(S().mu);
    S().steer_offset = offset;
}

int bf_get_steer(int* n_out)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (n_out) *n_out = (int)S().listen_mics.size();
    return S().steer_offset;
}

int bf_miso_listen_block(float* out, float mic_gain)
{
    // miso_loop's body (api.c:505-531): get_data; miso_pad(signals, out, adaptive_array, n, steer_offset); out[i] /= n; out[i] *= MIC_GAIN
    Entered in;
    State& s = in.s;
    const size_t N = (size_t)s.sz.n_samples;
    if (!out) { set_error("bf_miso_listen_block: null output"); return -1; }
    if (s.listen_mics.empty()) { set_error("bf_miso_listen_block: load_miso / load_pa has not been called"); poison(out, N); return -1; }
    std::vector<float> frame = published_frame(true);
    if (frame.empty()) { poison(out, N); return -1; }
    const std::string before = s.err;
    s.err.clear();
    std::vector<int> mics = s.listen_mics;     // run_miso_host uploads from a stable copy
    run_miso_host(bf::ALGO_PAD, s.tab[SLOT_PAD], loader_name(SLOT_PAD), false, frame.data(), out, mics.data(), (int)mics.size(), s.steer_offset, nullptr);
    if (!s.err.empty()) return -1;
    s.err = before;
    const float fn = (float)mics.size();
    for (size_t i = 0; i < N; ++i) {
        out[i] /= fn;
        out[i] *= mic_gain;
    }
    return 0;
}

// ---------------------------------------------------------------- device-resident batched path

int bf_das_device(int algo, const float* d_signals, int m_total, float* d_images, int image_stride, int frames,
                  const int* adaptive_array, int n, int dir_begin, int dir_end, void* stream)
{
    Entered in;
    const int slot = slot_of(algo);
    if (slot < 0) { set_error("bf_das_device: unknown algo %d", algo); return -1; }
    if (!d_signals || !d_images || !adaptive_array || frames < 1) { set_error("bf_das_device: null argument or frames < 1"); return -1; }
    if (!ensure_device()) return -1;
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    if (max_row >= m_total) { set_error("bf_das_device: adaptive_array names row %d but frames have %d rows", max_row, m_total); return -1; }
    bf::DasLaunch L{};
    if (!describe(algo, slot, n, &L)) return -1;
    if (!need_dir_range("bf_das_device", dir_begin, dir_end, L.n_dirs, image_stride)) return -1;
    L.signals = d_signals; L.images = d_images; L.m_total = m_total; L.frames = frames;
    L.dir_begin = dir_begin; L.dir_end = dir_end; L.image_stride = image_stride; L.image_origin = dir_begin;
    bf::DasPlan plan{};
    if (!plan_or_error(L, &plan)) return -1;
    if (!ensure_digest(in.s.tab[slot], L, plan, as_stream(stream))) return -1;
    return HIP_RC(bf::launch_das(L, plan, as_stream(stream)));
}

int bf_miso_device(int algo, const float* d_signals, int m_total, int frames, const int* adaptive_array, int n, const int* d_offsets, int beams,
                   float mic_gain, float* d_out, int out_stride, int* d_status, void* stream)
{
    static const char* who = "bf_miso_device";
    Entered in;
    if (algo == bf::ALGO_FIR_NAIVE) { set_error("bf_miso_device: algo BF_FIR_NAIVE has no MISO form in the reference"); return -1; }
    const int slot = slot_of(algo);
    if (slot < 0) { set_error("bf_miso_device: unknown algo %d", algo); return -1; }
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}, {d_offsets, "d_offsets"}, {d_out, "d_out"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "beams", beams, 1) || !need_min(who, "n", n, 1)) return -1;
    if (!need_min(who, "out_stride", out_stride, "N_SAMPLES", in.s.sz.n_samples)) return -1;
    if (!need_rows(who, adaptive_array, n, m_total) || !need_finite(who, "mic_gain", mic_gain)) return -1;
    if (!ensure_device()) return -1;
    const TableSet& t = in.s.tab[slot];
    if (!t.loaded) { set_error("bf_miso_device: %s has not been called", loader_name(slot)); return -1; }
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    bf::DasLaunch L{};
    bf::DasPlan plan{};
    if (!plan_one_beam(algo, t, n, m_total, d_signals, &L, &plan)) return -1;
    L.frames = frames;
    return HIP_RC(bf::launch_miso_batch(L, plan, d_offsets, beams, t.entries, mic_gain, d_out, out_stride, d_status, as_stream(stream)));
}

int bf_remove_sources_device(int algo, const float* d_signals, int m_total, int frames, const int* adaptive_array, int n, const int* d_offsets,
                             int beams, const float* d_beams, int beam_stride, float gain, float* d_residual, int* d_status, void* stream)
{
    static const char* who = "bf_remove_sources_device";
    Entered in;
    State& s = in.s;
    const int N = s.sz.n_samples;
    if (!need_pad_or_lerp(who, algo, true, "has no adjoint here (the subtraction exists for BF_PAD and BF_LERP)")) return -1;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}, {d_offsets, "d_offsets"}, {d_beams, "d_beams"}, {d_residual, "d_residual"}}))
        return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "beams", beams, 1) || !need_max(who, "beams", beams, BF_REMOVE_MAX_BEAMS)) return -1;
    if (!need_min(who, "n", n, 1) || !need_min(who, "beam_stride", beam_stride, "N_SAMPLES", N) || !need_rows(who, adaptive_array, n, m_total)) return -1;
    {
        std::vector<int> sorted(adaptive_array, adaptive_array + n);
        std::sort(sorted.begin(), sorted.end());
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end()) {
            set_error("%s: row %d is listed twice in adaptive_array; which beam sample to subtract from it would be ambiguous", who, *twice);
            return -1;
        }
    }
    if (!need_finite(who, "gain", gain)) return -1;
    if (!ensure_device()) return -1;
    const int slot = slot_of(algo);
    const TableSet& t = s.tab[slot];
    if (!t.loaded) { set_error("%s: %s has not been called", who, loader_name(slot)); return -1; }
    // frame row -> slot of the adaptive array, kept on the device while the array and m_total stay the same
    std::vector<int32_t> row_slot((size_t)m_total, -1);
    for (int i = 0; i < n; ++i) row_slot[(size_t)adaptive_array[i]] = i;
    if (row_slot != s.row_slot_host || !s.d_row_slot.p) {
        // launches already enqueued on the caller's (non-blocking) streams may still read the old copy
        if (s.d_row_slot.p && !HIP_OK(hipDeviceSynchronize())) return -1;
        s.row_slot_host.clear();
        if (!upload(s.d_row_slot, row_slot.data(), row_slot.size())) return -1;
        s.row_slot_host = row_slot;
    }
    const float c = gain / (float)n;
    static_assert(BF_REMOVE_MAX_BEAMS == bf::kRemoveMaxBeams, "the header's limit is the kernel's");
    return HIP_RC(bf::launch_remove_sources(algo, d_signals, d_residual, m_total, frames, N, n, s.d_row_slot.p, t.device(), t.entries, d_offsets, beams, d_beams,
                                            beam_stride, c, d_status, as_stream(stream)));
}

// ---------------------------------------------------------------- continuous-stream mode (pad / lerp)

// What both stream calls check before device bring-up.  `who` names the entry point in the message.
static bool stream_args_ok(const char* who, int algo, int m_total, int frames, int hop, const int* adaptive_array, int n)
{
    if (!need_pad_or_lerp(who, algo, false, "reads ahead of the window's end, which a causal stream cannot supply (continuous mode: BF_PAD, BF_LERP)")) return false;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "hop", hop, 1) || !need_hop_max(who, hop, S().sz.n_samples)) return false;
    return need_min(who, "n", n, 1) && need_rows(who, adaptive_array, n, m_total);
}

// The loaded table's side of the contract: H <= hop, and no entry that the loader had to clamp.
static bool stream_table_ok(const char* who, int algo, const TableSet& t, int slot, int hop)
{
    if (!t.loaded) { set_error("%s: %s has not been called", who, loader_name(slot)); return false; }
    const int H = bf::stream_history(algo, t.max_whole);
    if (H > hop) {
        set_error("%s: the loaded table needs H = %d samples of history but hop = %d (continuous mode wants H <= hop)", who, H, hop);
        return false;
    }
    if (t.clamped > 0) {
        set_error("%s: %d entries of the loaded table lie beyond N_SAMPLES = %d; a stream with hop <= N_SAMPLES cannot reach that far back", who, t.clamped,
                  S().sz.n_samples);
        return false;
    }
    return true;
}

int bf_stream_history(int algo)
{
    State& s = S();
    std::lock_guard<std::mutex> lock(s.mu);
    if (algo != bf::ALGO_PAD && algo != bf::ALGO_LERP) return -1;
    const TableSet& t = s.tab[slot_of(algo)];
    return t.loaded ? bf::stream_history(algo, t.max_whole) : -1;
}

int bf_miso_stream_device(int algo, const float* d_signals, int m_total, int frames, int hop, const float* d_prev, const int* adaptive_array, int n,
                          const int* d_offsets, int beams, float mic_gain, float* d_out, int out_stride, int* d_status, void* stream)
{
    static const char* who = "bf_miso_stream_device";
    Entered in;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}, {d_offsets, "d_offsets"}, {d_out, "d_out"}})) return -1;
    if (!stream_args_ok(who, algo, m_total, frames, hop, adaptive_array, n)) return -1;
    if (!need_min(who, "beams", beams, 1) || !need_min(who, "out_stride", out_stride, "N_SAMPLES", in.s.sz.n_samples)) return -1;
    if (!need_finite(who, "mic_gain", mic_gain)) return -1;
    if (!ensure_device()) return -1;
    const int slot = slot_of(algo);
    const TableSet& t = in.s.tab[slot];
    if (!stream_table_ok(who, algo, t, slot, hop)) return -1;
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    bf::DasLaunch L{};
    bf::DasPlan plan{};
    if (!plan_one_beam(algo, t, n, m_total, d_signals, &L, &plan)) return -1;
    L.frames = frames;
    return STRIDED_RC(STRIDED_STREAM_BEAM, algo, plan,
                      bf::launch_stream_beams(L, plan, d_prev, hop, d_offsets, beams, t.entries, mic_gain, d_out, out_stride, d_status, as_stream(stream)));
}

int bf_das_stream_device(int algo, const float* d_signals, int m_total, float* d_images, int image_stride, int frames, int hop, const float* d_prev,
                         const int* adaptive_array, int n, int dir_begin, int dir_end, void* stream)
{
    static const char* who = "bf_das_stream_device";
    Entered in;
    State& s = in.s;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {d_images, "d_images"}, {adaptive_array, "adaptive_array"}})) return -1;
    if (!stream_args_ok(who, algo, m_total, frames, hop, adaptive_array, n)) return -1;
    if (!need_dir_range(who, dir_begin, dir_end, s.sz.dirs(), image_stride)) return -1;
    if (!ensure_device()) return -1;
    const int slot = slot_of(algo);
    if (!stream_table_ok(who, algo, s.tab[slot], slot, hop)) return -1;
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    bf::DasLaunch L{};
    if (!describe(algo, slot, n, &L)) return -1;
    L.signals = d_signals; L.images = d_images; L.m_total = m_total; L.frames = frames;
    L.dir_begin = dir_begin; L.dir_end = dir_end; L.image_stride = image_stride; L.image_origin = dir_begin;
    bf::DasPlan plan{};
    const char* why = "";
    if (bf::plan_stream_maps(L, s.n_cus, &plan, &why) != 0) { set_error("%s: unsupported shape: %s", who, why); return -1; }
    if (STRIDED_RC(STRIDED_STREAM_MAP, algo, plan, bf::launch_stream_maps(L, plan, d_prev, hop, as_stream(stream))) != 0) return -1;
    s.last_variant = 9; s.last_rows = 0;
    return 0;
}

// ---------------------------------------------------------------- map values at listed directions

// What both select calls check before device bring-up, after their algorithm.
static bool select_args_ok(const char* who, const float* d_signals, int m_total, int frames, const float* d_prev, const int* adaptive_array, int n,
                           const int* d_offsets, int count, int per_frame, const float* d_power, int power_stride, const int* d_status)
{
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}, {d_offsets, "d_offsets"}, {d_power, "d_power"}})) return false;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "count", count, 1) || !need_min(who, "n", n, 1)) return false;
    if (!need_min(who, "power_stride", power_stride, "count", count) || !need_rows(who, adaptive_array, n, m_total)) return false;
    const u64 frame_bytes = sat_mul(sat_mul((u64)m_total, (u64)S().sz.n_samples), sizeof(float));
    const u64 list_bytes = sat_mul(sat_mul((u64)(per_frame ? frames : 1), (u64)count), sizeof(int));
    return need_disjoint(who, {{d_power, sat_mul(sat_mul((u64)frames, (u64)power_stride), sizeof(float)), "d_power"},
                               {d_status, sat_mul(sat_mul((u64)frames, (u64)count), sizeof(int)), "d_status"},
                               {d_signals, sat_mul((u64)frames, frame_bytes), "d_signals"},
                               {d_prev, frame_bytes, "d_prev"},
                               {d_offsets, list_bytes, "d_offsets"}}, 2);
}

// The launch both describe: the list is the direction range, d_power the images.  The adaptive array is already uploaded.
static bool plan_select_launch(const char* who, int algo, const TableSet& t, bool stream_mode, int n, int m_total, int frames, const float* d_signals, int count,
                               float* d_power, int power_stride, bf::DasLaunch* L, bf::DasPlan* plan)
{
    State& s = S();
    *L = bf::DasLaunch{};
    L->algo = algo;
    L->tab = t.device();
    L->n_mics = n; L->m_total = m_total; L->n_samples = s.sz.n_samples; L->n_taps = s.sz.n_taps; L->n_dirs = s.sz.dirs();
    L->dir_begin = 0; L->dir_end = count; L->image_stride = power_stride; L->image_origin = 0; L->frames = frames;
    L->signals = d_signals; L->images = d_power; L->mics = s.d_mics.p;
    const char* why = "";
    if (bf::plan_select(*L, stream_mode, s.n_cus, plan, &why) != 0) { set_error("%s: unsupported shape: %s", who, why); return false; }
    return true;
}

int bf_das_select_device(int algo, const float* d_signals, int m_total, int frames, const int* adaptive_array, int n, const int* d_offsets, int count,
                         int per_frame, float* d_power, int power_stride, int* d_status, void* stream)
{
    static const char* who = "bf_das_select_device";
    Entered in;
    if (algo == bf::ALGO_FIR_NAIVE) { set_error("%s: algo BF_FIR_NAIVE has no MISO form in the reference", who); return -1; }
    const int slot = slot_of(algo);
    if (slot < 0) { set_error("%s: unknown algo %d", who, algo); return -1; }
    if (!select_args_ok(who, d_signals, m_total, frames, nullptr, adaptive_array, n, d_offsets, count, per_frame, d_power, power_stride, d_status)) return -1;
    if (!ensure_device()) return -1;
    const TableSet& t = in.s.tab[slot];
    if (!t.loaded) { set_error("%s: %s has not been called", who, loader_name(slot)); return -1; }
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    bf::DasLaunch L{};
    bf::DasPlan plan{};
    if (!plan_select_launch(who, algo, t, false, n, m_total, frames, d_signals, count, d_power, power_stride, &L, &plan)) return -1;
    return STRIDED_RC(STRIDED_SELECT, algo, plan, bf::launch_select(L, plan, d_offsets, per_frame, t.entries, d_status, as_stream(stream)));
}

int bf_das_select_stream_device(int algo, const float* d_signals, int m_total, int frames, int hop, const float* d_prev, const int* adaptive_array, int n,
                                const int* d_offsets, int count, int per_frame, float* d_power, int power_stride, int* d_status, void* stream)
{
    static const char* who = "bf_das_select_stream_device";
    Entered in;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}})) return -1;
    if (!stream_args_ok(who, algo, m_total, frames, hop, adaptive_array, n)) return -1;
    if (!select_args_ok(who, d_signals, m_total, frames, d_prev, adaptive_array, n, d_offsets, count, per_frame, d_power, power_stride, d_status)) return -1;
    if (!ensure_device()) return -1;
    const int slot = slot_of(algo);
    const TableSet& t = in.s.tab[slot];
    if (!stream_table_ok(who, algo, t, slot, hop)) return -1;
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    bf::DasLaunch L{};
    bf::DasPlan plan{};
    if (!plan_select_launch(who, algo, t, true, n, m_total, frames, d_signals, count, d_power, power_stride, &L, &plan)) return -1;
    return STRIDED_RC(STRIDED_SELECT_HIST, algo, plan,
                      bf::launch_select_stream(L, plan, d_prev, hop, d_offsets, per_frame, t.entries, d_status, as_stream(stream)));
}

int bf_peak_offsets_device(const float* d_power, int frames, int image_stride, int n_dirs, int offset_per_dir, int* d_offsets, void* stream)
{
    static const char* who = "bf_peak_offsets_device";
    Entered in;
    if (!need_ptrs(who, {{d_power, "d_power"}, {d_offsets, "d_offsets"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "n_dirs", n_dirs, 1) || !need_min(who, "offset_per_dir", offset_per_dir, 1)) return -1;
    if (!need_map(who, "n_dirs", n_dirs, offset_per_dir, &image_stride)) return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_peak_offsets(d_power, frames, image_stride, n_dirs, offset_per_dir, d_offsets, as_stream(stream)));
}

int bf_peaks_device(const float* d_power, int frames, int image_stride, int rows, int cols, int radius, int k, float floor_rel, float floor_abs,
                    int offset_per_dir, int* d_offsets, float* d_values, int* d_counts, void* stream)
{
    static const char* who = "bf_peaks_device";
    Entered in;
    State& s = in.s;
    if (!need_ptrs(who, {{d_power, "d_power"}, {d_offsets, "d_offsets"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_map_dims(who, rows, cols, offset_per_dir)) return -1;
    if (!need_min(who, "k", k, 1) || !need_max(who, "k", k, BF_PEAKS_MAX_K) || !need_min(who, "radius", radius, 0)) return -1;
    if (!need_map(who, "rows * cols", (long long)rows * cols, offset_per_dir, &image_stride)) return -1;
    if (!std::isfinite(floor_rel) || floor_rel < 0.0f || floor_rel > 1.0f) { set_error("%s: floor_rel = %g is not in [0, 1]", who, (double)floor_rel); return -1; }
    if (!need_finite(who, "floor_abs", floor_abs)) return -1;
    if (!ensure_device()) return -1;
    const size_t work = bf::peaks_workspace_words(frames, rows, cols, k);
    if (work && !HIP_OK(s.peaks_work.reserve(work))) return -1;
    return HIP_RC(bf::launch_peaks(d_power, frames, image_stride, rows, cols, radius, k, floor_rel, floor_abs, offset_per_dir, d_offsets, d_values, d_counts,
                                   s.peaks_work.p, s.peaks_work.cap, as_stream(stream)));
}

int bf_track_state_words(int slots)
{
    return slots >= 1 && slots <= BF_TRACK_MAX_SLOTS ? 4 + 12 * slots : -1;
}

int bf_track_sources_device(const int* d_offsets, int frames, int k, int rows, int cols, int offset_per_dir, int slots, float gate, int max_miss, int min_hits,
                            float q, float r, void* d_state, int* d_track_offsets, int* d_track_ids, float* d_track_pos, int* d_match, int* d_counts,
                            void* stream)
{
    static const char* who = "bf_track_sources_device";
    static_assert(BF_TRACK_MAX_SLOTS == bf::kTrackMaxSlots, "the header's limit is the kernel's");
    Entered in;
    if (!need_ptrs(who, {{d_offsets, "d_offsets"}, {d_state, "d_state"}, {d_track_offsets, "d_track_offsets"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "k", k, 1) || !need_max(who, "k", k, BF_PEAKS_MAX_K)) return -1;
    if (!need_min(who, "slots", slots, 1) || !need_max(who, "slots", slots, BF_TRACK_MAX_SLOTS)) return -1;
    if (!need_map_dims(who, rows, cols, offset_per_dir) || !need_map(who, "rows * cols", (long long)rows * cols, offset_per_dir, nullptr)) return -1;
    if (!need_finite(who, "gate", gate, FINITE_GE0) || !need_min(who, "max_miss", max_miss, 0) || !need_min(who, "min_hits", min_hits, 1)) return -1;
    if (!need_finite(who, "q", q, FINITE_GE0) || !need_finite(who, "r", r, FINITE_GT0)) return -1;
    if (!ensure_device()) return -1;
    const float gate2 = gate * gate;                 // one float32 multiplication, as the definition says
    return HIP_RC(bf::launch_track_sources(d_offsets, frames, k, rows, cols, offset_per_dir, slots, gate2, max_miss, min_hits, q, r, static_cast<int*>(d_state),
                                           d_track_offsets, d_track_ids, d_track_pos, d_match, d_counts, as_stream(stream)));
}

int bf_fuse_boxes_device(const float* d_power, int frames, int image_stride, int rows, int cols, int offset_per_dir, const float* d_boxes,
                         const int* d_box_counts, int max_boxes, int img_w, int img_h, float conf, const int* d_src_offsets, int n_src, int* d_peak_offsets,
                         float* d_peak_power, int* d_center_offsets, int* d_rects, int* d_src_box, int* d_counts, void* stream)
{
    static const char* who = "bf_fuse_boxes_device";
    static_assert(BF_FUSE_MAX_SOURCES == bf::kFuseMaxSources, "the header's limit is the kernel's");
    static_assert(BF_FUSE_STAGE_MAX == bf::kFuseStageMax, "the header's bound is the kernel's");
    Entered in;
    if (!need_ptrs(who, {{d_power, "d_power"}, {d_boxes, "d_boxes"}, {d_peak_offsets, "d_peak_offsets"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_map_dims(who, rows, cols, offset_per_dir)) return -1;
    if (!need_min(who, "max_boxes", max_boxes, 1) || !need_min(who, "img_w", img_w, 1) || !need_min(who, "img_h", img_h, 1)) return -1;
    if (!need_map(who, "rows * cols", (long long)rows * cols, offset_per_dir, &image_stride)) return -1;
    if (!need_finite(who, "conf", conf) || !need_min(who, "n_src", n_src, 0) || !need_max(who, "n_src", n_src, BF_FUSE_MAX_SOURCES)) return -1;
    if (n_src > 0 && !d_src_offsets) { set_error("%s: d_src_offsets is null with n_src = %d", who, n_src); return -1; }
    if (n_src > 0 && !d_src_box) { set_error("%s: d_src_box is null with n_src = %d", who, n_src); return -1; }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_fuse_boxes(d_power, frames, image_stride, rows, cols, offset_per_dir, d_boxes, d_box_counts, max_boxes, img_w, img_h, conf,
                                        d_src_offsets, n_src, d_peak_offsets, d_peak_power, d_center_offsets, d_rects, d_src_box, d_counts, as_stream(stream)));
}

int bf_box_track_state_words(int slots)
{
    return slots >= 1 && slots <= BF_BOX_TRACK_MAX_SLOTS ? 4 + 20 * slots : -1;
}

int bf_track_boxes_device(const float* d_boxes, const int* d_n_boxes, int frames, int max_boxes, float conf, int slots, float iou_threshold, int max_age,
                          int min_hits, void* d_state, float* d_tracks, int* d_ids, int* d_match, float* d_live, int* d_counts, void* stream)
{
    static const char* who = "bf_track_boxes_device";
    static_assert(BF_BOX_TRACK_MAX_SLOTS == bf::kBoxTrackMaxSlots && BF_BOX_TRACK_MAX_BOXES == bf::kBoxTrackMaxBoxes, "the header's limits are the kernel's");
    Entered in;
    if (!need_ptrs(who, {{d_boxes, "d_boxes"}, {d_state, "d_state"}, {d_tracks, "d_tracks"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "max_boxes", max_boxes, 1) || !need_max(who, "max_boxes", max_boxes, BF_BOX_TRACK_MAX_BOXES)) return -1;
    if (!need_min(who, "slots", slots, 1) || !need_max(who, "slots", slots, BF_BOX_TRACK_MAX_SLOTS) || !need_finite(who, "conf", conf)) return -1;
    if (!std::isfinite(iou_threshold) || iou_threshold < 0.0f || iou_threshold > 1.0f) {
        set_error("%s: iou_threshold = %g is not in [0, 1]", who, (double)iou_threshold);
        return -1;
    }
    if (!need_min(who, "max_age", max_age, 0) || !need_min(who, "min_hits", min_hits, 0)) return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_track_boxes(d_boxes, d_n_boxes, frames, max_boxes, conf, slots, iou_threshold, max_age, min_hits, static_cast<int*>(d_state),
                                         d_tracks, d_ids, d_match, d_live, d_counts, as_stream(stream)));
}

// ---------------------------------------------------------------- boxes followed by the camera image, and the detector's hysteresis

int bf_match_boxes_device(const unsigned char* d_images, const unsigned char* d_prev, int frames, int height, int width, const float* d_boxes, int box_stride,
                          const int* d_n_boxes, int max_boxes, int t_pct, int s_pct, float* d_moved, float* d_score, int* d_shift, int* d_status, void* stream)
{
    static const char* who = "bf_match_boxes_device";
    static_assert(BF_MATCH_MAX_PIXELS == bf::kMatchMaxPixels && BF_MATCH_MAX_BOXES == bf::kMatchMaxBoxes && BF_MATCH_MAX_SIDE == bf::kMatchMaxSide,
                  "the header's limits are the kernel's");
    Entered in;
    if (!need_ptrs(who, {{d_images, "d_images"}, {d_boxes, "d_boxes"}, {d_moved, "d_moved"}, {d_score, "d_score"}, {d_status, "d_status"}})) return -1;
    if (!need_min(who, "frames", frames, 1)) return -1;
    if (!need_min(who, "height", height, 1) || !need_max(who, "height", height, BF_MATCH_MAX_SIDE)) return -1;
    if (!need_min(who, "width", width, 1) || !need_max(who, "width", width, BF_MATCH_MAX_SIDE)) return -1;
    if (!need_min(who, "max_boxes", max_boxes, 1) || !need_max(who, "max_boxes", max_boxes, BF_MATCH_MAX_BOXES) || !need_min(who, "box_stride", box_stride, 4)) return -1;
    if (!need_min(who, "t_pct", t_pct, 100) || !need_min(who, "s_pct", s_pct, "t_pct", t_pct) || !need_max(who, "s_pct", s_pct, 400)) return -1;
    if ((long long)frames * max_boxes > std::numeric_limits<int>::max()) {
        set_error("%s: frames * max_boxes = %lld does not fit an int", who, (long long)frames * max_boxes);
        return -1;
    }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_match_boxes(d_images, d_prev, frames, height, width, d_boxes, box_stride, d_n_boxes, max_boxes, t_pct, s_pct, d_moved, d_score,
                                         d_shift, d_status, as_stream(stream)));
}

int bf_smooth_state_words(int slots)
{
    return slots >= 1 && slots <= BF_SMOOTH_MAX_SLOTS ? 4 + 4 * slots : -1;
}

int bf_smooth_boxes_device(const float* d_boxes, const int* d_n_boxes, int max_boxes, float conf_low, float conf_high, float iou_threshold, float corr_threshold,
                           int slots, const float* d_moved, const float* d_score, const int* d_status, void* d_state, float* d_out, int* d_boosted, int* d_counts,
                           void* stream)
{
    static const char* who = "bf_smooth_boxes_device";
    static_assert(BF_SMOOTH_MAX_SLOTS == bf::kSmoothMaxSlots, "the header's limit is the kernel's");
    Entered in;
    if (!need_ptrs(who, {{d_boxes, "d_boxes"}, {d_moved, "d_moved"}, {d_score, "d_score"}, {d_status, "d_status"}, {d_state, "d_state"}, {d_out, "d_out"}})) return -1;
    if (!need_min(who, "max_boxes", max_boxes, 1) || !need_max(who, "max_boxes", max_boxes, BF_MATCH_MAX_BOXES)) return -1;
    if (!need_min(who, "slots", slots, 1) || !need_max(who, "slots", slots, BF_SMOOTH_MAX_SLOTS)) return -1;
    if (!need_finite(who, "conf_low", conf_low) || !need_finite(who, "conf_high", conf_high) || !need_finite(who, "iou_threshold", iou_threshold) ||
        !need_finite(who, "corr_threshold", corr_threshold))
        return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_smooth_boxes(d_boxes, d_n_boxes, max_boxes, conf_low, conf_high, iou_threshold, corr_threshold, slots, d_moved, d_score, d_status,
                                          static_cast<int*>(d_state), d_out, d_boosted, d_counts, as_stream(stream)));
}

// ---------------------------------------------------------------- band selection on the time-domain path

int bf_band_filter_device(const float* d_signals, int rows, int frames, int hop, const float* d_prev, const float* d_taps, int n_taps, int bands, float* d_out,
                          void* stream)
{
    static const char* who = "bf_band_filter_device";
    static_assert(BF_BAND_MAX_BANDS == bf::kBandMaxBands, "the header's limit is the kernel's");
    Entered in;
    const int N = in.s.sz.n_samples;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {d_taps, "d_taps"}, {d_out, "d_out"}})) return -1;
    if (!need_min(who, "rows", rows, 1) || !need_min(who, "frames", frames, 1) || !need_min(who, "bands", bands, 1) || !need_min(who, "n_taps", n_taps, 1)) return -1;
    if (!need_max(who, "bands", bands, BF_BAND_MAX_BANDS)) return -1;
    if (!need_fir_window(who, n_taps, hop, N, "the filter needs")) return -1;
    const u64 frame_bytes = sat_mul((u64)rows * N, sizeof(float)), in_bytes = sat_mul(frame_bytes, (u64)frames);
    if (!need_disjoint(who, {{d_out, sat_mul(in_bytes, (u64)bands), "d_out"},
                             {d_signals, in_bytes, "d_signals", " (frame f - 1 is read while frame f is written)"},
                             {d_prev, frame_bytes, "d_prev"}}, 1))
        return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_band_filter(d_signals, rows, frames, N, hop, d_prev, d_taps, n_taps, bands, d_out, as_stream(stream)));
}

// ---------------------------------------------------------------- filter-and-sum beams: one FIR per (beam, microphone)

int bf_filter_sum_device(const float* d_signals, int m_total, int frames, int hop, const float* d_prev, const int* adaptive_array, int n, const float* d_taps,
                         int n_taps, int beams, float* d_out, int out_stride, void* stream)
{
    static const char* who = "bf_filter_sum_device";
    static_assert(BF_FILTER_SUM_MAX_BEAMS == bf::kFilterSumMaxBeams, "the header's limit is the kernel's");
    Entered in;
    const int N = in.s.sz.n_samples;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}, {d_taps, "d_taps"}, {d_out, "d_out"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "n", n, 1) || !need_min(who, "beams", beams, 1) || !need_min(who, "n_taps", n_taps, 1)) return -1;
    if (!need_max(who, "beams", beams, BF_FILTER_SUM_MAX_BEAMS)) return -1;
    if (!need_fir_window(who, n_taps, hop, N, "the filters need")) return -1;
    if (!need_min(who, "out_stride", out_stride, "N_SAMPLES", N) || !need_rows(who, adaptive_array, n, m_total)) return -1;
    // d_out's span runs from its first float to the last one written: the floats behind the last row's N_SAMPLES are not part of it
    const u64 frame_bytes = sat_mul((u64)m_total * N, sizeof(float)), out_rows = (u64)frames * beams;
    if (!need_disjoint(who, {{d_out, sat_add(sat_mul(sat_mul(out_rows - 1, (u64)out_stride), sizeof(float)), N * sizeof(float)), "d_out"},
                             {d_signals, sat_mul(frame_bytes, (u64)frames), "d_signals"},
                             {d_prev, frame_bytes, "d_prev"},
                             {d_taps, sat_mul(sat_mul((u64)beams * n, (u64)n_taps), sizeof(float)), "d_taps"}}, 1))
        return -1;
    if (!ensure_device()) return -1;
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    return HIP_RC(bf::launch_filter_sum(d_signals, m_total, frames, N, hop, d_prev, in.s.d_mics.p, n, d_taps, n_taps, beams, d_out, out_stride, in.s.n_cus,
                                        as_stream(stream)));
}

int bf_filter_sum_waves(int waves) { return bf::filter_sum_waves(waves); }

// ---------------------------------------------------------------- null-steering taps designed on the device

int bf_lcmv_design_device(const double* d_tau, int dirs, int n, const int* d_offsets, int sources, int offset_per_dir, int n_taps, int bin_lo, int bin_hi, double rho,
                          double* d_gains, float* d_taps, int* d_kept, int* d_status, void* stream)
{
    static const char* who = "bf_lcmv_design_device";
    static_assert(BF_LCMV_MAX_SOURCES == bf::kLcmvMaxSources && BF_LCMV_MAX_TAPS == bf::kLcmvMaxTaps, "the header's limits are the kernels'");
    Entered in;
    if (!need_ptrs(who, {{d_tau, "d_tau"}, {d_offsets, "d_offsets"}, {d_gains, "d_gains"}, {d_taps, "d_taps"}, {d_kept, "d_kept"}, {d_status, "d_status"}})) return -1;
    if (!need_min(who, "dirs", dirs, 1) || !need_min(who, "n", n, 1) || !need_min(who, "sources", sources, 1) ||
        !need_min(who, "offset_per_dir", offset_per_dir, 1) || !need_min(who, "n_taps", n_taps, 1))
        return -1;
    if (!need_max(who, "sources", sources, BF_LCMV_MAX_SOURCES)) return -1;
    if (sources > n) {
        set_error("%s: sources = %d > n = %d (more constraints than microphones make the system singular)", who, sources, n);
        return -1;
    }
    if (!need_max(who, "n_taps", n_taps, BF_LCMV_MAX_TAPS)) return -1;
    if (!need_bins(who, bin_lo, bin_hi, n_taps)) return -1;
    if (!(rho > 0.0 && rho <= 1.0)) { set_error("%s: rho = %.17g is not in (0, 1]", who, rho); return -1; }
    const u64 S = (u64)sources, K = (u64)(bin_hi - bin_lo + 1);
    if (!need_disjoint(who, {{d_gains, sat_mul(sat_mul(S * K, (u64)n), 2 * sizeof(double)), "d_gains"},
                             {d_taps, sat_mul(sat_mul(S * (u64)n_taps, (u64)n), sizeof(float)), "d_taps"},
                             {d_kept, S * K * S * sizeof(int), "d_kept"},
                             {d_status, S * sizeof(int), "d_status"},
                             {d_tau, sat_mul(sat_mul((u64)dirs, (u64)n), sizeof(double)), "d_tau"},
                             {d_offsets, S * sizeof(int), "d_offsets"}}, 4))   // four outputs, two inputs
        return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_lcmv_design(d_tau, dirs, n, d_offsets, sources, offset_per_dir, n_taps, bin_lo, bin_hi, rho, d_gains, d_taps, d_kept, d_status,
                                         as_stream(stream)));
}

// ---------------------------------------------------------------- adaptive (MVDR) taps designed on the device from the frames' covariance

int bf_mvdr_design_device(const float* d_signals, int m_total, int frames, const int* adaptive_array, int n, int seg_first, int seg_hop, int segs,
                          const double* d_window, const double* d_tau, int dirs, const int* d_offsets, int sources, int offset_per_dir, int n_taps, int bin_lo,
                          int bin_hi, double loading, double* d_snap, double* d_cov, double* d_chol, double* d_gains, float* d_taps, int* d_status,
                          int* d_fallback, void* stream)
{
    static const char* who = "bf_mvdr_design_device";
    static_assert(BF_MVDR_MAX_MICS == bf::kMvdrMaxMics, "the header's limit is the kernels'");
    Entered in;
    const int N = in.s.sz.n_samples;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}, {d_tau, "d_tau"}, {d_offsets, "d_offsets"}, {d_snap, "d_snap"},
                         {d_cov, "d_cov"}, {d_chol, "d_chol"}, {d_gains, "d_gains"}, {d_taps, "d_taps"}, {d_status, "d_status"}, {d_fallback, "d_fallback"}}))
        return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "n", n, 1) || !need_min(who, "segs", segs, 1) || !need_min(who, "seg_hop", seg_hop, 1) ||
        !need_min(who, "dirs", dirs, 1) || !need_min(who, "sources", sources, 1) || !need_min(who, "offset_per_dir", offset_per_dir, 1) ||
        !need_min(who, "n_taps", n_taps, 1) || !need_min(who, "seg_first", seg_first, 0))
        return -1;
    if (!need_max(who, "n", n, BF_MVDR_MAX_MICS) || !need_max(who, "sources", sources, BF_LCMV_MAX_SOURCES) || !need_max(who, "n_taps", n_taps, BF_LCMV_MAX_TAPS))
        return -1;
    {
        const long long last = (long long)seg_first + (long long)(segs - 1) * seg_hop + n_taps;
        if (last > N) {
            set_error("%s: seg_first + (segs - 1) * seg_hop + n_taps = %lld > N_SAMPLES = %d (a segment would leave its window)", who, last, N);
            return -1;
        }
    }
    if (!need_bins(who, bin_lo, bin_hi, n_taps)) return -1;
    if (!std::isfinite(loading) || !(loading > 0.0)) { set_error("%s: loading = %.17g is not finite and > 0", who, loading); return -1; }
    if (!need_rows(who, adaptive_array, n, m_total)) return -1;
    const u64 S = (u64)sources, K = (u64)(bin_hi - bin_lo + 1), M = (u64)n, P = (u64)frames * (u64)segs, cplx = 2 * sizeof(double);
    if (!need_disjoint(who, {{d_snap, sat_mul(sat_mul(sat_mul(P, K), M), cplx), "d_snap"},
                             {d_cov, sat_mul(K * M * M, cplx), "d_cov"},
                             {d_chol, sat_mul(K * M * M, cplx), "d_chol"},
                             {d_gains, sat_mul(S * K * M, cplx), "d_gains"},
                             {d_taps, sat_mul(S * (u64)n_taps * M, sizeof(float)), "d_taps"},
                             {d_status, S * sizeof(int), "d_status"},
                             {d_fallback, K * sizeof(int), "d_fallback"},
                             {d_signals, sat_mul(sat_mul(sat_mul((u64)frames, (u64)m_total), (u64)N), sizeof(float)), "d_signals"},
                             {d_tau, sat_mul(sat_mul((u64)dirs, M), sizeof(double)), "d_tau"},
                             {d_offsets, S * sizeof(int), "d_offsets"},
                             {d_window, (u64)n_taps * sizeof(double), "d_window"}}, 7))   // seven outputs, four inputs (d_window only where given)
        return -1;
    if (!ensure_device()) return -1;
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    return HIP_RC(bf::launch_mvdr_design(d_signals, m_total, frames, N, in.s.d_mics.p, n, seg_first, seg_hop, segs, d_window, d_tau, dirs, d_offsets, sources,
                                         offset_per_dir, n_taps, bin_lo, bin_hi, loading, d_snap, d_cov, d_chol, d_gains, d_taps, d_status, d_fallback,
                                         as_stream(stream)));
}

// ---------------------------------------------------------------- the same taps from a covariance that is carried, weighted and forgotten

int bf_mvdr_learn_device(const float* d_signals, int m_total, int frames, const int* adaptive_array, int n, int seg_first, int seg_hop, int segs,
                         const double* d_window, const double* d_weights, double forget, const double* d_tau, int dirs, const int* d_offsets, int sources,
                         int offset_per_dir, int n_taps, int bin_lo, int bin_hi, double loading, double* d_acc, double* d_mass, int* d_used, double* d_snap,
                         double* d_cov, double* d_chol, double* d_gains, float* d_taps, int* d_status, int* d_fallback, void* stream)
{
    static const char* who = "bf_mvdr_learn_device";
    Entered in;
    const int N = in.s.sz.n_samples;
    if (!need_ptrs(who, {{adaptive_array, "adaptive_array"}, {d_tau, "d_tau"}, {d_offsets, "d_offsets"}, {d_acc, "d_acc"}, {d_mass, "d_mass"}, {d_used, "d_used"},
                         {d_cov, "d_cov"}, {d_chol, "d_chol"}, {d_gains, "d_gains"}, {d_taps, "d_taps"}, {d_status, "d_status"}, {d_fallback, "d_fallback"}}))
        return -1;
    if (!need_min(who, "frames", frames, 0)) return -1;
    if (frames > 0 && !need_ptrs(who, {{d_signals, "d_signals"}, {d_snap, "d_snap"}})) return -1;   // (frames == 0, the re-aim, reads no frame and writes no snapshot)
    if (!need_min(who, "n", n, 1) || !need_min(who, "segs", segs, 1) || !need_min(who, "seg_hop", seg_hop, 1) || !need_min(who, "dirs", dirs, 1) ||
        !need_min(who, "sources", sources, 1) || !need_min(who, "offset_per_dir", offset_per_dir, 1) || !need_min(who, "n_taps", n_taps, 1) ||
        !need_min(who, "seg_first", seg_first, 0))
        return -1;
    if (!need_max(who, "n", n, BF_MVDR_MAX_MICS) || !need_max(who, "sources", sources, BF_LCMV_MAX_SOURCES) || !need_max(who, "n_taps", n_taps, BF_LCMV_MAX_TAPS))
        return -1;
    {
        const long long last = (long long)seg_first + (long long)(segs - 1) * seg_hop + n_taps;
        if (last > N) {
            set_error("%s: seg_first + (segs - 1) * seg_hop + n_taps = %lld > N_SAMPLES = %d (a segment would leave its window)", who, last, N);
            return -1;
        }
    }
    if (!need_bins(who, bin_lo, bin_hi, n_taps)) return -1;
    if (!std::isfinite(loading) || !(loading > 0.0)) { set_error("%s: loading = %.17g is not finite and > 0", who, loading); return -1; }
    if (!(forget > 0.0 && forget <= 1.0)) { set_error("%s: forget = %.17g is not in (0, 1]", who, forget); return -1; }
    if (!need_rows(who, adaptive_array, n, m_total)) return -1;
    const bool learns = frames > 0;
    const u64 S = (u64)sources, K = (u64)(bin_hi - bin_lo + 1), M = (u64)n, P = (u64)frames * (u64)segs, cplx = 2 * sizeof(double);
    if (!need_disjoint(who, {{d_acc, sat_mul(K * M * M, cplx), "d_acc"},
                             {d_mass, sizeof(double), "d_mass"},
                             {d_used, 2 * sizeof(int), "d_used"},
                             {learns ? d_snap : nullptr, sat_mul(sat_mul(sat_mul(P, K), M), cplx), "d_snap"},
                             {d_cov, sat_mul(K * M * M, cplx), "d_cov"},
                             {d_chol, sat_mul(K * M * M, cplx), "d_chol"},
                             {d_gains, sat_mul(S * K * M, cplx), "d_gains"},
                             {d_taps, sat_mul(S * (u64)n_taps * M, sizeof(float)), "d_taps"},
                             {d_status, S * sizeof(int), "d_status"},
                             {d_fallback, K * sizeof(int), "d_fallback"},
                             {learns ? d_signals : nullptr, sat_mul(sat_mul(sat_mul((u64)frames, (u64)m_total), (u64)N), sizeof(float)), "d_signals"},
                             {d_tau, sat_mul(sat_mul((u64)dirs, M), sizeof(double)), "d_tau"},
                             {d_offsets, S * sizeof(int), "d_offsets"},
                             {learns ? d_window : nullptr, (u64)n_taps * sizeof(double), "d_window"},
                             {learns ? d_weights : nullptr, (u64)frames * sizeof(double), "d_weights"}}, 10))   // ten outputs (the state among them), five inputs
        return -1;
    if (!ensure_device()) return -1;
    int max_row = 0;
    if (learns && !upload_mics(adaptive_array, n, &max_row)) return -1;
    return HIP_RC(bf::launch_mvdr_learn(d_signals, m_total, frames, N, in.s.d_mics.p, n, seg_first, seg_hop, segs, d_window, d_weights, forget, d_tau, dirs, d_offsets,
                                        sources, offset_per_dir, n_taps, bin_lo, bin_hi, loading, d_acc, d_mass, d_used, d_snap, d_cov, d_chol, d_gains, d_taps,
                                        d_status, d_fallback, as_stream(stream)));
}

// ---------------------------------------------------------------- the output stage: beams at a sound card's rate

long long bf_resample_capacity(long long samples_in, int up, int down) { return bf::resample_capacity(samples_in, up, down); }

int bf_resample_device(const float* d_in, int rows, int frames, int n, int in_stride, int hop, const float* d_prev, const float* d_taps, int up, int down, int n_taps,
                       int* d_state, float gain, float* d_out, int out_stride, short* d_pcm, int* d_clip, int* d_count, void* stream)
{
    static const char* who = "bf_resample_device";
    static_assert(BF_RESAMPLE_MAX_PHASES == bf::kResampleMaxPhases && BF_RESAMPLE_MAX_TAPS == bf::kResampleMaxTaps, "the header's limits are the kernel's");
    constexpr int kMaxTable = 1 << 20;
    Entered in;
    if (!need_ptrs(who, {{d_in, "d_in"}, {d_taps, "d_taps"}, {d_state, "d_state"}, {d_count, "d_count"}})) return -1;
    if (!d_out && !d_pcm) { set_error("%s: d_out and d_pcm are both null", who); return -1; }
    if (!need_min(who, "rows", rows, 1) || !need_min(who, "frames", frames, 1) || !need_min(who, "n", n, 1) || !need_min(who, "up", up, 1) ||
        !need_min(who, "down", down, 1) || !need_min(who, "n_taps", n_taps, 1))
        return -1;
    if (!need_max(who, "up", up, BF_RESAMPLE_MAX_PHASES) || !need_max(who, "n_taps", n_taps, BF_RESAMPLE_MAX_TAPS)) return -1;
    if (up * n_taps > kMaxTable) { set_error("%s: up * n_taps = %d > %d", who, up * n_taps, kMaxTable); return -1; }
    if (down > 64LL * up) { set_error("%s: down = %d > 64 * up = %d", who, down, 64 * up); return -1; }
    if (!need_min(who, "hop", hop, 0) || !need_hop_max(who, hop, n, "n") || !need_min(who, "in_stride", in_stride, "n", n)) return -1;
    const bf::StreamLen sl = bf::stream_len(frames, hop, n);
    const long long S = sl.S;
    if (n_taps - 1 > sl.len) {
        set_error("%s: the filter needs n_taps - 1 = %d samples of history but a window adds %d to the stream (the history must be stream samples)", who,
                  n_taps - 1, sl.len);
        return -1;
    }
    if (!need_stream_len(who, sl, hop, "n")) return -1;
    const long long cap = bf::resample_capacity(S, up, down);
    if (cap > std::numeric_limits<int>::max()) { set_error("%s: cap = %lld does not fit an int", who, cap); return -1; }
    if (d_out && !need_min(who, "out_stride", out_stride, "cap", (int)cap)) return -1;
    if (!need_finite(who, "gain", gain)) return -1;
    // every span runs from its first element to the last one touched: the floats behind a last row's n (or cap) are not part of it
    const u64 in_rows = (u64)frames * rows;
    if (!need_disjoint(who, {{d_out, sat_add(sat_mul(sat_mul((u64)rows - 1, (u64)out_stride), sizeof(float)), (u64)cap * sizeof(float)), "d_out"},
                             {d_pcm, sat_mul((u64)cap * rows, sizeof(short)), "d_pcm"},
                             {d_clip, (u64)rows * sizeof(int), "d_clip"},
                             {d_state, 4 * sizeof(int), "d_state"},
                             {d_count, 2 * sizeof(int), "d_count"},
                             {d_in, sat_add(sat_mul(sat_mul(in_rows - 1, (u64)in_stride), sizeof(float)), (u64)n * sizeof(float)), "d_in"},
                             {d_prev, sat_add(sat_mul(sat_mul((u64)rows - 1, (u64)in_stride), sizeof(float)), (u64)n * sizeof(float)), "d_prev"},
                             {d_taps, (u64)up * n_taps * sizeof(float), "d_taps"}}, 5))   // five written ranges (the state and the meter among them), three read
        return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_resample(d_in, rows, frames, n, in_stride, hop, d_prev, d_taps, up, down, n_taps, d_state, gain, d_out, out_stride, d_pcm, d_clip,
                                      d_count, as_stream(stream)));
}

// ---------------------------------------------------------------- spectral frames of beam audio

long long bf_spectrogram_capacity(long long len, int hop_s) { return bf::spectrogram_capacity(len, hop_s); }

int bf_spectrogram_device(const float* d_in, int rows, int in_stride, int len, const int* d_len, float* d_hist, int* d_state, const float* d_window, int n_win,
                          int n_fft, int hop_s, const float* d_bank, const int* d_support, int n_bands, float scale, float floor_, float* d_out, int out_frames,
                          int* d_count, void* stream)
{
    static const char* who = "bf_spectrogram_device";
    static_assert(BF_SPECTROGRAM_MAX_BANDS == bf::kSpectrogramMaxBands, "the header's limit is the kernel's");
    Entered in;
    if (!need_ptrs(who, {{d_in, "d_in"}, {d_hist, "d_hist"}, {d_state, "d_state"}, {d_window, "d_window"}, {d_out, "d_out"}, {d_count, "d_count"}})) return -1;
    if (!need_min(who, "rows", rows, 1) || !need_min(who, "len", len, 0) || !need_min(who, "in_stride", in_stride, "len", len)) return -1;
    if (!need_pow2(who, "n_fft", n_fft, bf::kSpectrogramMinFft, bf::kSpectrogramMaxFft)) return -1;
    if (!need_min(who, "n_win", n_win, 1)) return -1;
    if (n_win > n_fft) { set_error("%s: n_win = %d > n_fft = %d", who, n_win, n_fft); return -1; }
    if (!need_min(who, "hop_s", hop_s, 1) || !need_min(who, "n_bands", n_bands, 1) || !need_max(who, "n_bands", n_bands, BF_SPECTROGRAM_MAX_BANDS)) return -1;
    const int n_bins = n_fft / 2 + 1;
    if (!d_bank && n_bands != n_bins) {
        set_error("%s: d_bank is null (the power spectrum) but n_bands = %d != n_fft / 2 + 1 = %d", who, n_bands, n_bins);
        return -1;
    }
    const long long cap = bf::spectrogram_capacity(len, hop_s);     // (<= len: it fits an int)
    if (!need_min(who, "out_frames", out_frames, "cap", (int)cap)) return -1;
    if (!need_finite(who, "scale", scale)) return -1;
    if (scale != 0.0f && !need_finite(who, "floor_", floor_, FINITE_GT0)) return -1;
    // every span runs from its first element to the last one touched
    const u64 out_slots = sat_add(sat_mul((u64)rows - 1, (u64)out_frames), (u64)cap);
    if (!need_disjoint(who, {{d_out, sat_mul(sat_mul(out_slots, (u64)n_bands), sizeof(float)), "d_out"},
                             {d_hist, sat_mul(sat_mul((u64)rows, (u64)(n_win - 1)), sizeof(float)), "d_hist"},
                             {d_state, 4 * sizeof(int), "d_state"},
                             {d_count, 2 * sizeof(int), "d_count"},
                             {d_in, sat_add(sat_mul(sat_mul((u64)rows - 1, (u64)in_stride), sizeof(float)), (u64)len * sizeof(float)), "d_in"},
                             {d_len, sizeof(int), "d_len"},
                             {d_window, (u64)n_win * sizeof(float), "d_window"},
                             {d_bank, (u64)n_bands * n_bins * sizeof(float), "d_bank"},
                             {d_support, (u64)n_bands * 2 * sizeof(int), "d_support"}}, 4))   // four written ranges (history and state among them), five read
        return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_spectrogram(d_in, rows, in_stride, len, d_len, d_hist, d_state, d_window, n_win, n_fft, hop_s, d_bank, d_support, n_bands, scale,
                                         floor_, d_out, out_frames, d_count, as_stream(stream)));
}

// ---------------------------------------------------------------- noise suppression of beam audio: STFT analysis, gains, overlap-add synthesis

long long bf_enhance_workspace(int rows, long long samples, int n_fft, int hop_s) { return bf::enhance_workspace(rows, samples, n_fft, hop_s); }

int bf_enhance_device(const float* d_in, int rows, int frames, int n, int in_stride, int hop, float* d_hist, float* d_ola, float* d_noise, float* d_prior,
                      int* d_state, const float* d_win_a, const float* d_win_s, int n_fft, int hop_s, const float* d_gain_in, float alpha, float a_noise, float g0,
                      float g1, float g_min, int n_init, float* d_work, float* d_out, int out_stride, float* d_power_out, float* d_gain_out, int* d_count,
                      void* stream)
{
    static const char* who = "bf_enhance_device";
    Entered in;
    if (!need_ptrs(who, {{d_in, "d_in"}, {d_hist, "d_hist"}, {d_ola, "d_ola"}, {d_state, "d_state"}, {d_win_a, "d_win_a"}, {d_win_s, "d_win_s"},
                         {d_work, "d_work"}, {d_out, "d_out"}, {d_count, "d_count"}}))
        return -1;
    const bool tracks = d_gain_in == nullptr;
    if (tracks && !need_ptrs(who, {{d_noise, "d_noise"}, {d_prior, "d_prior"}})) return -1;
    if (!need_min(who, "rows", rows, 1) || !need_min(who, "frames", frames, 1) || !need_min(who, "n", n, 1)) return -1;
    if (!need_min(who, "hop", hop, 0) || !need_hop_max(who, hop, n, "n") || !need_min(who, "in_stride", in_stride, "n", n)) return -1;
    const bf::StreamLen sl = bf::stream_len(frames, hop, n);
    const long long S = sl.S;
    if (!need_frame_grid(who, n_fft, hop_s) || !need_stream_len(who, sl, hop, "n")) return -1;
    if (!need_min(who, "out_stride", out_stride, "S", (int)S)) return -1;
    if (tracks) {
        if (!need_finite(who, "alpha", alpha, FINITE_GE0) || !need_finite(who, "a_noise", a_noise, FINITE_GE0) || !need_finite(who, "g0", g0, FINITE_GE0) ||
            !need_finite(who, "g1", g1) || !need_finite(who, "g_min", g_min, FINITE_GE0))
            return -1;
        if (alpha >= 1.0f) { set_error("%s: alpha = %g >= 1", who, (double)alpha); return -1; }
        if (a_noise >= 1.0f) { set_error("%s: a_noise = %g >= 1", who, (double)a_noise); return -1; }
        if (g1 <= g0) { set_error("%s: g1 = %g <= g0 = %g", who, (double)g1, (double)g0); return -1; }
        if (g_min > 1.0f) { set_error("%s: g_min = %g > 1", who, (double)g_min); return -1; }
        if (!need_min(who, "n_init", n_init, 1)) return -1;
    }
    const long long work = bf::enhance_workspace(rows, S, n_fft, hop_s);
    if (work < 0) { set_error("%s: no workspace for rows = %d, S = %lld, n_fft = %d, hop_s = %d", who, rows, S, n_fft, hop_s); return -1; }
    // every span runs from its first element to the last one touched
    const u64 n_bins = (u64)n_fft / 2 + 1, cap = (u64)bf::frame_cap(S, hop_s);
    const u64 cells = sat_mul(sat_mul(sat_mul((u64)rows, cap), n_bins), sizeof(float)), per_bin = (u64)rows * n_bins * sizeof(float);
    if (!need_disjoint(who, {{d_out, sat_add(sat_mul(sat_mul((u64)rows - 1, (u64)out_stride), sizeof(float)), (u64)S * sizeof(float)), "d_out"},
                             {d_work, sat_mul((u64)work, sizeof(float)), "d_work"},
                             {d_power_out, cells, "d_power_out"},
                             {d_gain_out, cells, "d_gain_out"},
                             {d_hist, (u64)rows * (n_fft - 1) * sizeof(float), "d_hist"},
                             {d_ola, (u64)rows * n_fft * sizeof(float), "d_ola"},
                             {tracks ? d_noise : nullptr, per_bin, "d_noise"},
                             {tracks ? d_prior : nullptr, per_bin, "d_prior"},
                             {d_state, 4 * sizeof(int), "d_state"},
                             {d_count, 2 * sizeof(int), "d_count"},
                             {d_in, sat_add(sat_mul(sat_mul((u64)frames * rows - 1, (u64)in_stride), sizeof(float)), (u64)n * sizeof(float)), "d_in"},
                             {d_win_a, (u64)n_fft * sizeof(float), "d_win_a"},
                             {d_win_s, (u64)n_fft * sizeof(float), "d_win_s"},
                             {d_gain_in, cells, "d_gain_in"}}, 10))   // ten written ranges (the carried state among them), four read
        return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_enhance(d_in, rows, frames, n, in_stride, hop, d_hist, d_ola, d_noise, d_prior, d_state, d_win_a, d_win_s, n_fft, hop_s, d_gain_in, alpha,
                                     a_noise, g0, g1, g_min, n_init, d_work, d_out, out_stride, d_power_out, d_gain_out, d_count, as_stream(stream)));
}

// ---------------------------------------------------------------- multichannel post-filter gains: the microphones' coherence behind the steering

long long bf_postfilter_workspace(int slots, long long samples, int n_fft, int hop_s) { return bf::postfilter_workspace(slots, samples, n_fft, hop_s); }

int bf_postfilter_device(const float* d_signals, int m_total, int frames, int n_samples, int hop, const int* adaptive_array, int n, const double* d_tau, int dirs,
                         const int* d_offsets, int slots, int offset_per_dir, float* d_hist, float* d_num, float* d_den, int* d_state, const float* d_window,
                         int n_fft, int hop_s, int lag, int den_mode, float beta, float g_min, float* d_work, float* d_steer, float* d_gains, float* d_num_out,
                         float* d_den_out, int* d_status, int* d_count, void* stream)
{
    static const char* who = "bf_postfilter_device";
    static_assert(BF_POSTFILTER_MAX_SLOTS == bf::kPostfilterMaxSlots && BF_POSTFILTER_MAX_SLOTS == BF_LCMV_MAX_SOURCES, "the header's limit is the kernel's");
    Entered in;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {adaptive_array, "adaptive_array"}, {d_tau, "d_tau"}, {d_offsets, "d_offsets"}, {d_hist, "d_hist"},
                         {d_num, "d_num"}, {d_den, "d_den"}, {d_state, "d_state"}, {d_window, "d_window"}, {d_work, "d_work"}, {d_steer, "d_steer"},
                         {d_gains, "d_gains"}, {d_status, "d_status"}, {d_count, "d_count"}}))
        return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "n_samples", n_samples, 1)) return -1;
    if (!need_min(who, "hop", hop, 0) || !need_hop_max(who, hop, n_samples, "n_samples")) return -1;
    if (!need_min(who, "n", n, 2) || !need_max(who, "n", n, BF_MVDR_MAX_MICS) || !need_rows(who, adaptive_array, n, m_total)) return -1;
    if (!need_min(who, "slots", slots, 1) || !need_max(who, "slots", slots, BF_POSTFILTER_MAX_SLOTS)) return -1;
    if (!need_min(who, "dirs", dirs, 1) || !need_min(who, "offset_per_dir", offset_per_dir, 1)) return -1;
    if (!need_frame_grid(who, n_fft, hop_s)) return -1;
    if (!need_min(who, "lag", lag, 0) || !need_max(who, "lag", lag, n_fft)) return -1;
    if (den_mode != 0 && den_mode != 1) { set_error("%s: den_mode = %d is not 0 (the microphones' mean power) or 1 (the beam's power)", who, den_mode); return -1; }
    if (!need_finite(who, "beta", beta, FINITE_GE0) || !need_finite(who, "g_min", g_min, FINITE_GE0)) return -1;
    if (beta >= 1.0f) { set_error("%s: beta = %g >= 1", who, (double)beta); return -1; }
    if (g_min > 1.0f) { set_error("%s: g_min = %g > 1", who, (double)g_min); return -1; }
    const bf::StreamLen sl = bf::stream_len(frames, hop, n_samples);
    const long long S = sl.S;
    if (!need_stream_len(who, sl, hop, "n_samples")) return -1;
    const long long work = bf::postfilter_workspace(slots, S, n_fft, hop_s);
    if (work < 0) { set_error("%s: no workspace for slots = %d, S = %lld, n_fft = %d, hop_s = %d", who, slots, S, n_fft, hop_s); return -1; }
    // every span runs from its first element to the last one touched
    const u64 n_bins = (u64)n_fft / 2 + 1, cap = (u64)bf::frame_cap(S, hop_s), H = (u64)n_fft - 1 + lag;
    const u64 cells = sat_mul(sat_mul((u64)slots * cap, n_bins), sizeof(float)), per_bin = (u64)slots * n_bins * sizeof(float);
    if (!need_disjoint(who, {{d_gains, cells, "d_gains"},
                             {d_num_out, cells, "d_num_out"},
                             {d_den_out, cells, "d_den_out"},
                             {d_steer, (u64)slots * n * n_bins * 2 * sizeof(float), "d_steer"},
                             {d_work, sat_mul((u64)work, sizeof(float)), "d_work"},
                             {d_status, (u64)slots * sizeof(int), "d_status"},
                             {d_count, 2 * sizeof(int), "d_count"},
                             {d_hist, (u64)n * H * sizeof(float), "d_hist"},
                             {d_num, per_bin, "d_num"},
                             {d_den, per_bin, "d_den"},
                             {d_state, (2 + (u64)slots) * sizeof(int), "d_state"},
                             {d_signals, sat_mul(sat_mul(sat_mul((u64)frames, (u64)m_total), (u64)n_samples), sizeof(float)), "d_signals"},
                             {d_tau, sat_mul(sat_mul((u64)dirs, (u64)n), sizeof(double)), "d_tau"},
                             {d_offsets, (u64)slots * sizeof(int), "d_offsets"},
                             {d_window, (u64)n_fft * sizeof(float), "d_window"}}, 11))   // eleven written ranges (the carried state among them), four read
        return -1;
    if (!ensure_device()) return -1;
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    return HIP_RC(bf::launch_postfilter(d_signals, m_total, frames, n_samples, hop, in.s.d_mics.p, n, d_tau, dirs, d_offsets, slots, offset_per_dir, d_hist, d_num,
                                        d_den, d_state, d_window, n_fft, hop_s, lag, den_mode, beta, g_min, d_work, d_steer, d_gains, d_num_out, d_den_out, d_status,
                                        d_count, as_stream(stream)));
}

// ---------------------------------------------------------------- phase-transform (PHAT) frames: every in-band bin weighted by |X_k|^-beta

int bf_whiten_device(const float* d_signals, int rows, int frames, const float* d_window, const int* bins, const float* beta, const float* gain, int bands,
                     float floor_rel, float floor_abs, float* d_out, void* stream)
{
    static const char* who = "bf_whiten_device";
    static_assert(BF_WHITEN_MAX_BANDS == bf::kWhitenMaxBands, "the header's limit is the kernel's");
    Entered in;
    const int N = in.s.sz.n_samples;
    if (!need_ptrs(who, {{d_signals, "d_signals"}, {bins, "bins"}, {beta, "beta"}, {gain, "gain"}, {d_out, "d_out"}})) return -1;
    if (!need_min(who, "rows", rows, 1) || !need_min(who, "frames", frames, 1) || !need_min(who, "bands", bands, 1)) return -1;
    if (!need_max(who, "bands", bands, BF_WHITEN_MAX_BANDS)) return -1;
    if (!need_pow2(who, "N_SAMPLES", N, bf::kWhitenMinN, bf::kWhitenMaxN)) return -1;
    const int n_bins = N / 2 + 1;
    bf::WhitenBands wb = {};
    for (int b = 0; b < bands; ++b) {
        wb.lo[b] = std::min(std::max(bins[2 * b], 0), n_bins);
        wb.hi[b] = std::min(std::max(bins[2 * b + 1], 0), n_bins);
        if (wb.lo[b] >= wb.hi[b]) {
            set_error("%s: band %d: bins [%d, %d) hold no bin of [0, N_SAMPLES / 2 + 1 = %d)", who, b, bins[2 * b], bins[2 * b + 1], n_bins);
            return -1;
        }
    }
    char name[32];
    for (int b = 0; b < bands; ++b) {
        snprintf(name, sizeof(name), "beta[%d]", b);
        if (!need_finite(who, name, beta[b], FINITE_GE0)) return -1;
        if (beta[b] > 1.0f) { set_error("%s: %s = %g > 1", who, name, (double)beta[b]); return -1; }
        wb.beta[b] = beta[b];
    }
    for (int b = 0; b < bands; ++b) {
        snprintf(name, sizeof(name), "gain[%d]", b);
        if (!need_finite(who, name, gain[b])) return -1;
        wb.gain[b] = gain[b];
    }
    if (!need_finite(who, "floor_rel", floor_rel, FINITE_GE0) || !need_finite(who, "floor_abs", floor_abs, FINITE_GE0)) return -1;
    const u64 in_bytes = sat_mul(sat_mul(sat_mul((u64)frames, (u64)rows), (u64)N), sizeof(float));
    if (!need_disjoint(who, {{d_out, sat_mul(in_bytes, (u64)bands), "d_out"},
                             {d_signals, in_bytes, "d_signals"},
                             {d_window, (u64)N * sizeof(float), "d_window"}}, 1))
        return -1;
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_whiten(d_signals, (long long)frames * rows, N, d_window, wb, bands, floor_rel, floor_abs, d_out, as_stream(stream)));
}

// ---------------------------------------------------------------- ingest (receiver.c:94-151)

static int ingest_common(const void* d_packets, int n_arrays, int rows, int columns, float* d_frame, hipStream_t stream)
{
    State& s = S();
    const int mics_out = n_arrays * rows * columns;
    if (n_arrays < 1 || rows < 1 || columns < 1 || mics_out > s.sz.n_microphones) {
        set_error("bf_ingest: n_arrays*rows*columns = %d does not fit N_MICROPHONES = %d", mics_out, s.sz.n_microphones);
        return -1;
    }
    const int stride = 8 + 4 * s.sz.n_microphones;   // sizeof(msg), receiver.h:51-59
    return HIP_RC(bf::launch_ingest(d_packets, stride, 8, s.sz.n_samples, mics_out, s.sz.n_microphones, rows, columns, d_frame, stream));
}

int bf_ingest_device(const void* d_packets, int n_arrays, int rows, int columns, float* d_frame, void* stream)
{
    Entered in;
    if (!d_packets || !d_frame) { set_error("bf_ingest_device: null argument"); return -1; }
    if (!ensure_device()) return -1;
    return ingest_common(d_packets, n_arrays, rows, columns, d_frame, as_stream(stream));
}

int bf_ingest(const void* packets, int n_arrays, int rows, int columns, float* frame)
{
    Entered in;
    State& s = in.s;
    if (!packets || !frame) { set_error("bf_ingest: null argument"); return -1; }
    const size_t out_n = (size_t)std::max(0, n_arrays * rows * columns) * s.sz.n_samples;
    if (!ensure_device()) { poison(frame, out_n); return -1; }
    const size_t in_bytes = (size_t)(8 + 4 * s.sz.n_microphones) * s.sz.n_samples;
    bool ok = HIP_OK(s.d_packets.reserve(in_bytes)) && HIP_OK(s.d_frame.reserve(out_n ? out_n : 1));
    ok = ok && HIP_OK(hipMemcpyAsync(s.d_packets.p, packets, in_bytes, hipMemcpyHostToDevice, s.stream));
    ok = ok && ingest_common(s.d_packets.p, n_arrays, rows, columns, s.d_frame.p, s.stream) == 0;
    ok = ok && HIP_OK(hipMemcpyAsync(frame, s.d_frame.p, out_n * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    ok = ok && HIP_OK(sync_short(s.stream));
    if (!ok) poison(frame, out_n);
    return ok ? 0 : -1;
}

int bf_ingest_stream_device(const void* d_packets, long long n_datagrams, int n_arrays, int rows, int columns, int hop, int frames, int m_total,
                            const unsigned char* d_row_mask, int protocol_ver, float* d_frames, int* d_status, void* stream)
{
    static const char* who = "bf_ingest_stream_device";
    Entered in;
    const int M = in.s.sz.n_microphones, N = in.s.sz.n_samples;
    if (!need_ptrs(who, {{d_packets, "d_packets"}, {d_frames, "d_frames"}})) return -1;
    if (!need_min(who, "frames", frames, 1) || !need_min(who, "hop", hop, 1)) return -1;
    if (!need_min(who, "n_arrays", n_arrays, 1) || !need_min(who, "rows", rows, 1) || !need_min(who, "columns", columns, 1)) return -1;
    const long long mics_out = (long long)n_arrays * rows * columns;
    if (mics_out > M) { set_error("bf_ingest_stream_device: n_arrays*rows*columns = %lld > N_MICROPHONES = %d", mics_out, M); return -1; }
    if (mics_out > m_total) { set_error("bf_ingest_stream_device: n_arrays*rows*columns = %lld > m_total = %d", mics_out, m_total); return -1; }
    const long long needed = (long long)(frames - 1) * hop + N;
    if (needed > n_datagrams) {
        set_error("bf_ingest_stream_device: (frames - 1) * hop + N_SAMPLES = %lld > n_datagrams = %lld", needed, n_datagrams);
        return -1;
    }
    if (reinterpret_cast<uintptr_t>(d_packets) & 3) { set_error("bf_ingest_stream_device: d_packets = %p is not 4-byte aligned", d_packets); return -1; }
    if (reinterpret_cast<uintptr_t>(d_frames) & 3) { set_error("bf_ingest_stream_device: d_frames = %p is not 4-byte aligned", (const void*)d_frames); return -1; }
    const long long tiles = (long long)frames * ((N + 63) / 64) * ((m_total + 63) / 64) + frames;
    if (tiles > 0x7fffff00ll) { set_error("bf_ingest_stream_device: frames = %d needs %lld workgroups, more than one launch holds", frames, tiles); return -1; }
    if (!ensure_device()) return -1;
    const int stride = 8 + 4 * M;   // sizeof(msg), receiver.h:51-59
    return HIP_RC(bf::launch_ingest_stream(d_packets, stride, N, M, (int)mics_out, rows, columns, hop, frames, m_total, d_row_mask, protocol_ver, n_arrays,
                                           d_frames, d_status, as_stream(stream)));
}

int bf_default_disabled_mics(int* out)
{
    const int n = (int)(sizeof(kDeadMics) / sizeof(kDeadMics[0]));
    if (out)
        for (int i = 0; i < n; ++i) out[i] = kDeadMics[i];
    return n;
}

// ---------------------------------------------------------------- heat-map post-processing (visual.py)

int bf_heatmap_colorize_device(const float* d_power, int frames, float threshold, float amount, float exponent, unsigned char* d_small,
                               int* d_should_overlay, void* stream)
{
    Entered in;
    if (!d_power || !d_small || !d_should_overlay || frames < 1) { set_error("bf_heatmap_colorize_device: null argument or frames < 1"); return -1; }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_colorize(d_power, frames, in.s.sz.res_x, in.s.sz.res_y, threshold, amount, exponent, d_small, d_should_overlay, as_stream(stream)));
}

int bf_heatmap_overlay_device(const unsigned char* d_small, int frames, int out_w, int out_h, unsigned char* d_prev, const unsigned char* d_camera,
                              unsigned char* d_out, float w_prev, float w_new, float w_cam, float w_heat, void* stream)
{
    Entered in;
    if (!d_small || !d_prev || !d_out || frames < 1 || out_w < 1 || out_h < 1) { set_error("bf_heatmap_overlay_device: bad argument"); return -1; }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_overlay(d_small, frames, in.s.sz.res_x, in.s.sz.res_y, out_w, out_h, d_prev, d_camera, d_out, w_prev, w_new, w_cam, w_heat,
                                     as_stream(stream)));
}

int bf_power_center_device(const float* d_power, int frames, float* d_centers, float* d_workspace, void* stream)
{
    Entered in;
    if (!d_power || !d_centers || !d_workspace || frames < 1) { set_error("bf_power_center_device: bad argument"); return -1; }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_power_center(d_power, frames, in.s.sz.res_x, in.s.sz.res_y, d_centers, d_workspace, as_stream(stream)));
}

int bf_letterbox_bgr8_device(const unsigned char* d_frame, int h, int w, unsigned char* d_out, int out_h, int out_w, int new_h, int new_w, int top, int left, int value,
                             void* stream)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!d_frame || !d_out || h < 1 || w < 1 || out_h < 1 || out_w < 1 || new_h < 1 || new_w < 1 || top < 0 || left < 0 || top + new_h > out_h || left + new_w > out_w ||
        value < 0 || value > 255) {
        set_error("bf_letterbox_bgr8_device: %d x %d -> %d x %d at (%d, %d) of %d x %d, border %d", h, w, new_h, new_w, top, left, out_h, out_w, value);
        return -1;
    }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_letterbox(d_frame, h, w, d_out, out_h, out_w, new_h, new_w, top, left, value, as_stream(stream)));
}

// ---------------------------------------------------------------- frequency-domain beamformers

// These calls (and the detector's decode and NMS below) check pointers and sizes in one expression, `args_ok`, under one refusal
// text; then the device comes up.
static bool sized_args_ready(const char* who, bool args_ok)
{
    if (!args_ok) { set_error("%s: null pointer or non-positive size", who); return false; }
    return ensure_device();
}

int bf_fd_steering_device(const double* d_tau, const double* d_freq, int n_dirs, int n_mics, int n_bins, float* d_are, float* d_aim, void* stream)
{
    Entered in;
    if (!sized_args_ready("bf_fd_steering_device", d_tau && d_freq && d_are && d_aim && n_dirs > 0 && n_mics > 0 && n_bins > 0)) return -1;
    return HIP_RC(bf::launch_fd_steering(d_tau, d_freq, n_dirs, n_mics, n_bins, d_are, d_aim, as_stream(stream)));
}

int bf_fd_dft_device(const float* d_frames, int m_total, int frames, const int* adaptive_array, int n, int bin_lo, int n_bins, float* d_xre_mf,
                     float* d_xim_mf, float* d_xre_fm, float* d_xim_fm, void* stream)
{
    Entered in;
    State& s = in.s;
    if (!sized_args_ready("bf_fd_dft_device", d_frames && adaptive_array && d_xre_mf && d_xim_mf && d_xre_fm && d_xim_fm && frames > 0 && n > 0 && n_bins > 0 && bin_lo >= 0)) return -1;
    if (bin_lo + n_bins > s.sz.n_samples / 2 + 1) { set_error("bf_fd_dft_device: bins [%d,%d) exceed N_SAMPLES/2+1 = %d", bin_lo, bin_lo + n_bins, s.sz.n_samples / 2 + 1); return -1; }
    int max_row = 0;
    if (!upload_mics(adaptive_array, n, &max_row)) return -1;
    if (max_row >= m_total) { set_error("bf_fd_dft_device: adaptive_array names row %d but frames have %d rows", max_row, m_total); return -1; }
    const long long key = ((long long)s.sz.n_samples << 40) ^ ((long long)bin_lo << 20) ^ n_bins;
    if (s.fd_tw_key != key || !s.fd_tw.p) {
        if (!HIP_OK(s.fd_tw.reserve(bf::fd_twiddle_floats(s.sz.n_samples, n_bins)))) return -1;
        if (!HIP_OK(bf::launch_fd_twiddles(s.sz.n_samples, bin_lo, n_bins, s.fd_tw.p, as_stream(stream)))) return -1;
        if (!HIP_OK(hipStreamSynchronize(as_stream(stream)))) return -1;     // once per (N, bin range): see ensure_digest
        s.fd_tw_key = key;
    }
    return HIP_RC(bf::launch_fd_dft(d_frames, s.d_mics.p, m_total, s.sz.n_samples, frames, n, bin_lo, n_bins, s.fd_tw.p, d_xre_mf, d_xim_mf, d_xre_fm, d_xim_fm, as_stream(stream)));
}

int bf_fd_das_power_device(const float* d_xre_mf, const float* d_xim_mf, const float* d_are, const float* d_aim, int frames, int n_mics, int n_dirs,
                           int n_bins, float* d_power, void* stream)
{
    Entered in;
    if (!sized_args_ready("bf_fd_das_power_device", d_xre_mf && d_xim_mf && d_are && d_aim && d_power && frames > 0 && n_mics > 0 && n_dirs > 0 && n_bins > 0)) return -1;
    if (!HIP_OK(in.s.fd_work.reserve(bf::fd_workspace_floats(frames, n_dirs, n_bins)))) return -1;
    return HIP_RC(bf::launch_fd_das_power(d_xre_mf, d_xim_mf, d_are, d_aim, frames, n_mics, n_dirs, n_bins, d_power, in.s.fd_work.p, in.s.fd_work.cap, as_stream(stream)));
}

int bf_fd_covariance_device(const float* d_xre_fm, const float* d_xim_fm, int frames, int n_mics, int n_bins, float* d_rre, float* d_rim, void* stream)
{
    Entered in;
    if (!sized_args_ready("bf_fd_covariance_device", d_xre_fm && d_xim_fm && d_rre && d_rim && frames > 0 && n_mics > 0 && n_bins > 0)) return -1;
    return HIP_RC(bf::launch_fd_covariance(d_xre_fm, d_xim_fm, frames, n_mics, n_bins, d_rre, d_rim, as_stream(stream)));
}

int bf_fd_cholesky_inverse_device(const float* d_rre, const float* d_rim, int n_mics, int n_bins, float loading, float* d_lire_t, float* d_liim_t,
                                  int* d_status, void* stream)
{
    Entered in;
    DevBuf<float>& work = in.s.fd_chol_work;
    if (!sized_args_ready("bf_fd_cholesky_inverse_device", d_rre && d_rim && d_lire_t && d_liim_t && d_status && n_mics > 0 && n_bins > 0)) return -1;
    if (n_mics > 256) { set_error("bf_fd_cholesky_inverse_device: %d mics; the blocked factorisation handles at most 256", n_mics); return -1; }
    if (!HIP_OK(work.reserve(bf::fd_cholesky_workspace_floats(n_mics, n_bins)))) return -1;     // (no blocks, nothing reserved: up to 128 mics)
    return HIP_RC(bf::launch_fd_cholesky_inverse(d_rre, d_rim, n_mics, n_bins, loading, d_lire_t, d_liim_t, d_status, work.p, work.cap, as_stream(stream)));
}

int bf_fd_mvdr_power_device(const float* d_lire_t, const float* d_liim_t, const float* d_are, const float* d_aim, int n_mics, int n_dirs, int n_bins,
                            float* d_power, void* stream)
{
    Entered in;
    if (!sized_args_ready("bf_fd_mvdr_power_device", d_lire_t && d_liim_t && d_are && d_aim && d_power && n_mics > 0 && n_dirs > 0 && n_bins > 0)) return -1;
    if (n_mics > 256) { set_error("bf_fd_mvdr_power_device: %d mics; at most 256", n_mics); return -1; }
    if (!HIP_OK(in.s.fd_work.reserve(bf::fd_workspace_floats(1, n_dirs, n_bins)))) return -1;
    return HIP_RC(bf::launch_fd_mvdr_power(d_lire_t, d_liim_t, d_are, d_aim, n_mics, n_dirs, n_bins, d_power, in.s.fd_work.p, in.s.fd_work.cap, as_stream(stream)));
}

// The 256-entry colour table of the colourise kernel (visual.py:26-49 generate_color_map("jet")), uint8 [256][3].
void bf_jet_lut(unsigned char* out768)
{
    struct Rgb { unsigned char r, g, b; };
    static const Rgb kJet[256] = {
#include "jet_lut.inc"
    };
    if (!out768) return;
    for (int i = 0; i < 256; ++i) { out768[3 * i] = kJet[i].r; out768[3 * i + 1] = kJet[i].g; out768[3 * i + 2] = kJet[i].b; }
}

// ---------------------------------------------------------------- detector post-processing

int bf_yolo_decode_device(const void* const raw[3], const int h[3], const int w[3], const int strides[3], const float* anchors, int batch, int nc,
                          int format, float conf_thres, float* d_boxes, float* d_scores, int* d_cls, void* stream)
{
    Entered in;
    const bool args_ok = raw && raw[0] && raw[1] && raw[2] && h && w && strides && anchors && d_boxes && d_scores && d_cls && batch > 0 && nc > 0;
    if (!sized_args_ready("bf_yolo_decode_device", args_ok)) return -1;
    return HIP_RC(bf::launch_yolo_decode(raw, h, w, strides, anchors, batch, nc, format, conf_thres, d_boxes, d_scores, d_cls, as_stream(stream)));
}

int bf_topk_candidates_device(const float* d_scores, const float* d_boxes, const int* d_cls, int batch, int total, int k, float* d_top_scores,
                              float* d_top_boxes, int* d_top_cls, int* d_counts, void* stream)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!d_scores || !d_boxes || !d_cls || !d_top_scores || !d_top_boxes || !d_top_cls || !d_counts) { set_error("bf_topk_candidates_device: null pointer"); return -1; }
    if (k < 1 || k > 1024 || batch < 1 || total < 1) { set_error("bf_topk_candidates_device: batch %d, %d boxes, k = %d (1..1024)", batch, total, k); return -1; }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_topk_candidates(d_scores, d_boxes, d_cls, batch, total, k, d_top_scores, d_top_boxes, d_top_cls, d_counts, as_stream(stream)));
}

static int upsample_concat_checked(const char* who, int eb, const void* d_a, const void* d_b, void* d_out, int batch, int h, int w, int ca, int cb, void* stream)
{
    std::lock_guard<std::mutex> lock(S().mu);
    const int E = 16 / eb;
    if (!d_a || !d_b || !d_out || batch < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || ca < E || cb < E || (ca % E) || (cb % E)) {
        set_error("%s: batch %d, %d x %d (even), %d + %d channels (multiples of %d)", who, batch, h, w, ca, cb, E);
        return -1;
    }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_upsample_concat(d_a, d_b, d_out, batch, h, w, ca, cb, eb, as_stream(stream)));
}
int bf_upsample_concat_device(const void* d_a, const void* d_b, void* d_out, int batch, int h, int w, int ca, int cb, void* stream)
{
    return upsample_concat_checked("bf_upsample_concat_device", 2, d_a, d_b, d_out, batch, h, w, ca, cb, stream);
}
int bf_upsample_concat_f32_device(const void* d_a, const void* d_b, void* d_out, int batch, int h, int w, int ca, int cb, void* stream)
{
    return upsample_concat_checked("bf_upsample_concat_f32_device", 4, d_a, d_b, d_out, batch, h, w, ca, cb, stream);
}

static int sppf_pool_checked(const char* who, int eb, void* d_buf, int batch, int h, int w, int c, void* stream)
{
    std::lock_guard<std::mutex> lock(S().mu);
    const int E = 16 / eb;
    if (!d_buf || batch < 1 || h < 1 || w < 1 || c < E || (c % E) || (long long)h * w > 2048) {
        set_error("%s: batch %d, %d x %d, %d channels (a multiple of %d; at most 2048 pixels per plane)", who, batch, h, w, c, E);
        return -1;
    }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_sppf_pool(d_buf, batch, h, w, c, eb, as_stream(stream)));
}
int bf_sppf_pool_device(void* d_buf, int batch, int h, int w, int c, void* stream) { return sppf_pool_checked("bf_sppf_pool_device", 2, d_buf, batch, h, w, c, stream); }
int bf_sppf_pool_f32_device(void* d_buf, int batch, int h, int w, int c, void* stream) { return sppf_pool_checked("bf_sppf_pool_f32_device", 4, d_buf, batch, h, w, c, stream); }

static int preprocess_checked(const char* who, int eb, const void* d_frames, void* d_out, int batch, int h, int w, int cpad, void* stream)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!d_frames || !d_out || batch < 1 || h < 1 || w < 1 || cpad < 3) { set_error("%s: batch %d, %d x %d, %d channels", who, batch, h, w, cpad); return -1; }
    if (!ensure_device()) return -1;
    return HIP_RC(bf::launch_preprocess_bgr8(d_frames, d_out, (long long)batch * h * w, cpad, eb, as_stream(stream)));
}
int bf_preprocess_bgr8_device(const void* d_frames, void* d_out, int batch, int h, int w, int cpad, void* stream)
{
    return preprocess_checked("bf_preprocess_bgr8_device", 2, d_frames, d_out, batch, h, w, cpad, stream);
}
int bf_preprocess_bgr8_f32_device(const void* d_frames, void* d_out, int batch, int h, int w, int cpad, void* stream)
{
    return preprocess_checked("bf_preprocess_bgr8_f32_device", 4, d_frames, d_out, batch, h, w, cpad, stream);
}

int bf_conv2d_use_dma_kernel(int enable) { return bf::conv_dma_switch(enable); }
int bf_conv2d_f32_mode(int mode) { return bf::conv_f32_mode(mode); }
int bf_fd_gemm_f32_mode(int mode) { return bf::gemm_f32_mode(mode); }

int bf_conv2d_weight_row(int kh, int kw, int c) { return kh > 0 && kw > 0 && c > 0 ? bf::conv_weight_row(2, kh, kw, c) : -1; }
int bf_conv2d_weight_row_f32(int kh, int kw, int c) { return kh > 0 && kw > 0 && c > 0 ? bf::conv_weight_row(4, kh, kw, c) : -1; }

// The argument checks of the convolution entry points and of bf_plan_conv2d (pointers as "not 16-byte aligned" flags: bf::kConvMisaligned*).
static bool conv2d_args_ok(const char* who, int eb, int batch, int h, int w, int c, int n, int kh, int kw, int stride, int pad, int ldy, bool has_res, int ldr,
                           unsigned misaligned, bool cat, bool has_x2, int c1, int ld1, int ld2, int up1)
{
    const int E = 16 / eb;
    if (batch < 1 || h < 1 || w < 1 || n < 1 || kh < 1 || kw < 1 || stride < 1 || pad < 0 || h + 2 * pad < kh || w + 2 * pad < kw) {
        set_error("%s: batch %d, %d x %d, window %d x %d, stride %d, pad %d", who, batch, h, w, kh, kw, stride, pad);
        return false;
    }
    if (c < 4 || (c & (c - 1)) != 0 || ((kw * c) % E) != 0 || (c < E && ((stride & 1) || (pad & 1) || (w & 1)))) {
        set_error("%s: %d input channels, window width %d, stride %d, pad %d, width %d: channels must be a power of two >= 4 with "
                  "kw * c a multiple of %d; float16 with 4 channels needs even stride, pad and width", who, c, kw, stride, pad, w, E);
        return false;
    }
    if (ldy < n || (has_res && ldr < n)) { set_error("%s: row strides %d / %d under %d output channels", who, ldy, ldr, n); return false; }
    if (misaligned & (bf::kConvMisalignedX | bf::kConvMisalignedW)) { set_error("%s: x and w must be 16-byte aligned", who); return false; }
    if (cat) {
        if (c1 < E || c1 > c || (c1 % E) || (ld1 % E) || ld1 < c1 || (c1 < c && (!has_x2 || (ld2 % E) || ld2 < c - c1 || (misaligned & bf::kConvMisalignedX2))) ||
            (up1 && ((h & 1) || (w & 1)))) {
            set_error("%s: sources of %d (pitch %d%s) + %d (pitch %d) channels for %d: whole 16-byte chunks of %d elements, 16-byte aligned; an upsampled "
                      "source needs even h and w", who, c1, ld1, up1 ? ", upsampled" : "", c - c1, ld2, c, E);
            return false;
        }
    }
    return true;
}

static unsigned conv2d_misaligned(const void* x, const void* w, const void* x2, const void* y, const void* res)
{
    const auto bit = [](const void* p, unsigned b) { return (reinterpret_cast<uintptr_t>(p) & 15) ? b : 0u; };
    return bit(x, bf::kConvMisalignedX) | bit(w, bf::kConvMisalignedW) | bit(x2, bf::kConvMisalignedX2) | bit(y, bf::kConvMisalignedY) | bit(res, bf::kConvMisalignedRes);
}

static int conv2d_checked(const char* who, int eb, const void* d_x, const void* d_w, const float* d_bias, void* d_y, int batch, int h, int w, int c, int n, int kh,
                          int kw, int stride, int pad, int silu, int ldy, const void* d_res, int ldr, void* stream, bool cat = false, const void* d_x2 = nullptr,
                          int c1 = 0, int ld1 = 0, int ld2 = 0, int up1 = 0)
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!d_x || !d_w || !d_y) { set_error("%s: null pointer", who); return -1; }
    if (!conv2d_args_ok(who, eb, batch, h, w, c, n, kh, kw, stride, pad, ldy, d_res != nullptr, ldr, conv2d_misaligned(d_x, d_w, d_x2, d_y, d_res), cat,
                        d_x2 != nullptr, c1, ld1, ld2, up1)) return -1;
    if (cat && c1 == c) d_x2 = nullptr;
    if (!ensure_device()) return -1;
    // (a plain dense source through the cat entry still takes the 1x1 path: ld1 = c selects it only when something differs -- force it with up1 / x2 / ld1)
    return HIP_RC(bf::launch_conv2d_nhwc(eb, d_x, d_w, d_bias, d_y, batch, h, w, c, n, kh, kw, stride, pad, silu, ldy, d_res, ldr, cat ? d_x2 : nullptr,
                                         cat ? c1 : c, cat ? ld1 : c, cat ? ld2 : 0, cat ? up1 : 0, as_stream(stream)));
}

static void conv2d_plan_out(const bf::ConvPlan& p, long long out[16])
{
    out[0] = p.elem_bytes; out[1] = p.family; out[2] = p.bm; out[3] = p.bn; out[4] = p.cpr; out[5] = p.cat; out[6] = p.split; out[7] = p.fast_tap;
    out[8] = p.wide; out[9] = p.grid_x; out[10] = p.grid_y; out[11] = p.lds_bytes; out[12] = p.row_env; out[13] = p.tap_env; out[14] = p.patch_env;
    out[15] = p.n_cus;
}

int bf_plan_conv2d(int elem_bytes, int batch, int h, int w, int c, int n, int kh, int kw, int stride, int pad, int ldy, int has_res, int ldr, int c1, int ld1,
                   int up1, int has_x2, int ld2, int misaligned, int use_dma_kernel, int f32_mode, int n_cus, long long out[16])
{
    std::lock_guard<std::mutex> lock(S().mu);
    const char* who = "bf_plan_conv2d";
    if (!out) { set_error("%s: out is null", who); return -1; }
    if (elem_bytes != 2 && elem_bytes != 4) { set_error("%s: element size %d (2 = float16, 4 = float32)", who, elem_bytes); return -1; }
    // the layer names a concatenation (the bf_conv1x1_cat_* entry) when anything differs from one dense source of c channels
    const bool cat = has_x2 != 0 || up1 != 0 || c1 != c || ld1 != c;
    if (cat && (kh != 1 || kw != 1 || stride != 1 || pad != 0)) {
        set_error("%s: two sources / a pitch / upsampling under a %d x %d window, stride %d, pad %d: 1x1 layers only", who, kh, kw, stride, pad);
        return -1;
    }
    if (!conv2d_args_ok(who, elem_bytes, batch, h, w, c, n, kh, kw, stride, pad, ldy, has_res != 0, ldr, (unsigned)misaligned, cat, has_x2 != 0, c1, ld1, ld2, up1))
        return -1;
    const bool x2 = has_x2 != 0 && !(cat && c1 == c);
    bf::ConvLayer L;
    L.elem_bytes = elem_bytes; L.B = batch; L.H = h; L.W = w; L.C = c; L.N = n; L.KH = kh; L.KW = kw; L.stride = stride; L.pad = pad;
    L.ldy = ldy; L.ldr = ldr; L.c1 = cat ? c1 : c; L.ld1 = cat ? ld1 : c; L.ld2 = cat ? ld2 : 0; L.up1 = cat ? up1 : 0;
    L.has_res = has_res != 0; L.has_x2 = x2; L.misaligned = (unsigned)misaligned & ~(x2 ? 0u : (unsigned)bf::kConvMisalignedX2);
    const int dma = use_dma_kernel < 0 ? bf::conv_dma_switch(-1) : (use_dma_kernel > 2 ? 1 : use_dma_kernel);       // (as the setters store them)
    const int mode = f32_mode < 0 ? bf::conv_f32_mode(-1) : (f32_mode != 0 ? 1 : 0);
    bf::ConvPlan p;
    if (bf::plan_conv2d(L, dma, mode, n_cus > 0 ? n_cus : 256, &p) != hipSuccess) {
        set_error("%s: the launch refuses this layer (%s)", who, hipGetErrorString(hipErrorInvalidValue));
        return -1;
    }
    conv2d_plan_out(p, out);
    return 0;
}

int bf_last_conv2d_plan(long long out[16])
{
    std::lock_guard<std::mutex> lock(S().mu);
    if (!out) { set_error("bf_last_conv2d_plan: out is null"); return -1; }
    bf::ConvPlan p;
    if (!bf::last_conv2d_plan(&p)) { set_error("bf_last_conv2d_plan: no convolution was launched in this process"); return -1; }
    conv2d_plan_out(p, out);
    return 0;
}

int bf_conv2d_nhwc_f16_device(const void* d_x, const void* d_w, const float* d_bias, void* d_y, int batch, int h, int w, int c, int n, int kh, int kw, int stride,
                              int pad, int silu, void* stream)
{
    return conv2d_checked("bf_conv2d_nhwc_f16_device", 2, d_x, d_w, d_bias, d_y, batch, h, w, c, n, kh, kw, stride, pad, silu, n, nullptr, 0, stream);
}

int bf_conv2d_nhwc_f16_into_device(const void* d_x, const void* d_w, const float* d_bias, void* d_y, int ldy, const void* d_res, int ldr, int batch, int h, int w,
                                   int c, int n, int kh, int kw, int stride, int pad, int silu, void* stream)
{
    return conv2d_checked("bf_conv2d_nhwc_f16_into_device", 2, d_x, d_w, d_bias, d_y, batch, h, w, c, n, kh, kw, stride, pad, silu, ldy, d_res, ldr, stream);
}

int bf_conv2d_nhwc_f32_device(const void* d_x, const void* d_w, const float* d_bias, void* d_y, int batch, int h, int w, int c, int n, int kh, int kw, int stride,
                              int pad, int silu, void* stream)
{
    return conv2d_checked("bf_conv2d_nhwc_f32_device", 4, d_x, d_w, d_bias, d_y, batch, h, w, c, n, kh, kw, stride, pad, silu, n, nullptr, 0, stream);
}

int bf_conv2d_nhwc_f32_into_device(const void* d_x, const void* d_w, const float* d_bias, void* d_y, int ldy, const void* d_res, int ldr, int batch, int h, int w,
                                   int c, int n, int kh, int kw, int stride, int pad, int silu, void* stream)
{
    return conv2d_checked("bf_conv2d_nhwc_f32_into_device", 4, d_x, d_w, d_bias, d_y, batch, h, w, c, n, kh, kw, stride, pad, silu, ldy, d_res, ldr, stream);
}

int bf_conv1x1_cat_nhwc_f16_device(const void* d_x1, int ld1, int c1, int up1, const void* d_x2, int ld2, const void* d_w, const float* d_bias, void* d_y, int ldy,
                                   const void* d_res, int ldr, int batch, int h, int w, int c, int n, int silu, void* stream)
{
    return conv2d_checked("bf_conv1x1_cat_nhwc_f16_device", 2, d_x1, d_w, d_bias, d_y, batch, h, w, c, n, 1, 1, 1, 0, silu, ldy, d_res, ldr, stream, true, d_x2, c1, ld1,
                          ld2, up1);
}

int bf_conv1x1_cat_nhwc_f32_device(const void* d_x1, int ld1, int c1, int up1, const void* d_x2, int ld2, const void* d_w, const float* d_bias, void* d_y, int ldy,
                                   const void* d_res, int ldr, int batch, int h, int w, int c, int n, int silu, void* stream)
{
    return conv2d_checked("bf_conv1x1_cat_nhwc_f32_device", 4, d_x1, d_w, d_bias, d_y, batch, h, w, c, n, 1, 1, 1, 0, silu, ldy, d_res, ldr, stream, true, d_x2, c1, ld1,
                          ld2, up1);
}

int bf_nms_device(const float* d_boxes, const float* d_scores, const int* d_cls, const int* d_counts, int batch, int k, float iou_thres, int max_det,
                  unsigned long long* d_mask, float* d_out, int* d_out_count, void* stream)
{
    Entered in;
    if (!sized_args_ready("bf_nms_device", d_boxes && d_scores && d_cls && d_counts && d_mask && d_out && d_out_count && batch > 0 && k > 0 && max_det > 0)) return -1;
    if (k > 4096) { set_error("bf_nms_device: k = %d candidates; at most 4096", k); return -1; }
    return HIP_RC(bf::launch_nms(d_boxes, d_scores, d_cls, d_counts, batch, k, iou_thres, max_det, d_mask, d_out, d_out_count, as_stream(stream)));
}

int bf_plan_das(int algo, int n, int frames, int dir_begin, int dir_end, int max_whole, int n_cus, long long out[10])
{
    Entered in;
    bf::DasLaunch L{};
    L.algo = algo; L.n_mics = n; L.m_total = n; L.n_samples = in.s.sz.n_samples; L.n_taps = in.s.sz.n_taps; L.n_dirs = in.s.sz.dirs();
    L.dir_begin = dir_begin; L.dir_end = dir_end; L.frames = frames; L.tab.max_whole = max_whole;
    bf::DasPlan p{};
    const char* why = "";
    if (bf::plan_das(L, n_cus > 0 ? n_cus : 256, &p, &why) != 0) { set_error("bf_plan_das: %s", why); return -1; }
    export_plan(p, out);
    return 0;
}

int bf_plan_das_select(int algo, int n, int frames, int count, int max_whole, int stream_mode, int n_cus, long long out[10])
{
    Entered in;
    bf::DasLaunch L{};
    L.algo = algo; L.n_mics = n; L.m_total = n; L.n_samples = in.s.sz.n_samples; L.n_taps = in.s.sz.n_taps; L.n_dirs = in.s.sz.dirs();
    L.dir_begin = 0; L.dir_end = count; L.frames = frames; L.tab.max_whole = max_whole;
    bf::DasPlan p{};
    const char* why = "";
    if (bf::plan_select(L, stream_mode != 0, n_cus > 0 ? n_cus : 256, &p, &why) != 0) { set_error("bf_plan_das_select: %s", why); return -1; }
    export_plan(p, out);
    return 0;
}

int bf_plan_das_stream(int algo, int n, int frames, int dir_begin, int dir_end, int max_whole, int n_cus, long long out[10])
{
    Entered in;
    if (!need_ptrs("bf_plan_das_stream", {{out, "out"}})) return -1;
    bf::DasLaunch L{};
    L.algo = algo; L.n_mics = n; L.m_total = n; L.n_samples = in.s.sz.n_samples; L.n_taps = in.s.sz.n_taps; L.n_dirs = in.s.sz.dirs();
    L.dir_begin = dir_begin; L.dir_end = dir_end; L.frames = frames; L.tab.max_whole = max_whole;
    bf::DasPlan p{};
    const char* why = "";
    if (bf::plan_stream_maps(L, n_cus > 0 ? n_cus : 256, &p, &why) != 0) { set_error("bf_plan_das_stream: %s", why); return -1; }
    export_plan(p, out);
    return 0;
}

int bf_last_strided_plan(long long out[12])
{
    Entered in;
    if (!need_ptrs("bf_last_strided_plan", {{out, "out"}})) return -1;
    if (!in.s.last_strided_set) { set_error("bf_last_strided_plan: no stream or listed-direction call was launched in this process"); return -1; }
    std::copy(in.s.last_strided, in.s.last_strided + 12, out);
    return 0;
}

}  // extern "C"
