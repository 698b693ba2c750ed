// libbbt_hip.so -- host side of the C ABI declared in include/bbt_hip.h.
// Plans, twiddle tables, launch geometry; the kernels are in bbt_kernels.hpp.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/bbt_hip.h"
#include "bbt_kernels.hpp"
#include "gen_kernels.hpp"
#include "big_kernels.hpp"
#include "gen2_host.hpp"
#include "gen_host.hpp"
#include "osm_geo.hpp"
#include "osm_launch.hpp"
#include "chan_geo.hpp"
#include "pfb_geo.hpp"
#include "tune.hpp"
#include "rtc.hpp"
#include "fold_kernels.hpp"
#include "phase_kernels.hpp"
#include "modulate_kernels.hpp"
#include "sk_kernels.hpp"
#include "dmt_kernels.hpp"
#include "sps_kernels.hpp"
#include "ffa_kernels.hpp"
#include "hsum_kernels.hpp"
#include "lspec_kernels.hpp"
#include "accel_kernels.hpp"
#include "rank_kernels.hpp"
#include "rmed_kernels.hpp"
#include "corr_kernels.hpp"
#include "r2c_kernels.hpp"
#include "gather_kernels.hpp"
#include "pack_kernels.hpp"
#include "psrfits_kernels.hpp"
#include "psrsearch_kernels.hpp"
#include "noise_kernels.hpp"

using namespace bbt;

#define BBT_VERSION 171

// ---------------------------------------------------------------------------
// errors
static thread_local std::string g_err;

static int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                      \
    } while (0)

#define ARG_TRY(cond, ...) \
    do {                   \
        if (!(cond)) return fail(__VA_ARGS__); \
    } while (0)

// are the arrays of 4-byte elements aligned to them? (a null pointer is)
static inline bool aligned4(const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) == 0;
}

// ---------------------------------------------------------------------------
// twiddle tables, per device
struct FftTables {
    cf* tw0 = nullptr;  // [16][T]   W_N^{tau c0}
    cf* tw1 = nullptr;  // [16][R2]  W_T^{b1 c1}
};
static std::mutex g_tab_mutex;
static std::map<std::pair<int, int>, FftTables> g_tables;  // (device, N)
static std::map<int, cf*> g_wroot;                         // device -> W_4096^m, then W_65536^i (i < 256)

static int upload(cf** dst, const std::vector<cf>& h) {
    HIP_TRY(hipMalloc((void**)dst, h.size() * sizeof(cf)));
    HIP_TRY(hipMemcpy(*dst, h.data(), h.size() * sizeof(cf), hipMemcpyHostToDevice));
    return 0;
}

static cf unit_root(long long k, long long n) {
    // exp(-2 pi i k / n), evaluated in double with exact octant reduction
    k %= n;
    const double a = -2.0 * M_PI * (double)k / (double)n;
    return make_float2((float)cos(a), (float)sin(a));
}

static int get_tables(int n, FftTables* out) {
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tab_mutex);
    auto it = g_tables.find({dev, n});
    if (it != g_tables.end()) {
        *out = it->second;
        return 0;
    }
    const int r2 = n / 256, t = n / 16;
    std::vector<cf> h0(16 * t), h1(16 * r2);
    for (int c = 0; c < 16; ++c)
        for (int tau = 0; tau < t; ++tau) h0[c * t + tau] = unit_root((long long)tau * c, n);
    for (int c = 0; c < 16; ++c)
        for (int b = 0; b < r2; ++b) h1[c * r2 + b] = unit_root((long long)b * c, t);
    FftTables ft;
    if (upload(&ft.tw0, h0)) return 1;
    if (upload(&ft.tw1, h1)) return 1;
    g_tables[{dev, n}] = ft;
    *out = ft;
    return 0;
}

// twiddles of the 8192- / 16384-point transforms (fft_big.hpp: BigGeo<N>::TW_*), cached per device
static std::map<std::pair<int, int>, cf*> g_big_tables;
static int get_big_table(int n, cf** out) {
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tab_mutex);
    auto it = g_big_tables.find({dev, n});
    if (it != g_big_tables.end()) {
        *out = it->second;
        return 0;
    }
    const int t = n / 16, m = t / 16, l = m / 16;
    std::vector<cf> h;
    h.reserve(4 * (size_t)(t + m + l));
    for (int c = 1; c <= 8; c *= 2)
        for (int i = 0; i < t; ++i) h.push_back(unit_root((long long)i * c, n));
    for (int c = 1; c <= 8; c *= 2)
        for (int i = 0; i < m; ++i) h.push_back(unit_root((long long)i * c, t));
    for (int c = 1; c <= 8; c *= 2)
        for (int i = 0; i < l; ++i) h.push_back(unit_root((long long)i * c, m));
    cf* d;
    if (upload(&d, h)) return 1;
    g_big_tables[{dev, n}] = d;
    *out = d;
    return 0;
}

static int get_wroot(cf** out) {
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tab_mutex);
    auto it = g_wroot.find(dev);
    if (it != g_wroot.end()) {
        *out = it->second;
        return 0;
    }
    std::vector<cf> h(4096 + 256);
    for (int m = 0; m < 4096; ++m) h[m] = unit_root(m, 4096);
    for (int m = 0; m < 256; ++m) h[4096 + m] = unit_root(m, 65536);
    cf* d;
    if (upload(&d, h)) return 1;
    g_wroot[dev] = d;
    *out = d;
    return 0;
}

// ---- lengths 2^a 3^b 5^c 7^d (fft_generic.hpp) ------------------------------
// (stage lists, workgroup size, split and tile rules: gen_host.hpp; BBT_RTC and the split of a
// plan: osm_geo.hpp)
static std::map<std::pair<int, int>, cf*> g_gen_tables;    // (device, n) -> stage twiddles; -n: stages reversed
static int get_gen_table(GenGeo* g, cf** out, bool reversed = false);
// The same stages in reversed order: what the inverse of a convolution runs (fft_generic.hpp,
// gen_conv_open), with its own stage tables.
static int get_reversed(const GenGeo& g, GenGeo* gr, cf** out) {
    *gr = g;
    for (int s = 0; s < g.nfac; ++s) gr->fac[s] = g.fac[g.nfac - 1 - s];
    return get_gen_table(gr, out, true);
}
static int make_big_twiddle(int64_t n, cf** lo, cf** hi);

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a
// kernel: set it once per (device, kernel) and check the result.
static int ensure_dyn_lds(const void* func, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = done.find({dev, func});
    if (it != done.end() && it->second >= bytes) return 0;
    HIP_TRY(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[{dev, func}] = bytes;
    return 0;
}

// Stage twiddles of the LDS Stockham transform of g->n points, stage after stage: stage s (radix
// R, Ns = product of the earlier radices) has its W_{Ns R}^{r k} at [g->woff[s] + (r - 1) Ns + k],
// r = 1 .. R - 1, k < Ns -- contiguous in k, which is what neighbouring lanes differ in, so a
// stage's twiddle loads are coalesced (gathered from one W_n^k table they touched up to 64 cache
// lines per wave instruction).  The first stage (Ns = 1) has none.  Fills g->woff.
static int get_gen_table(GenGeo* g, cf** out, bool reversed) {
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    const int n = g->n;
    int ns = 1, total = 0;
    for (int s = 0; s < g->nfac; ++s) {
        g->woff[s] = total;
        if (s > 0) total += (g->fac[s] - 1) * ns;
        ns *= g->fac[s];
    }
    std::lock_guard<std::mutex> lock(g_tab_mutex);
    const int key = reversed ? -n : n;
    auto it = g_gen_tables.find({dev, key});
    if (it != g_gen_tables.end()) {
        *out = it->second;
        return 0;
    }
    std::vector<cf> h((size_t)std::max(total, 1));
    ns = 1;
    for (int s = 0; s < g->nfac; ++s) {
        const int r_s = g->fac[s];
        if (s > 0)
            for (int r = 1; r < r_s; ++r)
                for (int k = 0; k < ns; ++k)
                    h[(size_t)g->woff[s] + (size_t)(r - 1) * ns + k] = unit_root((long long)r * k, (long long)ns * r_s);
        ns *= r_s;
    }
    cf* d;
    if (upload(&d, h)) return 1;
    g_gen_tables[{dev, key}] = d;
    *out = d;
    return 0;
}
// W_N^m = hi[m >> 12] * lo[m & 4095]  (per plan: depends on N)
static int make_big_twiddle(int64_t n, cf** lo, cf** hi) {
    std::vector<cf> l(4096), h((size_t)((n + 4095) / 4096));
    for (int i = 0; i < 4096; ++i) l[i] = unit_root(i, n);
    for (size_t j = 0; j < h.size(); ++j) h[j] = unit_root((long long)j * 4096, n);
    if (upload(lo, l) || upload(hi, h)) return 1;
    return 0;
}

// ---- the register-resident engine for those lengths, specialised at plan time ---------------
// (fft_gen2.hpp, gen2_kernels.hpp; compiled by rtc.hpp).  BBT_RTC=0: the LDS Stockham engine
// above runs every such length (as in rounds 2-4); BBT_RTC=require: a failing compilation is an
// error instead of a warning and a fall back to it.
static std::mutex g_g2_mutex;
static std::map<std::pair<int, std::string>, cf*> g_g2_tables;    // (device, stage list) -> tables
static int64_t g_rtc_modules = 0;
static double g_rtc_seconds = 0;
static int get_g2_table(const G2Plan& g, cf** out) {
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    std::string key = std::to_string(g.n);
    for (int s = 0; s < g.nfac; ++s) key += "," + std::to_string(g.fac[s]);
    std::lock_guard<std::mutex> lock(g_g2_mutex);
    auto it = g_g2_tables.find({dev, key});
    if (it != g_g2_tables.end()) {
        *out = it->second;
        return 0;
    }
    const std::vector<float> t = g2_tables(g);
    cf* d;
    HIP_TRY(hipMalloc((void**)&d, t.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    g_g2_tables[{dev, key}] = d;
    *out = d;
    return 0;
}
// source -> entry points.  0 = ok; 1 = not available (the caller falls back), with the reason in
// g_err; in `require` mode that is the error of the call.
static int g2_build(const std::string& source, const std::vector<const char*>& names, hipFunction_t* fns) {
    RtcModule* m;
    std::string log;
    const auto t0 = std::chrono::steady_clock::now();
    if (rtc_module(source, &m, &log)) return fail("run-time compilation of a generic-length kernel failed: %s", log.c_str());
    for (size_t i = 0; i < names.size(); ++i)
        if (rtc_function(m, names[i], &fns[i], &log)) return fail("%s", log.c_str());
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    {
        std::lock_guard<std::mutex> lock(g_g2_mutex);
        if (dt > 0.02) {                    // (a module that was compiled, not found in the process's cache)
            g_rtc_modules += 1;
            g_rtc_seconds += dt;
        }
    }
    if (getenv("BBT_RTC_VERBOSE")) fprintf(stderr, "bbt: rtc %.2f s\n%s", dt, source.c_str());
    return 0;
}
static void g2_warn_once(const char* what) {
    static std::once_flag once;
    std::call_once(once, [&] {
        fprintf(stderr, "baseband_tasks_amd: %s -- %s; lengths that are not powers of two run on the slower "
                        "general kernels (BBT_RTC=require makes this an error)\n", what, g_err.c_str());
    });
}
template <class... A>
static int g2_launch(hipFunction_t f, dim3 grid, dim3 block, hipStream_t st, A... a) {
    void* args[] = {(void*)&a...};
    HIP_TRY(hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, block.x, block.y, block.z, 0, st, args, nullptr));
    return 0;
}

struct DevicePool {
    std::mutex mu;
    struct Idle {
        void* ptr;
        hipStream_t freed_on;   // pool stream when the block was freed
    };
    std::map<int, std::multimap<size_t, Idle>> free_blocks;         // device -> size -> block
    std::map<void*, std::pair<size_t, int>> live;                   // block -> (size, device)
    size_t cached = 0;
    // The stream on which blocks of the pool are used (bbt_pool_set_stream).
    // Reuse of a freed block is ordered by that stream; a block freed under
    // another pool stream is handed out only after the device has drained.
    hipStream_t stream = nullptr;
    static size_t limit() {                      // cached (idle) bytes kept at most; BBT_POOL_MAX_GB
        static const size_t lim = [] {
            const char* e = getenv("BBT_POOL_MAX_GB");
            return (size_t)(e ? atof(e) : 96.0) << 30;
        }();
        return lim;
    }
    static bool enabled() {
        static const bool on = [] { const char* e = getenv("BBT_POOL"); return !(e && atoi(e) == 0); }();
        return on;
    }
};
static DevicePool g_pool;
extern "C" int bbt_pool_trim(void);

// ---------------------------------------------------------------------------
extern "C" {

const char* bbt_last_error(void) { return g_err.c_str(); }
int bbt_version(void) { return BBT_VERSION; }
int bbt_rtc_info(int* mode, int64_t* modules, double* seconds) {
    std::lock_guard<std::mutex> lock(g_g2_mutex);
    if (mode) *mode = rtc_mode();
    if (modules) *modules = g_rtc_modules;
    if (seconds) *seconds = g_rtc_seconds;
    return 0;
}

int bbt_device_count(int* count) {
    ARG_TRY(count, "bbt_device_count: null argument");
    HIP_TRY(hipGetDeviceCount(count));
    return 0;
}
int bbt_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return 0;
}
int bbt_get_device(int* device) {
    ARG_TRY(device, "bbt_get_device: null argument");
    HIP_TRY(hipGetDevice(device));
    return 0;
}
int bbt_device_name(char* buf, int buflen) {
    ARG_TRY(buf && buflen > 0, "bbt_device_name: bad buffer");
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, buflen, "%s (%s)", prop.name, prop.gcnArchName);
    return 0;
}

// Device memory comes from a caching pool: hipMalloc / hipFree of the GB-sized
// stream buffers a reader allocates per call cost milliseconds and hipFree
// synchronises the device, which would serialise consecutive calls.  Freed
// blocks are kept (per device, by size) and handed out again for requests of
// up to 1/8 less; reuse is ordered by the caller's stream, as every consumer of
// a block is enqueued on it before the block is freed (plans join their
// internal streams before returning).  BBT_POOL=0 disables caching.
int bbt_malloc(void** dev_ptr, size_t nbytes) {
    ARG_TRY(dev_ptr, "bbt_malloc: null argument");
    if (!nbytes) nbytes = 1;
    const size_t gran = nbytes >= (1u << 20) ? (size_t)2 << 20 : 512;
    const size_t want = (nbytes + gran - 1) / gran * gran;
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> lock(g_pool.mu);
        auto& free_blocks = g_pool.free_blocks[dev];
        auto it = free_blocks.lower_bound(want);
        if (it != free_blocks.end() && it->first - want <= want / 8) {
            const DevicePool::Idle idle = it->second;
            *dev_ptr = idle.ptr;
            g_pool.cached -= it->first;
            g_pool.live[idle.ptr] = {it->first, dev};
            free_blocks.erase(it);
            if (idle.freed_on != g_pool.stream) {
                // freed under another stream: its last users are not ordered
                // before work on the current pool stream -- drain the device
                HIP_TRY(hipDeviceSynchronize());
            }
            return 0;
        }
    }
    hipError_t e = hipMalloc(dev_ptr, want);
    if (e != hipSuccess) {                      // give cached blocks back and retry once
        (void)hipGetLastError();
        if (bbt_pool_trim()) return 1;
        e = hipMalloc(dev_ptr, want);
    }
    if (e != hipSuccess) {
        *dev_ptr = nullptr;
        return fail("bbt_malloc: hipMalloc of %zu bytes failed: %s", want, hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lock(g_pool.mu);
    g_pool.live[*dev_ptr] = {want, dev};
    return 0;
}
int bbt_free(void* dev_ptr) {
    if (!dev_ptr) return 0;
    {
        std::lock_guard<std::mutex> lock(g_pool.mu);
        auto it = g_pool.live.find(dev_ptr);
        if (it == g_pool.live.end()) return fail("bbt_free: pointer was not allocated by bbt_malloc");
        const size_t size = it->second.first;
        const int dev = it->second.second;
        g_pool.live.erase(it);
        if (g_pool.enabled() && g_pool.cached + size <= g_pool.limit()) {
            g_pool.free_blocks[dev].emplace(size, DevicePool::Idle{dev_ptr, g_pool.stream});
            g_pool.cached += size;
            return 0;
        }
    }
    HIP_TRY(hipFree(dev_ptr));
    return 0;
}
int bbt_pool_trim(void) {
    std::vector<void*> blocks;
    {
        std::lock_guard<std::mutex> lock(g_pool.mu);
        for (auto& per_dev : g_pool.free_blocks) {
            for (auto& b : per_dev.second) blocks.push_back(b.second.ptr);
            per_dev.second.clear();
        }
        g_pool.cached = 0;
    }
    for (void* b : blocks) HIP_TRY(hipFree(b));
    return 0;
}
int bbt_pool_set_stream(bbt_stream stream) {
    // A change of the pool stream drains the device once: blocks are tagged with the pool
    // stream at the time they are freed, and a block whose last kernels were queued on the
    // previous stream may be freed (by a garbage collector, at any time) only after the switch
    // -- it would then carry the new stream's tag and be handed out unordered.  After the
    // drain every idle and every live block is safe under the new stream.
    bool changed;
    {
        std::lock_guard<std::mutex> lock(g_pool.mu);
        changed = g_pool.stream != (hipStream_t)stream;
    }
    if (changed) HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lock(g_pool.mu);
    g_pool.stream = (hipStream_t)stream;
    if (changed)
        for (auto& per_dev : g_pool.free_blocks)
            for (auto& b : per_dev.second) b.second.freed_on = g_pool.stream;
    return 0;
}
int bbt_pool_info(int64_t* cached_bytes, int64_t* live_bytes) {
    std::lock_guard<std::mutex> lock(g_pool.mu);
    if (cached_bytes) *cached_bytes = (int64_t)g_pool.cached;
    if (live_bytes) {
        size_t n = 0;
        for (auto& l : g_pool.live) n += l.second.first;
        *live_bytes = (int64_t)n;
    }
    return 0;
}
int bbt_host_alloc(void** host_ptr, size_t nbytes) {
    ARG_TRY(host_ptr, "bbt_host_alloc: null argument");
    HIP_TRY(hipHostMalloc(host_ptr, nbytes ? nbytes : 1, hipHostMallocDefault));
    return 0;
}
int bbt_host_free(void* host_ptr) {
    if (host_ptr) HIP_TRY(hipHostFree(host_ptr));
    return 0;
}
int bbt_host_register(void* host_ptr, size_t nbytes) {
    ARG_TRY(host_ptr && nbytes, "bbt_host_register: null or empty range");
    HIP_TRY(hipHostRegister(host_ptr, nbytes, hipHostRegisterDefault));
    return 0;
}
int bbt_host_unregister(void* host_ptr) {
    if (host_ptr) HIP_TRY(hipHostUnregister(host_ptr));
    return 0;
}
int bbt_memset(void* dev_ptr, int value, size_t nbytes, bbt_stream stream) {
    HIP_TRY(hipMemsetAsync(dev_ptr, value, nbytes, (hipStream_t)stream));
    return 0;
}
int bbt_memcpy_h2d(void* dst, const void* src, size_t n, bbt_stream s) {
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, (hipStream_t)s));
    return 0;
}
int bbt_memcpy_d2h(void* dst, const void* src, size_t n, bbt_stream s) {
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, (hipStream_t)s));
    return 0;
}
int bbt_memcpy_d2d(void* dst, const void* src, size_t n, bbt_stream s) {
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return 0;
}
int bbt_memcpy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                 size_t height, int kind, bbt_stream s) {
    ARG_TRY(kind >= 0 && kind <= 2, "bbt_memcpy2d: kind must be 0 (h2d), 1 (d2h) or 2 (d2d)");
    const hipMemcpyKind k = kind == 0   ? hipMemcpyHostToDevice
                            : kind == 1 ? hipMemcpyDeviceToHost
                                        : hipMemcpyDeviceToDevice;
    if (width == 0 || height == 0) return 0;
    if (kind == 2) {
        // on the device: our own copy kernel when everything is a multiple of 4 bytes
        const uintptr_t all = (uintptr_t)dst | (uintptr_t)src | dpitch | spitch | width;
        const int eb = all % 16 == 0 ? 16 : (all % 8 == 0 ? 8 : (all % 4 == 0 ? 4 : 0));
        const long long wpr = eb ? (long long)(width / eb) : 0;
        int lg_le = 0;
        while ((1ll << lg_le) < wpr && lg_le < 8) ++lg_le;
        const long long rows_per_block = (256 >> lg_le) * 4;
        const long long gx = ((long long)height + rows_per_block - 1) / rows_per_block;
        const long long gy = (wpr + (1 << lg_le) - 1) >> lg_le;
        if (eb && wpr < (1ll << 31) && gx < (1ll << 31) && gy <= 65535) {
            const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
            hipStream_t st = (hipStream_t)s;
            if (eb == 16)
                hipLaunchKernelGGL((k_copy2d<float4>), grid, block, 0, st, (const float4*)src, (float4*)dst,
                                   (long long)height, (int)wpr, (int)wpr, (long long)(spitch / 16),
                                   (long long)(dpitch / 16), lg_le);
            else if (eb == 8)
                hipLaunchKernelGGL((k_copy2d<float2>), grid, block, 0, st, (const float2*)src, (float2*)dst,
                                   (long long)height, (int)wpr, (int)wpr, (long long)(spitch / 8),
                                   (long long)(dpitch / 8), lg_le);
            else
                hipLaunchKernelGGL((k_copy2d<float>), grid, block, 0, st, (const float*)src, (float*)dst,
                                   (long long)height, (int)wpr, (int)wpr, (long long)(spitch / 4),
                                   (long long)(dpitch / 4), lg_le);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, k, (hipStream_t)s));
    return 0;
}
int bbt_pad_streams(const void* in_dev, void* out_dev, int64_t n_rows, int n_in, int n_out,
                    int elem_bytes, bbt_stream s) {
    ARG_TRY(in_dev && out_dev, "bbt_pad_streams: null argument");
    ARG_TRY(n_rows >= 0 && n_in >= 1 && n_out >= n_in, "bbt_pad_streams: bad sizes");
    ARG_TRY(elem_bytes == 4 || elem_bytes == 8, "bbt_pad_streams: elem_bytes must be 4 or 8");
    if (n_rows == 0) return 0;
    int lg_le = 0;
    while ((1 << lg_le) < n_out && lg_le < 8) ++lg_le;
    const long long rows_per_block = (256 >> lg_le) * 4;
    const long long gx = (n_rows + rows_per_block - 1) / rows_per_block;
    const long long gy = ((long long)n_out + (1 << lg_le) - 1) >> lg_le;
    ARG_TRY(gx < (1ll << 31) && gy <= 65535, "bbt_pad_streams: too many elements for one call");
    const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    if (elem_bytes == 8)
        hipLaunchKernelGGL((k_copy2d<float2>), grid, block, 0, (hipStream_t)s, (const float2*)in_dev,
                           (float2*)out_dev, (long long)n_rows, n_out, n_in, (long long)n_in,
                           (long long)n_out, lg_le);
    else
        hipLaunchKernelGGL((k_copy2d<float>), grid, block, 0, (hipStream_t)s, (const float*)in_dev,
                           (float*)out_dev, (long long)n_rows, n_out, n_in, (long long)n_in,
                           (long long)n_out, lg_le);
    HIP_TRY(hipGetLastError());
    return 0;
}
int bbt_stream_create(bbt_stream* stream) {
    ARG_TRY(stream, "bbt_stream_create: null argument");
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (bbt_stream)s;
    return 0;
}
int bbt_stream_destroy(bbt_stream stream) {
    if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return 0;
}
int bbt_stream_sync(bbt_stream stream) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
int bbt_device_sync(void) {
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}
int bbt_event_create(bbt_event* ev) {
    ARG_TRY(ev, "bbt_event_create: null argument");
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *ev = (bbt_event)e;
    return 0;
}
int bbt_event_create_ordering(bbt_event* ev) {
    ARG_TRY(ev, "bbt_event_create_ordering: null argument");
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    *ev = (bbt_event)e;
    return 0;
}
int bbt_event_destroy(bbt_event ev) {
    if (ev) HIP_TRY(hipEventDestroy((hipEvent_t)ev));
    return 0;
}
int bbt_event_record(bbt_event ev, bbt_stream stream) {
    HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return 0;
}
int bbt_event_sync(bbt_event ev) {
    HIP_TRY(hipEventSynchronize((hipEvent_t)ev));
    return 0;
}
int bbt_event_query(bbt_event ev, int* done) {
    ARG_TRY(ev && done, "bbt_event_query: null argument");
    const hipError_t e = hipEventQuery((hipEvent_t)ev);
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        *done = 0;
        return 0;
    }
    HIP_TRY(e);
    *done = 1;
    return 0;
}
int bbt_stream_wait_event(bbt_stream stream, bbt_event ev) {
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
    return 0;
}
int bbt_event_elapsed_ms(bbt_event start, bbt_event stop, float* ms) {
    ARG_TRY(ms, "bbt_event_elapsed_ms: null argument");
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// overlap-save spectral multiply
// short-response convolution in the time domain (entry points further down)
struct bbt_fir_plan {
    int n_tap = 0, S = 0, npair = 0;
    int n_chunks = 0, pitch = 0, tap_pitch = 0;
    bool cplx = false;
    float2* tre = nullptr;
    float2* tim = nullptr;
};
static constexpr int BBT_FIR_R = 8;

// Events that only order streams of this device among each other (fork / join of the lanes, end
// of a call) and the per-pass timing events: no system-scope fence.  A default HIP event writes
// the caches back and invalidates them when it is recorded -- at every call boundary that emptied
// the Infinity Cache under the work buffers and cost both lanes 0.2-0.6 ms (round 4, measured:
// the lanes stood still after the last kernel of a call even with no cross-stream wait queued).
#define BBT_EV_ORDER (hipEventDisableTiming | hipEventDisableSystemFence)
struct bbt_osm_plan {
    // One call at a time per plan: the lanes' work buffers, the seam buffer,
    // the fork/join events and the timing vectors belong to the running call.
    std::mutex mu;
    int device = 0;
    int64_t n = 0;
    int S = 0, npair = 0, C = 0;
    // one stream (S == 1): pairs are made of two consecutive blocks (see SinglePair);
    // npair == 1 and the work buffers hold (chunk + 1) / 2 pairs of blocks
    bool single = false;
    int n1 = 1, n2 = 0;
    int outer = 1;  // 256 for three-level transforms (N > 2^20): N = outer * n1 * n2
    int chunk = 1;
    int cap = 1;                // blocks a lane's work buffer holds (>= chunk): regular runs go in launches of up to that many
    cf* resp = nullptr;        // [C][N1][N2], scaled 1/N
    int* resp_index = nullptr;  // [S]
    float2* work = nullptr;     // [chunk][npair][N1][N2] float4 (lane 0)
    size_t work_bytes = 0;      // per lane
    // Chunks alternate between `lanes` internal streams, each with its own
    // work buffer, so kernels of different chunks overlap: the bandwidth-bound
    // column passes of one chunk run beside the latency-bound row pass of
    // another and fill each other's launch tails.
    int lanes = 1;
    float2* lane_work[BBT_MAX_LANES] = {};
    hipStream_t lane_stream[BBT_MAX_LANES] = {};
    hipEvent_t ev_fork = nullptr, ev_join[BBT_MAX_LANES] = {};
    hipEvent_t ev_done = nullptr;   // end of the previous execute call (on whatever stream it ran)
    bool ev_done_set = false;
    // Deferred join (bbt_osm_plan_defer): a call that was given a completion event does not order
    // the caller's stream after its lanes.  The lanes then run on into the next call -- no drain
    // at the call boundary -- and what has to come after them (the seam pass of the fused
    // channelizer, the completion event) is queued on `tail_stream`.  Chunks keep alternating
    // between the lanes across calls (`lane_cursor`); the seam buffer has two turns so that the
    // seam pass of call i may still read its slots while the lanes of call i + 1 fill the others.
    hipStream_t tail_stream = nullptr;
    hipEvent_t defer_ev = nullptr;          // handed in for the NEXT execute call only
    bool last_forked_deferred = false;      // the previous call left its lanes unjoined
    int lane_cursor = 0;
    hipEvent_t ev_tail[2] = {nullptr, nullptr};   // seam pass of the last deferred call on turn i
    bool ev_tail_set[2] = {false, false};
    int seam_turn = 0;
    FftTables tab2;  // for N2
    FftTables tab1;  // for N1 == 256
    // four-step twiddles of two-level plans as tables (owned): W_{16 N1}^{k1 j} [N1][16] and
    // W_N^{k1 tau} [N1][N2 / 16]
    cf* tw4row = nullptr;
    cf* tw4base = nullptr;
    // three-level plans with the fused channelizer: the outer four-step factors of the row pass,
    // tw4o [outer][n2 / 16] = W_N^{tau k1o}, tw4u [outer][n1][16] = W_{16 n1}^{k1 j} W_65536^{k1o j}
    cf* tw4o = nullptr;
    cf* tw4u = nullptr;
    // the same twiddles applied by the 256-point column passes instead (col_twiddles):
    // twa [16][n2] = W_N^{tau n2}, twg [4][n2] = W_N^{16 n2 2^i}; BBT_OSM_TW_COL=0/1
    bool tw_col = false;
    cf* twa = nullptr;
    cf* twg = nullptr;
    cf* wroot = nullptr;
    cf* big_tw = nullptr;       // one-kernel plans of 8192 / 16384 samples (big_kernels.hpp): the transform's table (shared)
    // block lengths that are not powers of two (gen_kernels.hpp): N = n1 * n2,
    // n1 == 1 for N <= 8192
    bool generic = false;
    GenGeo g1 = {}, g2 = {}, g2r = {};      // g2r: the stages of g2 reversed (inverse of the row transform)
    cf* wn2r = nullptr;
    cf* wn1 = nullptr;          // W_{n1}^k (shared table)
    cf* wn2 = nullptr;          // W_{n2}^k (shared table)
    cf* tlo = nullptr;          // W_N^i, i < 4096        (owned)
    cf* thi = nullptr;          // W_N^{4096 j}           (owned)
    cf* tws = nullptr;          // W_N^{k1 m r}, [n1][g2.fac[0]], m = n2 / g2.fac[0]   (owned)
    int gen_ct = 1;             // columns per tile of the column passes
    // the same plan on the run-time specialised engine (gen2_kernels.hpp; null functions: not in use)
    bool rtc = false;
    G2Plan q1, q2, q2r;         // column transform (ct columns), row transform and its reversal
    cf* qw1 = nullptr;          // their stage tables (shared)
    cf* qw2 = nullptr;
    cf* qw2r = nullptr;
    hipFunction_t k2_small = nullptr, k2_first = nullptr, k2_row = nullptr, k2_last = nullptr;
    int n2p = 0;                // pitch of a row of the work buffer: n2 rounded up to whole 128-byte lines
    // pair-planar hand-over (bbt_osm_plan_set_layout; OsmChunk::in_plane / out_plane)
    long long in_plane = 0, out_plane = 0;
    // fused channelizer
    float2* seam = nullptr;     // [blocks][2][npair][n_chan] float4 (the turn in use)
    float2* seam_buf[2] = {nullptr, nullptr};
    size_t seam_bytes[2] = {0, 0};
    // the launches of the chunk being run (osm_launch.hpp; reused: no allocation in steady state)
    OsmKnobs knobs;
    std::vector<OsmLaunch> chunk_launches;

    // timing
    bool timing = false;
    bool timing_isolated = false;   // mode 2: single lane, passes do not overlap
    std::vector<hipEvent_t> ev;  // 4 per chunk launch: t0, tA, tB, tC
    std::vector<hipEvent_t> ev_free;   // recycled events
    int timing_stride = 4;          // events on every timing_stride-th chunk of a lane
    int64_t pass_launches[3] = {0, 0, 0};
    int64_t pass_blocks[3] = {0, 0, 0};      // blocks the timed launches of each pass covered
    std::vector<int> ev_nblk;                // lanes schedule: blocks of each timed chunk launch
    double acc_ms[3] = {0, 0, 0};
    int64_t launches = 0;
};

static int osm_flush_timing(bbt_osm_plan* p) {
    for (size_t i = 0; i + 3 < p->ev.size(); i += 4) {
        HIP_TRY(hipEventSynchronize(p->ev[i + 3]));
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, p->ev[i + k], p->ev[i + k + 1]));
            p->acc_ms[k] += ms;
            p->pass_launches[k] += 1;
            p->pass_blocks[k] += p->ev_nblk[i / 4];
        }
        p->launches += 1;
    }
    for (auto e : p->ev) p->ev_free.push_back(e);
    p->ev.clear();
    p->ev_nblk.clear();
    return 0;
}

// ---- running a chunk: the launches osm_launch.hpp lists ------------------------------------------
static_assert(fft_lds_elems(256) == FftGeo<256>::LDS_ELEMS && fft_lds_elems(512) == FftGeo<512>::LDS_ELEMS &&
                  fft_lds_elems(1024) == FftGeo<1024>::LDS_ELEMS && fft_lds_elems(2048) == FftGeo<2048>::LDS_ELEMS &&
                  fft_lds_elems(4096) == FftGeo<4096>::LDS_ELEMS && big_lds_elems(8192) == BigGeo<8192>::LDS_ELEMS &&
                  big_lds_elems(16384) == BigGeo<16384>::LDS_ELEMS && sizeof(v2) == 8 && sizeof(f4) == 16,
              "osm_launch.hpp: the exchange areas are not the templates'");

// One launch of the list: the only place that names the kernels of a chunk.  `chw`: the chunk as
// the row pass counts it (one stream: pairs of blocks).  A combination of parameters that has no
// instantiation is an error.
static int osm_dispatch(bbt_osm_plan* p, const OsmLaunch& l, const float2* in, float2* out, float2* work,
                        const OsmChunk& ch, const OsmChunk& chw, const SpecOut& so, hipStream_t st) {
    const dim3 grid(l.gx, l.gy), block(l.threads);
    const int S = l.single ? 1 : p->S;
#define BBT_GO(KERNEL_, ...)                                                      \
    {                                                                             \
        if (l.raise_lds && ensure_dyn_lds((const void*)KERNEL_, l.lds)) return 1; \
        hipLaunchKernelGGL(KERNEL_, grid, block, l.lds, st, __VA_ARGS__);         \
        return 0;                                                                 \
    }
    switch (l.family) {
        case OSM_COL16:
#define BBT_COL16(FIRST_, SPEC_, SINGLE_, PP_)                                      \
    if (l.first == FIRST_ && l.spec == SPEC_ && l.single == SINGLE_ && l.pp == PP_) \
        BBT_GO((k_osm_col16<FIRST_, SPEC_, SINGLE_, PP_>), in, out, work, ch, S, p->n2, so)
            BBT_COL16(true, false, true, 1) BBT_COL16(true, false, false, 8) BBT_COL16(true, false, false, 1)
            BBT_COL16(false, true, true, 1) BBT_COL16(false, false, true, 1) BBT_COL16(false, true, false, 8)
            BBT_COL16(false, false, false, 8) BBT_COL16(false, true, false, 1) BBT_COL16(false, false, false, 1)
#undef BBT_COL16
            break;
        case OSM_COL256: {
            SpecOut so_tw = so;
            if (l.tw) {
                so_tw.twa = p->twa;
                so_tw.twg = p->twg;
            }
            // (forward, spectra out, columns, detection, pairs, one stream, column length) -> instantiation
#define BBT_COL256(FIRST_, SPEC_, F_, DET_, PP_, SINGLE_, N1_)                                                           \
    if (l.first == FIRST_ && l.spec == SPEC_ && l.F == F_ && l.det == DET_ && l.pp == PP_ && l.single == SINGLE_ &&      \
        l.n == N1_)                                                                                                      \
        BBT_GO((k_osm_col256<FIRST_, SPEC_, F_, DET_, PP_, SINGLE_, N1_>), in, out, work, ch, S, l.row_len, p->tab1.tw0, \
               so_tw, N1_ == 256 ? nullptr : p->tab1.tw1)
#define BBT_COL256_PASS(FIRST_, SPEC_)                                                                     \
    BBT_COL256(FIRST_, SPEC_, 8, false, 1, true, 512) BBT_COL256(FIRST_, SPEC_, 8, false, 1, false, 512)   \
    BBT_COL256(FIRST_, SPEC_, 8, false, 1, true, 1024) BBT_COL256(FIRST_, SPEC_, 8, false, 1, false, 1024) \
    BBT_COL256(FIRST_, SPEC_, 16, false, 1, true, 256) BBT_COL256(FIRST_, SPEC_, 16, false, 1, false, 256) \
    BBT_COL256(FIRST_, SPEC_, (FIRST_ ? 64 : 32), false, 8, false, 256)
            BBT_COL256_PASS(true, false) BBT_COL256_PASS(false, true) BBT_COL256_PASS(false, false)
            BBT_COL256(false, true, 16, true, 1, false, 256)
            BBT_COL256(true, false, 64, false, 4, false, 256)
            BBT_COL256(false, true, 16, false, 4, false, 256) BBT_COL256(false, false, 16, false, 4, false, 256)
#undef BBT_COL256_PASS
#undef BBT_COL256
            break;
        }
        case OSM_ROWPASS:
            // (row length, channels) -> instantiation; nch == 0 is the plain row pass.
#define BBT_RP(N2_, NCH_)                                                                                           \
    if (l.n == N2_ && l.nch == NCH_)                                                                                \
        BBT_GO((k_osm_rowpass<N2_, NCH_>), work, p->n1, p->resp, p->resp_index, p->npair, p->tab2.tw0, p->tab2.tw1, \
               p->wroot, chw, p->outer, l.y0, p->tw4row, p->tw4base, p->tw_col ? (NCH_ ? 1 : 3) : 0, p->tw4o, p->tw4u)
            BBT_RP(256, 0) BBT_RP(512, 0) BBT_RP(1024, 0) BBT_RP(2048, 0) BBT_RP(4096, 0)
            BBT_RP(256, 2) BBT_RP(256, 4) BBT_RP(256, 8) BBT_RP(512, 2) BBT_RP(512, 4) BBT_RP(512, 8)
            BBT_RP(1024, 2) BBT_RP(1024, 4) BBT_RP(1024, 8) BBT_RP(2048, 2) BBT_RP(2048, 4) BBT_RP(2048, 8)
            BBT_RP(4096, 2) BBT_RP(4096, 4) BBT_RP(4096, 8)
            BBT_RP(256, 16) BBT_RP(256, 32) BBT_RP(256, 64) BBT_RP(256, 128)
            BBT_RP(512, 16) BBT_RP(512, 32) BBT_RP(512, 64) BBT_RP(512, 128)
            BBT_RP(1024, 16) BBT_RP(1024, 32) BBT_RP(1024, 64) BBT_RP(1024, 128)
            BBT_RP(2048, 16) BBT_RP(2048, 32) BBT_RP(2048, 64) BBT_RP(2048, 128)
            BBT_RP(4096, 16) BBT_RP(4096, 32) BBT_RP(4096, 64) BBT_RP(4096, 128)
            BBT_RP(256, 256)
            BBT_RP(512, 256) BBT_RP(512, 512)
            BBT_RP(1024, 256) BBT_RP(1024, 512) BBT_RP(1024, 1024)
            BBT_RP(2048, 256) BBT_RP(2048, 512) BBT_RP(2048, 1024) BBT_RP(2048, 2048)
            BBT_RP(4096, 256) BBT_RP(4096, 512) BBT_RP(4096, 1024) BBT_RP(4096, 2048) BBT_RP(4096, 4096)
#undef BBT_RP
            return fail("osm: no row pass for row length %d with %d channels", l.n, l.nch);
        case OSM_MID16:
            if (l.first) BBT_GO((k_osm_mid16<true>), work, p->n2, (int)p->n, p->wroot, l.mid_mode, l.y0)
            BBT_GO((k_osm_mid16<false>), work, p->n2, (int)p->n, p->wroot, l.mid_mode, l.y0)
        case OSM_SMALL:
#define BBT_SM(N_, PP_, SINGLE_)                         \
    if (l.n == N_ && l.pp == PP_ && l.single == SINGLE_) \
        BBT_GO((k_osm_small<N_, PP_, SINGLE_>), in, out, ch, S, p->resp, p->resp_index, p->tab2.tw0, p->tab2.tw1)
#define BBT_SM_N(N_) BBT_SM(N_, 1, true) BBT_SM(N_, 1, false) BBT_SM(N_, 2, false) BBT_SM(N_, 4, false)
            BBT_SM_N(256) BBT_SM_N(512) BBT_SM_N(1024) BBT_SM_N(2048) BBT_SM_N(4096)
            BBT_SM(256, 8, false) BBT_SM(512, 8, false) BBT_SM(1024, 8, false) BBT_SM(2048, 8, false)
#undef BBT_SM_N
#undef BBT_SM
            break;
        case OSM_SMALL_BIG:
#define BBT_SB(N_, SINGLE_)               \
    if (l.n == N_ && l.single == SINGLE_) \
        BBT_GO((k_osm_small_big<N_, SINGLE_>), in, out, ch, S, p->resp, p->resp_index, p->big_tw)
            BBT_SB(8192, true) BBT_SB(8192, false) BBT_SB(16384, true) BBT_SB(16384, false)
#undef BBT_SB
            break;
        case OSM_GEN_SMALL:
            BBT_GO(k_gen_osm_small, in, out, ch, p->S, p->resp, p->resp_index, p->g2, p->wn2, p->g2r, p->wn2r)
        case OSM_GEN_COL:
            if (l.first) BBT_GO((k_gen_col<true>), in, out, work, ch, p->S, p->n2, p->gen_ct, p->g1, p->wn1)
            BBT_GO((k_gen_col<false>), in, out, work, ch, p->S, p->n2, p->gen_ct, p->g1, p->wn1)
        case OSM_GEN_ROW:
            BBT_GO(k_gen_row, work, p->n1, p->resp, p->resp_index, p->npair, p->g2, p->wn2, p->g2r, p->wn2r, p->tlo,
                   p->thi, p->tws)
        case OSM_G2_SMALL:
            return g2_launch(p->k2_small, grid, block, st, (const float2*)in, out, ch, p->S, (const cf*)p->resp,
                             (const int*)p->resp_index, (const cf*)p->qw2, (const cf*)p->qw2r);
        case OSM_G2_FIRST:
        case OSM_G2_LAST:
            return g2_launch(l.family == OSM_G2_FIRST ? p->k2_first : p->k2_last, grid, block, st, (const float2*)in, out,
                             work, ch, p->S, p->n2, p->n2p, (const cf*)p->qw1);
        case OSM_G2_ROW:
            return g2_launch(p->k2_row, grid, block, st, work, p->n1, p->n2p, (const cf*)p->resp,
                             (const int*)p->resp_index, p->npair, (const cf*)p->qw2, (const cf*)p->qw2r,
                             (const cf*)p->tlo, (const cf*)p->thi, (const cf*)p->tws);
    }
#undef BBT_GO
    return fail("osm: no %s kernel for this plan (%d, %d pairs per workgroup, %d columns)", osm_family_name(l.family),
                l.n, l.pp, l.F);
}

static int osm_run_chunk(bbt_osm_plan* p, const float2* in, float2* out, const OsmChunk& ch_given,
                         const SpecOut& so, float2* work, hipStream_t st, bool sample = true) {
    OsmChunk ch = ch_given;
    ch.in_plane = p->in_plane;
    ch.out_plane = p->out_plane;
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    const bool timed = p->timing && sample;       // (events on this chunk's kernels)
    if (timed) {
        for (int i = 0; i < 4; ++i) {
            if (!p->ev_free.empty()) {
                e[i] = p->ev_free.back();
                p->ev_free.pop_back();
            } else {
                HIP_TRY(hipEventCreateWithFlags(&e[i], hipEventDisableSystemFence));
            }
        }
        HIP_TRY(hipEventRecord(e[0], st));
    }
    OsmLaunchPlan lp;
    lp.n = p->n;
    lp.generic = p->generic;
    lp.rtc = p->rtc;
    lp.single = p->single;
    lp.outer = p->outer;
    lp.n1 = p->n1;
    lp.n2 = p->n2;
    lp.n2p = p->n2p;
    lp.npair = p->npair;
    lp.S = p->S;
    lp.gen_ct = p->gen_ct;
    lp.q1_threads = p->q1.threads();
    lp.q1_ct = p->q1.ct;
    lp.q2_threads = p->q2.threads();
    lp.q2_ct = p->q2.ct;
    lp.tw_col = p->tw_col;
    OsmChunkFacts facts;
    facts.nblk = ch.nblk;
    facts.reg_count = ch.reg_count;
    facts.n_chan = so.n_chan;       // 0: plain overlap-save output
    facts.det = so.det != nullptr;
    facts.in_plane = ch.in_plane != 0;
    facts.timing = p->timing;
    if (const char* refusal = osm_chunk_launches(lp, facts, p->knobs, &p->chunk_launches)) return fail("%s", refusal);
    OsmChunk pairs_view;               // one stream: the work buffers hold pairs of blocks
    if (p->single) {
        pairs_view = ch;
        pairs_view.nblk = (ch.nblk + 1) / 2;
    }
    const OsmChunk& chw = p->single ? pairs_view : ch;       // what the row pass counts
    for (const OsmLaunch& l : p->chunk_launches) {
        if (osm_dispatch(p, l, in, out, work, ch, chw, so, st)) return 1;
        if (timed && (l.mark & 1)) HIP_TRY(hipEventRecord(e[1], st));
        if (timed && (l.mark & 2)) HIP_TRY(hipEventRecord(e[2], st));
    }
    HIP_TRY(hipGetLastError());
    if (timed) {
        HIP_TRY(hipEventRecord(e[3], st));
        for (int i = 0; i < 4; ++i) p->ev.push_back(e[i]);
        p->ev_nblk.push_back(ch.nblk);
        if (p->ev.size() >= 65536) return osm_flush_timing(p);   // (a flush waits for the events)
    }
    return 0;
}

// One execute call at a time per plan -- on the host (the mutex) and on the
// device: the work, staging and seam buffers belong to the running call, so a
// call queued on another stream than the previous one first waits for that
// call's last kernel.
//
// Deferred calls (bbt_osm_plan_defer) are the exception: a forking call that was
// given a completion event leaves the caller's stream unordered with respect to
// its lanes, and the next forking deferred call does not wait for it either --
// the lanes are in-order queues, a lane's work buffer is only ever touched from
// that lane, and everything else (the seam buffer) has two turns.  `fin` is the
// stream on which such a call ends: whatever must follow the lanes goes there.
// The completion event handed in by bbt_osm_plan_defer belongs to the NEXT execute call on the
// plan, whatever becomes of that call: every entry point takes it first thing, and if the call
// returns before anything was queued (an argument error, nothing to do) the event is recorded on
// the caller's stream as it stands.
struct DeferTake {
    hipEvent_t ev = nullptr;
    hipStream_t st;
    DeferTake(bbt_osm_plan* p, hipStream_t stream) : st(stream) {
        if (!p) return;
        std::lock_guard<std::mutex> lock(p->mu);
        ev = p->defer_ev;
        p->defer_ev = nullptr;
    }
    hipEvent_t hand_over() {
        hipEvent_t e = ev;
        ev = nullptr;
        return e;
    }
    void give_back(bbt_osm_plan* p) {        // (for an entry point that ends in another one)
        std::lock_guard<std::mutex> lock(p->mu);
        p->defer_ev = hand_over();
    }
    ~DeferTake() {
        if (ev) (void)hipEventRecord(ev, st);
    }
};

struct PlanCall {
    bbt_osm_plan* p;
    hipStream_t st;
    std::lock_guard<std::mutex> lock;
    hipEvent_t defer;           // the caller's completion event, or null
    bool fork;                  // chunks go to the lane streams
    bool deferred;              // ... and `st` is not joined after them
    hipStream_t fin;            // where the call ends
    hipStream_t run;            // where chunks that are not forked run: `st`, or -- a deferred call of a
                                // plan without lanes (one kernel per chunk) -- the tail stream, so that
                                // what the caller queues on `st` next (the upstream task's kernels for
                                // the following run) overlaps it
    PlanCall(bbt_osm_plan* plan, DeferTake& take, int64_t n_blocks)
        : p(plan), st(take.st), lock(plan->mu), defer(take.hand_over()) {
        const int64_t n_chunks = (n_blocks + p->chunk - 1) / p->chunk;
        const bool usual = !(p->timing && p->timing_isolated);
        const bool lanes_ok = p->lanes > 1 && usual && n_chunks > 0;
        const bool aside = p->lanes == 1 && usual;
        deferred = defer && p->tail_stream && (lanes_ok || aside);
        fork = lanes_ok && (n_chunks > 1 || deferred);
        fin = deferred ? p->tail_stream : st;
        run = deferred && !fork ? p->tail_stream : st;
        // (two deferred calls in a row: nothing of the earlier one is touched outside the lanes'
        // -- the tail stream's -- own order, see above)
        if (p->ev_done_set && !(deferred && p->last_forked_deferred))
            (void)hipStreamWaitEvent(st, p->ev_done, 0);
        if (run != st) {                   // the tail stream takes over from the caller's
            (void)hipEventRecord(p->ev_fork, st);
            (void)hipStreamWaitEvent(run, p->ev_fork, 0);
        }
    }
    ~PlanCall() {
        if (defer) (void)hipEventRecord(defer, fin);
        if (hipEventRecord(p->ev_done, fin) == hipSuccess) p->ev_done_set = true;
        p->last_forked_deferred = deferred;
    }
};

// Run all chunks, alternating lanes.  Returns with `call.st` ordered after every lane, or -- a
// deferred call -- with `call.fin` (the plan's tail stream) ordered after them instead.
template <class FillChunk>
static int osm_run_all(bbt_osm_plan* p, const float2* in, float2* out, int64_t n_blocks,
                       const SpecOut& so, const PlanCall& call, FillChunk fill) {
    hipStream_t st = call.st;
    const bool fork = call.fork;
    if (fork) {
        HIP_TRY(hipEventRecord(p->ev_fork, st));
        for (int l = 0; l < p->lanes; ++l) HIP_TRY(hipStreamWaitEvent(p->lane_stream[l], p->ev_fork, 0));
    }
    // (lanes keep alternating across deferred calls; a joined call starts on lane 0 as ever)
    const int l0 = call.deferred ? p->lane_cursor : 0;
    // regular runs (the fused channelizer's per-block shift and seam slot follow from the hop: osm_block)
    const bool regular_ok = osm_regular_ok(p->chunk, p->cap);
    const int mask = so.n_chan ? so.n_chan - 1 : 0;
    int64_t c = 0;
    auto launch = [&](const OsmChunk& ch) {
        const int l = fork ? (int)((l0 + c) % p->lanes) : 0;
        const bool sample = !fork || (c / p->lanes) % p->timing_stride == 0;
        ++c;
        return osm_run_chunk(p, in, out, ch, so, p->lane_work[l], fork ? p->lane_stream[l] : call.run, sample);
    };
    for (int64_t b0 = 0; b0 < n_blocks;) {
        OsmChunk ch = {};                  // (fields a caller's fill does not set stay 0)
        fill(ch.b[0], b0);
        int64_t run = 1;                   // blocks from b0 on that step regularly
        long long hop = 0;
        if (regular_ok && b0 + p->chunk < n_blocks) {
            OsmBlock nx = {};
            fill(nx, b0 + 1);
            hop = nx.in_off - ch.b[0].in_off;
            if (hop > 0 && osm_follows(ch.b[0], nx, hop, mask))
                for (run = 2; b0 + run < n_blocks; ++run) {
                    fill(nx, b0 + run);
                    if (!osm_follows(ch.b[0], nx, hop * run, mask)) break;
                }
        }
        if (run > p->chunk) {
            int64_t parts, per;            // (launches of equal size: osm_geo.hpp)
            osm_run_parts(run, p->chunk, p->cap, p->lanes, fork, &parts, &per);
            const OsmBlock first = ch.b[0];
            for (int64_t r0 = 0; r0 < run; r0 += per) {
                OsmChunk rc = {};
                rc.b[0] = first;
                rc.b[0].in_off += r0 * hop;
                rc.b[0].out_off += r0 * hop;
                rc.b[0].shift = (int)(((long long)first.shift - r0 * hop) & mask);
                rc.b[0].index = first.index + (int)r0;
                rc.reg_count = rc.nblk = (int)std::min(per, run - r0);
                rc.reg_hop = hop;
                rc.reg_mask = mask;
                if (launch(rc)) return 1;
            }
            b0 += run;
            continue;
        }
        ch.nblk = (int)((n_blocks - b0 < p->chunk) ? (n_blocks - b0) : p->chunk);
        for (int i = 1; i < ch.nblk; ++i) fill(ch.b[i], b0 + i);
        if (launch(ch)) return 1;
        b0 += ch.nblk;
    }
    if (fork) {
        if (call.deferred) p->lane_cursor = (int)((l0 + c) % p->lanes);
        for (int l = 0; l < p->lanes; ++l) {
            HIP_TRY(hipEventRecord(p->ev_join[l], p->lane_stream[l]));
            HIP_TRY(hipStreamWaitEvent(call.fin, p->ev_join[l], 0));
        }
    }
    return 0;
}

static int osm_check_blocks(const bbt_osm_plan* p, const char* who, int64_t n_blocks,
                            const int64_t* in_off, const int64_t* out_off,
                            const int32_t* valid_start, const int32_t* valid_count) {
    ARG_TRY(n_blocks >= 0, "%s: n_blocks=%lld < 0", who, (long long)n_blocks);
    ARG_TRY(n_blocks == 0 || (in_off && out_off && valid_start && valid_count),
            "%s: null descriptor array", who);
    for (int64_t b = 0; b < n_blocks; ++b) {
        ARG_TRY(in_off[b] >= 0 && out_off[b] >= 0, "%s: negative offset in block %lld", who,
                (long long)b);
        ARG_TRY(valid_start[b] >= 0 && valid_count[b] >= 0 &&
                    (int64_t)valid_start[b] + valid_count[b] <= p->n,
                "%s: block %lld keeps [%d, %d) outside [0, %lld)", who, (long long)b,
                valid_start[b], valid_start[b] + valid_count[b], (long long)p->n);
    }
    return 0;
}

template <int NCH>
static void launch_seam_fix(bbt_osm_plan* p, float2* out, const std::vector<SeamJob>& jobs,
                            const FftTables& tab, const SpecOut& so, hipStream_t st) {
    for (size_t j0 = 0; j0 < jobs.size(); j0 += BBT_SEAM_JOBS_PER_LAUNCH) {
        SeamJobs batch;
        const size_t n = std::min(jobs.size() - j0, (size_t)BBT_SEAM_JOBS_PER_LAUNCH);
        for (size_t i = 0; i < n; ++i) batch.j[i] = jobs[j0 + i];
        if (p->single)
            hipLaunchKernelGGL((k_seam_fix<NCH, true>), dim3((unsigned)n, 1), dim3(NCH / 16), 0, st, p->seam,
                               out, batch, 1, 1, tab.tw0, tab.tw1, so);
        else
            hipLaunchKernelGGL((k_seam_fix<NCH>), dim3((unsigned)n, p->npair), dim3(NCH / 16), 0, st,
                               p->seam, out, batch, p->S, p->npair, tab.tw0, tab.tw1, so);
    }
}

// ---- making a plan: what osm_geo.hpp decided, put on the device ----------------------------------
// The kernels specialised on a generic length (fft_gen2.hpp), compiled now; if that is not
// possible the plan runs on the general ones.  `why_not`: osm_levels found no plan for them.
// 1: an error (BBT_RTC=require), else p->rtc says whether they are in use.
static int osm_compile(bbt_osm_plan* p, const OsmGeo& geo, const OsmKnobs& knobs, const std::string& why_not) {
    bool ok = geo.compiled;
    if (!ok) fail("%s", why_not.c_str());
    if (ok) {
        const OsmSource src = osm_g2_source(geo);
        hipFunction_t f[3] = {};
        ok = !g2_build(src.text, src.names, f);
        if (ok && p->n1 == 1) {
            p->k2_small = f[0];
        } else if (ok) {
            p->k2_row = f[0];
            p->k2_first = f[1];
            p->k2_last = f[2];
        }
    }
    if (ok) ok = !(get_g2_table(p->q2, &p->qw2) || get_g2_table(p->q2r, &p->qw2r) ||
                   (p->n1 > 1 && get_g2_table(p->q1, &p->qw1)));
    if (!ok && knobs.rtc == 2) return 1;
    if (!ok) g2_warn_once("bbt_osm_plan_create");
    p->rtc = ok;
    return 0;
}

// Tables of a generic plan: the stages of both factors and the four-step twiddles between them.
static int osm_generic_tables(bbt_osm_plan* p, const OsmGeo& geo, const OsmKnobs& knobs, const std::string& why_not) {
    if (get_gen_table(&p->g2, &p->wn2) || get_reversed(p->g2, &p->g2r, &p->wn2r)) return 1;
    if (knobs.rtc && osm_compile(p, geo, knobs, why_not)) return 1;
    if (p->n1 == 1) return 0;
    if (get_gen_table(&p->g1, &p->wn1) || make_big_twiddle(p->n, &p->tlo, &p->thi)) return 1;
    // the uniform factors of the row kernel's four-step twiddles (GenRowSrc): the first
    // forward and the last inverse stage have radix r0
    const int r0 = p->rtc ? p->q2.fac[0] : p->g2.fac[0];
    const long long m = p->n2 / r0;
    std::vector<cf> t((size_t)p->n1 * r0);
    for (int k1 = 0; k1 < p->n1; ++k1)
        for (int r = 0; r < r0; ++r)
            t[(size_t)k1 * r0 + r] = unit_root((long long)k1 * m % p->n * r, p->n);
    return upload(&p->tws, t);
}

// Twiddle tables of a power-of-two plan.
static int osm_pow2_tables(bbt_osm_plan* p) {
    const int64_t n_fft = p->n;
    if (p->n2 > 4096) {
        if (get_big_table(p->n2, &p->big_tw)) return 1;
    } else if (get_tables(p->n2, &p->tab2)) {
        return 1;
    }
    if ((p->n1 == 256 || p->outer == 256) && get_tables(256, &p->tab1)) return 1;
    if ((p->n1 == 512 || p->n1 == 1024) && get_tables(p->n1, &p->tab1)) return 1;
    if (get_wroot(&p->wroot)) return 1;
    if (p->n1 == 1) return 0;
    // (three-level plans: these are the twiddles of the inner transform of n1 * n2 points)
    const int t = p->n2 / 16;
    const long long inner = (long long)p->n1 * p->n2;
    std::vector<cf> row((size_t)p->n1 * 16), base((size_t)p->n1 * t);
    for (int k1 = 0; k1 < p->n1; ++k1) {
        for (int j = 0; j < 16; ++j) row[(size_t)k1 * 16 + j] = unit_root((long long)k1 * j, 16ll * p->n1);
        for (int tau = 0; tau < t; ++tau)
            base[(size_t)k1 * t + tau] = unit_root((long long)k1 * tau, inner);
    }
    if (upload(&p->tw4row, row) || upload(&p->tw4base, base)) return 1;
    if (p->outer > 1) {
        std::vector<cf> o((size_t)p->outer * t), uu((size_t)p->outer * p->n1 * 16);
        for (int k1o = 0; k1o < p->outer; ++k1o) {
            for (int tau = 0; tau < t; ++tau) o[(size_t)k1o * t + tau] = unit_root((long long)k1o * tau, n_fft);
            for (int k1 = 0; k1 < p->n1; ++k1)
                for (int j = 0; j < 16; ++j) {
                    // W_{16 n1}^{k1 j} W_65536^{k1o j} as one angle over 65536 * 16 n1 / gcd ...: in double
                    const double a = -2.0 * M_PI * ((double)((long long)k1 * j % (16ll * p->n1)) / (16.0 * p->n1) +
                                                    (double)((long long)k1o * j % 65536) / 65536.0);
                    uu[((size_t)k1o * p->n1 + k1) * 16 + j] = make_float2((float)cos(a), (float)sin(a));
                }
        }
        if (upload(&p->tw4o, o) || upload(&p->tw4u, uu)) return 1;
    }
    // twiddles in the column passes: only with 256- / 512-point columns (T1 = n1 / 16 threads
    // per column, thread tau holds rows tau + T1 j: factors a g^j, a = W_N^{tau n2}, g = W_N^{T1 n2})
    if (p->n1 >= 256 && p->outer == 1) {
        const int t1 = p->n1 / 16;
        std::vector<cf> a((size_t)t1 * p->n2), g((size_t)4 * p->n2);
        for (int n2 = 0; n2 < p->n2; ++n2) {
            for (int i = 0; i < 4; ++i) g[(size_t)i * p->n2 + n2] = unit_root(((long long)t1 << i) * n2, n_fft);
            for (int tau = 0; tau < t1; ++tau) a[(size_t)tau * p->n2 + n2] = unit_root((long long)tau * n2, n_fft);
        }
        if (upload(&p->twa, a) || upload(&p->twg, g)) return 1;
        p->tw_col = true;
    }
    return 0;
}

// response: upload (if needed), permute to [C][N1][N2], scale by 1/N; then the streams' indices
static int osm_put_response(bbt_osm_plan* p, const void* resp, int resp_on_device, const std::vector<int>& idx) {
    const int64_t n_fft = p->n;
    const size_t rbytes = (size_t)p->C * n_fft * sizeof(cf);
    cf* nat = nullptr;
    if (resp_on_device) {
        nat = (cf*)resp;
    } else {
        if (hipMalloc((void**)&nat, rbytes) != hipSuccess ||
            hipMemcpy(nat, resp, rbytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail("bbt_osm_plan_create: uploading the response failed");
    }
    if (hipMalloc((void**)&p->resp, rbytes) != hipSuccess)
        return fail("bbt_osm_plan_create: hipMalloc(response) failed");
    // a device-resident response may still be being written on the caller's
    // (non-blocking) stream, which the null stream used below does not wait for
    if (resp_on_device && hipDeviceSynchronize() != hipSuccess)
        return fail("bbt_osm_plan_create: hipDeviceSynchronize failed");
    hipLaunchKernelGGL(k_permute_resp, dim3((unsigned)((n_fft + 255) / 256), p->C), dim3(256), 0, 0,
                       nat, p->resp, p->outer, p->n1, (long long)p->n2, 1.0f / (float)n_fft);
    hipError_t e = hipDeviceSynchronize();
    if (!resp_on_device) hipFree(nat);
    if (e != hipSuccess)
        return fail("bbt_osm_plan_create: response permutation failed: %s", hipGetErrorString(e));
    if (hipMalloc((void**)&p->resp_index, idx.size() * sizeof(int)) != hipSuccess ||
        hipMemcpy(p->resp_index, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice) !=
            hipSuccess)
        return fail("bbt_osm_plan_create: resp_index upload failed");
    return 0;
}

// the lanes' work buffers and streams, the tail stream and the events that order them
static int osm_make_lanes(bbt_osm_plan* p) {
    if (p->n1 > 1) {
        for (int l = 0; l < p->lanes; ++l) {
            if (hipMalloc((void**)&p->lane_work[l], p->work_bytes) != hipSuccess)
                return fail("bbt_osm_plan_create: hipMalloc(workspace %zu bytes) failed", p->work_bytes);
            if (p->lanes > 1 &&
                (hipStreamCreateWithFlags(&p->lane_stream[l], hipStreamNonBlocking) != hipSuccess ||
                 hipEventCreateWithFlags(&p->ev_join[l], BBT_EV_ORDER) != hipSuccess))
                return fail("bbt_osm_plan_create: creating the lane streams failed");
        }
        p->work = p->lane_work[0];
        if (p->lanes > 1 &&
            hipEventCreateWithFlags(&p->ev_fork, BBT_EV_ORDER) != hipSuccess)
            return fail("bbt_osm_plan_create: creating the fork event failed");
        if (p->lanes > 1) {
            if (hipStreamCreateWithFlags(&p->tail_stream, hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&p->ev_tail[0], BBT_EV_ORDER) != hipSuccess ||
                hipEventCreateWithFlags(&p->ev_tail[1], BBT_EV_ORDER) != hipSuccess)
                return fail("bbt_osm_plan_create: creating the tail stream failed");
        }
    }
    // (BBT_ASIDE=0, a development switch: one-kernel plans have no stream of their own and run
    // every call on the caller's)
    const char* aside_env = getenv("BBT_ASIDE");
    if (p->lanes == 1 && !(aside_env && !strcmp(aside_env, "0"))) {
        // (no lanes: a deferred call runs on the tail stream, beside what the caller queues next)
        if (hipStreamCreateWithFlags(&p->tail_stream, hipStreamNonBlocking) != hipSuccess ||
            (!p->ev_fork && hipEventCreateWithFlags(&p->ev_fork, BBT_EV_ORDER) != hipSuccess) ||
            hipEventCreateWithFlags(&p->ev_tail[0], BBT_EV_ORDER) != hipSuccess ||
            hipEventCreateWithFlags(&p->ev_tail[1], BBT_EV_ORDER) != hipSuccess)
            return fail("bbt_osm_plan_create: creating the tail stream failed");
    }
    if (hipEventCreateWithFlags(&p->ev_done, BBT_EV_ORDER) != hipSuccess)
        return fail("bbt_osm_plan_create: creating the completion event failed");
    return 0;
}

extern "C" {

int bbt_osm_plan_create(bbt_osm_plan** plan, int64_t n_fft, int n_stream, int n_resp,
                        const void* resp, int resp_on_device, const int32_t* resp_index) {
    ARG_TRY(plan && resp, "bbt_osm_plan_create: null argument");
    *plan = nullptr;
    // block length and stream count: checked, and the levels planned (osm_geo.hpp)
    const OsmKnobs knobs = osm_knobs_from_env();
    OsmGeo geo;
    std::string text;           // why osm_levels refuses, or why there is nothing to compile
    ARG_TRY(osm_levels(n_fft, n_stream, knobs, &geo, &text), "%s", text.c_str());
    ARG_TRY(n_resp >= 1, "bbt_osm_plan_create: n_resp=%d must be >= 1", n_resp);
    std::vector<int> idx(geo.single ? 2 : n_stream, 0);
    if (resp_index)
        for (int s = 0; s < n_stream; ++s) {
            ARG_TRY(resp_index[s] >= 0 && resp_index[s] < n_resp,
                    "bbt_osm_plan_create: resp_index[%d]=%d out of range", s, resp_index[s]);
            idx[s] = resp_index[s];
        }
    if (geo.single) idx[1] = idx[0];        // both halves of a pair of blocks are the one stream
    bbt_osm_plan* p = new bbt_osm_plan;
    auto bail = [&](int) {
        bbt_osm_plan_destroy(p);
        return 1;
    };
    if (hipGetDevice(&p->device) != hipSuccess) return bail(fail("hipGetDevice failed"));
    p->n = n_fft;
    p->S = n_stream;
    p->npair = geo.npair;
    p->single = geo.single;
    p->C = n_resp;
    p->generic = geo.generic;
    p->outer = geo.outer;
    p->n1 = geo.n1;
    p->n2 = geo.n2;
    p->g1 = geo.g1;
    p->g2 = geo.g2;
    p->gen_ct = geo.gen_ct;
    p->q1 = geo.q1;
    p->q2 = geo.q2;
    p->q2r = geo.q2r;
    // tables; generic lengths: the kernels compiled for the length, which the buffers depend on
    if (p->generic ? osm_generic_tables(p, geo, knobs, text) : osm_pow2_tables(p)) return bail(1);
    if (osm_put_response(p, resp, resp_on_device, idx)) return bail(1);
    osm_buffers(&geo, p->rtc, knobs);
    p->n2p = geo.n2p;
    p->chunk = geo.chunk;
    p->cap = geo.cap;
    p->lanes = geo.lanes;
    p->work_bytes = geo.work_bytes;
    p->timing_stride = knobs.timing_stride;
    p->knobs = knobs;
    if (osm_make_lanes(p)) return bail(1);
    *plan = p;
    return 0;
}

int bbt_osm_plan_destroy(bbt_osm_plan* p) {
    if (!p) return 0;
    // (a deferred call may still be running on the plan's own streams -- its caller has only
    // QUEUED the wait for it: nothing the kernels read goes before they are done)
    for (int l = 0; l < BBT_MAX_LANES; ++l)
        if (p->lane_stream[l]) hipStreamSynchronize(p->lane_stream[l]);
    if (p->tail_stream) hipStreamSynchronize(p->tail_stream);
    for (auto e : p->ev) hipEventDestroy(e);
    for (auto e : p->ev_free) hipEventDestroy(e);
    if (p->resp) hipFree(p->resp);
    if (p->resp_index) hipFree(p->resp_index);
    if (p->tw4row) hipFree(p->tw4row);
    if (p->tw4base) hipFree(p->tw4base);
    if (p->tw4o) hipFree(p->tw4o);
    if (p->tw4u) hipFree(p->tw4u);
    if (p->twa) hipFree(p->twa);
    if (p->twg) hipFree(p->twg);
    if (p->tlo) hipFree(p->tlo);
    if (p->thi) hipFree(p->thi);
    if (p->tws) hipFree(p->tws);
    for (int l = 0; l < BBT_MAX_LANES; ++l) {
        if (p->lane_stream[l]) {
            hipStreamSynchronize(p->lane_stream[l]);
            hipStreamDestroy(p->lane_stream[l]);
        }
        if (p->ev_join[l]) hipEventDestroy(p->ev_join[l]);
        if (p->lane_work[l]) hipFree(p->lane_work[l]);
    }
    if (p->tail_stream) {
        hipStreamSynchronize(p->tail_stream);
        hipStreamDestroy(p->tail_stream);
    }
    for (int i = 0; i < 2; ++i) {
        if (p->ev_tail[i]) hipEventDestroy(p->ev_tail[i]);
        if (p->seam_buf[i]) hipFree(p->seam_buf[i]);
    }
    if (p->ev_fork) hipEventDestroy(p->ev_fork);
    if (p->ev_done) hipEventDestroy(p->ev_done);
    delete p;
    return 0;
}

int bbt_osm_plan_info(const bbt_osm_plan* p, int64_t* workspace_bytes, int* chunk_blocks, int* n1,
                      int* n2) {
    ARG_TRY(p, "bbt_osm_plan_info: null plan");
    if (workspace_bytes) *workspace_bytes = (int64_t)p->work_bytes * p->lanes;
    if (chunk_blocks) *chunk_blocks = p->chunk;
    if (n1) *n1 = p->n1;
    if (n2) *n2 = p->n2;
    return 0;
}

int bbt_osm_plan_defer(bbt_osm_plan* p, bbt_event done) {
    ARG_TRY(p, "bbt_osm_plan_defer: null plan");
    std::lock_guard<std::mutex> lock(p->mu);
    p->defer_ev = (hipEvent_t)done;
    return 0;
}

int bbt_osm_plan_fusable(const bbt_osm_plan* p, int n_chan) {
    return p && osm_fusable(p->generic, p->single, p->outer, p->n1, p->n2, n_chan);
}

int bbt_osm_execute(bbt_osm_plan* p, const void* in_dev, void* out_dev, int64_t n_blocks,
                    const int64_t* in_off, const int64_t* out_off, const int32_t* valid_start,
                    const int32_t* valid_count, bbt_stream stream) {
    DeferTake take(p, (hipStream_t)stream);
    ARG_TRY(p && in_dev && out_dev, "bbt_osm_execute: null argument");
    if (osm_check_blocks(p, "bbt_osm_execute", n_blocks, in_off, out_off, valid_start, valid_count))
        return 1;
    SpecOut so = {};
    PlanCall call(p, take, n_blocks);
    return osm_run_all(p, (const float2*)in_dev, (float2*)out_dev, n_blocks, so, call,
                       [&](OsmBlock& blk, int64_t b) {
                           blk.in_off = in_off[b];
                           blk.out_off = out_off[b];
                           blk.valid_start = valid_start[b];
                           blk.valid_count = valid_count[b];
                           blk.shift = 0;
                           blk.index = (int)b;
                       });
}

int bbt_osm_execute_flat(bbt_osm_plan* p, const void* in_dev, void* out_dev, int64_t n_blocks,
                         const int64_t* in_off, const int64_t* out_elem_off, const int32_t* valid_start,
                         int32_t first_elem, const int32_t* valid_elems, bbt_stream stream) {
    const char* who = "bbt_osm_execute_flat";
    DeferTake take(p, (hipStream_t)stream);
    ARG_TRY(p && in_dev && out_dev, "%s: null argument", who);
    ARG_TRY(!p->generic && !p->single && p->n1 == 1 && p->outer == 1,
            "%s: only for power-of-two blocks of at most 4096 samples with an even stream count", who);
    ARG_TRY(n_blocks >= 0 && (n_blocks == 0 || (in_off && out_elem_off && valid_start && valid_elems)),
            "%s: bad descriptors", who);
    ARG_TRY(first_elem >= 0 && first_elem < p->S && first_elem % 2 == 0,
            "%s: first_elem=%d must be an even element of a row of %d", who, first_elem, p->S);
    for (int64_t b = 0; b < n_blocks; ++b)
        ARG_TRY(in_off[b] >= 0 && out_elem_off[b] >= 0 && out_elem_off[b] % 2 == 0 && valid_start[b] >= 0 &&
                    valid_elems[b] >= 0 && valid_elems[b] % 2 == 0 &&
                    (int64_t)valid_start[b] * p->S + first_elem + valid_elems[b] <= p->n * p->S,
                "%s: block %lld keeps elements outside the block", who, (long long)b);
    SpecOut so = {};
    PlanCall call(p, take, n_blocks);
    return osm_run_all(p, (const float2*)in_dev, (float2*)out_dev, n_blocks, so, call,
                       [&](OsmBlock& blk, int64_t b) {
                           blk.in_off = in_off[b];
                           blk.out_off = out_elem_off[b];
                           blk.valid_start = valid_start[b];
                           blk.valid_count = valid_elems[b];
                           blk.flat = 1;
                           blk.flat_sub = first_elem;
                       });
}

int bbt_osm_plan_set_layout(bbt_osm_plan* p, int64_t in_plane, int64_t out_plane) {
    ARG_TRY(p, "bbt_osm_plan_set_layout: null plan");
    ARG_TRY(in_plane >= 0 && out_plane >= 0, "bbt_osm_plan_set_layout: negative plane length");
    const bool pairs = !p->generic && !p->single && p->outer == 1 && p->S % 2 == 0;
    ARG_TRY(in_plane == 0 || (pairs && p->n1 == 256),
            "bbt_osm_plan_set_layout: pair-planar input needs a two-level plan with 256-point columns "
            "(blocks of 2^17 to 2^20 samples) of an even number of streams");
    ARG_TRY(out_plane == 0 || (pairs && p->n1 == 1),
            "bbt_osm_plan_set_layout: pair-planar output needs a one-kernel plan (blocks of at most "
            "4096 samples) of an even number of streams");
    std::lock_guard<std::mutex> lock(p->mu);
    p->in_plane = in_plane;
    p->out_plane = out_plane;
    return 0;
}

// Channelize(overlap-save task) as one call; with det_step > 0 the spectra are
// detected and integrated instead of stored (out_dev = float32 bins).
static int osm_channelized(bbt_osm_plan* p, const char* who, const void* in_dev, void* out_dev,
                           int64_t n_blocks, const int64_t* in_off, const int64_t* out_off,
                           const int32_t* valid_start, const int32_t* valid_count, int n_chan,
                           int64_t first_spectrum, int64_t n_spectra, int det_step, int det_mode,
                           float det_scale, hipStream_t st) {
    DeferTake take(p, st);
    ARG_TRY(p && in_dev && out_dev, "%s: null argument", who);
    ARG_TRY(!p->generic, "%s: the fused channelizer needs a power-of-two block length (got %lld)",
            who, (long long)p->n);
    ARG_TRY(p->n1 > 1 || p->outer > 1, "%s: block length %lld is too short to fuse", who,
            (long long)p->n);
    ARG_TRY(bbt_osm_plan_fusable(p, n_chan),
            "%s: n_chan=%d must be a power of two in [256, %d] (or 16..128 for blocks with 256 "
            "columns or of three levels, 2..8 for two-level blocks of up to 2^20 samples)", who, n_chan, p->n2);
    const bool small = n_chan < 256;
    ARG_TRY(!(small && det_step > 0), "%s: fused detection needs n_chan >= 256", who);
    ARG_TRY(!(p->single && det_step > 0), "%s: one-stream plans have no fused detection", who);
    ARG_TRY(first_spectrum >= 0 && n_spectra >= 0, "%s: bad spectrum range", who);
    if (osm_check_blocks(p, who, n_blocks, in_off, out_off, valid_start, valid_count)) return 1;
    for (int64_t b = 0; b < n_blocks; ++b)
        ARG_TRY(valid_count[b] >= n_chan, "%s: block %lld keeps %d samples < n_chan", who,
                (long long)b, valid_count[b]);
    if (n_blocks == 0 || n_spectra == 0) return 0;
    PlanCall call(p, take, n_blocks);
    FftTables tabc;
    GenGeo gsmall = {};
    cf* wsmall = nullptr;
    if (small ? (!gen_factor_7smooth(n_chan, &gsmall) || get_gen_table(&gsmall, &wsmall))
              : get_tables(n_chan, &tabc))
        return 1;
    // seam slots and jobs.  The slots are filled by the lanes and read by the seam pass at the
    // end of the call; a deferred call takes the turn the call before it did not use, after the
    // seam pass of the last call on that turn (two calls back, long done: no stall).
    const int turn = call.deferred ? (p->seam_turn ^= 1) : p->seam_turn;
    if (p->ev_tail_set[turn]) {
        HIP_TRY(hipStreamWaitEvent(st, p->ev_tail[turn], 0));
        if (!call.deferred) p->ev_tail_set[turn] = false;
    }
    const size_t need = (size_t)n_blocks * 2 * p->npair * n_chan * 16;
    if (need > p->seam_bytes[turn]) {
        if (p->seam_buf[turn]) HIP_TRY(hipFree(p->seam_buf[turn]));      // (waits for the device)
        p->seam_buf[turn] = nullptr;
        p->seam_bytes[turn] = 0;
        HIP_TRY(hipMalloc((void**)&p->seam_buf[turn], need));
        p->seam_bytes[turn] = need;
    }
    p->seam = p->seam_buf[turn];
    std::vector<SeamJob> jobs;
    for (int64_t b = 0; b + 1 < n_blocks; ++b) {
        const int64_t seam_pos = out_off[b] + valid_count[b];
        if (out_off[b + 1] != seam_pos || seam_pos % n_chan == 0) continue;   // not adjacent / aligned
        const int64_t s = seam_pos / n_chan;
        if (s < first_spectrum || s >= first_spectrum + n_spectra) continue;
        SeamJob j;
        j.spectrum = s - first_spectrum;
        j.first_block = (int)b;
        j.split = (int)(seam_pos - s * n_chan);
        jobs.push_back(j);
    }
    SpecOut so = {};
    so.seam = p->seam;
    so.s_base = first_spectrum;
    so.n_out = n_spectra;
    so.n_chan = n_chan;
    so.lg_chan = 0;
    while ((1 << so.lg_chan) < n_chan) ++so.lg_chan;
    so.n_fft = (int)p->n;
    so.small_l = small ? n_chan / 16 : 0;             // (0 below 16 channels)
    so.tiny_lg = n_chan < 16 ? so.lg_chan : 0;
    so.small_row = p->n2;
    if (det_step > 0) {
        so.det = (float*)out_dev;
        so.det_step = det_step;
        so.det_mode = det_mode;
        so.det_scale = det_scale;
    }
    if (osm_run_all(p, (const float2*)in_dev, (float2*)out_dev, n_blocks, so, call,
                    [&](OsmBlock& blk, int64_t b) {
                        blk.in_off = in_off[b];
                        blk.out_off = out_off[b];
                        blk.valid_start = valid_start[b];
                        blk.valid_count = valid_count[b];
                        // circular shift that puts spectrum boundaries on multiples of n_chan
                        int64_t o = ((int64_t)valid_start[b] - out_off[b]) % n_chan;
                        if (o < 0) o += n_chan;
                        blk.shift = (int)o;
                        blk.index = (int)b;
                    }))
        return 1;
    hipStream_t fin = call.fin;        // (a deferred call: the plan's tail stream, after the lanes)
    if (!jobs.empty() && small) {
        const size_t lds = (size_t)2 * n_chan * sizeof(f4);
        for (size_t j0 = 0; j0 < jobs.size(); j0 += BBT_SEAM_JOBS_PER_LAUNCH) {
            SeamJobs batch;
            const size_t n = std::min(jobs.size() - j0, (size_t)BBT_SEAM_JOBS_PER_LAUNCH);
            for (size_t i = 0; i < n; ++i) batch.j[i] = jobs[j0 + i];
            hipLaunchKernelGGL(k_seam_fix_gen, dim3((unsigned)n, p->npair), dim3(gen_threads(2 * n_chan)),
                               lds, fin, p->seam, (float2*)out_dev, batch, p->S, p->npair, gsmall, wsmall, so);
        }
        HIP_TRY(hipGetLastError());
    } else if (!jobs.empty()) {
        switch (n_chan) {
            case 256: launch_seam_fix<256>(p, (float2*)out_dev, jobs, tabc, so, fin); break;
            case 512: launch_seam_fix<512>(p, (float2*)out_dev, jobs, tabc, so, fin); break;
            case 1024: launch_seam_fix<1024>(p, (float2*)out_dev, jobs, tabc, so, fin); break;
            case 2048: launch_seam_fix<2048>(p, (float2*)out_dev, jobs, tabc, so, fin); break;
            case 4096: launch_seam_fix<4096>(p, (float2*)out_dev, jobs, tabc, so, fin); break;
        }
        HIP_TRY(hipGetLastError());
    }
    if (call.deferred) {
        HIP_TRY(hipEventRecord(p->ev_tail[turn], fin));
        p->ev_tail_set[turn] = true;
    }
    return 0;
}

int bbt_osm_execute_channelized(bbt_osm_plan* p, const void* in_dev, void* out_dev,
                                int64_t n_blocks, const int64_t* in_off, const int64_t* out_off,
                                const int32_t* valid_start, const int32_t* valid_count, int n_chan,
                                int64_t first_spectrum, int64_t n_spectra, bbt_stream stream) {
    return osm_channelized(p, "bbt_osm_execute_channelized", in_dev, out_dev, n_blocks, in_off,
                           out_off, valid_start, valid_count, n_chan, first_spectrum, n_spectra, 0,
                           0, 0.f, (hipStream_t)stream);
}

int bbt_osm_detect_bins_max(const bbt_osm_plan* p, int n_chan, int step) {
    return p ? osm_detect_bins_max(p->n2, n_chan, step) : -1;
}

int bbt_osm_execute_channelized_detect(bbt_osm_plan* p, const void* in_dev, void* out_dev,
                                       int64_t n_blocks, const int64_t* in_off,
                                       const int64_t* out_off, const int32_t* valid_start,
                                       const int32_t* valid_count, int n_chan,
                                       int64_t first_spectrum, int64_t n_bins, int step, int mode,
                                       int average, bbt_stream stream) {
    const char* who = "bbt_osm_execute_channelized_detect";
    DeferTake take(p, (hipStream_t)stream);
    ARG_TRY(p && out_dev, "%s: null argument", who);
    ARG_TRY(p->n1 == 256 && p->outer == 1,
            "%s: fused detection needs a two-level transform with 256 columns (block length 2^16..2^20)",
            who);
    ARG_TRY(step >= 1 && n_bins >= 0 && (mode == 0 || mode == 1), "%s: bad step/bins/mode", who);
    ARG_TRY(n_bins * (int64_t)step < (1ll << 40), "%s: too many spectra", who);
    // (step 1 -- Square / Power without integration -- stores every power itself: no bins, no zeroing)
    ARG_TRY(step == 1 || bbt_osm_detect_bins_max(p, n_chan, step) <= BBT_DET_MAX_BINS,
            "%s: step=%d is too short for %d channels on rows of %d (a workgroup would touch more "
            "than %d bins)", who, step, n_chan, p->n2, BBT_DET_MAX_BINS);
    const size_t out_bytes = (size_t)n_bins * n_chan * p->npair * (mode ? 4 : 2) * sizeof(float);
    if (out_bytes && step > 1) HIP_TRY(hipMemsetAsync(out_dev, 0, out_bytes, (hipStream_t)stream));
    take.give_back(p);
    return osm_channelized(p, who, in_dev, out_dev, n_blocks, in_off, out_off, valid_start,
                           valid_count, n_chan, first_spectrum, n_bins * step, step, mode,
                           average ? 1.0f / (float)step : 1.0f, (hipStream_t)stream);
}

int bbt_osm_execute_regular(bbt_osm_plan* p, const void* in_dev, void* out_dev, int64_t n_blocks,
                            int64_t in_off0, int64_t out_off0, int64_t hop, int32_t valid_start,
                            bbt_stream stream) {
    DeferTake take(p, (hipStream_t)stream);
    ARG_TRY(p, "bbt_osm_execute_regular: null plan");
    ARG_TRY(n_blocks >= 0 && hop > 0 && hop <= p->n, "bbt_osm_execute_regular: bad hop %lld",
            (long long)hop);
    if (!p->generic && p->n1 == 1 && p->outer == 1 && n_blocks > 0) {
        // one-kernel plans: the whole run as regular descriptors, up to 2^20 blocks per launch
        ARG_TRY(in_dev && out_dev && in_off0 >= 0 && out_off0 >= 0 && valid_start >= 0 &&
                    valid_start + hop <= p->n,
                "bbt_osm_execute_regular: blocks keep [%d, %lld) outside [0, %lld)", valid_start,
                (long long)(valid_start + hop), (long long)p->n);
        SpecOut so = {};
        PlanCall call(p, take, 0);         // (one-kernel plans have no lanes)
        const int64_t per_launch = std::min<int64_t>(1 << 20, ((1ll << 31) - 1) / p->npair);
        for (int64_t b0 = 0; b0 < n_blocks; b0 += per_launch) {
            OsmChunk ch = {};
            ch.reg_count = (int)std::min(per_launch, n_blocks - b0);
            ch.reg_hop = hop;
            ch.nblk = 1;
            ch.b[0].in_off = in_off0 + b0 * hop;
            ch.b[0].out_off = out_off0 + b0 * hop;
            ch.b[0].valid_start = valid_start;
            ch.b[0].valid_count = (int)hop;
            if (osm_run_chunk(p, (const float2*)in_dev, (float2*)out_dev, ch, so, nullptr, call.run)) return 1;
        }
        return 0;
    }
    std::vector<int64_t> io(n_blocks), oo(n_blocks);
    std::vector<int32_t> vs(n_blocks, valid_start), vc(n_blocks, (int32_t)hop);
    for (int64_t b = 0; b < n_blocks; ++b) {
        io[b] = in_off0 + b * hop;
        oo[b] = out_off0 + b * hop;
    }
    take.give_back(p);
    return bbt_osm_execute(p, in_dev, out_dev, n_blocks, io.data(), oo.data(), vs.data(),
                           vc.data(), stream);
}

int bbt_osm_timing_enable(bbt_osm_plan* p, int enable) {
    ARG_TRY(p, "bbt_osm_timing_enable: null plan");
    std::lock_guard<std::mutex> lock(p->mu);
    if (osm_flush_timing(p)) return 1;
    p->timing = enable != 0;
    p->timing_isolated = enable == 2;
    p->acc_ms[0] = p->acc_ms[1] = p->acc_ms[2] = 0;
    p->launches = 0;
    p->pass_launches[0] = p->pass_launches[1] = p->pass_launches[2] = 0;
    p->pass_blocks[0] = p->pass_blocks[1] = p->pass_blocks[2] = 0;
    return 0;
}

int bbt_osm_timing_read(bbt_osm_plan* p, double ms[3], int64_t* launches) {
    ARG_TRY(p && ms, "bbt_osm_timing_read: null argument");
    std::lock_guard<std::mutex> lock(p->mu);
    if (osm_flush_timing(p)) return 1;
    for (int k = 0; k < 3; ++k) ms[k] = p->acc_ms[k];
    if (launches) *launches = p->pass_launches[0];
    return 0;
}

int bbt_osm_timing_read_passes(bbt_osm_plan* p, double ms[3], int64_t launches[3], int64_t blocks[3]) {
    ARG_TRY(p && ms && launches && blocks, "bbt_osm_timing_read_passes: null argument");
    std::lock_guard<std::mutex> lock(p->mu);
    if (osm_flush_timing(p)) return 1;
    for (int k = 0; k < 3; ++k) {
        ms[k] = p->acc_ms[k];
        launches[k] = p->pass_launches[k];
        blocks[k] = p->pass_blocks[k];
    }
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// channelizer
struct bbt_chan_plan {
    int n = 0, S = 0, npair = 0, dir = -1;
    bool split_real = false;    // direction -2: one stream z = a + i b, output = half spectra of a and b
    FftTables tab;
    cf* wroot = nullptr;
    // 8192 / 16384 channels of stream pairs (fft_big.hpp)
    cf* big = nullptr;
    // channel counts that are not powers of two (gen_kernels.hpp)
    bool generic = false;
    GenGeo g = {};
    cf* wn = nullptr;
    int ct = 1;                 // stream pairs per workgroup tile
    // ... on the run-time specialised engine (gen2_kernels.hpp; null: not in use)
    G2Plan q;                   // q.ct columns per workgroup: cp stream pairs of q.ct / cp transforms
    int cp = 1;
    cf* qw = nullptr;
    hipFunction_t k2 = nullptr;
};

template <int N, int SIGN>
static void launch_short(const bbt_chan_plan* p, const float2* in, float2* out, int64_t n_fft,
                         float scale, hipStream_t st) {
    constexpr int R = (N <= 16) ? 1 : N / 16;
    constexpr int FPW = 256 / R;
    if constexpr (N <= 16) {
        if (p->S == 2) {                  // one pair: whole lines in and out, the transposition in LDS
            constexpr int T = 256;          // (128 for N = 16 -- four workgroups per CU instead of two -- measured no faster)
            constexpr size_t lds = T * (N + 1) * 16;
            if (ensure_dyn_lds((const void*)k_fft_tiny<N, SIGN, T>, lds) == 0) {
                hipLaunchKernelGGL((k_fft_tiny<N, SIGN, T>), dim3((unsigned)((n_fft + T - 1) / T)), dim3(T), lds, st,
                                   in, out, (long long)n_fft, scale);
                return;
            }
        }
    }
#define BBT_SHORT(PP_)                                                                         \
    {                                                                                          \
        constexpr int FPB = FPW / PP_;                                                         \
        const unsigned gx = (unsigned)((n_fft + FPB - 1) / FPB);                               \
        hipLaunchKernelGGL((k_fft_short<N, SIGN, PP_>), dim3(gx * (p->npair / PP_)), dim3(256), 0, \
                           st, in, out, (long long)n_fft, p->S, scale, p->wroot);              \
    }
    if (p->npair % 8 == 0) BBT_SHORT(8)
    else if (p->npair % 4 == 0) BBT_SHORT(4)
    else if (p->npair % 2 == 0) BBT_SHORT(2)
    else BBT_SHORT(1)
#undef BBT_SHORT
}

template <int N, int SIGN>
static void launch_rows(const bbt_chan_plan* p, const float2* in, float2* out, int64_t n_fft,
                        float scale, hipStream_t st) {
    constexpr int FPW = (N >= 1024) ? (4096 / N >= 4 ? 4 : 4096 / N) : (N == 512 ? 8 : 16);
    if (p->S == 1) {            // one stream: two consecutive transforms side by side
        const unsigned gx = (unsigned)(((n_fft + 1) / 2 + FPW - 1) / FPW);
        if (p->split_real) {    // ... of two real streams: half spectra out (forward) / in (inverse)
            hipLaunchKernelGGL((k_fft_rows<N, SIGN, FPW, true, true>), dim3(gx), dim3(FPW * N / 16), 0, st,
                               in, out, (long long)n_fft, 1, scale, p->tab.tw0, p->tab.tw1);
            return;
        }
        hipLaunchKernelGGL((k_fft_rows<N, SIGN, FPW, true>), dim3(gx), dim3(FPW * N / 16), 0, st, in, out,
                           (long long)n_fft, 1, scale, p->tab.tw0, p->tab.tw1);
        return;
    }
    // several pairs: the lanes over PP pairs first (k_fft_rows_pp) -- the largest of 8, 4, 2 that fits a
    // workgroup (1024 threads, 160 KiB of exchange area: 8 up to 2048 points, 4 at 4096) and that divides
    // the number of pairs.  Measured, Channelize(256 / 1024 / 4096) in G stream-samples/s: 16 streams
    // 174 / 150 / 165 -> 361 / 294 / 252, 2048 streams 87 / 114 / 124 -> 355 / 274 / 168 (two streams: 383 / 374 / 318)
    // with 8 / 4 / 2 pairs (round 4: as many as leave two workgroups per CU); whole 128-byte lines are worth
    // more than the second workgroup (round 5, 8 / 8 / 4 pairs): 16 streams 345 / 340 / 280, 128 streams
    // 357 / 343 / 279, 2048 streams 344 / 333 / 245.
    constexpr int CAP = N <= 2048 ? 8 : 4;
    const int cap = getenv("BBT_ROWS_CAP") ? atoi(getenv("BBT_ROWS_CAP")) : CAP;      // (dev)
#define BBT_ROWS_PP(PP_)                                                                                         \
    if ((PP_ * N / 16 <= 1024 && FftGeo<N>::LDS_ELEMS * sizeof(v2) * PP_ <= 160 * 1024) && PP_ <= cap &&        \
        p->npair % PP_ == 0 && n_fft * (p->npair / PP_) < (1ll << 31)) {                                        \
        constexpr int Q = (PP_ * N / 16 <= 1024 && FftGeo<N>::LDS_ELEMS * sizeof(v2) * PP_ <= 160 * 1024) ? PP_ : 1; \
        constexpr size_t lds = FftGeo<N>::LDS_ELEMS * sizeof(v2) * Q;                                            \
        if (ensure_dyn_lds((const void*)k_fft_rows_pp<N, SIGN, Q>, lds) == 0) {                                  \
            hipLaunchKernelGGL((k_fft_rows_pp<N, SIGN, Q>), dim3((unsigned)(n_fft * (p->npair / Q))),            \
                               dim3(Q * N / 16), lds, st, in, out, (long long)n_fft, p->S, scale, p->tab.tw0,    \
                               p->tab.tw1);                                                                      \
            return;                                                                                              \
        }                                                                                                        \
    }
    if (!p->split_real && p->S > 2 && !getenv("BBT_ROWS_NO_PP")) {
        BBT_ROWS_PP(8) BBT_ROWS_PP(4) BBT_ROWS_PP(2)
    }
#undef BBT_ROWS_PP
    const unsigned gx = (unsigned)((n_fft + FPW - 1) / FPW);
    if (p->split_real) {            // every stream z = a + i b of two real streams: half spectra out / in
        hipLaunchKernelGGL((k_fft_rows<N, SIGN, FPW, false, true>), dim3(gx * p->npair), dim3(FPW * N / 16), 0,
                           st, in, out, (long long)n_fft, p->S, scale, p->tab.tw0, p->tab.tw1);
        return;
    }
    hipLaunchKernelGGL((k_fft_rows<N, SIGN, FPW>), dim3(gx * p->npair), dim3(FPW * N / 16), 0, st, in,
                       out, (long long)n_fft, p->S, scale, p->tab.tw0, p->tab.tw1);
}

template <int SIGN>
static int chan_dispatch(const bbt_chan_plan* p, const float2* in, float2* out, int64_t n_fft,
                         float scale, hipStream_t st) {
    switch (p->n) {
        case 2: launch_short<2, SIGN>(p, in, out, n_fft, scale, st); break;
        case 4: launch_short<4, SIGN>(p, in, out, n_fft, scale, st); break;
        case 8: launch_short<8, SIGN>(p, in, out, n_fft, scale, st); break;
        case 16: launch_short<16, SIGN>(p, in, out, n_fft, scale, st); break;
        case 32: launch_short<32, SIGN>(p, in, out, n_fft, scale, st); break;
        case 64: launch_short<64, SIGN>(p, in, out, n_fft, scale, st); break;
        case 128: launch_short<128, SIGN>(p, in, out, n_fft, scale, st); break;
        case 256: launch_rows<256, SIGN>(p, in, out, n_fft, scale, st); break;
        case 512: launch_rows<512, SIGN>(p, in, out, n_fft, scale, st); break;
        case 1024: launch_rows<1024, SIGN>(p, in, out, n_fft, scale, st); break;
        case 2048: launch_rows<2048, SIGN>(p, in, out, n_fft, scale, st); break;
        case 4096: launch_rows<4096, SIGN>(p, in, out, n_fft, scale, st); break;
        default: return fail("channelize: unsupported n_chan %d", p->n);
    }
    return 0;
}

// (the scratch memory and the harness of the plans that time their candidates: tune.hpp)
extern "C" int bbt_tune_scratch(int release, int64_t* bytes) {
    TuneScratch& t = tune_scratch();
    std::lock_guard<std::mutex> lock(t.mu);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    auto& slot = t.buf[dev];
    if (bytes) *bytes = (int64_t)slot.second;
    if (release && slot.first) {
        HIP_TRY(hipFree(slot.first));
        slot = {nullptr, 0};
    }
    return 0;
}

// A candidate of a generic-length channelizer plan (chan_geo.hpp) with its kernel and its table,
// and the one place where a plan takes one.
struct ChanBuilt {
    ChanCandidate c;
    hipFunction_t k = nullptr;
    cf* w = nullptr;
};
// 0 = ok, 1 = not available (g_err says why).
static int chan_build(const ChanCandidate& c, ChanBuilt* b) {
    if (!c.ok()) return fail("%s", c.error.c_str());
    b->c = c;
    return g2_build(c.source, {"k_rows"}, &b->k) || get_g2_table(c.q, &b->w);
}
static void chan_apply(bbt_chan_plan* p, const ChanBuilt& b) {
    p->q = b.c.q;
    p->cp = b.c.cp;
    p->k2 = b.k;
    p->qw = b.w;
}
// The plan stays on the general kernel because the compiled ones are not to be had (g_err):
// 0 with one warning, 1 = error in `require` mode.
static int chan_stay_general(bbt_chan_plan* p) {
    if (rtc_mode() == 2) return 1;
    g2_warn_once("bbt_chan_plan_create");
    p->k2 = nullptr;
    return 0;
}
// The plan takes the candidate of `code`, untimed.
static int chan_take(bbt_chan_plan* p, int code, const ChanKnobs& knobs) {
    ChanBuilt b;
    if (chan_build(chan_g2_candidate(p->n, p->npair, p->dir, code % 100, code >= 100, knobs), &b)) return chan_stay_general(p);
    chan_apply(p, b);
    return 0;
}
// Choose among the candidates (and the general kernel) by timing them; 0 = ok (p->k2 null: the
// general kernel stays), 1 = error (only in `require` mode).
static int chan_pick(bbt_chan_plan* p, const ChanKnobs& knobs) {
    static TuneMemo<std::tuple<int, int, int, int>, int> chosen;       // (device, n, streams, direction) -> ChanCandidate::code, 0 = general
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const auto key = std::make_tuple(dev, p->n, p->S, p->dir);
    int remembered = -1;
    chosen.find(key, &remembered);
    const int pick = chan_untimed_code(remembered, knobs);
    if (pick == 0) return 0;                                           // (the general kernel won before)
    if (pick > 0) return chan_take(p, pick, knobs);
    const size_t per = (size_t)p->n * p->S * sizeof(cf);
    bool ready;
    int any = 0;
    {
        TuneBench bench(16 * per, (size_t)2 << 30, [&](size_t got) { return got / (2 * per) * per; });
        ready = bench.ready();
        if (ready) {
            const int64_t ns = (int64_t)(bench.size() / (2 * per));
            void *in = bench.base(), *out = bench.base() + ns * per;
            auto run = [&](hipStream_t st) { return bbt_chan_execute(p, in, out, ns, st); };
            p->k2 = nullptr;
            const float general_ms = bench.best_of(run);
            float best_ms = general_ms;
            ChanBuilt best;                                             // (k null: the general kernel)
            std::string why;
            const std::vector<ChanCandidate> list = chan_candidates(p->n, p->npair, p->dir, knobs, &why);
            if (list.empty()) fail("%s", why.c_str());
            for (const ChanCandidate& c : list) {
                ChanBuilt b;
                if (chan_build(c, &b)) continue;
                ++any;
                chan_apply(p, b);
                const float ms = bench.best_of(run);
                if (getenv("BBT_RTC_VERBOSE"))
                    fprintf(stderr, "bbt: Channelize(%d) x %d streams, %d points per thread, %d pairs x %d transforms per workgroup: "
                                    "%.3f ms (general %.3f)\n", p->n, p->S, c.code % 100, c.cp, c.q.ct / c.cp, ms,
                            best.k ? -1.f : general_ms);
                if (ms < best_ms) {
                    best_ms = ms;
                    best = b;
                }
            }
            chan_apply(p, best);
            if (any) chosen.remember(key, best.k ? best.c.code : 0);
        }
    }
    if (!ready) return chan_take(p, g2_pmax(BBT_G2_KIND_CHAN), knobs);      // (no scratch memory: the rule, untimed, and nothing remembered)
    return any ? 0 : chan_stay_general(p);
}

extern "C" {

int bbt_chan_plan_create(bbt_chan_plan** plan, int n_chan, int n_stream, int direction) {
    ARG_TRY(plan, "bbt_chan_plan_create: null argument");
    *plan = nullptr;
    ChanShape shape;
    std::string refusal;
    if (!chan_check(n_chan, n_stream, direction, &shape, &refusal)) return fail("%s", refusal.c_str());
    direction = shape.direction;
    const bool split_real = shape.split_real, big = shape.kind == CHAN_BIG, fast = shape.kind != CHAN_GENERIC && !big;
    bbt_chan_plan* p = new bbt_chan_plan;
    p->n = n_chan;
    p->S = n_stream;
    p->npair = n_stream / 2;
    p->dir = direction;
    p->split_real = split_real;
    if (big) {
        if (get_big_table(n_chan, &p->big)) {
            delete p;
            return 1;
        }
    } else if (!fast) {
        p->generic = true;
        if (!gen_factor_7smooth(n_chan, &p->g) || get_gen_table(&p->g, &p->wn)) {
            if (g_err.empty()) fail("bbt_chan_plan_create: cannot factor n_chan=%d", n_chan);
            delete p;
            return 1;
        }
        for (int ct = 8; ct >= 1; ct /= 2)           // (a power of two: gen_stage)
            if (p->npair % ct == 0 && (int64_t)n_chan * ct <= BBT_GEN_MAX_LEN) {
                p->ct = ct;
                break;
            }
        // The kernels compiled for this length -- and which of them.  A streaming transform wants few
        // registers and many waves, but how few depends on the length (MI355X, round 5, one stream
        // pair, 1 GB and more in HBM, Gsamples/s general | specialised at 20 / 16 / 10 points per
        // thread: 1536: 150 | 141 / 142 / 171, 2187: 119 | 122 / 167 / 164, 4374: 116 | 139 / 156 / 139,
        // 6174: 96 | 132 / 107 / 113, 6561: 119 | 121 / 147 / 151, 3000: 122 | 127 / 135 / 128, 1000: 164 |
        // 144 / 158 / 160, 360: 162 | 90 / 118 / 166; short transforms fill a wave with several of them:
        // 14: 25 -> 73, 30: 44 -> 71).  So the plan is made for 10, 16 and 20 points, each candidate --
        // and the general kernel -- is timed once on scratch memory, and the fastest is kept (a few
        // hundred milliseconds per new length and stream count, remembered for the process).
        // On four stream pairs and more each is also tried `wide`: as many pairs as fit a workgroup of
        // 1024 threads (whole lines: Channelize(3000) on 16 / 128 / 2048 streams 127 / 107 / 110 -> 200 / 201 / 203 G
        // stream-samples/s).  BBT_G2_TUNE=0: no timing, 10 points; BBT_G2_CHAN=none: the general kernels.
        const ChanKnobs knobs = chan_knobs_from_env();
        if (rtc_mode() && !knobs.general && chan_pick(p, knobs)) {
            delete p;
            return 1;
        }
    } else if ((n_chan >= 256 && get_tables(n_chan, &p->tab)) ||
               (n_chan < 256 && get_wroot(&p->wroot))) {
        delete p;
        return 1;
    }
    *plan = p;
    return 0;
}

int bbt_chan_plan_destroy(bbt_chan_plan* p) {
    delete p;
    return 0;
}

int bbt_chan_execute(bbt_chan_plan* p, const void* in_dev, void* out_dev, int64_t n_spectra,
                     bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_chan_execute: null argument");
    ARG_TRY(n_spectra >= 0, "bbt_chan_execute: n_spectra < 0");
    if (n_spectra == 0) return 0;
    // keep grid.x within limits: process in slabs
    const int64_t slab = (int64_t)1 << 20;
    const float2* in = (const float2*)in_dev;
    float2* out = (float2*)out_dev;
    if (p->big) {
        const float scale = p->dir < 0 ? 1.0f : 1.0f / (float)p->n;
        const int64_t per = std::max<int64_t>(1, ((int64_t)1 << 30) / p->npair);      // (grid.x < 2^31)
        for (int64_t s0 = 0; s0 < n_spectra; s0 += per) {
            const int64_t ns = std::min(per, n_spectra - s0);
            const int64_t off = s0 * p->n * p->S;
            const dim3 grid((unsigned)(ns * p->npair));
#define BBT_BIG_ROWS(N_, SIGN_)                                                                        \
    do {                                                                                               \
        constexpr size_t lds = BigGeo<N_>::LDS_ELEMS * sizeof(v2);                                     \
        if (ensure_dyn_lds((const void*)k_fft_rows_big<N_, SIGN_>, lds)) return 1;                     \
        hipLaunchKernelGGL((k_fft_rows_big<N_, SIGN_>), grid, dim3(N_ / 16), lds, (hipStream_t)stream, \
                           in + off, out + off, (long long)ns, p->S, scale, p->big);                   \
    } while (0)
            if (p->n == 8192) {
                if (p->dir < 0) BBT_BIG_ROWS(8192, -1); else BBT_BIG_ROWS(8192, +1);
            } else {
                if (p->dir < 0) BBT_BIG_ROWS(16384, -1); else BBT_BIG_ROWS(16384, +1);
            }
#undef BBT_BIG_ROWS
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    for (int64_t s0 = 0; s0 < n_spectra; s0 += slab) {
        const int64_t ns = (n_spectra - s0 < slab) ? n_spectra - s0 : slab;
        const int64_t off = s0 * p->n * p->S;
        if (p->generic && p->k2) {
            const int bt = p->q.ct / p->cp;
            const dim3 grid((unsigned)(((ns + bt - 1) / bt) * (p->npair / p->cp))), block(p->q.threads());
            if (g2_launch(p->k2, grid, block, (hipStream_t)stream, in + off, out + off, p->S, p->cp, (long long)ns,
                          p->dir < 0 ? 1.0f : 1.0f / (float)p->n, (const cf*)p->qw))
                return 1;
            continue;
        }
        if (p->generic) {
            const size_t lds = (size_t)p->n * p->ct * sizeof(f4);
            const dim3 grid((unsigned)(ns * (p->npair / p->ct))), block(gen_threads(p->n * p->ct));
            if (p->dir < 0) {
                if (ensure_dyn_lds((const void*)k_gen_fft_rows<-1>, lds)) return 1;
                hipLaunchKernelGGL((k_gen_fft_rows<-1>), grid, block, lds, (hipStream_t)stream, in + off,
                                   out + off, p->S, p->ct, 1.0f, p->g, p->wn);
            } else {
                if (ensure_dyn_lds((const void*)k_gen_fft_rows<+1>, lds)) return 1;
                hipLaunchKernelGGL((k_gen_fft_rows<+1>), grid, block, lds, (hipStream_t)stream, in + off,
                                   out + off, p->S, p->ct, 1.0f / (float)p->n, p->g, p->wn);
            }
            continue;
        }
        // (half spectra of a real pair: n/2 + 1 channels x 2 streams per spectrum on that side)
        const int64_t half_off = s0 * (p->n / 2 + 1) * 2 * p->S;
        int rc = (p->dir < 0)
                     ? chan_dispatch<-1>(p, in + off, out + (p->split_real ? half_off : off), ns, 1.0f,
                                         (hipStream_t)stream)
                     : chan_dispatch<+1>(p, in + (p->split_real ? half_off : off), out + off, ns,
                                         1.0f / (float)p->n, (hipStream_t)stream);
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// polyphase filter bank
struct bbt_pfb_plan {
    int n = 0, S = 0, npair = 0, n_tap = 0;
    bool split_real = false;    // n_stream -1: one stream z = a + i b of two real streams, half spectra out
    float* taps = nullptr;
    float* taps_quads = nullptr;   // window kernels: [column group][tap quad][thread] float4
    FftTables tab;
    FftTables tab4096;   // for the sliding-window kernel
    bool window = false;
    // several stream pairs per workgroup of the sliding-window kernel (pp > 1: geometry gn, tables tabg,
    // taps_quads permuted for gn / 16 threads)
    int pp = 1, gn = 4096, gl = 0;
    FftTables tabg;
    float* taps_quads_pp = nullptr;
    // many streams: the window as a streaming pass over whole rows (k_pfb_fir_rows), then the
    // transform in place through a channelizer plan (k_fft_rows_pp)
    bbt_chan_plan* two_pass = nullptr;
};

template <int N, int NTAP>
static void launch_pfb_window(const bbt_pfb_plan* p, const float2* in, float2* out, int64_t n_spec,
                              hipStream_t st) {
    constexpr int NG = 4096 / N;
    if (p->S == 1) {            // one stream: two groups of NG spectra side by side
        const unsigned gx = (unsigned)((n_spec + 2 * NG - 1) / (2 * NG));
        if (p->split_real)
            hipLaunchKernelGGL((k_pfb_window<N, NTAP, true, true>), dim3(gx), dim3(256), 0, st, in, out,
                               (long long)n_spec, 1, p->taps_quads, p->tab4096.tw0, p->tab4096.tw1);
        else
            hipLaunchKernelGGL((k_pfb_window<N, NTAP, true>), dim3(gx), dim3(256), 0, st, in, out,
                               (long long)n_spec, 1, p->taps_quads, p->tab4096.tw0, p->tab4096.tw1);
        return;
    }
    if (p->pp > 1) {            // several pairs per workgroup (many streams): pfb_route
        constexpr int GN = pfb_pp_geometry(N);
        const unsigned gy = (unsigned)((n_spec + GN / N - 1) / (GN / N));
        if (p->pp == 4)
            hipLaunchKernelGGL((k_pfb_window<N, NTAP, false, false, 4, GN>), dim3(gy * (p->npair / 4)),
                               dim3(GN / 16 * 4), 0, st, in, out, (long long)n_spec, p->S, p->taps_quads_pp,
                               p->tabg.tw0, p->tabg.tw1, p->gl);
        if constexpr (GN == 2048) {
            if (p->pp == 8)
                hipLaunchKernelGGL((k_pfb_window<N, NTAP, false, false, 8, GN>), dim3(gy * (p->npair / 8)),
                                   dim3(GN / 16 * 8), 0, st, in, out, (long long)n_spec, p->S, p->taps_quads_pp,
                                   p->tabg.tw0, p->tabg.tw1, p->gl);
        }
        return;
    }
    const unsigned gx = (unsigned)((n_spec + NG - 1) / NG);
    if (p->split_real)          // every stream z = a + i b of two real streams: half spectra out
        hipLaunchKernelGGL((k_pfb_window<N, NTAP, false, true>), dim3(gx * p->npair), dim3(256), 0, st, in, out,
                           (long long)n_spec, p->S, p->taps_quads, p->tab4096.tw0, p->tab4096.tw1);
    else
        hipLaunchKernelGGL((k_pfb_window<N, NTAP>), dim3(gx * p->npair), dim3(256), 0, st, in, out,
                           (long long)n_spec, p->S, p->taps_quads, p->tab4096.tw0, p->tab4096.tw1);
}

// the sliding-window variants: those of pfb_has_window (pfb_geo.hpp)
static void pfb_window_dispatch(const bbt_pfb_plan* p, const float2* in, float2* out, int64_t n_spec, hipStream_t st) {
#define BBT_PW(N_, T_)                                                                   \
    static_assert(pfb_has_window(N_, T_), "pfb_has_window must name every window kernel"); \
    if (p->n == N_ && p->n_tap == T_) return launch_pfb_window<N_, T_>(p, in, out, n_spec, st);
    BBT_PW(256, 4) BBT_PW(512, 4) BBT_PW(1024, 4) BBT_PW(2048, 4)
    BBT_PW(256, 8) BBT_PW(512, 8) BBT_PW(1024, 8) BBT_PW(2048, 8)
    BBT_PW(256, 12) BBT_PW(512, 12) BBT_PW(1024, 12) BBT_PW(2048, 12)
    BBT_PW(256, 16) BBT_PW(512, 16) BBT_PW(1024, 16) BBT_PW(2048, 16)
#undef BBT_PW
}

template <int N>
static void launch_pfb(const bbt_pfb_plan* p, const float2* in, float2* out, int64_t n_spec,
                       hipStream_t st) {
    constexpr int FPW = (N >= 1024) ? (4096 / N >= 4 ? 4 : 4096 / N) : (N == 512 ? 8 : 16);
    const unsigned gx = (unsigned)((n_spec + FPW - 1) / FPW);
    hipLaunchKernelGGL((k_pfb<N, FPW>), dim3(gx * p->npair), dim3(FPW * N / 16), 0, st, in, out,
                       (long long)n_spec, p->S, p->n_tap, p->taps, p->tab.tw0, p->tab.tw1);
}

#ifndef BBT_PFB_NI
#define BBT_PFB_NI 192                // spectra per sweep of the window pass (k_pfb_fir_rows): 96 -> 192 +2-5 %, 384 no better
#endif
// The one place where a plan takes a route (pfb_geo.hpp: PfbCandidate).  `two_pass`: the channelizer
// plan of the second pass, which the plan owns from here on if the route is two passes.
static void pfb_apply(bbt_pfb_plan* p, const PfbCandidate& c, bbt_chan_plan* two_pass) {
    p->two_pass = c.pp == 0 ? two_pass : nullptr;
    p->pp = c.pp > 1 ? c.pp : 1;
    p->gl = c.pp > 1 ? c.gl : 0;
}
// Which route the plan takes (pfb_geo.hpp: pfb_route): fixed, or the fastest of the candidates,
// timed once on scratch memory (tune.hpp) and remembered for the process.  0 = ok.
static int pfb_pick(bbt_pfb_plan* p, const PfbShape& shape, const PfbKnobs& knobs) {
    const PfbRoute route = pfb_route(knobs, shape);
    PfbCandidate best = route.fixed;
    static TuneMemo<std::tuple<int, int, int, int>, PfbCandidate> chosen;   // (device, channels, taps, streams) -> route
    std::tuple<int, int, int, int> key;
    bool timed = route.timed;
    if (timed) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        key = std::make_tuple(dev, p->n, p->n_tap, p->S);
        timed = !chosen.find(key, &best);
    }
    // (a timed plan makes the channelizer plan of the second pass before the comparison)
    bbt_chan_plan* tp = nullptr;
    if ((timed ? shape.two_ok : best.pp == 0) && bbt_chan_plan_create(&tp, p->n, p->S, -1)) return 1;
    if (timed) {
        const int n_tap = p->n_tap;
        const size_t per = (size_t)p->n * p->S * sizeof(cf);
        const auto t_start = std::chrono::steady_clock::now();
        auto trace = [&](const char* what, int x = 0, int y = 0) {
            if (!getenv("BBT_PFB_TRACE")) return;
            fprintf(stderr, "bbt: pfb_pick %d x %d on %d streams, %8.3f ms: %s %d %d\n", n_tap, p->n, p->S,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(), what, x, y);
            fflush(stderr);
        };
        trace("allocating");
        bool ready;
        {
            // (input: ns + n_tap - 1 spectra, zeroed; output: ns spectra)
            auto spectra = [&](size_t got) { return (int64_t)((got - (n_tap - 1) * per) / (2 * per)); };
            TuneBench bench((2 * 16 + n_tap) * per, (size_t)2 << 30, [&](size_t got) { return (spectra(got) + n_tap - 1) * per; });
            ready = bench.ready();
            trace("allocated");
            if (ready) {
                const int64_t ns = spectra(bench.size());
                void *in = bench.base(), *out = bench.base() + (ns + n_tap - 1) * per;
                float best_ms = 1e30f;
                for (const PfbCandidate& c : route.candidates) {
                    pfb_apply(p, c, tp);
                    trace("candidate", c.pp, c.gl);
                    const float ms = bench.best_of([&](hipStream_t st) { return bbt_pfb_execute(p, in, out, ns, st); });
                    if (getenv("BBT_RTC_VERBOSE"))
                        fprintf(stderr, "bbt: PolyphaseFilterBank %d x %d on %d streams, %s (pairs %d, order %d): %.3f ms\n", n_tap,
                                p->n, p->S, c.pp == 0 ? "two passes" : "one pass", c.pp, c.gl, ms);
                    if (ms < best_ms) {
                        best_ms = ms;
                        best = c;
                    }
                }
            }
            trace("timed");
        }
        trace("freed");
        if (ready) chosen.remember(key, best);           // (no scratch memory: the rule, and nothing remembered)
    }
    pfb_apply(p, best, tp);
    if (tp && !p->two_pass) bbt_chan_plan_destroy(tp);
    return 0;
}

extern "C" {

int bbt_pfb_plan_create(bbt_pfb_plan** plan, int n_tap, int n_chan, int n_stream,
                        const float* taps_host) {
    ARG_TRY(plan && taps_host, "bbt_pfb_plan_create: null argument");
    *plan = nullptr;
    PfbShape shape;
    std::string refusal;
    if (!pfb_check(n_tap, n_chan, n_stream, &shape, &refusal)) return fail("%s", refusal.c_str());
    bbt_pfb_plan* p = new bbt_pfb_plan;
    p->split_real = shape.split_real;
    p->n = n_chan;
    p->S = shape.S;
    p->npair = shape.npair;
    p->n_tap = n_tap;
    p->window = shape.window;
    p->gn = shape.gn;
    const bool pp_ok = shape.pp_ok;
    const size_t tb = (size_t)n_tap * n_chan * sizeof(float);
    if ((pp_ok && get_tables(p->gn, &p->tabg)) ||
        (p->window && get_tables(4096, &p->tab4096)) ||
        get_tables(n_chan, &p->tab) || hipMalloc((void**)&p->taps, tb) != hipSuccess ||
        hipMemcpy(p->taps, taps_host, tb, hipMemcpyHostToDevice) != hipSuccess) {
        if (g_err.empty()) fail("bbt_pfb_plan_create: tap upload failed");
        bbt_pfb_plan_destroy(p);
        return 1;
    }
    if (p->window) {
        // (pfb_tap_quads: T = 256 threads per pair; gn / 16 in the several-pairs form)
        for (int form = 0; form < (pp_ok ? 2 : 1); ++form) {
            const std::vector<float> perm = pfb_tap_quads(taps_host, n_tap, n_chan, form ? p->gn / 16 : 256);
            float** dst = form ? &p->taps_quads_pp : &p->taps_quads;
            if (hipMalloc((void**)dst, tb) != hipSuccess ||
                hipMemcpy(*dst, perm.data(), tb, hipMemcpyHostToDevice) != hipSuccess) {
                fail("bbt_pfb_plan_create: tap upload failed");
                bbt_pfb_plan_destroy(p);
                return 1;
            }
        }
    }
    if (pfb_pick(p, shape, pfb_knobs_from_env())) {
        bbt_pfb_plan_destroy(p);
        return 1;
    }
    *plan = p;
    return 0;
}

int bbt_pfb_plan_destroy(bbt_pfb_plan* p) {
    if (!p) return 0;
    if (p->two_pass) bbt_chan_plan_destroy(p->two_pass);
    if (p->taps_quads) hipFree(p->taps_quads);
    if (p->taps_quads_pp) hipFree(p->taps_quads_pp);
    if (p->taps) hipFree(p->taps);
    delete p;
    return 0;
}

int bbt_pfb_execute(bbt_pfb_plan* p, const void* in_dev, void* out_dev, int64_t n_spectra,
                    bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_pfb_execute: null argument");
    ARG_TRY(n_spectra >= 0, "bbt_pfb_execute: n_spectra < 0");
    if (n_spectra == 0) return 0;
    const int64_t slab = (int64_t)1 << 20;
    const float2* in = (const float2*)in_dev;
    float2* out = (float2*)out_dev;
    for (int64_t s0 = 0; s0 < n_spectra; s0 += slab) {
        const int64_t ns = (n_spectra - s0 < slab) ? n_spectra - s0 : slab;
        const int64_t off = s0 * p->n * p->S;
        hipStream_t st = (hipStream_t)stream;
        if (p->two_pass) {
            // (one launch of each pass per slab: in pieces whose windowed rows would stay in the
            // Infinity Cache between the passes -- 48 ... 192 MiB -- it is SLOWER, 93-147 against
            // 148-159 G stream-samples/s for 16 / 128 streams: shorter launches, nothing to overlap)
            constexpr int NI = BBT_PFB_NI;
            const long long row16 = (long long)p->n * p->npair;
            const dim3 grid((unsigned)((row16 + 255) / 256), (unsigned)((ns + NI - 1) / NI));
            const float4* src = reinterpret_cast<const float4*>(in + off);
            float4* dst = reinterpret_cast<float4*>(out + off);
            switch (p->n_tap) {
#define BBT_PF(T_) case T_: hipLaunchKernelGGL((k_pfb_fir_rows<T_, NI>), grid, dim3(256), 0, st, src, dst, (long long)ns, \
                                               row16, p->npair, p->n, p->taps); break;
                BBT_PF(4) BBT_PF(8) BBT_PF(12) BBT_PF(16)
#undef BBT_PF
                default: return fail("pfb: two passes need 4, 8, 12 or 16 taps");
            }
            if (bbt_chan_execute(p->two_pass, out + off, out + off, ns, stream)) return 1;
            continue;
        }
        if (p->window) {
            // input of slab s0 starts at spectrum s0 (same offset as the output, except
            // for half spectra of a real pair: n/2 + 1 channels x 2 streams per spectrum)
            const int64_t out_off = p->split_real ? s0 * (p->n / 2 + 1) * 2 * p->S : off;
            pfb_window_dispatch(p, in + off, out + out_off, ns, st);
            continue;
        }
        switch (p->n) {
            case 256: launch_pfb<256>(p, in + off, out + off, ns, st); break;
            case 512: launch_pfb<512>(p, in + off, out + off, ns, st); break;
            case 1024: launch_pfb<1024>(p, in + off, out + off, ns, st); break;
            case 2048: launch_pfb<2048>(p, in + off, out + off, ns, st); break;
            case 4096: launch_pfb<4096>(p, in + off, out + off, ns, st); break;
            default: return fail("pfb: unsupported n_chan %d", p->n);
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// detection + integration
extern "C" int bbt_detect_integrate(const void* in_dev, void* out_dev, int64_t n_out, int64_t step,
                                    int64_t n_elem, int mode, int average, bbt_stream stream) {
    ARG_TRY(in_dev && out_dev, "bbt_detect_integrate: null argument");
    ARG_TRY(n_out >= 0 && step >= 1 && n_elem >= 1, "bbt_detect_integrate: bad sizes");
    ARG_TRY(mode >= 0 && mode <= 2, "bbt_detect_integrate: mode must be 0 (square), 1 (power) or 2 (sum)");
    ARG_TRY(mode != 1 || n_elem % 2 == 0,
            "bbt_detect_integrate: power needs (X, Y) pairs, n_elem=%lld is odd", (long long)n_elem);
    if (n_out == 0) return 0;
    const long long q = mode == 1 ? n_elem / 2 : n_elem;
    const long long tiles = (q + 255) / 256;
    ARG_TRY(n_out * tiles < (1ll << 31), "bbt_detect_integrate: too many output elements for one call");
    const float scale = average ? 1.0f / (float)step : 1.0f;
    const dim3 grid((unsigned)(n_out * tiles)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0)
        hipLaunchKernelGGL((k_detect_integrate<0>), grid, block, 0, st, in_dev, out_dev,
                           (long long)n_out, (long long)step, q, scale);
    else if (mode == 1)
        hipLaunchKernelGGL((k_detect_integrate<1>), grid, block, 0, st, in_dev, out_dev,
                           (long long)n_out, (long long)step, q, scale);
    else
        hipLaunchKernelGGL((k_detect_integrate<2>), grid, block, 0, st, in_dev, out_dev,
                           (long long)n_out, (long long)step, q, scale);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int bbt_detect_power_axis(const void* in_dev, void* out_dev, int64_t n_out, int64_t step,
                                     int outer, int inner, int average, bbt_stream stream) {
    ARG_TRY(in_dev && out_dev, "bbt_detect_power_axis: null argument");
    ARG_TRY(n_out >= 0 && step >= 1 && outer >= 1 && inner >= 1, "bbt_detect_power_axis: bad sizes");
    if (n_out == 0) return 0;
    const long long total = (long long)n_out * outer * inner;
    ARG_TRY((total + 255) / 256 < (1ll << 31), "bbt_detect_power_axis: too many output elements for one call");
    hipLaunchKernelGGL(k_power_axis, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)in_dev, (float*)out_dev, (long long)n_out, (long long)step, outer, inner,
                       average ? 1.0f / (float)step : 1.0f);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// folding by a run table (fold_kernels.hpp)
extern "C" int bbt_fold_runs(const void* in_dev, void* out_dev, int64_t n_in, int64_t n_elem, int mode,
                             const int64_t* slot_ptr_dev, const int64_t* run_begin_dev,
                             const int64_t* run_end_dev, int64_t n_slot, const float* scale_dev,
                             int accumulate, void* work_dev, int64_t work_floats, bbt_stream stream) {
    ARG_TRY(in_dev && out_dev && slot_ptr_dev && run_begin_dev && run_end_dev,
            "bbt_fold_runs: null argument");
    ARG_TRY(n_in >= 0 && n_elem >= 1 && n_slot >= 0 && work_floats >= 0, "bbt_fold_runs: bad sizes");
    ARG_TRY(mode >= 0 && mode <= 2, "bbt_fold_runs: mode must be 0 (square), 1 (power) or 2 (sum)");
    ARG_TRY(mode != 1 || n_elem % 2 == 0,
            "bbt_fold_runs: power needs (X, Y) pairs, n_elem=%lld is odd", (long long)n_elem);
    ARG_TRY(accumulate == 0 || accumulate == 1, "bbt_fold_runs: accumulate must be 0 or 1");
    ARG_TRY(mode != 1 || ((uintptr_t)in_dev & 15) == 0, "bbt_fold_runs: power needs 16-byte aligned input");
    ARG_TRY(work_floats == 0 || work_dev, "bbt_fold_runs: work_floats > 0 needs a work area");
    if (n_slot == 0) return 0;
    // units: what one lane loads per sample (16 bytes where the row and the address allow)
    const long long in_bytes = mode == 2 ? 4 : 8;
    const long long elems_per_vec = 16 / in_bytes;
    const bool vec = mode == 1 || (n_elem % elems_per_vec == 0 && ((uintptr_t)in_dev & 15) == 0);
    const long long n_unit = vec ? n_elem / elems_per_vec : n_elem;
    const int outw = mode == 1 ? 4 : (mode == 0 ? (vec ? 2 : 1) : (vec ? 4 : 1));
    const long long n_out_f = n_unit * outw;
    int lg_tc = 0;
    while (lg_tc < 8 && (1ll << lg_tc) < n_unit) ++lg_tc;
    const int tt = 256 >> lg_tc;
    const long long tiles = (n_unit + (1ll << lg_tc) - 1) >> lg_tc;
    // split of each slot's samples over workgroups, from the arguments only: about 2048
    // workgroups in all (8 per CU), at most 64 shares, at least ~64 samples per lane on average,
    // and no more shares than the work area holds
    const long long base = tiles * n_slot;
    long long split = (2048 + base - 1) / base;
    split = std::min(split, 64ll);
    split = std::min(split, std::max(1ll, (long long)(n_in / (n_slot * tt * 64ll))));
    split = std::min(split, std::max(1ll, (long long)(work_floats / (n_slot * n_out_f))));
    if (!work_dev) split = 1;
    ARG_TRY(base * split < (1ll << 31), "bbt_fold_runs: too many slots x columns for one call");
    hipStream_t st = (hipStream_t)stream;
    float* out = (float*)out_dev;
    float* dst = split == 1 ? out : (float*)work_dev;
    const float* prev = split == 1 && accumulate ? out : nullptr;
    const float* sc = split == 1 ? scale_dev : nullptr;
    const long long stride = n_slot * n_out_f;
    const dim3 grid((unsigned)(base * split)), block(256);
#define BBT_FOLD_LAUNCH(M, V)                                                                            \
    hipLaunchKernelGGL((k_fold_gather<M, V>), grid, block, 0, st, in_dev, dst, (long long)n_in, n_unit,  \
                       lg_tc, tiles, (long long)n_slot, (int)split, (const long long*)slot_ptr_dev,      \
                       (const long long*)run_begin_dev, (const long long*)run_end_dev, prev, sc, stride)
    if (mode == 1) BBT_FOLD_LAUNCH(1, 1);
    else if (mode == 0 && vec) BBT_FOLD_LAUNCH(0, 1);
    else if (mode == 0) BBT_FOLD_LAUNCH(0, 0);
    else if (vec) BBT_FOLD_LAUNCH(2, 1);
    else BBT_FOLD_LAUNCH(2, 0);
#undef BBT_FOLD_LAUNCH
    HIP_TRY(hipGetLastError());
    if (split > 1) {
        const long long total = n_slot * n_out_f;
        ARG_TRY((total + 255) / 256 < (1ll << 31), "bbt_fold_runs: too many output elements for one call");
        hipLaunchKernelGGL(k_fold_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           (const float*)work_dev, out, (long long)n_slot, n_out_f, (int)split, stride,
                           scale_dev, accumulate);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// ---------------------------------------------------------------------------
// run tables from polynomial phases (phase_kernels.hpp)
static int64_t phase_tiles(int64_t n) { return (n + BBT_PHASE_TILE - 1) / BBT_PHASE_TILE; }

// work area: grid (int32 per cell, padded to 16 bytes) | sample tiles | cell tiles | n_run, status,
// n_occupied, pad | begin, slot, slot by position (run_cap each)
extern "C" int bbt_phase_runs_work(int64_t n_samples, int64_t n_cell, int64_t run_cap, int64_t* bytes) {
    ARG_TRY(bytes, "bbt_phase_runs_work: null argument");
    ARG_TRY(n_samples >= 0 && n_cell >= 0 && run_cap >= 0, "bbt_phase_runs_work: bad sizes");
    ARG_TRY(n_cell < (1ll << 40) && n_samples < (1ll << 40) && run_cap <= n_samples,
            "bbt_phase_runs_work: sizes out of range");
    *bytes = ((n_cell * 4 + 15) / 16) * 16 + 8 * (phase_tiles(n_samples) + phase_tiles(n_cell) + 4 + 3 * run_cap);
    return 0;
}

extern "C" int bbt_phase_runs(const void* pieces_dev, int64_t n_piece, int n_coeff, int64_t s_begin,
                              int64_t s_end, int64_t n_phase, const int64_t* rows_dev, int64_t n_row,
                              int64_t n_cell, int64_t slot0, int64_t n_slot, int64_t run_cap,
                              int64_t* slot_ptr_dev, int64_t* run_begin_dev, int64_t* run_end_dev,
                              int64_t* counts_dev, void* work_dev, int64_t work_bytes, int64_t* info,
                              bbt_stream stream) {
    ARG_TRY(pieces_dev && rows_dev && slot_ptr_dev && run_begin_dev && run_end_dev && counts_dev && work_dev && info,
            "bbt_phase_runs: null argument");
    ARG_TRY(n_piece >= 1 && n_piece < (1ll << 31) && n_coeff >= 1 && n_coeff <= 64 && n_phase >= 1 && n_row >= 1,
            "bbt_phase_runs: bad sizes");
    ARG_TRY(s_begin >= 0 && s_end > s_begin, "bbt_phase_runs: the pieces cover no samples");
    ARG_TRY(slot0 >= 0 && n_row * n_phase <= n_slot - slot0, "bbt_phase_runs: the rows do not fit the slots");
    ARG_TRY(n_cell >= 1 && run_cap >= 1 && run_cap <= s_end - s_begin && run_cap < (1ll << 31),
            "bbt_phase_runs: bad grid or run capacity");
    ARG_TRY(((uintptr_t)work_dev & 15) == 0, "bbt_phase_runs: the work area must be 16-byte aligned");
    const int64_t n = s_end - s_begin;
    int64_t need = 0;
    if (bbt_phase_runs_work(n, n_cell, run_cap, &need) != 0) return 1;
    ARG_TRY(work_bytes >= need, "bbt_phase_runs: work area of %lld bytes, %lld needed", (long long)work_bytes,
            (long long)need);
    const int64_t nt_s = phase_tiles(n), nt_c = phase_tiles(n_cell);
    ARG_TRY(nt_s < (1ll << 31) && nt_c < (1ll << 31) && n_slot < (1ll << 38), "bbt_phase_runs: too large for one call");
    hipStream_t st = (hipStream_t)stream;
    int* grid = (int*)work_dev;
    long long* w = (long long*)((char*)work_dev + ((n_cell * 4 + 15) / 16) * 16);
    long long* tile_s = w;
    long long* tile_c = tile_s + nt_s;
    long long* scalars = tile_c + nt_c;                      // n_run, status, n_occupied
    long long* begin_t = scalars + 4;
    long long* slot_t = begin_t + run_cap;
    long long* slot_sorted = slot_t + run_cap;
    const long long* q = (const long long*)pieces_dev;
    PhasePieces P;
    P.lo = q;
    P.m0 = q + (n_piece + 1);
    P.row = P.m0 + n_piece;
    P.dt0 = (const double*)(P.row + n_piece);
    P.step = P.dt0 + n_piece;
    P.ref_int = P.step + n_piece;
    P.ref_frac = P.ref_int + n_piece;
    P.coeff = P.ref_frac + n_piece;
    P.n_piece = (int)n_piece;
    P.n_coeff = n_coeff;
    const long long* rows = (const long long*)rows_dev;      // k0 | n_cycle | cell0
    HIP_TRY(hipMemsetAsync(grid, 0, (size_t)n_cell * 4, st));
    HIP_TRY(hipMemsetAsync(scalars, 0, 32, st));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)(n_row * n_phase) * 8, st));
    hipLaunchKernelGGL(k_phase_count, dim3((unsigned)nt_s), dim3(256), 0, st, P, (long long)n_phase, tile_s);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(256), 0, st, tile_s, (long long)nt_s, scalars, (long long)run_cap,
                       (const long long*)nullptr, scalars + 1);
    hipLaunchKernelGGL(k_phase_scatter, dim3((unsigned)nt_s), dim3(256), 0, st, P, (long long)n_phase,
                       (const long long*)tile_s, rows, rows + n_row, rows + 2 * n_row, (long long)n_row,
                       (long long)n_cell, (long long)slot0, (long long)run_cap, begin_t, slot_t, grid, scalars + 1);
    hipLaunchKernelGGL(k_grid_count, dim3((unsigned)nt_c), dim3(256), 0, st, (const int*)grid, (long long)n_cell, tile_c);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(256), 0, st, tile_c, (long long)nt_c, scalars + 2,
                       (long long)run_cap, (const long long*)scalars, scalars + 1);
    hipLaunchKernelGGL(k_grid_compact, dim3((unsigned)nt_c), dim3(256), 0, st, (const int*)grid, (long long)n_cell,
                       (const long long*)tile_c, (const long long*)begin_t, (const long long*)slot_t,
                       (const long long*)scalars, (long long)run_cap, (const long long*)(scalars + 1),
                       (long long)s_end, (long long)slot0, (long long)(n_row * n_phase), (long long*)run_begin_dev,
                       (long long*)run_end_dev, slot_sorted, (unsigned long long*)counts_dev);
    hipLaunchKernelGGL(k_slot_ptr, dim3((unsigned)((n_slot + 1 + 255) / 256)), dim3(256), 0, st,
                       (const long long*)slot_sorted, (const long long*)scalars, (long long)run_cap,
                       (const long long*)(scalars + 1), (long long)n_slot, (long long*)slot_ptr_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(info, scalars, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------
// modulation by a pulse profile (modulate_kernels.hpp)
static int modulate_args(const char* who, const void* in_dev, void* out_dev, int64_t n_in, int64_t n_float,
                         const float* gain_dev, int64_t n_phase, int64_t gain_stride, ModArgs* A) {
    ARG_TRY(in_dev && out_dev && gain_dev, "%s: null argument", who);
    ARG_TRY(n_in >= 1 && n_float >= 1 && n_phase >= 1 && gain_stride >= 0, "%s: bad sizes", who);
    ARG_TRY(n_float < (1ll << 30) && n_phase < (1ll << 31) && n_in <= (1ll << 41) / n_float,
            "%s: too large for one call", who);
    ARG_TRY(gain_stride == 0 || n_float == gain_stride || n_float == 2 * gain_stride,
            "%s: the gain stride must be 0 or the elements of a sample (%lld floats, stride %lld)", who,
            (long long)n_float, (long long)gain_stride);
    ARG_TRY(aligned4(in_dev, out_dev, gain_dev), "%s: arrays must be 4-byte aligned", who);
    A->in = (const float*)in_dev;
    A->out = (float*)out_dev;
    A->n_in = n_in;
    A->n_float = n_in * n_float;
    A->fps = (unsigned)n_float;
    A->gain = gain_dev;
    A->n_phase = n_phase;
    A->gs = (unsigned)gain_stride;
    A->cshift = gain_stride != 0 && n_float == 2 * gain_stride ? 1 : 0;
    return 0;
}

// one launch: 16-byte accesses where both arrays allow them, whole samples per access where the
// sample (and, for a gain per element, the gain table) allows that too
template <int ROUTE>
static int modulate_launch(const ModArgs& A, const ModRuns& R, const PhasePieces& P, hipStream_t st) {
    const bool wide = (((uintptr_t)A.in | (uintptr_t)A.out) & 15) == 0;
    const int w = wide ? 4 : 1;
    const bool one = !wide || (A.fps % 4 == 0 && (A.gs == 0 || ((uintptr_t)A.gain & 15) == 0));
    const long long n_acc = A.n_float / w;
    const long long tiles = std::max(1ll, (n_acc + BBT_MOD_TILE - 1) / BBT_MOD_TILE);
    const dim3 grid((unsigned)tiles), block(256);
    if (!wide) hipLaunchKernelGGL((k_modulate<ROUTE, 1, true>), grid, block, 0, st, A, R, P);
    else if (one) hipLaunchKernelGGL((k_modulate<ROUTE, 4, true>), grid, block, 0, st, A, R, P);
    else hipLaunchKernelGGL((k_modulate<ROUTE, 4, false>), grid, block, 0, st, A, R, P);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int bbt_modulate_runs(const void* in_dev, void* out_dev, int64_t n_in, int64_t n_float,
                                 const float* gain_dev, int64_t n_phase, int64_t gain_stride,
                                 const int64_t* run_begin_dev, const int64_t* run_bin_dev, int64_t n_run,
                                 bbt_stream stream) {
    ModArgs A;
    if (modulate_args("bbt_modulate_runs", in_dev, out_dev, n_in, n_float, gain_dev, n_phase, gain_stride, &A) != 0)
        return 1;
    ARG_TRY(run_begin_dev && run_bin_dev, "bbt_modulate_runs: null argument");
    ARG_TRY(n_run >= 1 && n_run <= n_in, "bbt_modulate_runs: bad sizes (%lld runs for %lld samples)", (long long)n_run,
            (long long)n_in);
    ModRuns R;
    R.begin = (const long long*)run_begin_dev;
    R.bin = (const long long*)run_bin_dev;
    R.n_run = n_run;
    PhasePieces P = {};
    return modulate_launch<0>(A, R, P, (hipStream_t)stream);
}

extern "C" int bbt_modulate_pieces(const void* in_dev, void* out_dev, int64_t n_in, int64_t n_float,
                                   const float* gain_dev, int64_t n_phase, int64_t gain_stride,
                                   const void* pieces_dev, int64_t n_piece, int n_coeff, bbt_stream stream) {
    ModArgs A;
    if (modulate_args("bbt_modulate_pieces", in_dev, out_dev, n_in, n_float, gain_dev, n_phase, gain_stride, &A) != 0)
        return 1;
    ARG_TRY(pieces_dev, "bbt_modulate_pieces: null argument");
    ARG_TRY(n_piece >= 1 && n_piece < (1ll << 31) && n_coeff >= 1 && n_coeff <= 64, "bbt_modulate_pieces: bad sizes");
    ARG_TRY(((uintptr_t)pieces_dev & 7) == 0, "bbt_modulate_pieces: the pieces must be 8-byte aligned");
    const long long* q = (const long long*)pieces_dev;
    PhasePieces P;
    P.lo = q;
    P.m0 = q + (n_piece + 1);
    P.row = P.m0 + n_piece;
    P.dt0 = (const double*)(P.row + n_piece);
    P.step = P.dt0 + n_piece;
    P.ref_int = P.step + n_piece;
    P.ref_frac = P.ref_int + n_piece;
    P.coeff = P.ref_frac + n_piece;
    P.n_piece = (int)n_piece;
    P.n_coeff = n_coeff;
    ModRuns R = {};
    return modulate_launch<1>(A, R, P, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// spectral kurtosis and excision (sk_kernels.hpp; the tiling is sk_geo.hpp's)
static int sk_args(const char* who, const void* x_dev, int64_t n_block, int64_t n, int64_t n_elem, int is_complex,
                   double averaged, int64_t group, bool aligned16, long long slab, SkArgs* A, SkGeo* g) {
    ARG_TRY(n >= 2 && n <= BBT_SK_MAX_N, "%s: n must be 2 ... 65536 (got %lld)", who, (long long)n);
    ARG_TRY(averaged > 0. && averaged <= 1e9, "%s: averaged must be positive", who);
    const char* err = sk_geo(n_block, n, n_elem, is_complex != 0, group, aligned16, slab, g);
    ARG_TRY(!err, "%s: %s", who, err ? err : "");
    ARG_TRY(n_block * n <= (1ll << 40) / n_elem, "%s: too large for one call", who);
    ARG_TRY(((uintptr_t)x_dev & (is_complex ? 7 : 3)) == 0, "%s: arrays must be aligned to their elements", who);
    A->x = x_dev;
    A->n_block = n_block, A->n = n, A->n_elem = n_elem;
    A->averaged = averaged;
    A->group = (int)group;
    return 0;
}

#define BBT_SK_LAUNCH(KERNEL)                                                                          \
    do {                                                                                               \
        const dim3 grid((unsigned)(g.n_tile * g.n_zgroup)), block(BBT_SK_THREADS);                     \
        if (is_complex && g.v == 2) hipLaunchKernelGGL((KERNEL<true, 2>), grid, block, 0, st, A, g);   \
        else if (is_complex) hipLaunchKernelGGL((KERNEL<true, 1>), grid, block, 0, st, A, g);          \
        else if (g.v == 4) hipLaunchKernelGGL((KERNEL<false, 4>), grid, block, 0, st, A, g);           \
        else hipLaunchKernelGGL((KERNEL<false, 1>), grid, block, 0, st, A, g);                         \
        HIP_TRY(hipGetLastError());                                                                    \
    } while (0)

extern "C" int bbt_sk_estimate(const void* x_dev, float* sk_dev, int64_t n_block, int64_t n, int64_t n_elem,
                               int is_complex, double averaged, bbt_stream stream) {
    ARG_TRY(x_dev && sk_dev, "bbt_sk_estimate: null argument");
    ARG_TRY(((uintptr_t)sk_dev & 3) == 0, "bbt_sk_estimate: sk must be 4-byte aligned");
    SkArgs A = {};
    SkGeo g = {};
    if (sk_args("bbt_sk_estimate", x_dev, n_block, n, n_elem, is_complex, averaged, 1, ((uintptr_t)x_dev & 15) == 0, 0,
                &A, &g) != 0)
        return 1;
    A.sk = sk_dev;
    hipStream_t st = (hipStream_t)stream;
    BBT_SK_LAUNCH(k_sk_estimate);
    return 0;
}

// bytes of a slab: BBT_SK_SLAB, or what the environment's BBT_SK_SLAB_KIB asks for (for measuring;
// no value of the output depends on it)
static long long sk_slab_bytes() {
    const char* e = getenv("BBT_SK_SLAB_KIB");
    if (e && *e) {
        const long long kib = atoll(e);
        if (kib >= 1 && kib <= (1 << 20)) return kib * 1024;
    }
    return BBT_SK_SLAB;
}

extern "C" int bbt_sk_excise(const void* x_dev, void* out_dev, int64_t n_block, int64_t n, int64_t n_elem,
                             int is_complex, double averaged, float lo, float hi, int64_t group, float* sk_or_null,
                             uint8_t* flags_or_null, bbt_stream stream) {
    ARG_TRY(x_dev && out_dev, "bbt_sk_excise: null argument");
    ARG_TRY(lo <= hi, "bbt_sk_excise: the limits must be ordered, lo <= hi");
    ARG_TRY(((uintptr_t)sk_or_null & 3) == 0, "bbt_sk_excise: sk must be 4-byte aligned");
    ARG_TRY(((uintptr_t)out_dev & (is_complex ? 7 : 3)) == 0, "bbt_sk_excise: arrays must be aligned to their elements");
    SkArgs A = {};
    SkGeo g = {};
    const bool aligned16 = (((uintptr_t)x_dev | (uintptr_t)out_dev) & 15) == 0;
    if (sk_args("bbt_sk_excise", x_dev, n_block, n, n_elem, is_complex, averaged, group, aligned16, sk_slab_bytes(), &A,
                &g) != 0)
        return 1;
    A.out = out_dev;
    A.sk = sk_or_null;
    A.flags = flags_or_null;
    A.lo = lo, A.hi = hi;
    hipStream_t st = (hipStream_t)stream;
    BBT_SK_LAUNCH(k_sk_excise);
    return 0;
}

// ---------------------------------------------------------------------------
// NumPy's normal stream (noise_kernels.hpp)
static int64_t noise_tiles(int64_t n_words) { return (n_words + BBT_NOISE_TILE - 1) / BBT_NOISE_TILE; }

// work area: counters (4 per frame) | totals | flags | tile offsets (int64 each) | tile counts
// (6 uint32 per tile) | tile maps | tile entry states (uint32 / int32 per tile)
extern "C" int bbt_philox_normal_work(int64_t n_frame, int64_t n_words, int64_t* bytes) {
    ARG_TRY(bytes, "bbt_philox_normal_work: null argument");
    ARG_TRY(n_frame >= 1 && n_frame <= 65535 && n_words >= 4 && n_words % 4 == 0 && n_words < (1ll << 40),
            "bbt_philox_normal_work: bad sizes");
    const int64_t tiles = n_frame * noise_tiles(n_words);
    *bytes = 8 * (6 * n_frame + tiles) + 4 * 8 * tiles;
    return 0;
}

extern "C" int bbt_philox_normal(const uint64_t* key, const uint64_t* counters, int64_t n_frame, int64_t n,
                                 int64_t n_words, double guard, float* out_dev, int64_t out_stride,
                                 void* work_dev, int64_t work_bytes, int64_t* totals, int64_t* flags,
                                 bbt_stream stream) {
    ARG_TRY(key && counters && out_dev && work_dev && totals && flags, "bbt_philox_normal: null argument");
    int64_t need = 0;
    if (bbt_philox_normal_work(n_frame, n_words, &need) != 0) return 1;
    ARG_TRY(n >= 1 && n <= out_stride && n < (1ll << 40), "bbt_philox_normal: bad frame length or stride");
    ARG_TRY(guard >= 0, "bbt_philox_normal: the guard must not be negative");
    ARG_TRY(work_bytes >= need, "bbt_philox_normal: work area of %lld bytes, %lld needed", (long long)work_bytes,
            (long long)need);
    ARG_TRY(((uintptr_t)work_dev & 15) == 0 && ((uintptr_t)out_dev & 3) == 0,
            "bbt_philox_normal: the work area must be 16-byte aligned, the output 4-byte aligned");
    const int64_t n_tile = noise_tiles(n_words);
    ARG_TRY(n_tile < (1ll << 31), "bbt_philox_normal: too many words for one call");
    hipStream_t st = (hipStream_t)stream;
    // the first block of a frame comes from the state's counter plus one
    std::vector<uint64_t> first((size_t)n_frame * 4);
    for (int64_t f = 0; f < n_frame; ++f) {
        bool carry = true;
        for (int i = 0; i < 4; ++i) {
            const uint64_t c = counters[f * 4 + i] + (carry ? 1 : 0);
            carry = carry && c == 0;
            first[f * 4 + i] = c;
        }
    }
    const int64_t tiles = n_frame * n_tile;
    nu64* ctr = (nu64*)work_dev;
    long long* total_d = (long long*)(ctr + 4 * n_frame);
    long long* flag_d = total_d + n_frame;
    long long* tile_off = flag_d + n_frame;
    unsigned* tile_cnt = (unsigned*)(tile_off + tiles);
    unsigned* tile_map = tile_cnt + 6 * tiles;
    int* tile_entry = (int*)(tile_map + tiles);
    HIP_TRY(hipMemcpyAsync(ctr, first.data(), (size_t)n_frame * 32, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                     // (pageable source: `first` may go)
    HIP_TRY(hipMemsetAsync(total_d, 0, (size_t)n_frame * 16, st));
    const dim3 grid((unsigned)n_tile, (unsigned)n_frame), block(256);
    hipLaunchKernelGGL(k_noise_count, grid, block, 0, st, (const nu64*)ctr, (nu64)key[0], (nu64)key[1],
                       (long long)n_words, (long long)n_tile, tile_map, tile_cnt);
    hipLaunchKernelGGL(k_noise_scan, dim3((unsigned)n_frame), block, 0, st, (const unsigned*)tile_map,
                       (const unsigned*)tile_cnt, (long long)n_tile, tile_entry, tile_off, total_d);
    hipLaunchKernelGGL(k_noise_emit, grid, block, 0, st, (const nu64*)ctr, (nu64)key[0], (nu64)key[1],
                       (long long)n_words, (long long)n_tile, (const int*)tile_entry, (const long long*)tile_off,
                       (long long)n, guard, out_dev, (long long)out_stride, flag_d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(totals, total_d, (size_t)n_frame * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flags, flag_d, (size_t)n_frame * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------
// Real2Complex (r2c_kernels.hpp)
struct bbt_r2c_plan {
    std::mutex mu;                  // one call at a time: the work buffers belong to the running call
    int device = 0;
    int64_t M = 0;
    int S = 0;
    bool one_pass = false;
    bool big = false;               // M = 16384: the four-stage one-workgroup transform (big_kernels.hpp)
    cf* big_tw = nullptr;           // its table (shared)
    // one pass: G / M and the transform's stages (run-time specialised kernel, or the general one)
    cf* resp = nullptr;
    GenGeo g = {}, gr = {};
    cf* wn = nullptr;
    cf* wnr = nullptr;
    bool rtc = false;
    G2Plan q, qr;
    cf* qw = nullptr;
    cf* qwr = nullptr;
    hipFunction_t k2 = nullptr;
    // multi-level: odd rows of four slots -> two-stream blocks, convolved by an overlap-save plan
    bbt_osm_plan* osm = nullptr;
    int64_t cap = 0;                // blocks the work buffers may hold
    int64_t alloc = 0;              // blocks they hold now (allocated by the first call that needs them)
    float* work_in = nullptr;
    float* work_out = nullptr;
    hipEvent_t ev_done = nullptr;   // end of the previous call (on whatever stream it ran)
    bool ev_done_set = false;
};

static void r2c_release(bbt_r2c_plan* p) {
    if (!p) return;
    int cur = 0;
    const bool switched = hipGetDevice(&cur) == hipSuccess && cur != p->device && hipSetDevice(p->device) == hipSuccess;
    if (p->ev_done_set) (void)hipEventSynchronize(p->ev_done);
    if (p->osm) bbt_osm_plan_destroy(p->osm);
    if (p->resp) (void)hipFree(p->resp);
    if (p->work_in) (void)hipFree(p->work_in);
    if (p->work_out) (void)hipFree(p->work_out);
    if (p->ev_done) (void)hipEventDestroy(p->ev_done);
    if (switched) (void)hipSetDevice(cur);
    delete p;
}

// G[j] = -i W_2M^j for 0 < j < M, G[0] = 0 (FFT-natural order), times `scale`; in double
static std::vector<cf> r2c_response(int64_t M, double scale) {
    std::vector<cf> h((size_t)M);
    h[0] = make_float2(0.f, 0.f);
    for (int64_t j = 1; j < M; ++j) {
        const double a = -M_PI * (double)j / (double)M;
        h[(size_t)j] = make_float2((float)(sin(a) * scale), (float)(-cos(a) * scale));
    }
    return h;
}

// bytes of each work buffer of the three-step route: 256 MiB, or what the environment's BBT_R2C_WORK_KIB asks
// for, in KiB, fractions allowed (a developer knob, read when a plan is made: tests make a call of a few
// groups run in several batches; no value of the output depends on it)
static int64_t r2c_work_bytes() {
    const char* e = getenv("BBT_R2C_WORK_KIB");
    if (e && *e) {
        const double kib = atof(e);
        if (kib > 0. && kib <= (double)(1 << 22)) return (int64_t)(kib * 1024.);
    }
    return int64_t(256) << 20;
}

extern "C" {

int bbt_r2c_plan_create(bbt_r2c_plan** plan, int64_t n_out, int n_stream) {
    return bbt_r2c_plan_create_ex(plan, n_out, n_stream, 0);
}

int bbt_r2c_plan_create_ex(bbt_r2c_plan** plan, int64_t n_out, int n_stream, int flags) {
    ARG_TRY(plan, "bbt_r2c_plan_create: null plan");
    ARG_TRY((flags & ~BBT_R2C_MULTI_LEVEL) == 0, "bbt_r2c_plan_create: unknown flags %d", flags);
    *plan = nullptr;
    ARG_TRY(n_stream >= 1, "bbt_r2c_plan_create: n_stream=%d must be at least 1", n_stream);
    ARG_TRY(n_out >= 2 && is_7smooth(n_out),
            "bbt_r2c_plan_create: n_out=%lld must be 2^a 3^b 5^c 7^d and at least 2", (long long)n_out);
    bbt_r2c_plan* p = new bbt_r2c_plan;
    auto bail = [&](int rc) { r2c_release(p); return rc; };
    if (hipGetDevice(&p->device) != hipSuccess) return bail(fail("bbt_r2c_plan_create: hipGetDevice failed"));
    p->M = n_out;
    p->S = n_stream;
    const bool multi = flags & BBT_R2C_MULTI_LEVEL;
    p->big = n_out == 16384 && !multi;
    p->one_pass = (n_out <= BBT_GEN_MAX_LEN || p->big) && !multi;
    if (p->big) {
        if (get_big_table((int)n_out, &p->big_tw)) return bail(1);
        if (upload(&p->resp, r2c_response(n_out, 1.0 / (double)n_out))) return bail(1);
    } else if (p->one_pass) {
        if (!gen_factor_7smooth(n_out, &p->g)) return bail(fail("bbt_r2c_plan_create: cannot factor %lld", (long long)n_out));
        if (get_gen_table(&p->g, &p->wn) || get_reversed(p->g, &p->gr, &p->wnr)) return bail(1);
        if (upload(&p->resp, r2c_response(n_out, 1.0 / (double)n_out))) return bail(1);
        if (rtc_mode()) {
            bool ok = g2_plan((int)n_out, 1, &p->q, g2_pmax(BBT_G2_KIND_ROW));
            if (ok) p->qr = g2_reversed(p->q);
            ok = ok && p->q.threads() <= 1024 && std::max(p->q.lds_elems, p->qr.lds_elems) * 8 <= 96 * 1024;
            if (!ok) fail("no stage list within a workgroup for %lld", (long long)n_out);
            if (ok) {
                const std::string w = p->q.threads() >= 448 ? "4" : "0";
                const std::string src = "#include \"gen2_kernels.hpp\"\n" + g2_trait_source("GA", p->q) +
                                        g2_trait_source("GB", p->qr) + "BBT_G2_KERNEL_R2C(k_r2c, GA, GB, " + w + ")\n";
                ok = !g2_build(src, {"k_r2c"}, &p->k2);
            }
            if (ok) ok = !(get_g2_table(p->q, &p->qw) || get_g2_table(p->qr, &p->qwr));
            if (!ok && rtc_mode() == 2) return bail(1);
            if (!ok) g2_warn_once("bbt_r2c_plan_create");
            p->rtc = ok;
        }
    } else {
        // two real streams a, b of a transform are one complex stream of the plan (a + i b)
        const std::vector<cf> h = r2c_response(n_out, 1.0);
        if (bbt_osm_plan_create(&p->osm, n_out, 2, 1, h.data(), 0, nullptr)) {
            const std::string why = g_err;
            return bail(fail("bbt_r2c_plan_create: no overlap-save plan for n_out=%lld: %s", (long long)n_out,
                             why.c_str()));
        }
        // work buffers of at most 256 MiB each (one block at least)
        p->cap = std::max<int64_t>(1, r2c_work_bytes() / (n_out * 16));
    }
    if (hipEventCreateWithFlags(&p->ev_done, hipEventDisableTiming) != hipSuccess)
        return bail(fail("bbt_r2c_plan_create: hipEventCreateWithFlags failed"));
    *plan = p;
    return 0;
}

int bbt_r2c_plan_destroy(bbt_r2c_plan* p) {
    r2c_release(p);
    return 0;
}

int bbt_r2c_plan_info(const bbt_r2c_plan* p, int* one_pass, int64_t* workspace_bytes) {
    ARG_TRY(p, "bbt_r2c_plan_info: null plan");
    if (one_pass) *one_pass = p->one_pass ? 1 : 0;
    if (workspace_bytes) {
        int64_t ws = 2 * p->alloc * p->M * 16;
        if (p->osm) {
            int64_t w = 0;
            int chunk, n1, n2;
            if (bbt_osm_plan_info(p->osm, &w, &chunk, &n1, &n2) == 0) ws += w;
        }
        *workspace_bytes = ws;
    }
    return 0;
}

int bbt_r2c_execute(bbt_r2c_plan* p, const void* in_dev, void* out_dev, int64_t n_frames, bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_r2c_execute: null argument");
    ARG_TRY(n_frames >= 0, "bbt_r2c_execute: n_frames=%lld", (long long)n_frames);
    ARG_TRY((uintptr_t)in_dev % 4 == 0, "bbt_r2c_execute: in_dev is not aligned to its float32 samples (4 bytes)");
    ARG_TRY((uintptr_t)out_dev % 8 == 0, "bbt_r2c_execute: out_dev is not aligned to its complex64 samples (8 bytes)");
    if (n_frames == 0) return 0;
    std::lock_guard<std::mutex> lock(p->mu);
    hipStream_t st = (hipStream_t)stream;
    const long long M = p->M, S = p->S, n_slot = n_frames * S, n_group = (n_slot + 3) / 4;
    ARG_TRY(n_group < (1ll << 31), "bbt_r2c_execute: too many frames x streams for one call");
    {   // (the sink reads the even input rows after other workgroups have written their output)
        const uintptr_t i0 = (uintptr_t)in_dev, i1 = i0 + (uintptr_t)(n_frames * 2 * M * S * 4);
        const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(n_frames * M * S * 8);
        ARG_TRY(i1 <= o0 || o1 <= i0, "bbt_r2c_execute: in_dev and out_dev must not overlap");
    }
    if (p->ev_done_set) HIP_TRY(hipStreamWaitEvent(st, p->ev_done, 0));
    const float* in = (const float*)in_dev;
    float2* out = (float2*)out_dev;
    if (p->one_pass) {
        // 16-byte accesses where four slots are neighbouring streams, 8-byte ones for pairs
        const uintptr_t al = (uintptr_t)in_dev | (uintptr_t)out_dev;
        const int vec = (S % 4 == 0 && (al & 15) == 0) ? 4 : (S % 2 == 0 && (al & 15) == 0) ? 2 : 1;
        if (p->big) {
            constexpr size_t lds = BigGeo<16384>::LDS_ELEMS * sizeof(v2);
#define BBT_R2C_BIG(V)                                                                                      \
    do {                                                                                                    \
        if (ensure_dyn_lds((const void*)k_r2c_big<16384, V>, lds)) return 1;                               \
        hipLaunchKernelGGL((k_r2c_big<16384, V>), dim3((unsigned)n_group), dim3(16384 / 16), lds, st, in, out, \
                           (int)S, (long long)n_slot, (const cf*)p->resp, (const cf*)p->big_tw);            \
    } while (0)
            if (vec == 4) BBT_R2C_BIG(4);
            else if (vec == 2) BBT_R2C_BIG(2);
            else BBT_R2C_BIG(1);
#undef BBT_R2C_BIG
            HIP_TRY(hipGetLastError());
        } else if (p->rtc) {
            if (g2_launch(p->k2, dim3((unsigned)n_group), dim3(p->q.threads()), st, in, out, (int)S,
                          (long long)n_slot, vec, (const cf*)p->resp, (const cf*)p->qw, (const cf*)p->qwr))
                return 1;
        } else {
            const size_t lds = (size_t)M * sizeof(f4);
            if (ensure_dyn_lds((const void*)k_r2c_gen, lds)) return 1;
            hipLaunchKernelGGL(k_r2c_gen, dim3((unsigned)n_group), dim3(gen_threads((int)M)), lds, st, in, out,
                               (int)S, (long long)n_slot, vec, (const cf*)p->resp, p->g, p->wn, p->gr, p->wnr);
            HIP_TRY(hipGetLastError());
        }
    } else {
        const int64_t need = std::min<int64_t>(p->cap, n_group);
        if (need > p->alloc) {
            // (a previous call may still use the smaller buffers: hipFree waits for the device)
            if (p->work_in) HIP_TRY(hipFree(p->work_in));
            if (p->work_out) HIP_TRY(hipFree(p->work_out));
            p->work_in = p->work_out = nullptr;
            p->alloc = 0;
            HIP_TRY(hipMalloc((void**)&p->work_in, (size_t)(need * M * 16)));
            HIP_TRY(hipMalloc((void**)&p->work_out, (size_t)(need * M * 16)));
            p->alloc = need;
        }
        for (int64_t g0 = 0; g0 < n_group; g0 += p->alloc) {
            const int64_t ng = std::min<int64_t>(p->alloc, n_group - g0);
            const long long total = M * 4 * ng;
            const dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 1 << 16));
            hipLaunchKernelGGL(k_r2c_gather, grid, dim3(256), 0, st, in, p->work_in, M, (int)S,
                               (long long)n_slot, (long long)g0, (long long)ng);
            HIP_TRY(hipGetLastError());
            if (bbt_osm_execute_regular(p->osm, p->work_in, p->work_out, ng, 0, 0, M, 0, stream)) return 1;
            hipLaunchKernelGGL(k_r2c_combine, grid, dim3(256), 0, st, in, (const float*)p->work_out, out,
                               M, (int)S, (long long)n_slot, (long long)g0, (long long)ng);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(p->ev_done, st));
    p->ev_done_set = true;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// shaping and combining: index maps (gather_kernels.hpp)
struct bbt_gather_plan {
    int device = 0;
    int n_src = 0, eb = 0, route = 0;
    int64_t R = 0;                          // output row, elements
    std::vector<int64_t> src_row;           // source rows, elements
    std::vector<int> used;                  // used sources, ascending (kernel slot u -> source)
    int64_t n_runs = 0;
    // element map (direct route, and the fall-back of the other two): (slot, byte offset)
    int2* tab_elem = nullptr;
    long long* stride_dev = nullptr;        // source rows in bytes, per slot
    // run copy: the same per 16-byte unit
    int2* tab16 = nullptr;
    // tile
    int T = 0, lds_bytes = 0;
    std::vector<GatherTileSrc> tile_src;    // per slot
    std::vector<int> tile_lo;               // start of the staged stretch in the source row, bytes
    std::vector<char> tile_vec;             // stretch is whole 16-byte pieces
    GatherTileSrc* tile_src_dev = nullptr;
    int2* tab_tile = nullptr;
    // host copies, uploaded by the first execute call (a plan can be made, and its route asked for,
    // without a device)
    std::mutex mu;
    bool uploaded = false;
    std::vector<long long> h_stride;
    std::vector<int2> h_elem, h_16, h_tile;
};

static int gather_upload_all(bbt_gather_plan* p);

static void gather_release(bbt_gather_plan* p) {
    if (!p) return;
    int cur = 0;
    const bool switched = hipGetDevice(&cur) == hipSuccess && cur != p->device && hipSetDevice(p->device) == hipSuccess;
    if (p->tab_elem) (void)hipFree(p->tab_elem);
    if (p->stride_dev) (void)hipFree(p->stride_dev);
    if (p->tab16) (void)hipFree(p->tab16);
    if (p->tile_src_dev) (void)hipFree(p->tile_src_dev);
    if (p->tab_tile) (void)hipFree(p->tab_tile);
    if (switched) (void)hipSetDevice(cur);
    delete p;
}

template <typename V> static int gather_upload(V** dst, const std::vector<V>& h) {
    HIP_TRY(hipMalloc((void**)dst, std::max<size_t>(h.size(), 1) * sizeof(V)));
    if (!h.empty()) HIP_TRY(hipMemcpy(*dst, h.data(), h.size() * sizeof(V), hipMemcpyHostToDevice));
    return 0;
}

// LDS layout of a tile of T samples (gather_kernels.hpp); returns the bytes it takes
static int gather_tile_layout(int eb, int T, const std::vector<int>& len, std::vector<GatherTileSrc>* out) {
    const int G = eb < 4 ? 4 : eb, rowsh = eb >= 8 ? 8 : 7, bank_row = 1 << rowsh;
    int np = 1;
    while (np < (int)len.size() && np < bank_row / G) np *= 2;
    int64_t end = 0;
    for (size_t u = 0; u < len.size(); ++u) {
        GatherTileSrc s = {};
        s.len = len[u];
        const int padded = len[u] + (len[u] >> rowsh) * G;
        s.pitch = (padded + G - 1) / G * G;
        const int64_t base = (end + bank_row - 1) / bank_row * bank_row + (int64_t)(u % np) * (bank_row / np);
        end = base + (int64_t)T * s.pitch;
        if (end > (1 << 30)) return 1 << 30;
        s.lds_base = (int)base;
        if (out) out->push_back(s);
    }
    return (int)end;
}

extern "C" {

int bbt_gather_plan_create(bbt_gather_plan** plan, int n_src, const int64_t* src_row_elems, int64_t out_row_elems,
                           const int32_t* map_src, const int64_t* map_elem, int elem_bytes) {
    return bbt_gather_plan_create_ex(plan, n_src, src_row_elems, out_row_elems, map_src, map_elem, elem_bytes,
                                     BBT_GATHER_AUTO);
}

int bbt_gather_plan_create_ex(bbt_gather_plan** plan, int n_src, const int64_t* src_row_elems, int64_t out_row_elems,
                              const int32_t* map_src, const int64_t* map_elem, int elem_bytes, int route) {
    ARG_TRY(plan, "bbt_gather_plan_create: null plan");
    *plan = nullptr;
    ARG_TRY(src_row_elems && map_src && map_elem, "bbt_gather_plan_create: null argument");
    ARG_TRY(n_src >= 1 && n_src <= BBT_GATHER_MAX_SRC, "bbt_gather_plan_create: n_src=%d must be 1 to %d", n_src,
            BBT_GATHER_MAX_SRC);
    ARG_TRY(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8 || elem_bytes == 16,
            "bbt_gather_plan_create: elem_bytes=%d must be 1, 2, 4, 8 or 16", elem_bytes);
    ARG_TRY(route >= BBT_GATHER_AUTO && route <= BBT_GATHER_DIRECT, "bbt_gather_plan_create: unknown route %d", route);
    const int eb = elem_bytes;
    const int64_t R = out_row_elems;
    ARG_TRY(R >= 1 && R * eb < (int64_t(1) << 31), "bbt_gather_plan_create: out_row_elems=%lld must be at least 1 "
            "and the row below 2 GiB", (long long)R);
    for (int s = 0; s < n_src; ++s)
        ARG_TRY(src_row_elems[s] >= 1 && src_row_elems[s] * eb < (int64_t(1) << 31),
                "bbt_gather_plan_create: src_row_elems[%d]=%lld must be at least 1 and the row below 2 GiB", s,
                (long long)src_row_elems[s]);
    std::vector<int> slot((size_t)n_src, -1);
    for (int64_t j = 0; j < R; ++j) {
        ARG_TRY(map_src[j] >= 0 && map_src[j] < n_src, "bbt_gather_plan_create: map_src[%lld]=%d out of range (%d sources)",
                (long long)j, (int)map_src[j], n_src);
        ARG_TRY(map_elem[j] >= 0 && map_elem[j] < src_row_elems[map_src[j]],
                "bbt_gather_plan_create: map_elem[%lld]=%lld out of range (source %d has rows of %lld)", (long long)j,
                (long long)map_elem[j], (int)map_src[j], (long long)src_row_elems[map_src[j]]);
        slot[(size_t)map_src[j]] = 0;
    }
    bbt_gather_plan* p = new bbt_gather_plan;
    auto bail = [&](int rc) { gather_release(p); return rc; };
    p->n_src = n_src;
    p->eb = eb;
    p->R = R;
    p->src_row.assign(src_row_elems, src_row_elems + n_src);
    for (int s = 0; s < n_src; ++s)
        if (slot[(size_t)s] == 0) {
            slot[(size_t)s] = (int)p->used.size();
            p->used.push_back(s);
        }
    const size_t nu = p->used.size();
    // runs: maximal stretches where source and element advance together
    struct Run { int64_t out, elem, len; int u; };
    std::vector<Run> runs;
    std::vector<int64_t> lo(nu, INT64_MAX), hi(nu, 0);
    for (int64_t j = 0; j < R; ++j) {
        const int u = slot[(size_t)map_src[j]];
        if (!runs.empty() && runs.back().u == u && runs.back().elem + runs.back().len == map_elem[j]) ++runs.back().len;
        else runs.push_back({j, map_elem[j], 1, u});
        lo[(size_t)u] = std::min(lo[(size_t)u], map_elem[j]);
        hi[(size_t)u] = std::max(hi[(size_t)u], map_elem[j] + 1);
    }
    p->n_runs = (int64_t)runs.size();
    bool run_ok = (R * eb) % 16 == 0;
    for (size_t u = 0; u < nu && run_ok; ++u) run_ok = (p->src_row[(size_t)p->used[u]] * eb) % 16 == 0;
    for (size_t r = 0; r < runs.size() && run_ok; ++r)
        run_ok = (runs[r].out * eb) % 16 == 0 && (runs[r].elem * eb) % 16 == 0 && (runs[r].len * eb) % 16 == 0;
    // tile: the stretch of each source row the map uses, widened to whole 16-byte pieces where the row allows
    std::vector<int> len(nu);
    int64_t staged = 0;
    p->tile_lo.resize(nu);
    p->tile_vec.resize(nu);
    for (size_t u = 0; u < nu; ++u) {
        int64_t b0 = lo[u] * eb, b1 = hi[u] * eb;
        const bool vec = (p->src_row[(size_t)p->used[u]] * eb) % 16 == 0;
        if (vec) {
            b0 = b0 / 16 * 16;
            b1 = (b1 + 15) / 16 * 16;
        }
        p->tile_lo[u] = (int)b0;
        p->tile_vec[u] = vec ? 1 : 0;
        len[u] = (int)(b1 - b0);
        staged += b1 - b0;
    }
    // T: a multiple of the fewest samples whose output is whole 16-byte chunks (m), as many as fit
    // half the budget if those are eight at least (more workgroups per CU), else the whole budget
    int m = 1;
    while ((m * R * eb) % 16) m *= 2;
    int T = 0;
    for (int budget = BBT_GATHER_LDS_BYTES / 2; budget <= BBT_GATHER_LDS_BYTES && !T; budget *= 2)
        for (int t = 512 / m * m; t >= m; t -= m)
            if (gather_tile_layout(eb, t, len, nullptr) <= budget) {
                if (t >= 8 || budget == BBT_GATHER_LDS_BYTES) T = t;
                break;
            }
    const bool tile_ok = T >= 1;
    if (route == BBT_GATHER_RUN_COPY && !run_ok)
        return bail(fail("bbt_gather_plan_create: the run-copy route needs runs, rows and offsets of whole 16-byte units"));
    if (route == BBT_GATHER_TILE && !tile_ok)
        return bail(fail("bbt_gather_plan_create: the rows used (%lld bytes per sample) leave no tile in %d "
                         "bytes of LDS", (long long)staged, BBT_GATHER_LDS_BYTES));
    if (route == BBT_GATHER_AUTO)
        // (a tile stages whole stretches: not worth it where the map uses less than a quarter of them)
        route = run_ok ? BBT_GATHER_RUN_COPY : (tile_ok && staged <= 4 * R * eb) ? BBT_GATHER_TILE : BBT_GATHER_DIRECT;
    p->route = route;
    std::vector<long long> stride(nu);
    for (size_t u = 0; u < nu; ++u) stride[u] = (long long)(p->src_row[(size_t)p->used[u]] * eb);
    std::vector<int2> te((size_t)R);
    for (int64_t j = 0; j < R; ++j) te[(size_t)j] = make_int2(slot[(size_t)map_src[j]], (int)(map_elem[j] * eb));
    p->h_stride = stride;
    p->h_elem = te;
    if (route == BBT_GATHER_RUN_COPY) {
        std::vector<int2> t16((size_t)(R * eb / 16));
        for (size_t q = 0; q < t16.size(); ++q) t16[q] = te[q * (size_t)(16 / eb)];
        p->h_16 = t16;
    } else if (route == BBT_GATHER_TILE) {
        p->T = T;
        p->lds_bytes = gather_tile_layout(eb, T, len, &p->tile_src);
        const int G = eb < 4 ? 4 : eb, rowsh = eb >= 8 ? 8 : 7;
        for (size_t u = 0; u < nu; ++u) p->tile_src[u].stride = stride[u];
        std::vector<int2> tt((size_t)R);
        for (int64_t j = 0; j < R; ++j) {
            const int u = te[(size_t)j].x, r = te[(size_t)j].y - p->tile_lo[(size_t)u];
            tt[(size_t)j] = make_int2(p->tile_src[(size_t)u].lds_base + r + (r >> rowsh) * G, p->tile_src[(size_t)u].pitch);
        }
        p->h_tile = tt;
    }
    *plan = p;
    return 0;
}

}  // extern "C"

static int gather_upload_all(bbt_gather_plan* p) {
    std::lock_guard<std::mutex> lock(p->mu);
    if (p->uploaded) return 0;
    HIP_TRY(hipGetDevice(&p->device));
    if (gather_upload(&p->stride_dev, p->h_stride) || gather_upload(&p->tab_elem, p->h_elem)) return 1;
    if (p->route == BBT_GATHER_RUN_COPY && gather_upload(&p->tab16, p->h_16)) return 1;
    if (p->route == BBT_GATHER_TILE &&
        (gather_upload(&p->tile_src_dev, p->tile_src) || gather_upload(&p->tab_tile, p->h_tile)))
        return 1;
    p->uploaded = true;
    return 0;
}

extern "C" {

int bbt_gather_plan_destroy(bbt_gather_plan* p) {
    gather_release(p);
    return 0;
}

int bbt_gather_plan_info(const bbt_gather_plan* p, int* route, int64_t* n_runs, int* tile_samples, int* lds_bytes) {
    ARG_TRY(p, "bbt_gather_plan_info: null plan");
    if (route) *route = p->route;
    if (n_runs) *n_runs = p->n_runs;
    if (tile_samples) *tile_samples = p->T;
    if (lds_bytes) *lds_bytes = p->lds_bytes;
    return 0;
}

int bbt_gather_execute(bbt_gather_plan* p, const void* const* src_dev, const int64_t* src_first_sample, void* out_dev,
                       int64_t n_samples, bbt_stream stream) {
    ARG_TRY(p && src_dev && out_dev, "bbt_gather_execute: null argument");
    ARG_TRY(n_samples >= 0, "bbt_gather_execute: n_samples=%lld", (long long)n_samples);
    if (n_samples == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int eb = p->eb;
    const size_t nu = p->used.size();
    const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(n_samples * p->R * eb);
    ARG_TRY(o0 % (uintptr_t)eb == 0, "bbt_gather_execute: out_dev is not aligned to the element size %d", eb);
    GatherPtrs ptrs = {};
    bool al16 = o0 % 16 == 0;
    for (size_t u = 0; u < nu; ++u) {
        const int s = p->used[u];
        ARG_TRY(src_dev[s], "bbt_gather_execute: null source %d", s);
        const int64_t first = src_first_sample ? src_first_sample[s] : 0;
        ARG_TRY(first >= 0, "bbt_gather_execute: src_first_sample[%d]=%lld is negative", s, (long long)first);
        const int64_t row = p->src_row[(size_t)s] * eb;
        const uintptr_t i0 = (uintptr_t)src_dev[s] + (uintptr_t)(first * row), i1 = i0 + (uintptr_t)(n_samples * row);
        ARG_TRY(i0 % (uintptr_t)eb == 0, "bbt_gather_execute: source %d is not aligned to the element size %d", s, eb);
        ARG_TRY(i1 <= o0 || o1 <= i0, "bbt_gather_execute: out_dev overlaps source %d", s);
        ptrs.p[u] = (const char*)i0;
        al16 = al16 && i0 % 16 == 0;
    }
    if (gather_upload_all(p)) return 1;
    const long long total_rows = n_samples;
    auto grid_for = [](long long units) {
        return dim3((unsigned)std::max<long long>(1, std::min<long long>((units + BBT_GATHER_THREADS - 1) / BBT_GATHER_THREADS, 8192)));
    };
#define BBT_GATHER_MAP(E, TAB, ROW)                                                                              \
    hipLaunchKernelGGL((k_gather_map<E>), grid_for(total_rows * (long long)(ROW)), dim3(BBT_GATHER_THREADS), 0, st, \
                       ptrs, (const long long*)p->stride_dev, (int)nu, (const int2*)(TAB), (int)(ROW), (E*)out_dev, \
                       total_rows)
    if (p->route == BBT_GATHER_RUN_COPY && al16) {
        BBT_GATHER_MAP(GatherB16, p->tab16, p->R * eb / 16);
    } else if (p->route == BBT_GATHER_TILE) {
        unsigned long long vec_mask = 0;
        for (size_t u = 0; u < nu; ++u) {
            ptrs.p[u] += p->tile_lo[u];
            if (p->tile_vec[u] && (uintptr_t)ptrs.p[u] % 16 == 0) vec_mask |= 1ull << u;
        }
        const long long n_tiles = (n_samples + p->T - 1) / p->T;
        const dim3 grid((unsigned)std::min<long long>(n_tiles, 1 << 16));
        const int vec_out = (o0 % 16 == 0 && ((long long)p->T * p->R * eb) % 16 == 0) ? 1 : 0;
#define BBT_GATHER_TILE_K(E)                                                                                       \
    hipLaunchKernelGGL((k_gather_tile<E>), grid, dim3(BBT_GATHER_THREADS), (size_t)p->lds_bytes, st, ptrs, vec_mask, \
                       (const GatherTileSrc*)p->tile_src_dev, (int)nu, (const int2*)p->tab_tile, (int)p->R,         \
                       (E*)out_dev, total_rows, p->T, vec_out)
        switch (eb) {
            case 1: BBT_GATHER_TILE_K(unsigned char); break;
            case 2: BBT_GATHER_TILE_K(unsigned short); break;
            case 4: BBT_GATHER_TILE_K(unsigned); break;
            case 8: BBT_GATHER_TILE_K(GatherB8); break;
            default: BBT_GATHER_TILE_K(GatherB16); break;
        }
#undef BBT_GATHER_TILE_K
    } else {
        switch (eb) {
            case 1: BBT_GATHER_MAP(unsigned char, p->tab_elem, p->R); break;
            case 2: BBT_GATHER_MAP(unsigned short, p->tab_elem, p->R); break;
            case 4: BBT_GATHER_MAP(unsigned, p->tab_elem, p->R); break;
            case 8: BBT_GATHER_MAP(GatherB8, p->tab_elem, p->R); break;
            default: BBT_GATHER_MAP(GatherB16, p->tab_elem, p->R); break;
        }
    }
#undef BBT_GATHER_MAP
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// integer sample shifts
struct bbt_shift_plan {
    int n_elem = 0, elem_bytes = 0;      // as given
    int* offset = nullptr;
    // neighbours with equal offsets merged into one wider element (used when the
    // buffers of a call are aligned to it)
    int merged_n_elem = 0, merged_bytes = 0;
    int* merged_offset = nullptr;
    // tiled form (k_shift_tiled): per group of merged elements that fill a cache line, the
    // smallest offset and the span of the offsets; 0 groups: gather only
    int n_group = 0, window = 0;
    int* group_lo = nullptr;
    int* group_span = nullptr;
};

extern "C" int bbt_shift_plan_destroy(bbt_shift_plan* p);
extern "C" int bbt_shift_plan_create(bbt_shift_plan** plan, int n_elem, int elem_bytes,
                                     const int32_t* offsets_host) {
    ARG_TRY(plan && offsets_host, "bbt_shift_plan_create: null argument");
    *plan = nullptr;
    ARG_TRY(n_elem >= 1, "bbt_shift_plan_create: n_elem=%d must be >= 1", n_elem);
    ARG_TRY(elem_bytes == 4 || elem_bytes == 8, "bbt_shift_plan_create: elem_bytes must be 4 or 8");
    for (int e = 0; e < n_elem; ++e)
        ARG_TRY(offsets_host[e] >= 0, "bbt_shift_plan_create: offset[%d]=%d is negative", e,
                offsets_host[e]);
    // merge aligned groups of 2 (4) neighbouring elements that move together, up to 16 bytes
    int m = 1;
    while (m * 2 * elem_bytes <= 16 && n_elem % (m * 2) == 0) {
        bool same = true;
        for (int e = 0; e < n_elem && same; e += m * 2)
            for (int k = 1; k < m * 2 && same; ++k) same = offsets_host[e + k] == offsets_host[e];
        if (!same) break;
        m *= 2;
    }
    std::vector<int> merged(n_elem / m);
    for (int e = 0; e < n_elem / m; ++e) merged[e] = offsets_host[e * m];
    bbt_shift_plan* p = new bbt_shift_plan;
    p->n_elem = n_elem;
    p->elem_bytes = elem_bytes;
    p->merged_n_elem = n_elem / m;
    p->merged_bytes = elem_bytes * m;
    if (hipMalloc((void**)&p->offset, (n_elem + merged.size()) * sizeof(int)) != hipSuccess ||
        hipMemcpy(p->offset, offsets_host, n_elem * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->offset + n_elem, merged.data(), merged.size() * sizeof(int),
                  hipMemcpyHostToDevice) != hipSuccess) {
        fail("bbt_shift_plan_create: uploading the offsets failed");
        if (p->offset) hipFree(p->offset);
        delete p;
        return 1;
    }
    p->merged_offset = p->offset + n_elem;
    // groups of merged elements that fill a 128-byte line: the tiled kernel stages their input
    // lines in LDS.  Window: 1024 rows (128 KiB, one workgroup per CU) when some group's offsets
    // span more than 128 rows, else 512 (two per CU); half of it is output rows.
    const int g_elems = 128 / p->merged_bytes;
    if (p->merged_bytes >= 8 && p->merged_n_elem % g_elems == 0) {
        const int ng = p->merged_n_elem / g_elems;
        std::vector<int> lo(ng), span(ng);
        int tiled = 0, widest = 0;
        for (int g = 0; g < ng; ++g) {
            int a = merged[g * g_elems], b = a;
            for (int k = 1; k < g_elems; ++k) {
                a = std::min(a, merged[g * g_elems + k]);
                b = std::max(b, merged[g * g_elems + k]);
            }
            lo[g] = a;
            span[g] = b - a;
            if (span[g] <= 512) {
                ++tiled;
                widest = std::max(widest, span[g]);
            }
        }
        if (2 * tiled >= ng) {                 // (mostly scattered offsets: the gather kernel as before)
            if (hipMalloc((void**)&p->group_lo, 2 * ng * sizeof(int)) != hipSuccess ||
                hipMemcpy(p->group_lo, lo.data(), ng * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(p->group_lo + ng, span.data(), ng * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
                fail("bbt_shift_plan_create: uploading the group table failed");
                bbt_shift_plan_destroy(p);
                return 1;
            }
            p->group_span = p->group_lo + ng;
            p->n_group = ng;
            p->window = widest > 128 ? 1024 : 512;
        }
    }
    *plan = p;
    return 0;
}

extern "C" int bbt_shift_plan_destroy(bbt_shift_plan* p) {
    if (!p) return 0;
    if (p->offset) hipFree(p->offset);
    if (p->group_lo) hipFree(p->group_lo);
    delete p;
    return 0;
}

extern "C" int bbt_shift_execute(bbt_shift_plan* p, const void* in_dev, void* out_dev,
                                 int64_t n_out, bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_shift_execute: null argument");
    ARG_TRY(n_out >= 0, "bbt_shift_execute: n_out < 0");
    if (n_out == 0) return 0;
#ifndef BBT_SHIFT_ITER
#define BBT_SHIFT_ITER 2     // rows per thread: 1 2.83, 2 3.17, 4 3.02, 8 2.95, 16 2.29 TB/s (128 x 8-byte elements, offsets over 1000 rows)
#endif
    constexpr int ITER = BBT_SHIFT_ITER;
    const bool wide = (((uintptr_t)in_dev | (uintptr_t)out_dev) % (uintptr_t)p->merged_bytes) == 0;
    const int n_elem = wide ? p->merged_n_elem : p->n_elem;
    const int bytes = wide ? p->merged_bytes : p->elem_bytes;
    const int* offset = wide ? p->merged_offset : p->offset;
    int lg_le = 0;
    while ((1 << lg_le) < n_elem && lg_le < 8) ++lg_le;
    const long long rows_per_block = (256 >> lg_le) * ITER;
    const long long gx = (n_out + rows_per_block - 1) / rows_per_block;
    const long long gy = ((long long)n_elem + (1 << lg_le) - 1) >> lg_le;
    ARG_TRY(gx < (1ll << 31) && gy <= 65535, "bbt_shift_execute: too many elements for one call");
    const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (wide && p->n_group) {
        const int rows = p->window / 2;
        const long long tx = (n_out + rows - 1) / rows;
        ARG_TRY(tx < (1ll << 31) && p->n_group <= 65535, "bbt_shift_execute: too many elements for one call");
        const dim3 tgrid((unsigned)tx, (unsigned)p->n_group);
        const size_t lds = (size_t)p->window * 128;
        if (bytes == 16) {
            if (ensure_dyn_lds((const void*)k_shift_tiled<float4>, lds)) return 1;
            hipLaunchKernelGGL((k_shift_tiled<float4>), tgrid, block, lds, st, (const float4*)in_dev, (float4*)out_dev,
                               (long long)n_out, n_elem, offset, p->group_lo, p->group_span, p->window);
        } else {
            if (ensure_dyn_lds((const void*)k_shift_tiled<float2>, lds)) return 1;
            hipLaunchKernelGGL((k_shift_tiled<float2>), tgrid, block, lds, st, (const float2*)in_dev, (float2*)out_dev,
                               (long long)n_out, n_elem, offset, p->group_lo, p->group_span, p->window);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (bytes == 16)
        hipLaunchKernelGGL((k_shift_samples<float4, ITER>), grid, block, 0, st, (const float4*)in_dev,
                           (float4*)out_dev, (long long)n_out, n_elem, lg_le, offset);
    else if (bytes == 8)
        hipLaunchKernelGGL((k_shift_samples<float2, ITER>), grid, block, 0, st, (const float2*)in_dev,
                           (float2*)out_dev, (long long)n_out, n_elem, lg_le, offset);
    else
        hipLaunchKernelGGL((k_shift_samples<float, ITER>), grid, block, 0, st, (const float*)in_dev,
                           (float*)out_dev, (long long)n_out, n_elem, lg_le, offset);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// what the sections of the search chain share (dmt, sps, ffa, hsum, lspec, accel, rank, rmed, corr)

// A tiling or routing knob from the environment: the value of `name` if it is one of `allowed`, else 0,
// which stands for the section's default.  The contract of every knob below: it is read at every call,
// for measuring and for the tests that walk the tilings and routes; no value of the output depends on
// it; anything else leaves the default.
static int env_knob(const char* name, std::initializer_list<int> allowed) {
    const char* e = getenv(name);
    if (e && *e) {
        const int v = atoi(e);
        for (int a : allowed)
            if (v == a) return v;
    }
    return 0;
}

// The scratch a plan owns, grown on demand and never shrunk.  One plan serves one stream at a time:
// the scratch is the plan's.
struct PlanScratch {
    void* ptr = nullptr;
    size_t bytes = 0;
    int reserve(size_t need) {
        if (need <= bytes) return 0;
        if (ptr) HIP_TRY(hipFree(ptr));          // (waits for the launches that use it)
        ptr = nullptr, bytes = 0;
        HIP_TRY(hipMalloc(&ptr, need));
        bytes = need;
        return 0;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr, bytes = 0;
    }
};

// ---------------------------------------------------------------------------
// incoherent dedispersion over many trial DMs (dmt_kernels.hpp; the tiling is dmt_geo.hpp's)
struct bbt_dmt_plan {
    int ndm = 0, nchan = 0, n_rest = 0, ndm_pad = 0, span = 0;
    int* tab = nullptr;              // [nchan][ndm_pad], padding entries 0
    PlanScratch scratch;             // the transposed chunk
};

// BBT_DMT_TILE: output times of a workgroup (64, 128, 256); BBT_DMT_TRIALS: trials a thread holds
// (1, 2, 4, 8, 16).
static int dmt_env_tile() { return env_knob("BBT_DMT_TILE", {64, 128, 256}); }
static int dmt_env_trials() { return env_knob("BBT_DMT_TRIALS", {1, 2, 4, 8, 16}); }

extern "C" int bbt_dmt_plan_destroy(bbt_dmt_plan* p) {
    if (!p) return 0;
    if (p->tab) hipFree(p->tab);
    p->scratch.release();
    delete p;
    return 0;
}

extern "C" int bbt_dmt_plan_create(bbt_dmt_plan** plan, const int32_t* offsets_host, int64_t ndm, int64_t nchan,
                                   int64_t n_rest) {
    ARG_TRY(plan && offsets_host, "bbt_dmt_plan_create: null argument");
    *plan = nullptr;
    const char* err = dmt_sizes(ndm, nchan, n_rest);
    ARG_TRY(!err, "bbt_dmt_plan_create: %s", err ? err : "");
    long long span = 0;
    for (long long i = 0; i < (long long)ndm * nchan; ++i) span = std::max<long long>(span, offsets_host[i]);
    err = dmt_check_table(offsets_host, (long long)ndm * nchan, span);
    ARG_TRY(!err, "bbt_dmt_plan_create: %s", err ? err : "");
    bbt_dmt_plan* p = new bbt_dmt_plan;
    p->ndm = (int)ndm, p->nchan = (int)nchan, p->n_rest = (int)n_rest, p->span = (int)span;
    p->ndm_pad = dmt_pad_ndm((int)ndm);
    std::vector<int> tab((size_t)nchan * p->ndm_pad, 0);
    for (long long d = 0; d < ndm; ++d)
        for (long long c = 0; c < nchan; ++c) tab[(size_t)c * p->ndm_pad + d] = offsets_host[d * nchan + c];
    if (hipMalloc((void**)&p->tab, tab.size() * sizeof(int)) != hipSuccess ||
        hipMemcpy(p->tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        fail("bbt_dmt_plan_create: uploading the table failed");
        bbt_dmt_plan_destroy(p);
        return 1;
    }
    *plan = p;
    return 0;
}

extern "C" int bbt_dmt_plan_info(const bbt_dmt_plan* p, int64_t* span, int* tile_t, int* trials,
                                 int64_t* scratch_bytes) {
    ARG_TRY(p, "bbt_dmt_plan_info: null argument");
    const int t = dmt_env_tile(), b = dmt_env_trials();
    if (span) *span = p->span;
    if (tile_t) *tile_t = t ? t : BBT_DMT_TILE;
    if (trials) *trials = b ? b : BBT_DMT_DB;
    if (scratch_bytes) *scratch_bytes = (int64_t)p->scratch.bytes;
    return 0;
}

// out[i][d][r], i < n_out, from in[t][c][r], t < n_in.  One plan serves one stream at a time: the
// scratch is the plan's.
extern "C" int bbt_dmt_execute(bbt_dmt_plan* p, const float* in_dev, int64_t n_in, float* out_dev, int64_t n_out,
                               bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_dmt_execute: null argument");
    ARG_TRY(aligned4(in_dev, out_dev), "bbt_dmt_execute: arrays must be 4-byte aligned");
    DmtGeo g = {};
    const char* err = dmt_geo(n_in, n_out, p->nchan, p->n_rest, p->ndm, p->span, dmt_env_tile(), dmt_env_trials(), &g);
    ARG_TRY(!err, "bbt_dmt_execute: %s (n_in=%lld, n_out=%lld, span=%d)", err ? err : "", (long long)n_in,
            (long long)n_out, p->span);
    if (p->scratch.reserve((size_t)g.scratch * sizeof(float))) return 1;
    float* scratch = (float*)p->scratch.ptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dmt_transpose, dim3((unsigned)g.tr_t, (unsigned)g.tr_e), dim3(BBT_DMT_THREADS), 0, st, in_dev,
                       scratch, (long long)n_in, p->nchan * p->n_rest, g.pitch);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)g.n_wg), block(BBT_DMT_THREADS);
    switch (g.db) {
        case 1: hipLaunchKernelGGL((k_dmt_sweep<1>), grid, block, 0, st, scratch, p->tab, out_dev, g); break;
        case 2: hipLaunchKernelGGL((k_dmt_sweep<2>), grid, block, 0, st, scratch, p->tab, out_dev, g); break;
        case 4: hipLaunchKernelGGL((k_dmt_sweep<4>), grid, block, 0, st, scratch, p->tab, out_dev, g); break;
        case 8: hipLaunchKernelGGL((k_dmt_sweep<8>), grid, block, 0, st, scratch, p->tab, out_dev, g); break;
        default: hipLaunchKernelGGL((k_dmt_sweep<16>), grid, block, 0, st, scratch, p->tab, out_dev, g); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// single-pulse search on the (time, DM) plane (sps_kernels.hpp; the tiling is sps_geo.hpp's)
struct bbt_sps_plan {
    long long n = 0, n_elem = 0;
    int K = 0;
    PlanScratch scratch;             // the partial sums between passes
};

// BBT_SPS_WIDTH: elements of a boxcar workgroup (16, 32, 64); BBT_SPS_FUSE: levels per pass (1, 2, 3);
// BBT_SPS_SPLIT: threads that share a (block, element) at most (1, 2, 4, 8, 16); BBT_SPS_STD_ROWS: threads
// along the segments in Standardize (1, 2, 4, 8, 16).
static int sps_env_width() { return env_knob("BBT_SPS_WIDTH", {16, 32, 64}); }
static int sps_env_fuse() { return env_knob("BBT_SPS_FUSE", {1, 2, 3}); }
static int sps_env_split() { return env_knob("BBT_SPS_SPLIT", {1, 2, 4, 8, 16}); }
static int sps_env_rows() { return env_knob("BBT_SPS_STD_ROWS", {1, 2, 4, 8, 16}); }

// out[b * n + t][e] = (x[b * n + t][e] - mean) * (1 / sd) of block b < n_block, element e < n_elem
extern "C" int bbt_sps_standardize(const float* x_dev, float* out_dev, int64_t n_block, int64_t n, int64_t n_elem,
                                   bbt_stream stream) {
    ARG_TRY(x_dev && out_dev, "bbt_sps_standardize: null argument");
    ARG_TRY(aligned4(x_dev, out_dev), "bbt_sps_standardize: arrays must be 4-byte aligned");
    StdGeo g = {};
    const char* err = sps_std_geo(n_block, n, n_elem, sps_env_rows(), &g);
    ARG_TRY(!err, "bbt_sps_standardize: %s (n_block=%lld, n=%lld, n_elem=%lld)", err ? err : "", (long long)n_block,
            (long long)n, (long long)n_elem);
    hipLaunchKernelGGL(k_sps_standardize, dim3((unsigned)g.n_wg), dim3(BBT_SPS_THREADS), 0, (hipStream_t)stream, x_dev,
                       out_dev, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int bbt_sps_plan_destroy(bbt_sps_plan* p) {
    if (!p) return 0;
    p->scratch.release();
    delete p;
    return 0;
}

extern "C" int bbt_sps_plan_create(bbt_sps_plan** plan, int64_t n, int64_t n_widths, int64_t n_elem) {
    ARG_TRY(plan, "bbt_sps_plan_create: null argument");
    *plan = nullptr;
    const char* err = sps_sizes(n, n_widths, n_elem);
    ARG_TRY(!err, "bbt_sps_plan_create: %s", err ? err : "");
    bbt_sps_plan* p = new bbt_sps_plan;
    p->n = n, p->K = (int)n_widths, p->n_elem = n_elem;
    *plan = p;
    return 0;
}

// the tiling the next call will use and the bytes of scratch the plan holds (plan may be null: the
// tiling only); scales: 13 floats, c_k
extern "C" int bbt_sps_plan_info(const bbt_sps_plan* p, int* width, int* fuse, int* split, int* std_rows,
                                 int64_t* scratch_bytes, float* scales) {
    const int w = sps_env_width(), f = sps_env_fuse(), s = sps_env_split(), r = sps_env_rows();
    if (width) *width = w ? w : BBT_SPS_WIDTH;
    if (fuse) *fuse = f ? f : BBT_SPS_FUSE;
    if (split) *split = s ? s : BBT_SPS_SPLIT;
    if (std_rows) *std_rows = r ? r : BBT_SPS_STD_ROWS;
    if (scratch_bytes) *scratch_bytes = p ? (int64_t)p->scratch.bytes : 0;
    if (scales)
        for (int k = 0; k < BBT_SPS_MAX_WIDTHS; ++k) scales[k] = sps_scale(k);
    return 0;
}

template <int F>
static void sps_launch(const bbt_sps_plan* p, const SpsGeo& g, const float* in_dev, float* out_dev, hipStream_t st) {
    float* scratch = (float*)p->scratch.ptr;
    float* buf[2] = {scratch, scratch + (g.n_pass > 2 ? g.n_in * g.n_elem : 0)};
    const float* src = in_dev;
    for (int q = 0; q < g.n_pass; ++q) {
        const SpsPass ps = sps_pass(g, q);
        float* dst = ps.store ? buf[q & 1] : nullptr;
        const float c0 = g.c[ps.k0], c1 = ps.levels > 1 ? g.c[ps.k0 + 1] : 0.f, c2 = ps.levels > 2 ? g.c[ps.k0 + 2] : 0.f;
        hipLaunchKernelGGL((k_sps_pass<F>), dim3((unsigned)ps.n_wg), dim3(BBT_SPS_THREADS), 0, st, src, dst, out_dev, g,
                           ps.k0, ps.blocks, (int)ps.store, (int)(q == 0), (int)(q == g.n_pass - 1), c0, c1, c2);
        src = dst;
    }
}

// best[b][3][e], b < n_blocks, from in[t][e], t < n_in, n_in >= n_blocks * n: windows may run on into
// in[n_blocks * n ...] as far as n_in goes.  One plan serves one stream at a time: the scratch is the plan's.
extern "C" int bbt_sps_execute(bbt_sps_plan* p, const float* in_dev, int64_t n_in, float* out_dev, int64_t n_blocks,
                               bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_sps_execute: null argument");
    ARG_TRY(aligned4(in_dev, out_dev), "bbt_sps_execute: arrays must be 4-byte aligned");
    SpsGeo g = {};
    const char* err = sps_geo(n_in, n_blocks, p->n, p->K, p->n_elem, sps_env_width(), sps_env_fuse(), sps_env_split(), &g);
    ARG_TRY(!err, "bbt_sps_execute: %s (n_in=%lld, n_blocks=%lld, n=%lld)", err ? err : "", (long long)n_in,
            (long long)n_blocks, p->n);
    if (p->scratch.reserve((size_t)g.scratch * sizeof(float))) return 1;
    hipStream_t st = (hipStream_t)stream;
    switch (g.fuse) {
        case 1: sps_launch<1>(p, g, in_dev, out_dev, st); break;
        case 2: sps_launch<2>(p, g, in_dev, out_dev, st); break;
        default: sps_launch<3>(p, g, in_dev, out_dev, st); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// fast-folding period search on the (time, DM) plane (ffa_kernels.hpp; the tiling is ffa_geo.hpp's)
struct bbt_ffa_plan {
    long long n = 0, p_lo = 0, p_hi = 0, n_elem = 0, max_mp = 0;
    int K = 0;
    PlanScratch scratch;             // the running segment sums, the c_k, the two buffers of the passes
};

// BBT_FFA_FUSE: stages per pass (1, 2, 3); BBT_FFA_WIDTH: columns of an S/N workgroup at most (4, 8, 16,
// 32).
static int ffa_env_fuse() { return env_knob("BBT_FFA_FUSE", {1, 2, 3}); }
static int ffa_env_width() { return env_knob("BBT_FFA_WIDTH", {4, 8, 16, 32}); }

extern "C" int bbt_ffa_plan_destroy(bbt_ffa_plan* p) {
    if (!p) return 0;
    p->scratch.release();
    delete p;
    return 0;
}

extern "C" int bbt_ffa_plan_create(bbt_ffa_plan** plan, int64_t n, int64_t p_lo, int64_t p_hi, int64_t n_widths,
                                   int64_t n_elem) {
    ARG_TRY(plan, "bbt_ffa_plan_create: null argument");
    *plan = nullptr;
    const char* err = ffa_sizes(n, p_lo, p_hi, n_widths, n_elem);
    ARG_TRY(!err, "bbt_ffa_plan_create: %s", err ? err : "");
    bbt_ffa_plan* p = new bbt_ffa_plan;
    p->n = n, p->p_lo = p_lo, p->p_hi = p_hi, p->K = (int)n_widths, p->n_elem = n_elem;
    p->max_mp = ffa_max_mp(n, p_lo, p_hi);
    *plan = p;
    return 0;
}

// the tiling the next call will use, the bytes of scratch the plan holds and the floats of scratch it needs
// per column; for a base period `period` of the plan (else 0) its rows of data, rows and the 10 scales a_k
extern "C" int bbt_ffa_plan_info(const bbt_ffa_plan* p, int64_t period, int* fuse, int* width, int64_t* rows,
                                 int64_t* padded_rows, int64_t* scratch_bytes, int64_t* column_floats, float* scales) {
    const int f = ffa_env_fuse(), w = ffa_env_width();
    if (fuse) *fuse = f ? f : BBT_FFA_FUSE;
    if (width) *width = w ? w : BBT_FFA_WIDTH;
    if (scratch_bytes) *scratch_bytes = p ? (int64_t)p->scratch.bytes : 0;
    if (column_floats) *column_floats = p ? ffa_scratch(p->n, p->max_mp, 1) : 0;
    if (rows) *rows = 0;
    if (padded_rows) *padded_rows = 0;
    if (p && period) {
        ARG_TRY(period >= p->p_lo && period < p->p_hi, "bbt_ffa_plan_info: the period is not one of the plan's");
        long long m, M;
        int L;
        ffa_rows(p->n, period, &m, &M, &L);
        if (rows) *rows = m;
        if (padded_rows) *padded_rows = M;
        if (scales)
            for (int k = 0; k < BBT_FFA_MAX_WIDTHS; ++k) scales[k] = k < p->K ? ffa_scale(period, m, k) : 0.f;
    }
    return 0;
}

static void ffa_launch_pass(const FfaGeo& g, const FfaPass& ps, const float* src, float* dst, int first, hipStream_t st) {
    const dim3 grid((unsigned)ps.n_wg), block(BBT_FFA_THREADS);
    switch (ps.lv) {
        case 1: hipLaunchKernelGGL((k_ffa_pass<1>), grid, block, 0, st, src, dst, g, ps.s0, first); break;
        case 2: hipLaunchKernelGGL((k_ffa_pass<2>), grid, block, 0, st, src, dst, g, ps.s0, first); break;
        default: hipLaunchKernelGGL((k_ffa_pass<3>), grid, block, 0, st, src, dst, g, ps.s0, first); break;
    }
}

// best[p - p_lo][4][e], pa <= p < pb, e0 <= e < e0 + ne, of out[p_hi - p_lo][4][n_elem], from the block
// in[i][e], i < n, e < n_elem; the other cells of out are not touched.  One plan serves one stream at a
// time: the scratch is the plan's.
extern "C" int bbt_ffa_execute(bbt_ffa_plan* p, const float* in_dev, float* out_dev, int64_t e0, int64_t ne, int64_t pa,
                               int64_t pb, bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_ffa_execute: null argument");
    ARG_TRY(aligned4(in_dev, out_dev), "bbt_ffa_execute: arrays must be 4-byte aligned");
    ARG_TRY(pa >= p->p_lo && pa < pb && pb <= p->p_hi, "bbt_ffa_execute: the periods %lld ... %lld are not the plan's",
            (long long)pa, (long long)pb);
    const int fuse = ffa_env_fuse(), width = ffa_env_width();
    FfaGeo g = {};
    for (long long q = pa; q < pb; ++q) {                       // (every refusal comes before any launch)
        const char* err = ffa_geo(p->n, q, p->K, p->n_elem, e0, ne, fuse, width, &g);
        ARG_TRY(!err, "bbt_ffa_execute: %s (p=%lld, e0=%lld, ne=%lld)", err ? err : "", q, (long long)e0, (long long)ne);
    }
    if (p->scratch.reserve((size_t)ffa_scratch(p->n, p->max_mp, ne) * sizeof(float))) return 1;
    hipStream_t st = (hipStream_t)stream;
    double* pre = (double*)p->scratch.ptr;                     // (hipMalloc aligns far beyond 8 bytes)
    float* c = (float*)p->scratch.ptr + 2 * ffa_prefix(p->n) * ne;
    float* buf[2] = {c + BBT_FFA_MAX_WIDTHS * ne, c + (BBT_FFA_MAX_WIDTHS + p->max_mp) * ne};
    const float* x = in_dev + e0;
    const dim3 block(BBT_FFA_THREADS);
    const unsigned per_column = (unsigned)((ne + BBT_FFA_THREADS - 1) / BBT_FFA_THREADS);
    const long long n_seg = p->n / BBT_FFA_SEG * ne;
    if (n_seg) hipLaunchKernelGGL(k_ffa_segments, dim3((unsigned)((n_seg + BBT_FFA_THREADS - 1) / BBT_FFA_THREADS)), block, 0, st, x, pre, g);
    hipLaunchKernelGGL(k_ffa_prefix, dim3(per_column), block, 0, st, pre, g);
    for (long long q = pa; q < pb; ++q) {
        ffa_geo(p->n, q, p->K, p->n_elem, e0, ne, fuse, width, &g);
        hipLaunchKernelGGL(k_ffa_total, dim3(per_column), block, 0, st, x, pre, c, g);
        const float* src = x;
        for (int i = 0; i < g.n_pass; ++i) {
            const FfaPass ps = ffa_pass(g, i);
            ffa_launch_pass(g, ps, src, buf[i & 1], (int)(i == 0), st);
            src = buf[i & 1];
        }
        float* part = buf[g.n_pass & 1];
        hipLaunchKernelGGL(k_ffa_snr, dim3((unsigned)(g.n_et * g.n_rg)), block, 0, st, src, c, part, g);
        hipLaunchKernelGGL(k_ffa_merge, dim3((unsigned)((ne + BBT_FFA_MERGE_NX - 1) / BBT_FFA_MERGE_NX)), block, 0, st, part,
                           out_dev + (q - p->p_lo) * 4 * p->n_elem + e0, p->n_elem, g);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// periodicity search on stacked fluctuation spectra (hsum_kernels.hpp; the tiling is hsum_geo.hpp's)
struct bbt_hsum_plan {
    long long nbin = 0, n = 0, lo = 0, n_elem = 0;
    int K = 0;
    float c[BBT_HSUM_MAX_LEVELS] = {};
};

// BBT_HSUM_WIDTH: elements of a search workgroup (16, 32, 64); BBT_HSUM_SPLIT: threads that share a
// (spectrum, block, element) at most (1, 2, 4, 8, 16); BBT_HSUM_ROWS: threads along the segments in Whiten
// (1, 2, 4, 8, 16).
static int hsum_env_width() { return env_knob("BBT_HSUM_WIDTH", {16, 32, 64}); }
static int hsum_env_split() { return env_knob("BBT_HSUM_SPLIT", {1, 2, 4, 8, 16}); }
static int hsum_env_rows() { return env_knob("BBT_HSUM_ROWS", {1, 2, 4, 8, 16}); }

// out[s][j][e] = x[s][j][e] * (1 / mean of the block of m bins that holds j), +0 for j < skip
extern "C" int bbt_hsum_whiten(const float* x_dev, float* out_dev, int64_t n_spec, int64_t nbin, int64_t n_elem,
                               int64_t m, int64_t skip, bbt_stream stream) {
    ARG_TRY(x_dev && out_dev, "bbt_hsum_whiten: null argument");
    ARG_TRY(aligned4(x_dev, out_dev), "bbt_hsum_whiten: arrays must be 4-byte aligned");
    WhitenGeo g = {};
    const char* err = hsum_whiten_geo(n_spec, nbin, n_elem, m, skip, hsum_env_rows(), &g);
    ARG_TRY(!err, "bbt_hsum_whiten: %s (n_spec=%lld, nbin=%lld, n_elem=%lld, m=%lld, skip=%lld)", err ? err : "",
            (long long)n_spec, (long long)nbin, (long long)n_elem, (long long)m, (long long)skip);
    hipLaunchKernelGGL(k_hsum_whiten, dim3((unsigned)g.n_wg), dim3(BBT_HSUM_THREADS), 0, (hipStream_t)stream, x_dev,
                       out_dev, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int bbt_hsum_plan_destroy(bbt_hsum_plan* p) {
    delete p;
    return 0;
}

// scales_host: n_levels floats, c_L = float32(sqrt(averaged / 2^L)) as the caller rounded them
extern "C" int bbt_hsum_plan_create(bbt_hsum_plan** plan, int64_t nbin, int64_t n, int64_t n_levels, int64_t lo,
                                    int64_t n_elem, const float* scales_host) {
    ARG_TRY(plan && scales_host, "bbt_hsum_plan_create: null argument");
    *plan = nullptr;
    const char* err = hsum_sizes(nbin, n, n_levels, lo, n_elem);
    ARG_TRY(!err, "bbt_hsum_plan_create: %s", err ? err : "");
    for (int L = 0; L < (int)n_levels; ++L)
        ARG_TRY(scales_host[L] > 0.f && scales_host[L] < __builtin_inff(),
                "bbt_hsum_plan_create: the scales must be finite and > 0");
    bbt_hsum_plan* p = new bbt_hsum_plan;
    p->nbin = nbin, p->n = n, p->K = (int)n_levels, p->lo = lo, p->n_elem = n_elem;
    for (int L = 0; L < p->K; ++L) p->c[L] = scales_host[L];
    *plan = p;
    return 0;
}

// the tiling the next call will use (plan may be null: the tiling only); scales: 6 floats, the plan's c_L
// (0 beyond its levels, and for a null plan)
extern "C" int bbt_hsum_plan_info(const bbt_hsum_plan* p, int* width, int* split, int* rows, float* scales) {
    const int w = hsum_env_width(), s = hsum_env_split(), r = hsum_env_rows();
    if (width) *width = w ? w : BBT_HSUM_WIDTH;
    if (split) *split = s ? s : BBT_HSUM_SPLIT;
    if (rows) *rows = r ? r : BBT_HSUM_ROWS;
    if (scales)
        for (int L = 0; L < BBT_HSUM_MAX_LEVELS; ++L) scales[L] = p ? p->c[L] : 0.f;
    return 0;
}

// best[s][b][3][e], s < n_spec, b < ceil(nbin / n), from in[s][j][e], j < nbin
extern "C" int bbt_hsum_execute(bbt_hsum_plan* p, const float* in_dev, int64_t n_spec, float* out_dev,
                                bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_hsum_execute: null argument");
    ARG_TRY(aligned4(in_dev, out_dev), "bbt_hsum_execute: arrays must be 4-byte aligned");
    HsumGeo g = {};
    const char* err = hsum_geo(n_spec, p->nbin, p->n, p->K, p->lo, p->n_elem, hsum_env_width(), hsum_env_split(), &g);
    ARG_TRY(!err, "bbt_hsum_execute: %s (n_spec=%lld, nbin=%lld, n=%lld)", err ? err : "", (long long)n_spec, p->nbin,
            p->n);
    for (int L = 0; L < BBT_HSUM_MAX_LEVELS; ++L) g.c[L] = p->c[L];
    const dim3 grid((unsigned)g.n_wg), block(BBT_HSUM_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (g.K) {
        case 1: hipLaunchKernelGGL((k_hsum_search<1>), grid, block, 0, st, in_dev, out_dev, g); break;
        case 2: hipLaunchKernelGGL((k_hsum_search<2>), grid, block, 0, st, in_dev, out_dev, g); break;
        case 3: hipLaunchKernelGGL((k_hsum_search<3>), grid, block, 0, st, in_dev, out_dev, g); break;
        case 4: hipLaunchKernelGGL((k_hsum_search<4>), grid, block, 0, st, in_dev, out_dev, g); break;
        case 5: hipLaunchKernelGGL((k_hsum_search<5>), grid, block, 0, st, in_dev, out_dev, g); break;
        default: hipLaunchKernelGGL((k_hsum_search<6>), grid, block, 0, st, in_dev, out_dev, g); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// fluctuation spectra of 2^15 ... 2^22 points (lspec_kernels.hpp; every index is lspec_geo.hpp's)
struct bbt_lspec_plan {
    long long n = 0, stack = 0, n_elem = 0;
    float2 *tw1 = nullptr, *tw2 = nullptr, *tw_hi = nullptr, *tw_lo = nullptr;
    PlanScratch scratch;             // 8 n bytes per column pair of a launch, between the two passes
};

// BBT_LSPEC_THREADS: threads of a workgroup of both passes (256, 512, 1024): which thread moves which
// cell changes with it.
static int lspec_env_threads() {
    const int t = env_knob("BBT_LSPEC_THREADS", {256, 512, 1024});
    return t ? t : BBT_LSPEC_THREADS;
}

// count entries exp(-2 pi i j mult / len), j < count, made in float64 and rounded once
static int lspec_table(float2** dst, long long count, long long mult, long long len) {
    std::vector<float2> h((size_t)count);
    const double unit = -2. * 3.14159265358979323846264338327950288 / (double)len;
    for (long long j = 0; j < count; ++j) {
        const long long m = (j * mult) % len;                   // reduced in integers first
        h[(size_t)j] = make_float2((float)std::cos(unit * (double)m), (float)std::sin(unit * (double)m));
    }
    HIP_TRY(hipMalloc((void**)dst, h.size() * sizeof(float2)));
    HIP_TRY(hipMemcpy(*dst, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int bbt_lspec_plan_destroy(bbt_lspec_plan* p) {
    if (!p) return 0;
    for (float2* t : {p->tw1, p->tw2, p->tw_hi, p->tw_lo})
        if (t) (void)hipFree(t);
    p->scratch.release();
    delete p;
    return 0;
}

extern "C" int bbt_lspec_plan_create(bbt_lspec_plan** plan, int64_t n, int64_t stack, int64_t n_elem) {
    ARG_TRY(plan, "bbt_lspec_plan_create: null argument");
    *plan = nullptr;
    const char* err = lspec_sizes(n, stack, n_elem);
    ARG_TRY(!err, "bbt_lspec_plan_create: %s (n=%lld, stack=%lld, n_elem=%lld)", err ? err : "", (long long)n,
            (long long)stack, (long long)n_elem);
    LspecGeo g = {};
    err = lspec_geo(n, n_elem, 1, 0, &g);
    ARG_TRY(!err, "bbt_lspec_plan_create: %s", err ? err : "");
    bbt_lspec_plan* p = new bbt_lspec_plan;
    p->n = n, p->stack = stack, p->n_elem = n_elem;
    const long long lo = 1ll << BBT_LSPEC_TW_LO_LOG2;
    if (lspec_table(&p->tw1, g.n1 / 2, 1, g.n1) || lspec_table(&p->tw2, g.n2 / 2, 1, g.n2) ||
        lspec_table(&p->tw_hi, n / lo, lo, n) || lspec_table(&p->tw_lo, lo, 1, n)) {
        bbt_lspec_plan_destroy(p);
        return 1;
    }
    *plan = p;
    return 0;
}

// the split and the tiling, and what a call under `budget` bytes of scratch (<= 0: the default) takes:
// pairs per launch and the bytes of scratch
extern "C" int bbt_lspec_plan_info(const bbt_lspec_plan* p, int64_t budget, int* n1, int* n2, int* cols, int* pairs,
                                   int* threads, int64_t* pairs_per_launch, int64_t* scratch_bytes) {
    ARG_TRY(p, "bbt_lspec_plan_info: null argument");
    LspecGeo g = {};
    const long long per = lspec_pairs_per_launch(p->n, p->n_elem, budget > 0 ? budget : BBT_LSPEC_BUDGET);
    const char* err = lspec_geo(p->n, p->n_elem, per, 0, &g);
    ARG_TRY(!err, "bbt_lspec_plan_info: %s", err ? err : "");
    if (n1) *n1 = g.n1;
    if (n2) *n2 = g.n2;
    if (cols) *cols = g.c1;
    if (pairs) *pairs = g.cp;
    if (threads) *threads = lspec_env_threads();
    if (pairs_per_launch) *pairs_per_launch = per;
    if (scratch_bytes) *scratch_bytes = 8 * p->n * per;
    return 0;
}

// out[m][k][e], m < n_spec, k <= n / 2, from in[t][e], t < n_in, n_in >= n_spec * stack * n
extern "C" int bbt_lspec_execute(bbt_lspec_plan* p, const float* in_dev, int64_t n_in, float* out_dev,
                                 int64_t n_spec, int64_t budget, bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_lspec_execute: null argument");
    ARG_TRY(aligned4(in_dev, out_dev), "bbt_lspec_execute: arrays must be 4-byte aligned");
    ARG_TRY(n_spec >= 1, "bbt_lspec_execute: no whole transform (n_spec=%lld)", (long long)n_spec);
    ARG_TRY(n_spec <= BBT_LSPEC_MAX_VALUES / (p->n * p->stack * p->n_elem),
            "bbt_lspec_execute: more than 2^40 values in one call");
    ARG_TRY(n_in >= n_spec * p->stack * p->n, "bbt_lspec_execute: %lld samples are not %lld stacks of %lld x %lld",
            (long long)n_in, (long long)n_spec, p->stack, p->n);
    const long long per = lspec_pairs_per_launch(p->n, p->n_elem, budget > 0 ? budget : BBT_LSPEC_BUDGET);
    const long long n_launch = lspec_n_launch(p->n_elem, per);
    LspecGeo g = {};
    for (long long i : {0ll, n_launch - 1}) {
        const char* err = lspec_geo(p->n, p->n_elem, per, i, &g);
        ARG_TRY(!err, "bbt_lspec_execute: %s (n=%lld, n_elem=%lld)", err ? err : "", p->n, p->n_elem);
    }
    if (p->scratch.reserve((size_t)(8 * p->n * per))) return 1;
    float2* scratch = (float2*)p->scratch.ptr;
    hipStream_t st = (hipStream_t)stream;
    const float scale = 1.f / (float)p->stack;
    const dim3 block((unsigned)lspec_env_threads());
    const long long nbin = p->n / 2 + 1;
    for (long long m = 0; m < n_spec; ++m)
        for (long long q = 0; q < p->stack; ++q) {
            const float* x = in_dev + (m * p->stack + q) * p->n * p->n_elem;
            float* o = out_dev + m * nbin * p->n_elem;
            const int mode = q == 0 ? 0 : (q + 1 < p->stack ? 1 : 2);
            for (long long i = 0; i < n_launch; ++i) {
                lspec_geo(p->n, p->n_elem, per, i, &g);
                hipLaunchKernelGGL(k_lspec_first, dim3((unsigned)g.n_wg1), block, 0, st, x,
                                   scratch, p->tw1, p->tw_hi, p->tw_lo, g);
                hipLaunchKernelGGL(k_lspec_last, dim3((unsigned)g.n_wg2), block, 0, st, scratch, o,
                                   p->tw2, g, mode, scale);
            }
        }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// acceleration trials (accel_kernels.hpp; the rule and every index are accel_geo.hpp's)
struct bbt_accel_plan {
    long long n = 0, n_elem = 0, n_acc = 0;
    double k_min = 0., k_max = 0.;
    double* factors = nullptr;       // the k_j on the device, float64
};

// BBT_ACCEL_ROUTE: 0 automatic, 1 the window wherever it fits, 2 direct.
static int accel_env_route() { return env_knob("BBT_ACCEL_ROUTE", {1, 2}); }

extern "C" int bbt_accel_plan_destroy(bbt_accel_plan* p) {
    if (!p) return 0;
    if (p->factors) (void)hipFree(p->factors);
    delete p;
    return 0;
}

extern "C" int bbt_accel_plan_create(bbt_accel_plan** plan, int64_t n, int64_t n_elem, const double* factors_host,
                                     int64_t n_acc) {
    ARG_TRY(plan && factors_host, "bbt_accel_plan_create: null argument");
    *plan = nullptr;
    const char* err = accel_sizes(n, n_elem, n_acc);
    ARG_TRY(!err, "bbt_accel_plan_create: %s (n=%lld, n_elem=%lld, n_acc=%lld)", err ? err : "", (long long)n,
            (long long)n_elem, (long long)n_acc);
    double k_min = factors_host[0], k_max = factors_host[0];
    for (int64_t j = 0; j < n_acc; ++j) {
        const double k = factors_host[j];
        ARG_TRY(accel_factor_ok(n, k), "bbt_accel_plan_create: factor %lld, %g, is beyond |k| n <= 1/4 (n=%lld)",
                (long long)j, k, (long long)n);
        k_min = k < k_min ? k : k_min, k_max = k > k_max ? k : k_max;
    }
    bbt_accel_plan* p = new bbt_accel_plan;
    p->n = n, p->n_elem = n_elem, p->n_acc = n_acc, p->k_min = k_min, p->k_max = k_max;
    if (hipMalloc((void**)&p->factors, (size_t)n_acc * sizeof(double)) != hipSuccess ||
        hipMemcpy(p->factors, factors_host, (size_t)n_acc * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        bbt_accel_plan_destroy(p);
        ARG_TRY(false, "bbt_accel_plan_create: no device table of %lld factors", (long long)n_acc);
    }
    *plan = p;
    return 0;
}

// For output rows [out_first, out_first + n_out): the route a launch takes now (1: the window wherever it
// fits, 2: direct), the rows of a tile, the LDS bytes the window kernel declares, the input rows the run
// needs (first, count) and whether that window, taken as one tile, would fit the LDS.
extern "C" int bbt_accel_plan_info(const bbt_accel_plan* p, int64_t out_first, int64_t n_out, int* route, int* rows,
                                   int64_t* lds_bytes, int64_t* win_first, int64_t* win_rows, int* fits) {
    ARG_TRY(p, "bbt_accel_plan_info: null argument");
    ARG_TRY(out_first >= 0 && n_out >= 1, "bbt_accel_plan_info: no rows");
    ARG_TRY(n_out <= BBT_ACCEL_MAX_VALUES && out_first <= BBT_ACCEL_MAX_VALUES - n_out,
            "bbt_accel_plan_info: rows beyond 2^40");
    long long lo, hi;
    accel_window(p->n, p->k_min, p->k_max, out_first, out_first + n_out - 1, &lo, &hi);
    AccelGeo g = {};
    const char* err = accel_geo(p->n, p->n_elem, p->n_acc, 4, p->k_min, p->k_max, lo, hi - lo + 1, out_first, n_out, &g);
    ARG_TRY(!err, "bbt_accel_plan_info: %s", err ? err : "");
    if (route) *route = accel_route(accel_env_route(), g);
    if (rows) *rows = g.rows;
    if (lds_bytes) *lds_bytes = BBT_ACCEL_LDS_BYTES;
    if (win_first) *win_first = lo;
    if (win_rows) *win_rows = hi - lo + 1;
    if (fits) *fits = (hi - lo + 1) * p->n_elem * 4 <= BBT_ACCEL_LDS_BYTES;
    return 0;
}

// out[g - out_first][j][e] = in[q n + src(i, j) - in_first][e] for the global rows g = q n + i of
// [out_first, out_first + n_out); in_dev holds global rows [in_first, in_first + n_in)
extern "C" int bbt_accel_execute(bbt_accel_plan* p, const float* in_dev, int64_t in_first, int64_t n_in,
                                 float* out_dev, int64_t out_first, int64_t n_out, bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_accel_execute: null argument");
    ARG_TRY(aligned4(in_dev, out_dev), "bbt_accel_execute: arrays must be 4-byte aligned");
    const bool wide = p->n_elem % 4 == 0 && (((uintptr_t)in_dev | (uintptr_t)out_dev) & 15) == 0;
    AccelGeo g = {};
    const char* err = accel_geo(p->n, p->n_elem, p->n_acc, wide ? 16 : 4, p->k_min, p->k_max, in_first, n_in,
                                out_first, n_out, &g);
    ARG_TRY(!err, "bbt_accel_execute: %s (rows %lld + %lld from a piece %lld + %lld, n=%lld)", err ? err : "",
            (long long)out_first, (long long)n_out, (long long)in_first, (long long)n_in, p->n);
    const int route = accel_route(accel_env_route(), g);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.n_tile, (unsigned)g.n_seg), block(BBT_ACCEL_THREADS);
    if (wide) {
        const uint4* x = (const uint4*)in_dev;
        uint4* o = (uint4*)out_dev;
        if (route == 1) hipLaunchKernelGGL((k_accel<uint4, true>), grid, block, 0, st, x, o, p->factors, g);
        else hipLaunchKernelGGL((k_accel<uint4, false>), grid, block, 0, st, x, o, p->factors, g);
    } else {
        const unsigned* x = (const unsigned*)in_dev;
        unsigned* o = (unsigned*)out_dev;
        if (route == 1) hipLaunchKernelGGL((k_accel<unsigned, true>), grid, block, 0, st, x, o, p->factors, g);
        else hipLaunchKernelGGL((k_accel<unsigned, false>), grid, block, 0, st, x, o, p->factors, g);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// block median / MAD by selection (rank_kernels.hpp; the tiling is rank_geo.hpp's)

// BBT_RANK_ROUTE: lds (wherever the block fits), global, or auto; BBT_RANK_DIGIT: bits of a radix digit
// (4, 8); BBT_RANK_WIDTH: elements of a workgroup (16, 32, 64).  The route is a word, so it is read here,
// under the same contract as `env_knob`.
static int rank_env_route() {
    const char* e = getenv("BBT_RANK_ROUTE");
    if (e && !strcmp(e, "lds")) return BBT_RANK_ROUTE_LDS;
    if (e && !strcmp(e, "global")) return BBT_RANK_ROUTE_GLOBAL;
    return BBT_RANK_ROUTE_AUTO;
}
static int rank_env_digit() { return env_knob("BBT_RANK_DIGIT", {4, 8}); }
static int rank_env_width() { return env_knob("BBT_RANK_WIDTH", {16, 32, 64}); }

static int rank_launch(const RankGeo& g, const float* x, float* out, float* med, float* mad, hipStream_t st) {
    const dim3 grid((unsigned)g.n_wg), block(BBT_RANK_THREADS);
    const size_t lds = (size_t)g.lds_bytes;
    const bool in_lds = g.route == BBT_RANK_ROUTE_LDS;
    // (up to 72 KiB of dynamic LDS: beyond what a kernel may take unasked)
    const void* func = g.digit == 4 ? (in_lds ? (const void*)k_rank<4, true> : (const void*)k_rank<4, false>)
                                    : (in_lds ? (const void*)k_rank<8, true> : (const void*)k_rank<8, false>);
    if (ensure_dyn_lds(func, BBT_RANK_LDS_BYTES)) return 1;
    if (g.digit == 4) {
        if (in_lds) hipLaunchKernelGGL((k_rank<4, true>), grid, block, lds, st, x, out, med, mad, g);
        else hipLaunchKernelGGL((k_rank<4, false>), grid, block, lds, st, x, out, med, mad, g);
    } else {
        if (in_lds) hipLaunchKernelGGL((k_rank<8, true>), grid, block, lds, st, x, out, med, mad, g);
        else hipLaunchKernelGGL((k_rank<8, false>), grid, block, lds, st, x, out, med, mad, g);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// med[s][b][e] (and mad[s][b][e]) of block b < ceil((nbin - skip) / m) of spectrum s < n_spec; NaN where flagged
extern "C" int bbt_rank_stats(const float* x_dev, float* med_dev, float* mad_dev, int64_t n_spec, int64_t nbin,
                              int64_t n_elem, int64_t m, int64_t skip, bbt_stream stream) {
    ARG_TRY(x_dev && med_dev, "bbt_rank_stats: null argument");
    ARG_TRY(aligned4(x_dev, med_dev, mad_dev), "bbt_rank_stats: arrays must be 4-byte aligned");
    RankGeo g = {};
    const char* err = rank_geo(n_spec, nbin, n_elem, m, skip, rank_env_width(), rank_env_digit(), rank_env_route(), &g);
    ARG_TRY(!err, "bbt_rank_stats: %s (n_spec=%lld, nbin=%lld, n_elem=%lld, m=%lld, skip=%lld)", err ? err : "",
            (long long)n_spec, (long long)nbin, (long long)n_elem, (long long)m, (long long)skip);
    g.mode = BBT_RANK_STATS, g.with_mad = mad_dev != nullptr;
    return rank_launch(g, x_dev, nullptr, med_dev, mad_dev, (hipStream_t)stream);
}

// out[b * n + t][e] = (x[b * n + t][e] - med) * (1 / (1.4826 mad)) of block b < n_block, element e < n_elem
extern "C" int bbt_rank_standardize(const float* x_dev, float* out_dev, int64_t n_block, int64_t n, int64_t n_elem,
                                    bbt_stream stream) {
    ARG_TRY(x_dev && out_dev, "bbt_rank_standardize: null argument");
    ARG_TRY(aligned4(x_dev, out_dev), "bbt_rank_standardize: arrays must be 4-byte aligned");
    RankGeo g = {};
    const char* err = rank_std_geo(n_block, n, n_elem, rank_env_width(), rank_env_digit(), rank_env_route(), &g);
    ARG_TRY(!err, "bbt_rank_standardize: %s (n_block=%lld, n=%lld, n_elem=%lld)", err ? err : "", (long long)n_block,
            (long long)n, (long long)n_elem);
    g.mode = BBT_RANK_STANDARDIZE;
    return rank_launch(g, x_dev, out_dev, nullptr, nullptr, (hipStream_t)stream);
}

// out[s][j][e] = x[s][j][e] * (1 / (med / ratio)) with the median of the block of m bins that holds j, +0 for j < skip
extern "C" int bbt_rank_whiten(const float* x_dev, float* out_dev, int64_t n_spec, int64_t nbin, int64_t n_elem,
                               int64_t m, int64_t skip, double ratio, bbt_stream stream) {
    ARG_TRY(x_dev && out_dev, "bbt_rank_whiten: null argument");
    ARG_TRY(aligned4(x_dev, out_dev), "bbt_rank_whiten: arrays must be 4-byte aligned");
    ARG_TRY(ratio > 0. && ratio < __builtin_inf(), "bbt_rank_whiten: ratio must be finite and > 0");
    RankGeo g = {};
    const char* err = rank_geo(n_spec, nbin, n_elem, m, skip, rank_env_width(), rank_env_digit(), rank_env_route(), &g);
    ARG_TRY(!err, "bbt_rank_whiten: %s (n_spec=%lld, nbin=%lld, n_elem=%lld, m=%lld, skip=%lld)", err ? err : "",
            (long long)n_spec, (long long)nbin, (long long)n_elem, (long long)m, (long long)skip);
    g.mode = BBT_RANK_WHITEN, g.ratio = ratio;
    return rank_launch(g, x_dev, out_dev, nullptr, nullptr, (hipStream_t)stream);
}

// the route (1 lds, 2 global), digit and width a launch of these sizes takes, the LDS bytes of a workgroup,
// and lds_rows[3]: the longest block the lds route takes at widths 16, 32, 64 with that digit.  No device.
extern "C" int bbt_rank_info(int64_t n_spec, int64_t nbin, int64_t n_elem, int64_t m, int64_t skip, int* route,
                             int* digit, int* width, int64_t* lds_bytes, int64_t* lds_rows) {
    RankGeo g = {};
    const char* err = rank_geo(n_spec, nbin, n_elem, m, skip, rank_env_width(), rank_env_digit(), rank_env_route(), &g);
    ARG_TRY(!err, "bbt_rank_info: %s (n_spec=%lld, nbin=%lld, n_elem=%lld, m=%lld, skip=%lld)", err ? err : "",
            (long long)n_spec, (long long)nbin, (long long)n_elem, (long long)m, (long long)skip);
    if (route) *route = g.route;
    if (digit) *digit = g.digit;
    if (width) *width = g.nx;
    if (lds_bytes) *lds_bytes = g.lds_bytes;
    if (lds_rows) {
        const int d = rank_env_digit() ? rank_env_digit() : BBT_RANK_DIGIT_LDS;
        lds_rows[0] = rank_lds_rows(16, d), lds_rows[1] = rank_lds_rows(32, d), lds_rows[2] = rank_lds_rows(64, d);
    }
    return 0;
}

// ---------------------------------------------------------------------------
// sliding-median baseline: RunningMedian, Detrend (rmed_kernels.hpp; the tiling is rmed_geo.hpp's)
struct bbt_rmed_plan {
    long long width = 0, scrunch = 0, n_elem = 0;
    PlanScratch scratch;             // c[c0 ... c1) and m[m0 ... m1) of a call (scrunch > 1); the flags travel in them
};

// BBT_RMED_TILE: elements of a workgroup (16, 32, 64); BBT_RMED_ROWS: medians of a workgroup at most (16 ...
// 1024); BBT_RMED_SELECT: 1 a fresh radix descent per median, 2 the walk from median to median.
static int rmed_env_tile() { return env_knob("BBT_RMED_TILE", {16, 32, 64}); }
static int rmed_env_rows() { return env_knob("BBT_RMED_ROWS", {16, 32, 64, 128, 256, 512, 1024}); }
static int rmed_env_select() { return env_knob("BBT_RMED_SELECT", {BBT_RMED_SELECT_RADIX, BBT_RMED_SELECT_WALK}); }

extern "C" int bbt_rmed_plan_destroy(bbt_rmed_plan* p) {
    if (!p) return 0;
    p->scratch.release();
    delete p;
    return 0;
}

extern "C" int bbt_rmed_plan_create(bbt_rmed_plan** plan, int64_t width, int64_t scrunch, int64_t n_elem) {
    ARG_TRY(plan, "bbt_rmed_plan_create: null argument");
    *plan = nullptr;
    const char* err = rmed_sizes(width, scrunch, n_elem);
    ARG_TRY(!err, "bbt_rmed_plan_create: %s (width=%lld, scrunch=%lld, n_elem=%lld)", err ? err : "", (long long)width,
            (long long)scrunch, (long long)n_elem);
    bbt_rmed_plan* p = new bbt_rmed_plan;
    p->width = width, p->scrunch = scrunch, p->n_elem = n_elem;
    *plan = p;
    return 0;
}

// For the call that makes output samples [out_first, out_first + n_out) of a stream of n_rows scrunch rows:
// the method (1 radix, 2 walk), the tile width, the medians of a workgroup, the LDS bytes of a workgroup, the
// scratch bytes of the call, and the input samples it needs (first, count).  No device.
extern "C" int bbt_rmed_info(int64_t width, int64_t scrunch, int64_t n_elem, int64_t n_rows, int64_t out_first,
                             int64_t n_out, int* method, int* tile, int* rows, int64_t* lds_bytes,
                             int64_t* scratch_bytes, int64_t* in_first, int64_t* in_count) {
    RmedGeo g = {};
    const char* err = rmed_sizes(width, scrunch, n_elem);
    if (!err && (n_rows < 1 || n_rows > BBT_RMED_MAX_ROWS / scrunch)) err = "the stream must have 1 ... 2^40 / scrunch rows";
    long long first = 0, count = 0;
    if (!err && out_first >= 0 && n_out >= scrunch) {
        long long m0, m1, c0, c1;
        rmed_need(scrunch, width / 2, n_rows, out_first / scrunch, (out_first + n_out) / scrunch, &m0, &m1, &c0, &c1);
        first = c0 * scrunch, count = (c1 - c0) * scrunch;
    }
    if (!err)
        err = rmed_geo(width, scrunch, n_elem, n_rows, first, count, out_first, n_out, rmed_env_tile(), rmed_env_rows(),
                       rmed_env_select(), &g);
    ARG_TRY(!err, "bbt_rmed_info: %s (width=%lld, scrunch=%lld, n_elem=%lld, n_rows=%lld, out_first=%lld, n_out=%lld)",
            err ? err : "", (long long)width, (long long)scrunch, (long long)n_elem, (long long)n_rows,
            (long long)out_first, (long long)n_out);
    if (method) *method = g.method;
    if (tile) *tile = g.nx;
    if (rows) *rows = g.run;
    if (lds_bytes) *lds_bytes = g.lds_bytes;
    if (scratch_bytes) *scratch_bytes = g.scratch_bytes;
    if (in_first) *in_first = first;
    if (in_count) *in_count = count;
    return 0;
}

// out[i - out_first][e], out_first <= i < out_first + n_out, the baseline (mode 0) or x minus it (mode 1), from
// in[i - in_first][e], in_first <= i < in_first + n_in, of a stream of n_rows scrunch rows.  One plan serves one
// stream at a time: the scratch is the plan's.
extern "C" int bbt_rmed_execute(bbt_rmed_plan* p, const float* in_dev, int64_t in_first, int64_t n_in, float* out_dev,
                                int64_t out_first, int64_t n_out, int64_t n_rows, int mode, bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_rmed_execute: null argument");
    ARG_TRY(aligned4(in_dev, out_dev), "bbt_rmed_execute: arrays must be 4-byte aligned");
    ARG_TRY(mode == BBT_RMED_BASELINE || mode == BBT_RMED_DETREND, "bbt_rmed_execute: mode must be 0 (baseline) or 1 (detrend)");
    RmedGeo g = {};
    const char* err = rmed_geo(p->width, p->scrunch, p->n_elem, n_rows, in_first, n_in, out_first, n_out, rmed_env_tile(),
                               rmed_env_rows(), rmed_env_select(), &g);
    ARG_TRY(!err, "bbt_rmed_execute: %s (n_rows=%lld, in_first=%lld, n_in=%lld, out_first=%lld, n_out=%lld)",
            err ? err : "", (long long)n_rows, (long long)in_first, (long long)n_in, (long long)out_first, (long long)n_out);
    g.mode = mode;
    const long long n_c = g.c1 - g.c0, E = g.n_elem;
    const long long wg_scrunch = (n_c * E + BBT_RMED_THREADS - 1) / BBT_RMED_THREADS;
    const long long wg_apply = (g.n_out * E + BBT_RMED_THREADS - 1) / BBT_RMED_THREADS;
    ARG_TRY(wg_scrunch < (1ll << 31) && wg_apply < (1ll << 31), "bbt_rmed_execute: too many values for one launch");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.n_wg), block(BBT_RMED_THREADS);
    const size_t lds = (size_t)g.lds_bytes;
    const float* x_c0 = in_dev + (g.c0 * g.S - g.in_first) * E;               // the first sample of scrunch row c0
    if (g.S == 1) {
        if (ensure_dyn_lds((const void*)k_rmed_select<true>, BBT_RANK_LDS_BYTES)) return 1;
        hipLaunchKernelGGL((k_rmed_select<true>), grid, block, lds, st, (const unsigned*)x_c0, g.c0, out_dev, g);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (ensure_dyn_lds((const void*)k_rmed_select<false>, BBT_RANK_LDS_BYTES)) return 1;
    if (p->scratch.reserve((size_t)g.scratch_bytes)) return 1;
    unsigned* c = (unsigned*)p->scratch.ptr;
    unsigned* m = c + n_c * E;
    hipLaunchKernelGGL(k_rmed_scrunch, dim3((unsigned)wg_scrunch), block, 0, st, x_c0, c, n_c, E, (int)g.S);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_rmed_select<false>), grid, block, lds, st, (const unsigned*)c, g.c0, (float*)m, g);
    HIP_TRY(hipGetLastError());
    const float* x_out = in_dev + (g.out_first - g.in_first) * E;
    hipLaunchKernelGGL(k_rmed_apply, dim3((unsigned)wg_apply), block, 0, st, x_out, (const unsigned*)m, out_dev, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// cross-products of up to 64 inputs: Correlate (corr_kernels.hpp; the cutting is corr_geo.hpp's)
struct bbt_corr_plan {
    long long A = 0, E = 0, inner = 0, n = 0;
    int average = 0;
    long long carried = -1;          // the sample up to which `carry` holds the sums of an unfinished block, or -1
    PlanScratch scratch;             // [segment][element][baseline] of a piece, float32 pairs
    PlanScratch carry;               // [element][baseline], float64 pairs
};

// BBT_CORR_PACK: elements that share a 32 x 32 tile (1 ... 8, at most 32 / (2 n_inputs)); BBT_CORR_WAVES: waves
// of a workgroup (1, 2, 4).
static int corr_env_pack() { return env_knob("BBT_CORR_PACK", {1, 2, 3, 4, 5, 6, 7, 8}); }
static int corr_env_waves() { return env_knob("BBT_CORR_WAVES", {1, 2, 4}); }

extern "C" int bbt_corr_plan_destroy(bbt_corr_plan* p) {
    if (!p) return 0;
    p->scratch.release();
    p->carry.release();
    delete p;
    return 0;
}

extern "C" int bbt_corr_plan_create(bbt_corr_plan** plan, int64_t n_inputs, int64_t n_elem, int64_t inner, int64_t n,
                                    int average) {
    ARG_TRY(plan, "bbt_corr_plan_create: null argument");
    *plan = nullptr;
    const char* err = corr_sizes(n_inputs, n_elem, n);
    if (!err && (inner < 1 || n_elem % inner)) err = "inner must divide n_elem";
    ARG_TRY(!err, "bbt_corr_plan_create: %s (n_inputs=%lld, n_elem=%lld, inner=%lld, n=%lld)", err ? err : "",
            (long long)n_inputs, (long long)n_elem, (long long)inner, (long long)n);
    bbt_corr_plan* p = new bbt_corr_plan;
    p->A = n_inputs, p->E = n_elem, p->inner = inner, p->n = n, p->average = average != 0;
    *plan = p;
    return 0;
}

// For the piece [first, first + count) of a stream: the elements that share a tile, the tiles of a wave, the
// waves of a workgroup, the LDS bytes of a workgroup, the scratch bytes and the segments of the piece.  No
// device.
extern "C" int bbt_corr_info(int64_t n_inputs, int64_t n_elem, int64_t n, int64_t first, int64_t count, int* pack,
                             int* tiles, int* waves, int64_t* lds_bytes, int64_t* scratch_bytes, int64_t* n_seg) {
    CorrGeo g = {};
    const char* err = corr_geo(n_inputs, n_elem, n, first, count, corr_env_pack(), corr_env_waves(), &g);
    ARG_TRY(!err, "bbt_corr_info: %s (n_inputs=%lld, n_elem=%lld, n=%lld, first=%lld, count=%lld)", err ? err : "",
            (long long)n_inputs, (long long)n_elem, (long long)n, (long long)first, (long long)count);
    if (pack) *pack = g.pack;
    if (tiles) *tiles = g.n_tile;
    if (waves) *waves = g.waves;
    if (lds_bytes) *lds_bytes = g.lds_bytes;
    if (scratch_bytes) *scratch_bytes = g.scratch_bytes;
    if (n_seg) *n_seg = g.n_seg;
    return 0;
}

// in_dev: samples [first, first + count) of the stream, whole segments.  The blocks that end in the piece
// are written to out_dev, which begins at block out_block0 and holds n_out_blocks.  A piece that begins
// inside a block must follow the piece that ended there.
extern "C" int bbt_corr_execute(bbt_corr_plan* p, const void* in_dev, int64_t first, int64_t count, void* out_dev,
                                int64_t out_block0, int64_t n_out_blocks, bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_corr_execute: null argument");
    ARG_TRY(((((uintptr_t)in_dev) | ((uintptr_t)out_dev)) & 7) == 0, "bbt_corr_execute: arrays must be 8-byte aligned");
    CorrGeo g = {};
    const char* err = corr_geo(p->A, p->E, p->n, first, count, corr_env_pack(), corr_env_waves(), &g);
    ARG_TRY(!err, "bbt_corr_execute: %s (first=%lld, count=%lld)", err ? err : "", (long long)first, (long long)count);
    ARG_TRY(g.seg0 == 0 || p->carried == first,
            "bbt_corr_execute: a piece that begins inside a block must follow the piece that ended there (first=%lld)",
            (long long)first);
    ARG_TRY(out_block0 >= 0 && n_out_blocks >= 0 && (g.blk1 == g.blk0 || (out_block0 <= g.blk0 && g.blk1 <= out_block0 + n_out_blocks)),
            "bbt_corr_execute: the output [%lld, %lld) does not hold the blocks [%lld, %lld) that end in the piece",
            (long long)out_block0, (long long)(out_block0 + n_out_blocks), (long long)g.blk0, (long long)g.blk1);
    const long long n_val = 2 * g.E * g.B;
    const long long wg_finish = (n_val + 255) / 256;
    ARG_TRY(wg_finish < (1ll << 31), "bbt_corr_execute: too many values for one launch");
    const bool ends_inside = first + count != g.blk1 * g.n;
    if (p->scratch.reserve((size_t)g.scratch_bytes)) return 1;
    if ((g.seg0 || ends_inside) && p->carry.reserve((size_t)n_val * 8)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.n_wg), block(64 * g.waves);
    const size_t lds = (size_t)g.lds_bytes;
    const float* x = (const float*)in_dev;
    float* sc = (float*)p->scratch.ptr;
    switch (g.T) {
    case 1: hipLaunchKernelGGL((k_corr_gram<1>), grid, block, lds, st, x, sc, g); break;
    case 2: hipLaunchKernelGGL((k_corr_gram<2>), grid, block, lds, st, x, sc, g); break;
    case 3: hipLaunchKernelGGL((k_corr_gram<3>), grid, block, lds, st, x, sc, g); break;
    default: hipLaunchKernelGGL((k_corr_gram<4>), grid, block, lds, st, x, sc, g); break;
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_corr_finish, dim3((unsigned)wg_finish), dim3(256), 0, st, (const float*)sc, (double*)p->carry.ptr,
                       (float*)out_dev, g, p->inner, (long long)out_block0, p->average);
    HIP_TRY(hipGetLastError());
    p->carried = ends_inside ? first + count : -1;
    return 0;
}

// ---------------------------------------------------------------------------
// real-stream glue
extern "C" int bbt_real_op(const void* in_dev, void* out_dev, int op, int64_t n_total, int n_chan,
                           int n_stream, bbt_stream stream) {
    ARG_TRY(in_dev && out_dev, "bbt_real_op: null argument");
    ARG_TRY(op >= 0 && op <= 6, "bbt_real_op: op must be 0..6");
    ARG_TRY(n_total >= 0, "bbt_real_op: n_total < 0");
    ARG_TRY(op != 2 || (n_chan >= 2 && n_chan % 2 == 0 && n_stream >= 1),
            "bbt_real_op: half-to-full needs an even n_chan and n_stream >= 1");
    ARG_TRY(op < 4 || (n_chan >= 2 && n_chan % 2 == 0 && n_stream >= 2 && n_stream % 2 == 0),
            "bbt_real_op: splitting / merging two real streams needs even n_chan and n_stream");
    if (n_total == 0) return 0;
    ARG_TRY((n_total + 255) / 256 < (1ll << 31), "bbt_real_op: too many elements for one call");
    const dim3 grid((unsigned)((n_total + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (op) {
        case 0: hipLaunchKernelGGL((k_real_ops<0>), grid, block, 0, st, in_dev, out_dev, (long long)n_total, n_chan, n_stream); break;
        case 1: hipLaunchKernelGGL((k_real_ops<1>), grid, block, 0, st, in_dev, out_dev, (long long)n_total, n_chan, n_stream); break;
        case 2: hipLaunchKernelGGL((k_real_ops<2>), grid, block, 0, st, in_dev, out_dev, (long long)n_total, n_chan, n_stream); break;
        case 3: hipLaunchKernelGGL((k_real_ops<3>), grid, block, 0, st, in_dev, out_dev, (long long)n_total, n_chan, n_stream); break;
        case 4: hipLaunchKernelGGL((k_real_ops<4>), grid, block, 0, st, in_dev, out_dev, (long long)n_total, n_chan, n_stream); break;
        case 6: hipLaunchKernelGGL((k_real_ops<4, true>), grid, block, 0, st, in_dev, out_dev, (long long)n_total, n_chan, n_stream); break;
        default: hipLaunchKernelGGL((k_real_ops<5>), grid, block, 0, st, in_dev, out_dev, (long long)n_total, n_chan, n_stream); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// per-stream complex factor
extern "C" int bbt_chirp(void* out_dev, int64_t n, int n_col, const double* freq_hz, const double* sideband,
                         const double* ref_hz, double rate_hz, double d_dm, double offset_s, bbt_stream stream) {
    ARG_TRY(out_dev && freq_hz && sideband && ref_hz, "bbt_chirp: null argument");
    ARG_TRY(n >= 1 && n_col >= 1 && n_col <= 65535 && rate_hz > 0, "bbt_chirp: bad sizes");
    std::vector<double4> h(n_col);
    for (int c = 0; c < n_col; ++c) {
        ARG_TRY(ref_hz[c] > 0, "bbt_chirp: reference frequency %g of column %d is not positive", ref_hz[c], c);
        h[c] = make_double4(freq_hz[c], sideband[c], ref_hz[c], 0.);
    }
    double4* col = nullptr;
    HIP_TRY(hipMalloc((void**)&col, sizeof(double4) * n_col));
    hipError_t e = hipMemcpyAsync(col, h.data(), sizeof(double4) * n_col, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_chirp, dim3((unsigned)((n + 255) / 256), n_col), dim3(256), 0, (hipStream_t)stream,
                           (float2*)out_dev, (long long)n, col, rate_hz, d_dm, offset_s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);     // (the host copy of `col` goes with this frame)
    hipFree(col);
    if (e != hipSuccess) return fail("bbt_chirp: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int bbt_scale_streams(const void* in_dev, void* out_dev, int64_t n_samples, int n_elem,
                                 const void* factor_dev, bbt_stream stream) {
    ARG_TRY(in_dev && out_dev && factor_dev, "bbt_scale_streams: null argument");
    ARG_TRY(n_samples >= 0 && n_elem >= 1, "bbt_scale_streams: bad sizes");
    const long long total = (long long)n_samples * n_elem;
    if (total == 0) return 0;
    ARG_TRY((total + 255) / 256 < (1ll << 31), "bbt_scale_streams: too many elements for one call");
    hipLaunchKernelGGL(k_scale_streams, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const float2*)in_dev, (float2*)out_dev, total, n_elem,
                       (const float2*)factor_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// short-response convolution in the time domain

extern "C" int bbt_fir_plan_create(bbt_fir_plan** plan, int n_tap, int n_stream,
                                   const void* response_host) {
    ARG_TRY(plan && response_host, "bbt_fir_plan_create: null argument");
    *plan = nullptr;
    ARG_TRY(n_tap >= 1 && n_tap <= 1024, "bbt_fir_plan_create: n_tap=%d must be in [1, 1024]", n_tap);
    ARG_TRY(n_stream == 1 || (n_stream >= 2 && n_stream % 2 == 0),
            "bbt_fir_plan_create: n_stream=%d must be 1 or even (pad other odd counts)", n_stream);
    constexpr int R = BBT_FIR_R;
    bbt_fir_plan* p = new bbt_fir_plan;
    p->n_tap = n_tap;
    p->S = n_stream;
    p->npair = n_stream == 1 ? 1 : n_stream / 2;
    p->n_chunks = (n_tap + R - 1 + R - 1) / R;           // inputs u = r + m < n_tap + R - 1
    p->pitch = 256 + p->n_chunks;
    while (p->pitch % 16 != 2) ++p->pitch;
    p->tap_pitch = R * p->n_chunks + 2 * R;              // R - 1 zeros in front, zeros behind
    const cf* resp = (const cf*)response_host;           // (n_tap, n_stream), reference order
    std::vector<float2> re((size_t)p->npair * p->tap_pitch, make_float2(0.f, 0.f)), im(re);
    for (int sp = 0; sp < p->npair; ++sp)
        for (int m = 0; m < n_tap; ++m) {
            const cf a = resp[(size_t)(n_tap - 1 - m) * n_stream + 2 * sp];
            const cf b = n_stream == 1 ? a          // one stream: both halves of the time range
                                       : resp[(size_t)(n_tap - 1 - m) * n_stream + 2 * sp + 1];
            re[(size_t)sp * p->tap_pitch + (R - 1) + m] = make_float2(a.x, b.x);
            im[(size_t)sp * p->tap_pitch + (R - 1) + m] = make_float2(a.y, b.y);
            if (a.y != 0.f || b.y != 0.f) p->cplx = true;
        }
    if (upload(&p->tre, re) || upload(&p->tim, im)) {
        if (p->tre) hipFree(p->tre);
        delete p;
        return 1;
    }
    *plan = p;
    return 0;
}

extern "C" int bbt_fir_plan_destroy(bbt_fir_plan* p) {
    if (!p) return 0;
    if (p->tre) hipFree(p->tre);
    if (p->tim) hipFree(p->tim);
    delete p;
    return 0;
}

extern "C" int bbt_fir_execute(bbt_fir_plan* p, const void* in_dev, void* out_dev, int64_t n_out,
                               bbt_stream stream) {
    ARG_TRY(p && in_dev && out_dev, "bbt_fir_execute: null argument");
    ARG_TRY(n_out >= 0, "bbt_fir_execute: n_out=%lld is negative", (long long)n_out);
    if (n_out == 0) return 0;
    constexpr int R = BBT_FIR_R;
    const long long n_in = n_out + p->n_tap - 1;
    // (one stream: the grid covers the first half of the outputs, a thread's second filter the other half)
    const long long covered = p->S == 1 ? (n_out + 1) / 2 : n_out;
    const long long tiles = (covered + 256 * R - 1) / (256 * R);
    ARG_TRY(tiles * p->npair < (1ll << 31), "bbt_fir_execute: too large for one call");
    const size_t lds = (size_t)R * p->pitch * sizeof(float4);
    const dim3 grid((unsigned)(tiles * p->npair));
    if (p->cplx)
        hipLaunchKernelGGL((k_fir<R, true>), grid, dim3(256), lds, (hipStream_t)stream,
                           (const float2*)in_dev, (float2*)out_dev, n_in, (long long)n_out, p->S,
                           p->tre, p->tim, p->tap_pitch, p->n_chunks, p->pitch);
    else
        hipLaunchKernelGGL((k_fir<R, false>), grid, dim3(256), lds, (hipStream_t)stream,
                           (const float2*)in_dev, (float2*)out_dev, n_in, (long long)n_out, p->S,
                           p->tre, p->tim, p->tap_pitch, p->n_chunks, p->pitch);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// sampler frames -> float32 / complex64 (k_unpack)
extern "C" int bbt_unpack_masked(const void* raw_dev, void* out_dev, int64_t n_frames, int frame_bytes,
                                 int header_bytes, int bits, int samples_per_frame, int n_thread,
                                 int n_elem, int code, const void* valid_dev, bbt_stream stream);
extern "C" int bbt_unpack(const void* raw_dev, void* out_dev, int64_t n_frames, int frame_bytes,
                          int header_bytes, int bits, int samples_per_frame, int n_thread,
                          int n_elem, int code, bbt_stream stream) {
    return bbt_unpack_masked(raw_dev, out_dev, n_frames, frame_bytes, header_bytes, bits,
                             samples_per_frame, n_thread, n_elem, code, nullptr, stream);
}
extern "C" int bbt_unpack_masked(const void* raw_dev, void* out_dev, int64_t n_frames, int frame_bytes,
                                 int header_bytes, int bits, int samples_per_frame, int n_thread,
                                 int n_elem, int code, const void* valid_dev, bbt_stream stream) {
    ARG_TRY(raw_dev && out_dev, "bbt_unpack: null argument");
    ARG_TRY(n_frames >= 0 && n_thread >= 1 && n_frames % n_thread == 0,
            "bbt_unpack: %lld frames are not whole sets of %d threads", (long long)n_frames, n_thread);
    ARG_TRY(code == 0 || code == 1, "bbt_unpack: code must be 0 (VDIF levels) or 1 (two's complement)");
    ARG_TRY(code == 0 ? (bits == 1 || bits == 2 || bits == 4 || bits == 8 || bits == 16)
                      : (bits == 8 || bits == 16),
            "bbt_unpack: %d bits per component are not supported for code %d", bits, code);
    ARG_TRY(frame_bytes > header_bytes && header_bytes >= 0 && frame_bytes % 4 == 0 &&
                header_bytes % 4 == 0,
            "bbt_unpack: frame of %d bytes with a header of %d", frame_bytes, header_bytes);
    ARG_TRY(samples_per_frame >= 1 && n_elem >= 1 &&
                (int64_t)samples_per_frame * n_elem * bits <= (int64_t)(frame_bytes - header_bytes) * 8,
            "bbt_unpack: %d samples of %d components at %d bits do not fit the payload",
            samples_per_frame, n_elem, bits);
    if (n_frames == 0) return 0;
    ARG_TRY(n_frames < (1ll << 31), "bbt_unpack: too many frames for one call");
    const long long per_frame = (long long)samples_per_frame * n_elem;
    ARG_TRY(per_frame * bits < (1ll << 32), "bbt_unpack: frames of %lld components are too long",
            per_frame);
    // components decoded per thread: adjacent in payload and output, 16-byte aligned stores
    const int g = n_elem % 4 == 0 ? 4 : (n_elem % 2 == 0 ? 2 : 1);
    const long long by = (per_frame / g + 256 * BBT_UNPACK_ITER - 1) / (256 * BBT_UNPACK_ITER);
    ARG_TRY(by <= 65535, "bbt_unpack: frames of %lld components are too long", per_frame);
    const dim3 grid((unsigned)n_frames, (unsigned)by);
    int lg_e = -1;
    for (int k = 0; k < 16; ++k)
        if ((1 << k) == n_elem) lg_e = k;
#define BBT_UNPACK_B(G_, B_)                                                                       \
    hipLaunchKernelGGL((k_unpack<G_, B_>), grid, dim3(256), 0, (hipStream_t)stream,                \
                       (const unsigned char*)raw_dev, (float*)out_dev, frame_bytes, header_bytes,  \
                       bits, samples_per_frame, n_thread, n_elem, code, (const unsigned char*)valid_dev, lg_e)
#define BBT_UNPACK(G_)                                  \
    switch (bits) {                                     \
        case 1: BBT_UNPACK_B(G_, 1); break;             \
        case 2: BBT_UNPACK_B(G_, 2); break;             \
        case 4: BBT_UNPACK_B(G_, 4); break;             \
        case 8: BBT_UNPACK_B(G_, 8); break;             \
        default: BBT_UNPACK_B(G_, 0); break;            \
    }
    if (g == 4) { BBT_UNPACK(4) }
    else if (g == 2) { BBT_UNPACK(2) }
    else { BBT_UNPACK(1) }
#undef BBT_UNPACK_B
#undef BBT_UNPACK
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// float32 / complex64 -> coded words and binary16 (pack_kernels.hpp): the encoders of the compact
// HDF5 payloads.  Decoding coded words is bbt_unpack with header_bytes = 0.
#define BBT_PACK_MAX (1ll << 40)
static bool aligned16(const void* a, const void* b) {
    return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;
}
extern "C" int bbt_pack(const void* in_dev, void* out_dev, int64_t n_comp, int bits, int code,
                        bbt_stream stream) {
    ARG_TRY(in_dev && out_dev, "bbt_pack: null argument");
    ARG_TRY(code == 0, "bbt_pack: code must be 0 (VDIF levels)");
    ARG_TRY(bits == 1 || bits == 2 || bits == 4 || bits == 8 || bits == 16,
            "bbt_pack: %d bits per component are not supported", bits);
    ARG_TRY(n_comp >= 0 && n_comp <= BBT_PACK_MAX, "bbt_pack: %lld components (0 .. 2^40)", (long long)n_comp);
    ARG_TRY((((uintptr_t)in_dev | (uintptr_t)out_dev) & 3u) == 0, "bbt_pack: pointers must be 4-byte aligned");
    if (n_comp == 0) return 0;
    const long long per = 32 / bits, n_words = (n_comp + per - 1) / per;
    const bool vec = aligned16(in_dev, out_dev);
#define BBT_PACK_V(B_, W_, V_)                                                                          \
    hipLaunchKernelGGL((k_pack<B_, W_, V_>),                                                            \
                       dim3((unsigned)((n_words + (long long)BBT_PACK_THREADS * W_ - 1) /              \
                                       ((long long)BBT_PACK_THREADS * W_))),                            \
                       dim3(BBT_PACK_THREADS), 0, (hipStream_t)stream, (const float*)in_dev,            \
                       (unsigned*)out_dev, (long long)n_comp, n_words)
#define BBT_PACK(B_, W_)                        \
    do {                                        \
        if (vec) BBT_PACK_V(B_, W_, true);      \
        else BBT_PACK_V(B_, W_, false);         \
    } while (0)
    switch (bits) {                 // (words per thread: see pack_kernels.hpp)
        case 1: BBT_PACK(1, 1); break;
        case 2: BBT_PACK(2, 1); break;
        case 4: BBT_PACK(4, 2); break;
        case 8: BBT_PACK(8, 4); break;
        default: BBT_PACK(16, 4); break;
    }
#undef BBT_PACK
#undef BBT_PACK_V
    HIP_TRY(hipGetLastError());
    return 0;
}

static int half_launch(const void* in_dev, void* out_dev, int64_t n, bool to_half, bbt_stream stream,
                       const char* who) {
    ARG_TRY(in_dev && out_dev, "%s: null argument", who);
    ARG_TRY(n >= 0 && n <= BBT_PACK_MAX, "%s: %lld values (0 .. 2^40)", who, (long long)n);
    const uintptr_t f = (uintptr_t)(to_half ? in_dev : (const void*)out_dev);
    const uintptr_t h = (uintptr_t)(to_half ? (const void*)out_dev : in_dev);
    ARG_TRY((f & 3u) == 0 && (h & 1u) == 0, "%s: pointers must be aligned to their elements", who);
    if (n == 0) return 0;
    const long long per_block = (long long)BBT_PACK_THREADS * BBT_HALF_PER;
    const dim3 grid((unsigned)((n + per_block - 1) / per_block));
    const bool vec = aligned16(in_dev, out_dev);
    if (to_half) {
        if (vec)
            hipLaunchKernelGGL((k_to_half<true>), grid, dim3(BBT_PACK_THREADS), 0, (hipStream_t)stream,
                               (const float*)in_dev, (unsigned short*)out_dev, (long long)n);
        else
            hipLaunchKernelGGL((k_to_half<false>), grid, dim3(BBT_PACK_THREADS), 0, (hipStream_t)stream,
                               (const float*)in_dev, (unsigned short*)out_dev, (long long)n);
    } else {
        if (vec)
            hipLaunchKernelGGL((k_from_half<true>), grid, dim3(BBT_PACK_THREADS), 0, (hipStream_t)stream,
                               (const unsigned short*)in_dev, (float*)out_dev, (long long)n);
        else
            hipLaunchKernelGGL((k_from_half<false>), grid, dim3(BBT_PACK_THREADS), 0, (hipStream_t)stream,
                               (const unsigned short*)in_dev, (float*)out_dev, (long long)n);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
extern "C" int bbt_to_half(const void* in_dev, void* out_dev, int64_t n, bbt_stream stream) {
    return half_launch(in_dev, out_dev, n, true, stream, "bbt_to_half");
}
extern "C" int bbt_from_half(const void* in_dev, void* out_dev, int64_t n, bbt_stream stream) {
    return half_launch(in_dev, out_dev, n, false, stream, "bbt_from_half");
}

// ---------------------------------------------------------------------------
// PSRFITS fold-mode rows (psrfits_kernels.hpp): float32 profiles (row, bin, chan, pol) <-> big-endian
// int16 codes (row, pol, chan, bin) with a scale and an offset per (row, pol, chan).  The tiling is
// psrfits_geo.hpp's; `x_dev` is the array of floats, read or written.
static int psrfits_shape(const char* who, int64_t n_row, int64_t n_bin, int64_t n_chan, int64_t n_pol,
                         const void* x_dev, const void* codes_dev, PsrFitsGeo* g) {
    ARG_TRY(n_row >= 0 && n_bin >= 1 && n_chan >= 1 && n_pol >= 1,
            "%s: %lld rows of %lld bins, %lld channels, %lld polarizations", who, (long long)n_row,
            (long long)n_bin, (long long)n_chan, (long long)n_pol);
    ARG_TRY(n_chan < (1ll << 31) && n_pol < (1ll << 31) && n_chan * n_pol < (1ll << 31) && n_bin < (1ll << 31),
            "%s: an axis of 2^31 or more elements", who);
    ARG_TRY((double)n_row * (double)n_bin * (double)(n_chan * n_pol) <= (double)BBT_PACK_MAX,
            "%s: more than 2^40 samples", who);
    const char* bad = psrfits_geo(n_bin, n_chan, n_pol, ((uintptr_t)x_dev & 15u) == 0,
                                  ((uintptr_t)codes_dev & 3u) == 0, g);
    ARG_TRY(!bad, "%s: %s", who, bad ? bad : "");
    ARG_TRY(n_row * g->n_tile < (1ll << 31), "%s: too many tiles for one call", who);
    return 0;
}
extern "C" int bbt_psrfits_encode(const void* x_dev, void* codes_dev, void* scl_dev, void* offs_dev,
                                  void* n_finite_dev, int64_t n_row, int64_t n_bin, int64_t n_chan,
                                  int64_t n_pol, bbt_stream stream) {
    ARG_TRY(x_dev && codes_dev && scl_dev && offs_dev && n_finite_dev, "bbt_psrfits_encode: null argument");
    PsrFitsGeo g;
    if (psrfits_shape("bbt_psrfits_encode", n_row, n_bin, n_chan, n_pol, x_dev, codes_dev, &g)) return 1;
    ARG_TRY((((uintptr_t)x_dev | (uintptr_t)scl_dev | (uintptr_t)offs_dev | (uintptr_t)n_finite_dev) & 3u) == 0 &&
                ((uintptr_t)codes_dev & 1u) == 0,
            "bbt_psrfits_encode: pointers must be aligned to their elements");
    if (n_row == 0) return 0;
#define BBT_PSR_ENC(T_, V_)                                                                                   \
    hipLaunchKernelGGL((k_psrfits_encode<T_, V_>), dim3((unsigned)(n_row * g.n_tile)), dim3(BBT_PSRFITS_THREADS), \
                       0, (hipStream_t)stream, (const float*)x_dev, (unsigned short*)codes_dev,               \
                       (float*)scl_dev, (float*)offs_dev, (int*)n_finite_dev, (long long)n_bin,               \
                       (long long)n_chan, (long long)n_pol, g.n_tile)
    if (g.tc == 32) {
        if (g.vec) BBT_PSR_ENC(32, true);
        else BBT_PSR_ENC(32, false);
    } else {
        if (g.vec) BBT_PSR_ENC(4, true);
        else BBT_PSR_ENC(4, false);
    }
#undef BBT_PSR_ENC
    HIP_TRY(hipGetLastError());
    return 0;
}
extern "C" int bbt_psrfits_decode(const void* codes_dev, const void* scl_dev, const void* offs_dev,
                                  const void* wts_dev, float zero_off, void* out_dev, int64_t n_row,
                                  int64_t n_bin, int64_t n_chan, int64_t n_pol, bbt_stream stream) {
    ARG_TRY(codes_dev && scl_dev && offs_dev && out_dev, "bbt_psrfits_decode: null argument");
    PsrFitsGeo g;
    if (psrfits_shape("bbt_psrfits_decode", n_row, n_bin, n_chan, n_pol, out_dev, codes_dev, &g)) return 1;
    ARG_TRY((((uintptr_t)out_dev | (uintptr_t)scl_dev | (uintptr_t)offs_dev | (uintptr_t)wts_dev) & 3u) == 0 &&
                ((uintptr_t)codes_dev & 1u) == 0,
            "bbt_psrfits_decode: pointers must be aligned to their elements");
    ARG_TRY(zero_off == zero_off, "bbt_psrfits_decode: zero_off is not a number");
    if (n_row == 0) return 0;
#define BBT_PSR_DEC(T_, V_)                                                                                   \
    hipLaunchKernelGGL((k_psrfits_decode<T_, V_>), dim3((unsigned)(n_row * g.n_tile)), dim3(BBT_PSRFITS_THREADS), \
                       0, (hipStream_t)stream, (const unsigned short*)codes_dev, (const float*)scl_dev,       \
                       (const float*)offs_dev, (const float*)wts_dev, zero_off, (float*)out_dev,              \
                       (long long)n_bin, (long long)n_chan, (long long)n_pol, g.n_tile)
    if (g.tc == 32) {
        if (g.vec) BBT_PSR_DEC(32, true);
        else BBT_PSR_DEC(32, false);
    } else {
        if (g.vec) BBT_PSR_DEC(4, true);
        else BBT_PSR_DEC(4, false);
    }
#undef BBT_PSR_DEC
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// PSRFITS search-mode rows (psrsearch_kernels.hpp): float32 samples (row, sample, chan, pol) <->
// unsigned codes of 1, 2, 4 or 8 bits (row, sample, pol, chan), packed along the channels, with a
// scale and an offset per (row, pol, chan).  The tiling is psrsearch_geo.hpp's.
static int psrsearch_shape(const char* who, int64_t n_row, int64_t nsblk, int64_t n_chan, int64_t n_pol, int nbits,
                           const void* codes_dev, PsrSearchGeo* g) {
    ARG_TRY(n_row >= 0, "%s: %lld rows", who, (long long)n_row);
    const char* bad = psrsearch_geo(nsblk, n_chan, n_pol, nbits, ((uintptr_t)codes_dev & 3u) == 0, g);
    ARG_TRY(!bad, "%s: %s (%lld samples a row, %lld channels, %lld polarizations, %d bits)", who, bad ? bad : "",
            (long long)nsblk, (long long)n_chan, (long long)n_pol, nbits);
    ARG_TRY((double)n_row * (double)nsblk * (double)(n_chan * n_pol) <= (double)BBT_PACK_MAX,
            "%s: more than 2^40 samples", who);
    ARG_TRY(n_row * g->n_tile < (1ll << 31), "%s: too many tiles for one call", who);
    return 0;
}
#define BBT_PSRSEARCH_LAUNCH(K_, ...)                                                                       \
    do {                                                                                                    \
        const dim3 grid((unsigned)(n_row * g.n_tile)), block(BBT_PSRSEARCH_THREADS);                        \
        switch (nbits * 2 + g.vec) {                                                                        \
            case 2: hipLaunchKernelGGL((K_<1, false>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;  \
            case 3: hipLaunchKernelGGL((K_<1, true>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;   \
            case 4: hipLaunchKernelGGL((K_<2, false>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;  \
            case 5: hipLaunchKernelGGL((K_<2, true>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;   \
            case 8: hipLaunchKernelGGL((K_<4, false>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;  \
            case 9: hipLaunchKernelGGL((K_<4, true>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;   \
            case 16: hipLaunchKernelGGL((K_<8, false>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break; \
            default: hipLaunchKernelGGL((K_<8, true>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;  \
        }                                                                                                   \
    } while (0)
extern "C" int bbt_psrsearch_encode(const void* x_dev, void* codes_dev, void* scl_dev, void* offs_dev,
                                    void* n_finite_dev, int64_t n_row, int64_t nsblk, int64_t n_chan,
                                    int64_t n_pol, int nbits, double nsigma, bbt_stream stream) {
    ARG_TRY(x_dev && codes_dev && scl_dev && offs_dev && n_finite_dev, "bbt_psrsearch_encode: null argument");
    PsrSearchGeo g;
    if (psrsearch_shape("bbt_psrsearch_encode", n_row, nsblk, n_chan, n_pol, nbits, codes_dev, &g)) return 1;
    ARG_TRY((((uintptr_t)x_dev | (uintptr_t)scl_dev | (uintptr_t)offs_dev | (uintptr_t)n_finite_dev) & 3u) == 0,
            "bbt_psrsearch_encode: pointers must be aligned to their elements");
    ARG_TRY(nsigma > 0. && nsigma < HUGE_VAL, "bbt_psrsearch_encode: nsigma must be positive and finite");
    if (n_row == 0) return 0;
    BBT_PSRSEARCH_LAUNCH(k_psrsearch_encode, (const float*)x_dev, (unsigned char*)codes_dev, (float*)scl_dev,
                         (float*)offs_dev, (int*)n_finite_dev, (long long)nsblk, (long long)n_chan,
                         (long long)n_pol, nsigma, g);
    HIP_TRY(hipGetLastError());
    return 0;
}
extern "C" int bbt_psrsearch_decode(const void* codes_dev, const void* scl_dev, const void* offs_dev,
                                    const void* wts_dev, float zero_off, void* out_dev, int64_t n_row,
                                    int64_t nsblk, int64_t n_chan, int64_t n_pol, int nbits, bbt_stream stream) {
    ARG_TRY(codes_dev && scl_dev && offs_dev && out_dev, "bbt_psrsearch_decode: null argument");
    PsrSearchGeo g;
    if (psrsearch_shape("bbt_psrsearch_decode", n_row, nsblk, n_chan, n_pol, nbits, codes_dev, &g)) return 1;
    ARG_TRY((((uintptr_t)out_dev | (uintptr_t)scl_dev | (uintptr_t)offs_dev | (uintptr_t)wts_dev) & 3u) == 0,
            "bbt_psrsearch_decode: pointers must be aligned to their elements");
    ARG_TRY(zero_off == zero_off, "bbt_psrsearch_decode: zero_off is not a number");
    if (n_row == 0) return 0;
    BBT_PSRSEARCH_LAUNCH(k_psrsearch_decode, (const unsigned char*)codes_dev, (const float*)scl_dev,
                         (const float*)offs_dev, (const float*)wts_dev, zero_off, (float*)out_dev,
                         (long long)nsblk, (long long)n_chan, (long long)n_pol, g);
    HIP_TRY(hipGetLastError());
    return 0;
}
#undef BBT_PSRSEARCH_LAUNCH

// ---------------------------------------------------------------------------
// multi-GPU: one process per GPU, RCCL over xGMI.  The path
// has no data-path collective; these are the two it uses around it: the
// broadcast of the response (chirp) at plan time and the optional all-gather
// of the outputs.  librccl is loaded on first use (dlopen), so the library
// itself loads on hosts without it.
struct bbt_comm {
    ncclComm_t nccl = nullptr;
    int rank = 0, world = 1;
};
namespace {
struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclBroadcast) broadcast = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mutex;

int rccl_load() {
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.handle) return 0;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return fail("bbt_comm: cannot load librccl: %s", dlerror());
    RcclApi api;
    api.handle = h;
    api.get_unique_id = (decltype(api.get_unique_id))dlsym(h, "ncclGetUniqueId");
    api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(h, "ncclCommInitRank");
    api.comm_destroy = (decltype(api.comm_destroy))dlsym(h, "ncclCommDestroy");
    api.broadcast = (decltype(api.broadcast))dlsym(h, "ncclBroadcast");
    api.all_gather = (decltype(api.all_gather))dlsym(h, "ncclAllGather");
    api.error_string = (decltype(api.error_string))dlsym(h, "ncclGetErrorString");
    if (!api.get_unique_id || !api.comm_init_rank || !api.comm_destroy || !api.broadcast ||
        !api.all_gather || !api.error_string)
        return fail("bbt_comm: librccl lacks a required symbol");
    g_rccl = api;
    return 0;
}
}  // namespace

#define RCCL_TRY(expr)                                                                         \
    do {                                                                                       \
        ncclResult_t r_ = (expr);                                                              \
        if (r_ != ncclSuccess) return fail("%s failed: %s", #expr, g_rccl.error_string(r_));   \
    } while (0)

extern "C" {

int bbt_comm_unique_id(void* id_out, size_t id_bytes) {
    ARG_TRY(id_out && id_bytes >= sizeof(ncclUniqueId), "bbt_comm_unique_id: need a buffer of %zu bytes",
            sizeof(ncclUniqueId));
    if (rccl_load()) return 1;
    ncclUniqueId id;
    RCCL_TRY(g_rccl.get_unique_id(&id));
    memcpy(id_out, &id, sizeof id);
    return 0;
}

int bbt_comm_init(bbt_comm** comm, int n_ranks, int rank, const void* id, size_t id_bytes) {
    ARG_TRY(comm && id, "bbt_comm_init: null argument");
    *comm = nullptr;
    ARG_TRY(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "bbt_comm_init: rank %d of %d", rank, n_ranks);
    ARG_TRY(id_bytes >= sizeof(ncclUniqueId), "bbt_comm_init: the id must hold %zu bytes",
            sizeof(ncclUniqueId));
    if (rccl_load()) return 1;
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    bbt_comm* c = new bbt_comm;
    c->rank = rank;
    c->world = n_ranks;
    ncclResult_t r = g_rccl.comm_init_rank(&c->nccl, n_ranks, uid, rank);
    if (r != ncclSuccess) {
        delete c;
        return fail("ncclCommInitRank failed: %s", g_rccl.error_string(r));
    }
    *comm = c;
    return 0;
}

int bbt_comm_destroy(bbt_comm* comm) {
    if (!comm) return 0;
    if (comm->nccl) g_rccl.comm_destroy(comm->nccl);
    delete comm;
    return 0;
}

int bbt_bcast_chirp(bbt_comm* comm, void* resp_dev, int64_t n_complex, int root, bbt_stream stream) {
    ARG_TRY(comm && resp_dev, "bbt_bcast_chirp: null argument");
    ARG_TRY(n_complex >= 0 && root >= 0 && root < comm->world, "bbt_bcast_chirp: bad count or root");
    if (n_complex == 0) return 0;
    RCCL_TRY(g_rccl.broadcast(resp_dev, resp_dev, (size_t)n_complex * 2, ncclFloat32, root, comm->nccl,
                              (hipStream_t)stream));
    return 0;
}

int bbt_gather_output(bbt_comm* comm, const void* send_dev, void* recv_dev, int64_t bytes_per_rank,
                      bbt_stream stream) {
    ARG_TRY(comm && send_dev && recv_dev, "bbt_gather_output: null argument");
    ARG_TRY(bytes_per_rank >= 0, "bbt_gather_output: negative size");
    if (bytes_per_rank == 0) return 0;
    if (bytes_per_rank % 4 == 0)
        RCCL_TRY(g_rccl.all_gather(send_dev, recv_dev, (size_t)bytes_per_rank / 4, ncclFloat32,
                                   comm->nccl, (hipStream_t)stream));
    else
        RCCL_TRY(g_rccl.all_gather(send_dev, recv_dev, (size_t)bytes_per_rank, ncclUint8, comm->nccl,
                                   (hipStream_t)stream));
    return 0;
}

}  // extern "C"
