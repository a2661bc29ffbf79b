// The engine's caching device allocator, the device-to-device copy kernels and the MHE_ALLOC_TRACE
// debugging aid.
#pragma once

// process-wide counts for mhe_alloc_stats: allocations that succeeded only after the cache was
// released, and allocations that failed (including injected ones)
static std::atomic<unsigned long long> g_alloc_retries{ 0 }, g_alloc_failures{ 0 };

// Stream-ordered allocation for the engine's transient buffers (every Ciphertext temporary of the
// SEAL surface).  The runtime's stream-ordered pool (hipMallocAsync/hipFreeAsync) was observed on
// this image to hand out memory that was still live: bootstrapping's cached plaintexts and guard
// regions were overwritten even with kernels serialised, and disappeared with plain hipMalloc.
// So the engine keeps its own cache: a freed block records an event on the freeing stream and goes
// to a free list by size; an allocation reuses a block of the same rounded size (waiting on its
// event when it comes from another stream) or calls hipMalloc.  Memory is returned to the device
// only when hipMalloc fails (then every cached block is released and the call retried).
namespace
{
struct CachedBlock
{
    void *p;
    size_t size;
    hipStream_t st;
    hipEvent_t ev;
};
struct DevAlloc
{
    std::mutex mu;
    std::map<void *, size_t> live;
    std::multimap<size_t, CachedBlock> free_blocks;
    std::vector<hipEvent_t> ev_pool;
    size_t cached = 0, in_use = 0;
    int contexts = 0; // live engine contexts on this device: the cache is returned when the last goes
};
DevAlloc &dev_alloc()
{
    static DevAlloc a[64];
    int d = 0;
    (void)hipGetDevice(&d);
    return a[d & 63];
}
size_t round_size(size_t b)
{
    if (b == 0) b = 1;
    if (b < ((size_t)1 << 20)) return (b + 4095) & ~(size_t)4095;
    return (b + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
}
void release_cached(DevAlloc &a)
{
    // caller holds a.mu
    (void)hipDeviceSynchronize();
    for (auto &kv : a.free_blocks)
    {
        (void)hipFree(kv.second.p);
        a.ev_pool.push_back(kv.second.ev);
    }
    a.free_blocks.clear();
    a.cached = 0;
}
} // namespace

static void release_cached_blocks()
{
    DevAlloc &a = dev_alloc();
    std::lock_guard<std::mutex> g(a.mu);
    release_cached(a);
}

// context lifetime on the current device (mhe_ctx_create / mhe_ctx_destroy): when the last context
// of a device goes, its cached blocks go back to the device, so another process (or a later
// engine) on the same GPU gets that memory
extern "C" __attribute__((visibility("hidden"))) void mhe_internal_ctx_count(int delta)
{
    DevAlloc &a = dev_alloc();
    std::lock_guard<std::mutex> g(a.mu);
    a.contexts += delta;
    if (a.contexts <= 0)
    {
        a.contexts = 0;
        release_cached(a);
    }
}

extern "C" __attribute__((visibility("hidden"))) hipError_t mhe_internal_alloc(void **p, size_t bytes, hipStream_t st)
{
    DevAlloc &a = dev_alloc();
    const size_t sz = round_size(bytes);
    std::lock_guard<std::mutex> g(a.mu);
    auto it = a.free_blocks.lower_bound(sz);
    auto best = a.free_blocks.end();
    for (auto j = it; j != a.free_blocks.end() && j->first <= sz + sz / 4; ++j)
        if (best == a.free_blocks.end() || j->second.st == st)
        {
            best = j;
            if (j->second.st == st) break;
        }
    if (best != a.free_blocks.end())
    {
        CachedBlock b = best->second;
        a.free_blocks.erase(best);
        a.cached -= b.size;
        if (b.st != st)
        {
            hipError_t e = hipStreamWaitEvent(st, b.ev, 0);
            if (e != hipSuccess) return e;
        }
        a.ev_pool.push_back(b.ev);
        a.live[b.p] = b.size;
        a.in_use += b.size;
        *p = b.p;
        return hipSuccess;
    }
    hipError_t e = hipMalloc(p, sz);
    if (e != hipSuccess)
    {
        (void)hipGetLastError();
        release_cached(a);
        e = hipMalloc(p, sz);
        if (e != hipSuccess)
        {
            g_alloc_failures.fetch_add(1);
            return e;
        }
        g_alloc_retries.fetch_add(1);
    }
    a.live[*p] = sz;
    a.in_use += sz;
    return hipSuccess;
}

extern "C" __attribute__((visibility("hidden"))) hipError_t mhe_internal_free(void *p, hipStream_t st)
{
    if (!p) return hipSuccess;
    DevAlloc &a = dev_alloc();
    std::lock_guard<std::mutex> g(a.mu);
    auto it = a.live.find(p);
    if (it == a.live.end()) return hipErrorInvalidValue;
    const size_t sz = it->second;
    a.live.erase(it);
    a.in_use -= sz;
    hipEvent_t ev = nullptr;
    if (!a.ev_pool.empty())
    {
        ev = a.ev_pool.back();
        a.ev_pool.pop_back();
    }
    else
    {
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipEventRecord(ev, st);
    if (e != hipSuccess) return e;
    a.free_blocks.emplace(sz, CachedBlock{ p, sz, st, ev });
    a.cached += sz;
    return hipSuccess;
}

// Device-to-device copies run as a kernel on the caller's stream (ordered with the stream's other
// kernels by construction, at HBM speed) rather than hipMemcpyAsync's copy engines.
__global__ void k_copy16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

__global__ void k_copy8(u64 *__restrict__ dst, const u64 *__restrict__ src, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

extern "C" __attribute__((visibility("hidden"))) hipError_t mhe_internal_copy_d2d(void *dst, const void *src,
                                                                                  size_t bytes, hipStream_t st)
{
    if (!bytes || dst == src) return hipSuccess;
    const uintptr_t a = (uintptr_t)dst | (uintptr_t)src;
    if ((a & 15) == 0 && (bytes & 15) == 0)
    {
        const size_t cnt = bytes / 16;
        const unsigned grid = (unsigned)std::min<size_t>((cnt + 255) / 256, 4096);
        hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, st, (uint4 *)dst, (const uint4 *)src, cnt);
        return hipGetLastError();
    }
    if ((a & 7) == 0 && (bytes & 7) == 0)
    {
        const size_t cnt = bytes / 8;
        const unsigned grid = (unsigned)std::min<size_t>((cnt + 255) / 256, 4096);
        hipLaunchKernelGGL(k_copy8, dim3(grid), dim3(256), 0, st, (u64 *)dst, (const u64 *)src, cnt);
        return hipGetLastError();
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
}

// ------------------------------------------------------------------------ MHE_ALLOC_TRACE
// MHE_ALLOC_TRACE=1: track live stream-ordered allocations and report double frees, frees of
// unknown pointers and overlapping live ranges (debugging aid)
static std::mutex g_trace_mu;
static std::map<uintptr_t, size_t> g_live;
static int trace_on()
{
    static int on = -1;
    if (on < 0)
    {
        const char *e = getenv("MHE_ALLOC_TRACE");
        on = e && e[0] >= '1';
    }
    return on;
}

// trace mode: the range [p, p + words) must lie inside one live stream-ordered allocation
static void trace_range(const char *fn, const char *what, const void *p, size_t words)
{
    if (!trace_on() || !p) return;
    std::lock_guard<std::mutex> g(g_trace_mu);
    const uintptr_t a = (uintptr_t)p, e = a + words * 8;
    auto it = g_live.upper_bound(a);
    if (it == g_live.begin()) return; // not a tracked allocation (workspace, hipMalloc)
    --it;
    if (it->first + it->second < a) return;
    if (e > it->first + it->second)
        fprintf(stderr, "[alloc-trace] %s: %s range [%p, +%zu words) exceeds allocation %p of %zu words by %zu words\n",
                fn, what, p, words, (void *)it->first, it->second / 8, (size_t)(e - (it->first + it->second)) / 8);
}
// trace level 2: at every instrumented entry, synchronise and check the first 4 KiB of every live
// allocation's guard; a hit names the previous instrumented call as the writer
static const char *g_prev_fn = "(none)";
static size_t g_prev_info[4];
static void trace_check_all(const char *fn, size_t i0, size_t i1, size_t i2, size_t i3)
{
    static int lvl = -1;
    if (lvl < 0)
    {
        const char *e = getenv("MHE_ALLOC_TRACE");
        lvl = e ? atoi(e) : 0;
    }
    if (lvl < 2) return;
    (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> g(g_trace_mu);
    std::vector<unsigned char> buf(4096);
    for (auto &kv : g_live)
    {
        (void)hipMemcpy(buf.data(), (const char *)kv.first + kv.second, 4096, hipMemcpyDeviceToHost);
        bool bad = false;
        for (unsigned char b : buf) bad |= b != 0xAB;
        if (bad)
        {
            fprintf(stderr, "[alloc-trace] guard of %#lx (%zu words) hit before %s; previous call %s(%zu, %zu, %zu, %zu)\n",
                    (unsigned long)kv.first, kv.second / 8, fn, g_prev_fn, g_prev_info[0], g_prev_info[1],
                    g_prev_info[2], g_prev_info[3]);
            (void)hipMemset((char *)kv.first + kv.second, 0xAB, (size_t)16 << 20); // re-arm
        }
    }
    g_prev_fn = fn;
    g_prev_info[0] = i0;
    g_prev_info[1] = i1;
    g_prev_info[2] = i2;
    g_prev_info[3] = i3;
}
#define TRC(a, b, cc, d) trace_check_all(__func__, (size_t)(a), (size_t)(b), (size_t)(cc), (size_t)(d))
