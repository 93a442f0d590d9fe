// runtime.cpp — device life-cycle, streams, memory and error plumbing of libsvtav1_hip.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "common.hpp"

namespace svthip {

// Process state: one device per process, one pool of streams for the threads that pass stream == NULL.
#ifndef SVT_HIP_STREAM_POOL
#define SVT_HIP_STREAM_POOL 8
#endif
namespace {
constexpr int STREAM_POOL = SVT_HIP_STREAM_POOL;
struct Process {
    std::atomic<int> device{-1};  // the device every entry point works on; -1 until svt_hip_init succeeds
    std::atomic<int> sticky{-1};  // first device ever bound: streams / per-thread buffers / once-uploaded tables live there
    std::atomic<int> cus{0};
    std::mutex       mutex;       // svt_hip_init / svt_hip_shutdown
    // The "calling thread's private stream" (stream == NULL in the API): a host such as the encoder has dozens of worker threads, and
    // creating a HIP stream costs milliseconds (a hardware queue) -- 25 ms per first call of a thread inside the patched encoder.
    // Threads draw from a small pool instead: thread k uses stream k mod POOL.  Two threads that share a stream only wait for each
    // other's work in svt_hip_stream_sync; order inside one thread is kept, which is all the API promises.  Entries are created under
    // pool_mutex (by svt_hip_init, or on demand) and published with release / read with acquire.
    std::atomic<hipStream_t> pool[STREAM_POOL];
    std::mutex               pool_mutex;
    std::atomic<int>         next_thread{0};
};
Process g;
}  // namespace

ThreadState &tls() {
    static thread_local ThreadState t;
    return t;
}

void set_error(const char *fmt, ...) {
    ThreadState &t = tls();
    va_list      ap;
    va_start(ap, fmt);
    vsnprintf(t.err, sizeof(t.err), fmt, ap);
    va_end(ap);
}
int32_t refuse(const char *fmt, ...) {
    ThreadState &t = tls();
    va_list      ap;
    va_start(ap, fmt);
    vsnprintf(t.err, sizeof(t.err), fmt, ap);
    va_end(ap);
    return SVT_HIP_ERR_BAD_PARAMETER;
}

bool ensure_init() {
    const int dev = g.device.load();
    if (dev >= 0) {
        // each host thread must select the device once
        ThreadState &t = tls();
        if (!t.bound) {
            if (hipSetDevice(dev) != hipSuccess)
                return false;
            t.bound = true;
        }
        return true;
    }
    // not initialised (or shut down): never pick a device silently — a rank that forgot svt_hip_init(local_rank) would
    // otherwise run on GPU 0
    set_error("library not initialised: call svt_hip_init(device_ordinal) first");
    return false;
}
int cu_count() { return g.cus.load(std::memory_order_relaxed); }

namespace {
WarmupFn g_warmups[64];
int      g_n_warmups = 0;
}  // namespace
WarmupRegistrar::WarmupRegistrar(WarmupFn fn) {
    if (g_n_warmups < 64)
        g_warmups[g_n_warmups++] = fn;
}
void run_module_warmups(hipStream_t st) {
    for (int i = 0; i < g_n_warmups; i++) g_warmups[i](st);
}

hipStream_t resolve_stream(void *stream) {
    if (stream)
        return (hipStream_t)stream;
    ThreadState &t = tls();
    if (t.slot < 0)
        t.slot = g.next_thread.fetch_add(1) % STREAM_POOL;
    hipStream_t s = g.pool[t.slot].load(std::memory_order_acquire);
    if (!s) {
        std::lock_guard<std::mutex> lk(g.pool_mutex);
        s = g.pool[t.slot].load(std::memory_order_relaxed);
        if (!s) {
            // streams belong to the device that is current when they are created: bind this thread first
            (void)ensure_init();
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
                set_error("cannot create a stream for the calling thread");
                return nullptr;  // the legacy default stream: callers carry on, correct but serialised
            }
            g.pool[t.slot].store(s, std::memory_order_release);
        }
    }
    return s;
}

hipError_t ensure_event(hipEvent_t &ev) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }

hipError_t GuardedBuf::acquire(size_t bytes, size_t grow_to, bool host_writes, hipStream_t st, const char **what) {
    hipError_t e;
    *what = "hipEventCreate";
    if ((e = ensure_event(ev)) != hipSuccess)
        return e;
    const bool grow = bytes > cap;
    if (pending && (host_writes || grow)) {
        *what = "hipEventSynchronize";
        if ((e = hipEventSynchronize(ev)) != hipSuccess)
            return e;
        pending = false;
    } else if (pending) {
        *what = "hipStreamWaitEvent";
        if ((e = hipStreamWaitEvent(st, ev, 0)) != hipSuccess)
            return e;
    }
    if (grow) {  // nothing in flight refers to it any more
        if (dev)
            (void)hipFree(dev);
        if (pinned)
            (void)hipHostFree(pinned);
        dev = pinned = nullptr, cap = 0;
        *what = "hipMalloc";
        if ((e = hipMalloc((void **)&dev, grow_to)) != hipSuccess)
            return dev = nullptr, e;
        *what = "hipHostMalloc";
        if (host_writes && (e = hipHostMalloc((void **)&pinned, grow_to, hipHostMallocDefault)) != hipSuccess) {
            (void)hipFree(dev);
            return dev = pinned = nullptr, e;
        }
        cap = grow_to;
    }
    return hipSuccess;
}
hipError_t GuardedBuf::release(hipStream_t st) {
    hipError_t e = hipEventRecord(ev, st);
    if (e == hipSuccess)
        pending = true;
    else  // the event cannot guard the buffer: let its user finish now
        (void)hipStreamSynchronize(st);
    return e;
}

TierBCall::TierBCall(const char *fn, void *stream) : fn_(fn) {
    if (!ensure_init())
        status_ = SVT_HIP_ERR_NO_DEVICE;
    else
        st_ = resolve_stream(stream);
}
void *TierBCall::fail(hipError_t e, const char *what) {
    if (ok())  // the first failure is the one reported
        set_error("%s: %s: %s", fn_, what, hipGetErrorString(e));
    status_ = SVT_HIP_ERR_RUNTIME;
    return nullptr;
}
bool TierBCall::hold(GuardedBuf &b, size_t bytes, size_t grow_to, bool host_writes) {
    if (!ok())
        return false;
    if (b.held)
        return fail(hipErrorInvalidValue, "buffer still held by an enclosing call") != nullptr;
    const char      *what;
    const hipError_t e = b.acquire(bytes, grow_to, host_writes, st_, &what);
    if (e != hipSuccess)
        return fail(e, what) != nullptr;
    b.held = true, held_[n_held_++] = &b;
    return true;
}
void *TierBCall::stage(const void *host, size_t bytes) {
    ThreadState &t = tls();
    GuardedBuf  &s = t.ring[t.ring_next];
    if (!hold(s, bytes, bytes < 65536 ? 65536 : bytes * 2, true))
        return nullptr;
    t.ring_next = (t.ring_next + 1) % 4;
    memcpy(s.pinned, host, bytes);
    const hipError_t e = hipMemcpyAsync(s.dev, s.pinned, bytes, hipMemcpyHostToDevice, st_);
    return e == hipSuccess ? s.dev : fail(e, "hipMemcpyAsync");
}
void *TierBCall::take(GuardedBuf &b, size_t bytes, size_t grow_to) {
    ThreadState &t = tls();
    if (&b == &t.txfm_perm)  // whoever takes it may grow or overwrite it: the last transform batch's counters are gone
        t.txfm_fast_stream = nullptr, t.txfm_fast_hdr = nullptr;
    return hold(b, bytes, grow_to, false) ? b.dev : nullptr;
}
void TierBCall::release() {
    for (int i = 0; i < n_held_; i++) {
        const hipError_t e = held_[i]->release(st_);
        if (e != hipSuccess)
            fail(e, "hipEventRecord");
        held_[i]->held = false;
    }
    n_held_ = 0;
}
bool TierBCall::check(hipError_t e, const char *what) {
    if (e != hipSuccess)
        fail(e, what);
    return ok();
}
int32_t TierBCall::finish() {
    const hipError_t e = ok() ? hipGetLastError() : hipSuccess;
    if (e != hipSuccess)
        fail(e, "launch");
    release();
    return status_;
}

// ---- Tier A failure handling (common.hpp) ----
namespace {
struct SavedSlot {
    char   name[96];
    void **slot;
    void  *cpu_fn;
};
std::mutex        g_slots_mutex;
SavedSlot         g_slots[512];
int               g_n_slots = 0;
std::atomic<bool> g_tier_a_broken{false};
std::atomic<int>  g_inject{-1};  // test hook: the n-th SVT_HIP_CHECK_FATAL from now fails (svt_hip_debug_inject_failure)
}  // namespace

[[noreturn]] void tier_a_throw(const char *fmt, ...) {
    TierAError e;
    va_list    ap;
    va_start(ap, fmt);
    vsnprintf(e.what, sizeof(e.what), fmt, ap);
    va_end(ap);
    throw e;
}
bool tier_a_broken() { return g_tier_a_broken.load(std::memory_order_relaxed); }
void tier_a_fail(const char *leaf, const char *what) {
    std::lock_guard<std::mutex> lk(g_slots_mutex);
    if (g_tier_a_broken.exchange(true))
        return;
    int restored = 0;
    for (int i = 0; i < g_n_slots; i++)
        if (g_slots[i].slot && g_slots[i].cpu_fn)
            *g_slots[i].slot = g_slots[i].cpu_fn, restored++;
    fprintf(stderr, "libsvtav1_hip: %s: %s -- HIP hot path disabled, %d RTCD pointers restored to the CPU kernels\n", leaf, what,
            restored);
}
void *tier_a_cpu(const char *leaf) {
    {
        std::lock_guard<std::mutex> lk(g_slots_mutex);
        for (int i = 0; i < g_n_slots; i++)
            if (strcmp(g_slots[i].name, leaf) == 0 && g_slots[i].cpu_fn)
                return g_slots[i].cpu_fn;
    }
    fprintf(stderr, "libsvtav1_hip fatal: %s_hip failed and no CPU function was saved for it (svt_hip_install_rtcd was not used): %s\n",
            leaf, svt_hip_last_error());
    abort();
}
static void remember_slot(const char *stem, void **slot, void *cpu_fn) {
    std::lock_guard<std::mutex> lk(g_slots_mutex);
    for (int i = 0; i < g_n_slots; i++)
        if (strcmp(g_slots[i].name, stem) == 0) {
            g_slots[i].slot = slot, g_slots[i].cpu_fn = cpu_fn;
            return;
        }
    if (g_n_slots < (int)(sizeof(g_slots) / sizeof(g_slots[0]))) {
        snprintf(g_slots[g_n_slots].name, sizeof(g_slots[g_n_slots].name), "%s", stem);
        g_slots[g_n_slots].slot = slot, g_slots[g_n_slots].cpu_fn = cpu_fn;
        g_n_slots++;
    }
}
bool tier_a_inject_now() {
    int v = g_inject.load();
    while (v >= 0) {
        if (g_inject.compare_exchange_weak(v, v - 1))
            return v == 0;
    }
    return false;
}

uint8_t *Scratch::device(size_t bytes) {
    if (bytes > dev_cap) {
        if (dev)
            (void)hipFree(dev);
        size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes * 2;
        if (tier_a_inject_now() || hipMalloc((void **)&dev, cap + 256) != hipSuccess) {
            dev = nullptr, dev_cap = 0;
            tier_a_throw("hipMalloc(%zu) for the Tier A scratch buffer failed", cap);
        }
        dev_cap = cap;
    }
    return dev;
}
uint8_t *Scratch::host(size_t bytes, size_t keep) {
    if (bytes > pinned_cap) {
        size_t   cap   = bytes < (1u << 20) ? (1u << 20) : bytes * 2;
        uint8_t *grown = nullptr;
        if (hipHostMalloc((void **)&grown, cap + 256, hipHostMallocDefault) != hipSuccess)
            tier_a_throw("hipHostMalloc(%zu) for the Tier A scratch buffer failed", cap);
        if (pinned) {
            memcpy(grown, pinned, keep);
            (void)hipHostFree(pinned);
        }
        pinned = grown, pinned_cap = cap;
    }
    return pinned;
}
[[noreturn]] void fatal(const char *what) { tier_a_throw("%s: %s", what, svt_hip_last_error()); }

TierAStage::TierAStage(const char *leaf, bool ready) {
    if (!ready)
        fatal(leaf);
    st_ = resolve_stream(nullptr);
}
size_t TierAStage::reserve(size_t bytes) {
    if (d_)
        tier_a_throw("Tier A staging: region reserved after the device buffer was sized");
    const size_t off = used_;
    used_ += up256(bytes);
    h_ = tls().scratch.host(used_ + 256, off);
    return off;
}
size_t TierAStage::in(const void *src, size_t bytes, size_t slack) {
    const size_t off = reserve(bytes + slack);
    if (src)
        memcpy(h_ + off, src, bytes);
    in_end_ = off + bytes;
    return off;
}
size_t TierAStage::in_rows(const void *src, size_t src_pitch, size_t rows, size_t row_bytes) {
    const size_t off = in(nullptr, rows * row_bytes);
    copy_rows(h_ + off, row_bytes, src, src_pitch, rows, row_bytes);
    return off;
}
uint8_t *TierAStage::device() {
    if (!d_)
        d_ = tls().scratch.device(used_ + 256);
    return d_;
}
void TierAStage::h2d(size_t off, size_t bytes) {
    SVT_HIP_CHECK_FATAL(hipMemcpyAsync(device() + off, h_ + off, bytes, hipMemcpyHostToDevice, st_));
}
void TierAStage::finish(size_t off, size_t bytes, size_t off2, size_t bytes2) {
    SVT_HIP_CHECK_FATAL(hipGetLastError());
    SVT_HIP_CHECK_FATAL(hipMemcpyAsync(h_ + off, device() + off, bytes, hipMemcpyDeviceToHost, st_));
    if (bytes2)
        SVT_HIP_CHECK_FATAL(hipMemcpyAsync(h_ + off2, d_ + off2, bytes2, hipMemcpyDeviceToHost, st_));
    SVT_HIP_CHECK_FATAL(hipStreamSynchronize(st_));
}

}  // namespace svthip

using namespace svthip;

extern "C" {

int32_t svt_hip_compute_units(void) { return cu_count(); }

int32_t svt_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int32_t svt_hip_init(int32_t device_ordinal) {
    std::lock_guard<std::mutex> lk(g.mutex);
    int                         n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device visible");
        return SVT_HIP_ERR_NO_DEVICE;
    }
    if (device_ordinal < 0 || device_ordinal >= n)
        return refuse("device ordinal %d out of range (%d devices)", device_ordinal, n);
    // per-thread streams, scratch buffers and the once-uploaded constant tables stay on the first device: one process
    // = one GPU (the multi-GPU layout is one process per GPU)
    if (g.sticky.load() >= 0 && g.sticky.load() != device_ordinal)
        return refuse("already bound to device %d: one process drives one GPU", g.sticky.load());
    SVT_HIP_CHECK(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    SVT_HIP_CHECK(hipGetDeviceProperties(&prop, device_ordinal));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library is built for gfx950 (MI355X) only", device_ordinal,
                  prop.gcnArchName);
        return SVT_HIP_ERR_NO_DEVICE;
    }
    g.cus.store(prop.multiProcessorCount);
    if (g.sticky.load() < 0) {  // load every translation unit's code object now instead of inside the first calls of the host's worker
                                // threads, and create the stream pool here: a worker thread's first call created its slot's stream under
                                // the pool lock, and the six picture-analysis threads of the encoder, all starting at once, paid 16 ms each
        {
            std::lock_guard<std::mutex> pk(g.pool_mutex);
            for (int i = 0; i < STREAM_POOL; i++) {
                hipStream_t s = nullptr;
                if (!g.pool[i].load(std::memory_order_relaxed) && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess)
                    g.pool[i].store(s, std::memory_order_release);  // a slot that stays empty is created on demand by resolve_stream
            }
        }
        run_module_warmups(nullptr);
        SVT_HIP_CHECK(hipDeviceSynchronize());  // a failed warm-up leaves the library uninitialised: the next svt_hip_init repeats it
    }
    g.sticky.store(device_ordinal);
    g.device.store(device_ordinal);
    return SVT_HIP_OK;
}

void svt_hip_shutdown(void) {
    std::lock_guard<std::mutex> lk(g.mutex);
    g.device.store(-1);
}

const char *svt_hip_last_error(void) { return tls().err; }
const char *svt_hip_version(void) { return "svtav1-hip 0.1 (gfx950)"; }

int32_t svt_hip_malloc(void **dptr, size_t bytes) {
    if (!dptr)
        return SVT_HIP_ERR_BAD_PARAMETER;
    if (!ensure_init())
        return SVT_HIP_ERR_NO_DEVICE;
    // +256 B beyond what was asked for: a defensive margin, not part of any contract (the documented contracts — e.g. the
    // plane contract of include/svt_hip_me.h — hold for caller-allocated memory of the exact size)
    SVT_HIP_CHECK(hipMalloc(dptr, bytes + 256));
    return SVT_HIP_OK;
}
int32_t svt_hip_free(void *dptr) {
    SVT_HIP_CHECK(hipFree(dptr));
    return SVT_HIP_OK;
}
int32_t svt_hip_memset(void *dptr, int value, size_t bytes, void *stream) {
    TierBCall c("svt_hip_memset", stream);
    if (!c.ok())
        return c.status();
    c.check(hipMemsetAsync(dptr, value, bytes, c.stream()), "hipMemsetAsync");
    return c.finish();
}
int32_t svt_hip_upload(void *dptr, const void *hptr, size_t bytes, void *stream) {
    TierBCall c("svt_hip_upload", stream);
    if (!c.ok())
        return c.status();
    c.check(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, c.stream()), "hipMemcpyAsync");
    return c.finish();
}
int32_t svt_hip_download(void *hptr, const void *dptr, size_t bytes, void *stream) {
    TierBCall c("svt_hip_download", stream);
    if (!c.ok())
        return c.status();
    c.check(hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, c.stream()), "hipMemcpyAsync");
    return c.finish();
}
int32_t svt_hip_upload_2d(void *dptr, size_t dpitch, const void *hptr, size_t hpitch, size_t width_bytes,
                          size_t height, void *stream) {
    TierBCall c("svt_hip_upload_2d", stream);
    if (!c.ok())
        return c.status();
    c.check(hipMemcpy2DAsync(dptr, dpitch, hptr, hpitch, width_bytes, height, hipMemcpyHostToDevice,
                                   c.stream()), "hipMemcpy2DAsync");
    return c.finish();
}
int32_t svt_hip_download_2d(void *hptr, size_t hpitch, const void *dptr, size_t dpitch, size_t width_bytes, size_t height,
                            void *stream) {
    TierBCall c("svt_hip_download_2d", stream);
    if (!c.ok())
        return c.status();
    c.check(hipMemcpy2DAsync(hptr, hpitch, dptr, dpitch, width_bytes, height, hipMemcpyDeviceToHost, c.stream()), "hipMemcpy2DAsync");
    return c.finish();
}
int32_t svt_hip_host_alloc(void **hptr, size_t bytes) {
    if (!hptr)
        return SVT_HIP_ERR_BAD_PARAMETER;
    if (!ensure_init())
        return SVT_HIP_ERR_NO_DEVICE;
    SVT_HIP_CHECK(hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
    return SVT_HIP_OK;
}
int32_t svt_hip_host_free(void *hptr) {
    if (hptr)
        SVT_HIP_CHECK(hipHostFree(hptr));
    return SVT_HIP_OK;
}
int32_t svt_hip_copy(void *d_dst, const void *d_src, size_t bytes, void *stream) {
    TierBCall c("svt_hip_copy", stream);
    if (!c.ok())
        return c.status();
    c.check(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, c.stream()), "hipMemcpyAsync");
    return c.finish();
}
int32_t svt_hip_stream_create(void **stream) {
    if (!stream)
        return SVT_HIP_ERR_BAD_PARAMETER;
    if (!ensure_init())
        return SVT_HIP_ERR_NO_DEVICE;
    hipStream_t s;
    SVT_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return SVT_HIP_OK;
}
int32_t svt_hip_stream_destroy(void *stream) {
    SVT_HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
    return SVT_HIP_OK;
}
int32_t svt_hip_stream_sync(void *stream) {
    TierBCall c("svt_hip_stream_sync", stream);
    if (!c.ok())
        return c.status();
    c.check(hipStreamSynchronize(c.stream()), "hipStreamSynchronize");
    return c.finish();
}

}  // extern "C"

// ---- RTCD installation: <reference pointer name> -> this library's <name>_hip export, resolved through the
// dynamic symbol table of the library itself so that the list can never drift from what is exported.
#include <dlfcn.h>

extern "C" void *svt_hip_rtcd_lookup(const char *name) {
    // the two RTCD pointers of the path whose variables have no svt_ prefix (aom_dsp_rtcd.h:838, :861)
    if (name && strcmp(name, "downsample_2d") == 0)
        name = "svt_aom_downsample_2d";
    if (name && strcmp(name, "sad_16b_kernel") == 0)  // aom_dsp_rtcd.h:861
        name = "svt_aom_sad_16b_kernel";
    if (!name || strncmp(name, "svt_", 4) != 0 || strncmp(name, "svt_hip_", 8) == 0 || strlen(name) > 200)
        return nullptr;
    static void *self = [] {
        Dl_info info;
        if (!dladdr((void *)&svt_hip_rtcd_lookup, &info) || !info.dli_fname)
            return (void *)nullptr;
        return dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD);
    }();
    if (!self)
        return nullptr;
    char sym[256];
    snprintf(sym, sizeof(sym), "%s_hip", name);
    return dlsym(self, sym);
}

// Whether a Tier A leaf has failed over (public, read-only: a host reports it; tests assert it stays 0).
extern "C" int32_t svt_hip_tier_a_failed_over(void) { return svthip::g_tier_a_broken.load() ? 1 : 0; }

// Test hooks (declared in svt_hip.h under "test hooks"): the n-th Tier A device check from now on reports a failure (n = 0: the
// next one; n < 0: off); and a way to clear the latch again between tests.  Inert unless the process was started with
// SVTAV1_HIP_TEST_HOOKS=1 -- a production host cannot trip them by accident (reading the latch always works).
static bool test_hooks_enabled() {
    static const bool on = [] {
        const char *e = getenv("SVTAV1_HIP_TEST_HOOKS");
        return e && e[0] == '1';
    }();
    return on;
}
extern "C" void svt_hip_debug_inject_failure(int32_t n) {
    if (test_hooks_enabled())
        svthip::g_inject.store(n);
}
extern "C" int32_t svt_hip_debug_tier_a_broken(int32_t reset) {
    const int32_t was = svthip::g_tier_a_broken.load() ? 1 : 0;
    if (reset && test_hooks_enabled())
        svthip::g_tier_a_broken.store(false);
    return was;
}

extern "C" int32_t svt_hip_install_rtcd(const SvtHipRtcdBinding *b, uint32_t n, uint32_t *n_installed) {
    if (n_installed)
        *n_installed = 0;
    if (!b && n)
        return svthip::refuse("svt_hip_install_rtcd: null binding table");
    if (!svthip::ensure_init())
        return SVT_HIP_ERR_NO_DEVICE;  // nothing installed: the caller keeps its CPU pointers
    if (svthip::tier_a_broken()) {
        svthip::set_error("svt_hip_install_rtcd: the HIP path was disabled after a device failure");
        return SVT_HIP_ERR_RUNTIME;
    }
    uint32_t done = 0;
    for (uint32_t i = 0; i < n; i++) {
        void *fn = b[i].slot ? svt_hip_rtcd_lookup(b[i].name) : nullptr;
        if (fn) {
            // the export's stem is what TIER_A_CALL looks the CPU function up by (two pointers have no svt_ prefix)
            const char *stem = strcmp(b[i].name, "downsample_2d") == 0 ? "svt_aom_downsample_2d"
                : (strcmp(b[i].name, "sad_16b_kernel") == 0 ? "svt_aom_sad_16b_kernel" : b[i].name);
            if (*b[i].slot != fn)
                svthip::remember_slot(stem, b[i].slot, *b[i].slot);
            *b[i].slot = fn, done++;
        }
    }
    if (n_installed)
        *n_installed = done;
    return SVT_HIP_OK;
}
