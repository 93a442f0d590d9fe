// common.hpp — shared host-side helpers of libsvtav1_hip (gfx950 only; no CUDA / multi-backend paths).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/svt_hip.h"
#include "../../include/svt_hip_me.h"

namespace svthip {

// Thread-local error text returned by svt_hip_last_error().
void set_error(const char *fmt, ...);
// Refusal of an argument: sets the text, returns SVT_HIP_ERR_BAD_PARAMETER.
int32_t refuse(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

// Calling thread's pooled stream unless the caller passed its own.
hipStream_t resolve_stream(void *stream);

// Grow-only per-thread device + pinned scratch used by the Tier A (host-pointer) entry points.  host() keeps the first
// `keep` bytes when it has to grow; device() keeps nothing.
struct Scratch {
    uint8_t *dev    = nullptr;
    uint8_t *pinned = nullptr;
    size_t   dev_cap = 0, pinned_cap = 0;
    uint8_t *device(size_t bytes);
    uint8_t *host(size_t bytes, size_t keep = 0);
};

bool ensure_init();
int  cu_count();                         // compute units of the device, queried once by svt_hip_init
hipError_t ensure_event(hipEvent_t &ev); // creates ev (no timing) unless it exists: the one place events are made

// Grow-only device buffer of one thread, with a pinned twin of the same size when the host fills it, and one event that
// guards it against its previous user, which may sit on another stream.  acquire() makes it safe to use on st: when the
// host is going to write the twin, or when the buffer has to grow, it waits for the buffer's OWN event on the host (never
// for the device, never through a bare free); otherwise st waits for the event.  release() records the event behind the
// work that uses the buffer.  After a failed growth the buffer is empty (dev == pinned == nullptr, cap == 0).
struct GuardedBuf {
    uint8_t   *dev = nullptr, *pinned = nullptr;
    size_t     cap = 0;
    hipEvent_t ev  = nullptr;
    bool       pending = false;  // ev was recorded and the host has not waited for it since
    bool       held    = false;  // a live TierBCall owns it
    // grows to grow_to (>= bytes) when bytes > cap; *what names the HIP call that failed
    hipError_t acquire(size_t bytes, size_t grow_to, bool host_writes, hipStream_t st, const char **what);
    hipError_t release(hipStream_t st);
};

// Everything a host thread owns on the device: the library's only per-thread object (tls(), runtime.cpp).
struct ThreadState {
    char       err[512] = "";      // svt_hip_last_error()
    bool       bound    = false;   // hipSetDevice done
    int        slot     = -1;      // index into the stream pool
    GuardedBuf ring[4];            // staging slots for descriptor arrays that arrive in host memory (TierBCall::stage)
    int        ring_next = 0;
    Scratch    scratch;            // Tier A staging (TierAStage)
    GuardedBuf wiener_aux;         // raw first moments of svt_hip_wiener_stats
    GuardedBuf txfm_perm;          // transform batch: fallback counters and list, block permutation of the grouped launch (txfm.hip)
    hipStream_t     txfm_fast_stream = nullptr;  // stream and counters of the last transform batch if it ran lean + fallback
    const uint32_t *txfm_fast_hdr    = nullptr;  // (svt_hip_debug_txfm_fallback_blocks)
    hipEvent_t produced = nullptr; // svt_hip_publish_reference: producer stream -> side stream
};
ThreadState &tls();

// The host side of one Tier B entry point.  Every exported svt_hip_* function that enqueues work (a kernel, a copy, a memset, a
// synchronisation) opens one on its stack, at the point where its checks ask for the device:
//     if (!jobs || !n) return refuse("svt_hip_x: bad argument");  // argument checks: no device needed
//     TierBCall c("svt_hip_x", stream);                       // ensure_init + resolve_stream
//     const Job *d_jobs = (const Job *)c.stage(jobs, bytes);   // host array -> next ring slot -> device
//     void *aux = c.take(tls().wiener_aux, bytes, 2 * bytes);  // event-guarded per-thread device buffer
//     if (!c.ok()) return c.status();
//     if (!c.check(hipMemsetAsync(out, 0, 8, c.stream()), "hipMemsetAsync")) return c.status();  // any other HIP call
//     hipLaunchKernelGGL(..., c.stream(), d_jobs, aux);
//     return c.finish();                                       // launch check, events recorded
// A failure reads "svt_hip_x: <step>: <HIP's text>", whichever entry point it happens in.  Three kinds of function have no scope and
// keep SVT_HIP_CHECK: the life-cycle calls that enqueue nothing (init, malloc / free, host_alloc / host_free, stream_create /
// stream_destroy, the debug read-back, shard.cpp); the readiness helpers (txfm_ready(), tf_filter.hip's ready() and the table uploads
// behind their call_once), which keep their own ensure_init() because Tier A leaves reach them through TierAStage's `ready`; and
// launch helpers that a Tier A leaf shares (tf_noise.hip's launch()), which take the scope's stream from their Tier B caller.
// The status is sticky: after a failed step stage(), take() and check() do nothing and return nullptr / false.  Whatever the scope took is
// given back -- its event recorded on the stream -- by finish() or, on any earlier return, by the destructor, so no slot
// can be reused while an upload from it or a kernel that reads it is still in flight.  A nested scope (tf_filter_picture
// -> me_frames) claims the next ring slot and never touches the outer scope's.  No allocation happens on the launch path
// once the buffers have grown.
class TierBCall {
public:
    TierBCall(const char *fn, void *stream);
    ~TierBCall() { release(); }
    TierBCall(const TierBCall &)            = delete;
    TierBCall &operator=(const TierBCall &) = delete;
    bool        ok() const { return status_ == SVT_HIP_OK; }
    int32_t     status() const { return status_; }
    hipStream_t stream() const { return st_; }
    void       *stage(const void *host, size_t bytes);                 // 64 KiB minimum, x2 when it grows
    void       *take(GuardedBuf &b, size_t bytes, size_t grow_to);     // grows to grow_to when bytes > b.cap
    bool        check(hipError_t e, const char *what);                 // a HIP call made on the scope's behalf; false once the scope has failed
    int32_t     finish();

private:
    void       *fail(hipError_t e, const char *what);
    bool        hold(GuardedBuf &b, size_t bytes, size_t grow_to, bool host_writes);
    void        release();
    const char *fn_;
    hipStream_t st_     = nullptr;
    int32_t     status_ = SVT_HIP_OK;
    GuardedBuf *held_[6];
    int         n_held_ = 0;
};

// The host side of a batch export whose descriptors two instantiations of one kernel share, each walking all n and skipping the other's:
// refusal unless have_pointers, nothing for an empty batch, else one scope with `small` on min(n, small_per_cu per compute unit)
// workgroups of small_threads and `large` likewise; a workgroup strides over the descriptors when there are more than its grid holds.
template <class... Params, class... Args>
int32_t launch_two_classes(const char *fn, bool have_pointers, uint32_t n, void *stream, void (*small)(Params...), uint32_t small_threads, uint32_t small_per_cu,
                           void (*large)(Params...), uint32_t large_threads, uint32_t large_per_cu, const Args &...args) {
    if (!have_pointers)
        return refuse("%s: bad argument", fn);
    if (n == 0)
        return SVT_HIP_OK;
    TierBCall c(fn, stream);
    if (!c.ok())
        return c.status();
    hipLaunchKernelGGL(small, dim3(std::min(n, (uint32_t)cu_count() * small_per_cu)), dim3(small_threads), 0, c.stream(), args...);
    hipLaunchKernelGGL(large, dim3(std::min(n, (uint32_t)cu_count() * large_per_cu)), dim3(large_threads), 0, c.stream(), args...);
    return c.finish();
}

// The HIP runtime loads the code object of a translation unit when the first of its kernels is launched (hundreds of milliseconds for
// the whole library, paid by whichever encoder threads come first: 23 ms per call of the first 35 calls inside the patched encoder).
// Every .hip file registers one empty kernel; svt_hip_init launches them all, so the cost is paid once, at initialisation.
typedef void (*WarmupFn)(hipStream_t);
struct WarmupRegistrar {
    explicit WarmupRegistrar(WarmupFn fn);
};
void run_module_warmups(hipStream_t st);

}  // namespace svthip

#define SVT_HIP_MODULE_WARMUP(tag)                                                                                  \
    namespace {                                                                                                     \
    __global__ void svt_hip_warmup_##tag() {}                                                                       \
    void svt_hip_warmup_launch_##tag(hipStream_t st) { hipLaunchKernelGGL(svt_hip_warmup_##tag, dim3(1), dim3(64), 0, st); } \
    svthip::WarmupRegistrar svt_hip_warmup_registrar_##tag(svt_hip_warmup_launch_##tag);                             \
    }

#define SVT_HIP_CHECK(expr)                                                                        \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            svthip::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SVT_HIP_ERR_RUNTIME;                                                            \
        }                                                                                          \
    } while (0)

// ---- Tier A failure handling (SURVEY.md 8b "never abort") ---------------------------------------------------------------
// A Tier A leaf has the reference's signature and cannot report an error.  When a HIP call fails inside one (device lost,
// out of memory ...) it throws TierAError; the exported wrapper (TIER_A_CALL) catches it, and tier_a_fail() then, ONCE per
// process: logs the cause, puts the CPU function pointers that svt_hip_install_rtcd() had replaced back into the encoder's
// RTCD slots and latches the library as broken.  The failing call itself — and any call that was already on its way into a
// leaf on another thread — is completed by the restored CPU function with the same arguments, so the encoder carries on with
// its own kernels and an intact bitstream.  Without an installer-saved CPU pointer (the leaf was called directly, e.g.
// through ctypes) there is nothing to fall back on: the process stops with the error message, as before.
// How a leaf is defined and staged: TIER_A_LEAF and TierAStage below.
namespace svthip {
struct TierAError {
    char what[256];
};
[[noreturn]] void tier_a_throw(const char *fmt, ...);
bool              tier_a_broken();
void              tier_a_fail(const char *leaf, const char *what);
void             *tier_a_cpu(const char *leaf);  // saved CPU function of <leaf> (never NULL: stops the process otherwise)
bool              tier_a_inject_now();           // test hook (svt_hip_debug_inject_failure)
}  // namespace svthip

#define SVT_HIP_CHECK_FATAL(expr)                                                                            \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess || svthip::tier_a_inject_now())                                                 \
            svthip::tier_a_throw("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Body of every exported Tier A function: NAME = the reference's pointer name, IMPL_EXPR = the call that does the work,
// ARGS = the parenthesised argument list for the CPU function.
#define TIER_A_CALL(NAME, IMPL_EXPR, ARGS)                             \
    do {                                                               \
        typedef decltype(&NAME##_hip) TierAFn_;                        \
        if (__builtin_expect(!svthip::tier_a_broken(), 1)) {           \
            try {                                                      \
                return IMPL_EXPR;                                      \
            } catch (const svthip::TierAError &e_) {                   \
                svthip::tier_a_fail(#NAME, e_.what);                   \
            }                                                          \
        }                                                              \
        return ((TierAFn_)svthip::tier_a_cpu(#NAME))ARGS;              \
    } while (0)

// A hand-written leaf is written once:
//     TIER_A_LEAF(uint32_t, svt_nxm_sad_kernel, (const uint8_t *src, uint32_t src_stride, ...), (src, src_stride, ...)) {
//         ...body; fails by throwing through fatal() / SVT_HIP_CHECK_FATAL...
//     }
// This expands to the exported `extern "C" RET NAME_hip PARAMS` (it must match the prototype in include/*.h), whose body is
// TIER_A_CALL, and to the head of the file-local function that the braces after the macro complete.
#define TIER_A_LEAF(RET, NAME, PARAMS, ARGS)                                        \
    static RET NAME##_leaf PARAMS;                                                  \
    extern "C" RET NAME##_hip PARAMS { TIER_A_CALL(NAME, NAME##_leaf ARGS, ARGS); } \
    static RET NAME##_leaf PARAMS

namespace svthip {

inline size_t     up256(size_t v) { return (v + 255) / 256 * 256; }
[[noreturn]] void fatal(const char *what);  // throws TierAError "<what>: <svt_hip_last_error()>"

// rows x row_bytes between two pitched buffers (pitches in bytes)
inline void copy_rows(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t rows, size_t row_bytes) {
    for (size_t r = 0; r < rows; r++) memcpy((uint8_t *)dst + r * dst_pitch, (const uint8_t *)src + r * src_pitch, row_bytes);
}

// Staging of one Tier A leaf call in the calling thread's Scratch.  A bump allocator hands out regions: offsets, 256-byte
// aligned, the same in the pinned and in the device buffer.  The leaf uploads what the kernel reads, launches on stream(),
// and finish() brings the results back.  Every HIP call in here goes through SVT_HIP_CHECK_FATAL.
//     TierAStage s("leaf name");                        // throws unless the library is initialised
//     const size_t a = s.in(src, n), r = s.out(4);      // reserve (and fill) every region first ...
//     s.upload();                                       // ... [0, end of the last in()) goes up in one copy
//     hipLaunchKernelGGL(k, ..., s.stream(), s.dev(a), s.dev<uint32_t>(r));
//     s.finish(r, 4);                                   // launch check, copy back, synchronise
//     return *s.host<uint32_t>(r);
// A host() pointer is valid until the next in() / out(): the pinned buffer may grow (it keeps its content).  No region can be
// reserved after dev() / h2d() has sized the device buffer.
class TierAStage {
public:
    explicit TierAStage(const char *leaf, bool ready = ensure_init());
    // reserves bytes (+ slack that a kernel may read past the data); copies bytes from src unless src is NULL
    size_t in(const void *src, size_t bytes, size_t slack = 0);
    // rows x row_bytes read at src_pitch, stored packed (pitch = row_bytes)
    size_t in_rows(const void *src, size_t src_pitch, size_t rows, size_t row_bytes);
    size_t out(size_t bytes) { return reserve(bytes); }
    template <class T = uint8_t> T *host(size_t off) const { return (T *)(h_ + off); }
    template <class T = uint8_t> T *dev(size_t off) { return (T *)(device() + off); }
    hipStream_t stream() const { return st_; }
    void h2d(size_t off, size_t bytes);
    void upload() { h2d(0, in_end_); }
    void finish(size_t off, size_t bytes, size_t off2 = 0, size_t bytes2 = 0);
    // rows x row_bytes of the packed region at off, written at dst_pitch
    void out_rows(void *dst, size_t dst_pitch, size_t off, size_t rows, size_t row_bytes) const {
        copy_rows(dst, dst_pitch, h_ + off, row_bytes, rows, row_bytes);
    }

private:
    size_t      reserve(size_t bytes);
    uint8_t    *device();
    hipStream_t st_;
    uint8_t    *h_ = nullptr, *d_ = nullptr;
    size_t      used_ = 0, in_end_ = 0;
};

}  // namespace svthip
