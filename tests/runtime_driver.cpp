// runtime_driver.cpp -- csrc/runtime.cpp (thread state, guarded buffers, the Tier B call scope, svt_hip_init) against a fake HIP
// runtime in host memory, for tests/test_runtime_host.py.  Built with g++ under the address / undefined-behaviour sanitizers and,
// for the threads scenario, the thread sanitizer: the failure paths no GPU test may provoke run here.
//
// The fake: "device" memory is host memory.  A host-to-device hipMemcpyAsync is only QUEUED on its stream, with a checksum of its
// source; it is carried out when something waits for the stream (hipEventSynchronize of an event recorded behind it,
// hipStreamSynchronize, hipDeviceSynchronize, or a hipStreamWaitEvent of another stream that is itself being waited for).  When it
// is carried out the source is summed again: a pinned slot that was overwritten while its upload was in flight shows up as an
// "overwritten" error.  Freeing memory a queued copy still refers to is an "early free" error.  The n-th fallible call (or the k-th
// call of a named function) can be told to fail; frees are not numbered: the library ignores their status, as it always has.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "../svt-av1-mod-by-patman_amd/csrc/common.hpp"

using namespace svthip;

// ------------------------------------------------------------------------------------------------ the fake runtime
namespace fake {
struct Stream;
struct Event {
    Stream *stream = nullptr;  // where it was last recorded ...
    size_t  ticket = 0;        // ... and behind how many operations of that stream
};
struct Op {
    enum { COPY, WAIT } kind;
    void       *dst;
    const void *src;
    size_t      bytes;
    uint64_t    sum;
    Event       ev;  // WAIT: the event's state when the wait was issued
};
struct Stream {
    std::deque<Op> queue;
    size_t         issued = 0, done = 0;
};

std::mutex               mu;  // one lock for the whole fake
std::vector<Stream *>    streams;
Stream                   null_stream;
std::map<void *, size_t> allocs;
long                     n_calls = 0, fail_at = -1;
const char              *fail_name = nullptr;
int                      fail_name_skip = 0, fail_name_count = 0;
int  n_device_sync = 0, n_event_sync = 0, n_overwritten = 0, n_early_free = 0, n_uploads_done = 0;
bool pending_error = false;  // what hipGetLastError reports once

uint64_t checksum(const void *p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
    return h;
}
bool fails(const char *name) {  // called with mu held, once per fallible call
    bool f = n_calls++ == fail_at;
    if (fail_name && strcmp(name, fail_name) == 0 && fail_name_skip-- <= 0 && fail_name_count-- > 0)
        f = true;
    return f;
}
Stream *of(hipStream_t s) { return s ? (Stream *)s : &null_stream; }
void    drain(Stream *s, size_t upto) {
    while (s->done < upto) {
        Op op = s->queue.front();
        s->queue.pop_front();
        if (op.kind == Op::WAIT) {
            if (op.ev.stream && op.ev.stream != s)
                drain(op.ev.stream, op.ev.ticket);
        } else {
            if (checksum(op.src, op.bytes) != op.sum)
                n_overwritten++;
            memcpy(op.dst, op.src, op.bytes);
            n_uploads_done++;
        }
        s->done++;
    }
}
void drain_all() {
    drain(&null_stream, null_stream.issued);
    for (Stream *s : streams) drain(s, s->issued);
}
void release(void *p) {
    auto it = allocs.find(p);
    if (it == allocs.end())
        return;
    const uint8_t *lo = (const uint8_t *)p, *hi = lo + it->second;
    auto           refers = [&](const Stream &s) {
        for (const Op &op : s.queue)
            if (op.kind == Op::COPY && (((const uint8_t *)op.src >= lo && (const uint8_t *)op.src < hi) ||
                                        ((const uint8_t *)op.dst >= lo && (const uint8_t *)op.dst < hi)))
                return true;
        return false;
    };
    bool early = refers(null_stream);
    for (Stream *s : streams) early = early || refers(*s);
    if (early) {
        n_early_free++;
        drain_all();  // keep the process itself sound: the error has been counted
    }
    allocs.erase(it);
    free(p);
}
hipError_t alloc(void **p, size_t bytes) {
    *p        = malloc(bytes ? bytes : 1);
    allocs[*p] = bytes;
    return hipSuccess;
}
}  // namespace fake

#define FAKE_CALL(name)                        \
    std::lock_guard<std::mutex> lk_(fake::mu); \
    if (fake::fails(name))                     \
    return hipErrorUnknown

extern "C" {
const char *hipGetErrorString(hipError_t) { return "fake device error"; }
hipError_t  hipGetLastError(void) {
    FAKE_CALL("hipGetLastError");
    return hipSuccess;
}
hipError_t hipGetDeviceCount(int *n) {
    FAKE_CALL("hipGetDeviceCount");
    *n = 1;
    return hipSuccess;
}
hipError_t hipSetDevice(int) {
    FAKE_CALL("hipSetDevice");
    return hipSuccess;
}
hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int) {  // (the header maps the name to its versioned symbol)
    FAKE_CALL("hipGetDeviceProperties");
    memset(prop, 0, sizeof(*prop));
    strcpy(prop->gcnArchName, "gfx950:sramecc+:xnack-");
    prop->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
    std::lock_guard<std::mutex> lk_(fake::mu);
    fake::n_device_sync++;
    if (fake::fails("hipDeviceSynchronize"))
        return hipErrorUnknown;
    fake::drain_all();
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
    FAKE_CALL("hipStreamCreateWithFlags");
    fake::streams.push_back(new fake::Stream);
    *s = (hipStream_t)fake::streams.back();
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }  // streams live as long as the process: events may name them
hipError_t hipStreamSynchronize(hipStream_t s) {
    FAKE_CALL("hipStreamSynchronize");
    fake::drain(fake::of(s), fake::of(s)->issued);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    FAKE_CALL("hipEventCreateWithFlags");
    *e = (hipEvent_t) new fake::Event;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    FAKE_CALL("hipEventRecord");
    *(fake::Event *)e = {fake::of(s), fake::of(s)->issued};
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    std::lock_guard<std::mutex> lk_(fake::mu);
    fake::n_event_sync++;
    if (fake::fails("hipEventSynchronize"))
        return hipErrorUnknown;
    const fake::Event ev = *(fake::Event *)e;
    if (ev.stream)
        fake::drain(ev.stream, ev.ticket);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    FAKE_CALL("hipStreamWaitEvent");
    fake::Op op{};
    op.kind = fake::Op::WAIT, op.ev = *(fake::Event *)e;
    fake::of(s)->queue.push_back(op), fake::of(s)->issued++;
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes) {
    FAKE_CALL("hipMalloc");
    return fake::alloc(p, bytes);
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) {
    FAKE_CALL("hipHostMalloc");
    return fake::alloc(p, bytes);
}
hipError_t hipFree(void *p) {
    std::lock_guard<std::mutex> lk_(fake::mu);
    fake::release(p);
    return hipSuccess;
}
hipError_t hipHostFree(void *p) {
    std::lock_guard<std::mutex> lk_(fake::mu);
    fake::release(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    FAKE_CALL("hipMemcpyAsync");
    if (kind != hipMemcpyHostToDevice) {  // downloads and device copies see everything issued before them
        fake::drain(fake::of(s), fake::of(s)->issued);
        memcpy(dst, src, bytes);
        return hipSuccess;
    }
    fake::Op op{};
    op.kind = fake::Op::COPY, op.dst = dst, op.src = src, op.bytes = bytes, op.sum = fake::checksum(src, bytes);
    fake::of(s)->queue.push_back(op), fake::of(s)->issued++;
    return hipSuccess;
}
// linked by runtime.cpp, used by no scenario
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipMemcpy2DAsync(void *, size_t, const void *, size_t, size_t, size_t, hipMemcpyKind, hipStream_t) { return hipErrorNotSupported; }
}  // extern "C"

// ------------------------------------------------------------------------------------------------ scenarios
#define REQUIRE(cond)                                                                   \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "runtime_driver: %s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            exit(2);                                                                    \
        }                                                                               \
    } while (0)

namespace {

struct Staged {  // what a call left on the device, and what it must hold once its stream has drained
    const void          *dev = nullptr;
    std::vector<uint8_t> want;
    bool                 intact() const { return dev && memcmp(dev, want.data(), want.size()) == 0; }
};

std::vector<uint8_t> pattern(size_t bytes, int tag) {
    std::vector<uint8_t> v(bytes);
    for (size_t i = 0; i < bytes; i++) v[i] = (uint8_t)(i * 7 + tag * 31 + (i >> 8));
    return v;
}
// the caller's array is dead the moment the call returns
void *stage_and_forget(TierBCall &c, size_t bytes, int tag, Staged *out) {
    std::vector<uint8_t> host = pattern(bytes, tag);
    void                *dev  = c.stage(host.data(), bytes);
    if (out)
        out->dev = dev, out->want = host;
    memset(host.data(), 0xFF, bytes);
    return dev;
}

// One Tier-B-shaped call: a scope, two staged arrays, both per-thread device buffers, the launch check.
int32_t tier_b_call(void *stream, size_t bytes1, size_t bytes2, size_t aux_bytes, int tag, Staged *s1 = nullptr, Staged *s2 = nullptr) {
    TierBCall c("runtime_driver_call", stream);
    void     *d1 = stage_and_forget(c, bytes1, tag, s1);
    void     *d2 = stage_and_forget(c, bytes2, tag + 1, s2);
    void     *a  = c.take(tls().wiener_aux, aux_bytes, 2 * aux_bytes);
    void     *p  = c.take(tls().txfm_perm, 4096, 4096);
    if (!c.ok()) {
        REQUIRE(!(d1 && d2 && a && p));
        REQUIRE(!c.stage(&tag, sizeof(tag)) && !c.take(tls().txfm_perm, 16, 16));  // the status is sticky
        return c.status();  // the destructor gives back what was taken
    }
    REQUIRE(d1 && d2 && a && p && d1 != d2);
    return c.finish();
}

void *new_stream() {
    void *s = nullptr;
    REQUIRE(svt_hip_stream_create(&s) == SVT_HIP_OK && s);
    return s;
}
void clean_at_exit() {
    std::lock_guard<std::mutex> lk(fake::mu);
    fake::drain_all();
    REQUIRE(fake::n_overwritten == 0);
    REQUIRE(fake::n_early_free == 0);
}

// script <n>: two clean calls fill the four slots and size the buffers; the third reuses two slots, makes one of them and one
// buffer grow, and has its n-th fallible runtime call fail (n < 0: none); a clean call on another stream follows.
int script(long n) {
    REQUIRE(svt_hip_init(0) == SVT_HIP_OK);
    void *s[4] = {new_stream(), new_stream(), new_stream(), new_stream()};
    REQUIRE(tier_b_call(s[0], 1000, 3000, 512, 1) == SVT_HIP_OK);
    REQUIRE(tier_b_call(s[1], 2000, 500, 512, 3) == SVT_HIP_OK);
    REQUIRE(svt_hip_init(-1) == SVT_HIP_ERR_BAD_PARAMETER);  // leaves a text behind that is not the scripted call's
    {
        std::lock_guard<std::mutex> lk(fake::mu);
        fake::n_calls = 0, fake::fail_at = n;
    }
    const int32_t rc = tier_b_call(s[2], 700, 100000, 4096, 5);
    long          n_calls;
    {
        std::lock_guard<std::mutex> lk(fake::mu);
        n_calls = fake::n_calls, fake::fail_at = -1;
    }
    const char *err = svt_hip_last_error();
    if (n >= 0 && n < n_calls) {
        REQUIRE(rc == SVT_HIP_ERR_RUNTIME);
        REQUIRE(strstr(err, "runtime_driver_call: hip") || strstr(err, "runtime_driver_call: launch"));
        REQUIRE(strstr(err, "fake device error"));
    } else {
        REQUIRE(rc == SVT_HIP_OK);
    }
    Staged a, b;
    REQUIRE(tier_b_call(s[3], 900, 1200, 512, 7, &a, &b) == SVT_HIP_OK);
    REQUIRE(svt_hip_stream_sync(s[3]) == SVT_HIP_OK);
    REQUIRE(a.intact() && b.intact());
    clean_at_exit();
    printf("calls %ld rc %d\n", n_calls, rc);
    return 0;
}

// ring: 9 calls on 9 streams through the 4 slots, nothing synchronised by the caller.
int ring() {
    REQUIRE(svt_hip_init(0) == SVT_HIP_OK);
    Staged staged[9];
    for (int i = 0; i < 9; i++) {
        TierBCall c("ring", new_stream());
        REQUIRE(stage_and_forget(c, 300 + 100 * i, i, &staged[i]));
        REQUIRE(c.finish() == SVT_HIP_OK);
    }
    clean_at_exit();
    for (int i = 5; i < 9; i++) REQUIRE(staged[i].intact());  // the last user of each slot
    REQUIRE(fake::n_uploads_done == 9);
    printf("event_syncs %d\n", fake::n_event_sync);
    return 0;
}

// grow: slot 0 and the Wiener buffer grow while the work that used them, on another stream, has not drained.
int grow() {
    REQUIRE(svt_hip_init(0) == SVT_HIP_OK);
    Staged first;
    {
        TierBCall c("grow", new_stream());
        REQUIRE(stage_and_forget(c, 1024, 1, &first) && c.take(tls().wiener_aux, 1024, 2048));
        REQUIRE(c.finish() == SVT_HIP_OK);
    }
    for (int i = 0; i < 3; i++) {  // slots 1 .. 3
        TierBCall c("grow", new_stream());
        REQUIRE(stage_and_forget(c, 256, 2 + i, nullptr) && c.finish() == SVT_HIP_OK);
    }
    REQUIRE(fake::n_uploads_done == 0);
    Staged big;
    {
        TierBCall c("grow", new_stream());
        REQUIRE(stage_and_forget(c, 200000, 9, &big) && c.take(tls().wiener_aux, 1 << 20, 2 << 20));
        REQUIRE(c.finish() == SVT_HIP_OK);
    }
    REQUIRE(tls().ring[0].cap == 400000 && tls().wiener_aux.cap == (2u << 20));
    clean_at_exit();
    REQUIRE(big.intact());
    printf("device_syncs %d\n", fake::n_device_sync);
    return 0;
}

// nested: an inner scope on the same stream, as svt_hip_tf_filter_picture -> svt_hip_me_frames.
int nested() {
    REQUIRE(svt_hip_init(0) == SVT_HIP_OK);
    void  *st = new_stream();
    Staged outer, outer2, inner;
    {
        TierBCall c("outer", st);
        REQUIRE(stage_and_forget(c, 5000, 1, &outer));
        {
            TierBCall d("inner", st);
            REQUIRE(stage_and_forget(d, 5000, 2, &inner));
            REQUIRE(d.finish() == SVT_HIP_OK);
        }
        REQUIRE(stage_and_forget(c, 100, 3, &outer2));
        REQUIRE(c.finish() == SVT_HIP_OK);
    }
    REQUIRE(outer.dev != inner.dev && outer.dev != outer2.dev && inner.dev != outer2.dev);
    REQUIRE(svt_hip_stream_sync(st) == SVT_HIP_OK);
    REQUIRE(outer.intact() && inner.intact() && outer2.intact());
    {  // a scope that would wrap the ring onto a slot an enclosing scope still holds is refused, not served
        TierBCall c("outer", st);
        REQUIRE(stage_and_forget(c, 64, 4, nullptr));
        for (int i = 0; i < 3; i++) {
            TierBCall d("inner", st);
            REQUIRE(stage_and_forget(d, 64, 5 + i, nullptr) && d.finish() == SVT_HIP_OK);
        }
        TierBCall d("inner", st);
        REQUIRE(!stage_and_forget(d, 64, 9, nullptr) && d.finish() == SVT_HIP_ERR_RUNTIME);
        REQUIRE(c.finish() == SVT_HIP_OK);
    }
    clean_at_exit();
    return 0;
}

// failed_init: the warm-up's synchronisation fails once; the next svt_hip_init must run the warm-up again.
int failed_init() {
    fake::fail_name = "hipDeviceSynchronize", fake::fail_name_count = 1;
    REQUIRE(svt_hip_init(0) == SVT_HIP_ERR_RUNTIME);
    REQUIRE(!ensure_init());
    REQUIRE(svt_hip_init(0) == SVT_HIP_OK);
    REQUIRE(ensure_init());
    REQUIRE(svt_hip_init(0) == SVT_HIP_OK);  // and only while it has not succeeded
    printf("device_syncs %d\n", fake::n_device_sync);
    return 0;
}

// threads: pool slots 2 .. 5 cannot be created during svt_hip_init, so worker threads create them on demand while others read the pool.
int threads() {
    fake::fail_name = "hipStreamCreateWithFlags", fake::fail_name_skip = 2, fake::fail_name_count = 4;
    REQUIRE(svt_hip_init(0) == SVT_HIP_OK);
    REQUIRE(fake::streams.size() == 4);
    int                      bad[16] = {};
    std::vector<std::thread> pool;
    for (int t = 0; t < 16; t++)
        pool.emplace_back([t, &bad] {
            for (int i = 0; i < 50; i++) {
                TierBCall c("threads", nullptr);
                if (!c.stream() || !stage_and_forget(c, 200 + t, t + i, nullptr) || !c.take(tls().wiener_aux, 64u << (i / 10), 128u << (i / 10)) ||
                    c.finish() != SVT_HIP_OK)
                    bad[t]++;
            }
        });
    for (std::thread &th : pool) th.join();
    for (int t = 0; t < 16; t++) REQUIRE(bad[t] == 0);
    REQUIRE(fake::streams.size() == 8);
    clean_at_exit();
    REQUIRE(fake::n_uploads_done == 16 * 50);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "script"))
        return script(argc > 2 ? atol(argv[2]) : -1);
    if (!strcmp(what, "ring"))
        return ring();
    if (!strcmp(what, "grow"))
        return grow();
    if (!strcmp(what, "nested"))
        return nested();
    if (!strcmp(what, "failed_init"))
        return failed_init();
    if (!strcmp(what, "threads"))
        return threads();
    fprintf(stderr, "usage: runtime_driver script [n] | ring | grow | nested | failed_init | threads\n");
    return 64;
}
