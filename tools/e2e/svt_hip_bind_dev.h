/*
 * svt_hip_bind_dev.h — what the Tier B glue files (svt_hip_bind_{me,tf,tpl,lf,pa,txt}.c) share: the resolved device API of
 * libsvtav1_hip.so, PCIe byte counters, and the DEVICE-RESIDENT PICTURE MIRRORS of SURVEY.md 8b "Ownership" ("the shim owns
 * device mirrors ... per-picture device planes keyed by picture number").
 *
 * A mirror is the device copy of one host buffer of the encoder (a plane of an EbPictureBufferDesc, a gathered mode-info
 * grid ...), identified by the host address and a TAG the caller derives from what the buffer holds (picture number, which
 * processing stage wrote it last).  hd_mirror_get() uploads only when the cache has no copy with that tag; a source picture
 * that used to cross PCIe once as ME source, up to five times as ME reference, once per temporal-filter window it is part of
 * and again for the TPL dispenser now crosses once.  Entries are dropped at the reference's own hand-over points (the hooks
 * call hd_mirror_drop when a stage is about to rewrite a buffer on the CPU) and by LRU above a byte budget
 * (SVTAV1_HIP_MIRROR_MB, default 6144).  SVTAV1_HIP_MIRROR_VERIFY=1 (the tests set it) downloads every hit and compares it
 * with the host buffer: a stale mirror is reported ("STALE mirror") and replaced — the tests assert the message never appears.
 */
#ifndef SVT_HIP_BIND_DEV_H
#define SVT_HIP_BIND_DEV_H

#include <stddef.h>
#include <stdint.h>

#include "svt_hip.h"

/* Entry points of libsvtav1_hip.so are looked up by name; their types come from the declarations of include/svt_hip*.h:
 *     HD_FN(svt_hip_me_frames);  ...  HD_SYM(sym, svt_hip_me_frames);  ...  p_svt_hip_me_frames(job, 1, NULL) */
#define HD_LOOKUP(sym, name) ((__typeof__(name) *)(sym)(#name))
#define HD_FN(name) static __typeof__(name) *p_##name
#define HD_SYM(sym, name) (p_##name = HD_LOOKUP(sym, name))

typedef struct HipDev {
    __typeof__(svt_hip_malloc)      *malloc_;
    __typeof__(svt_hip_free)        *free_;
    __typeof__(svt_hip_upload)      *upload;
    __typeof__(svt_hip_download)    *download;
    __typeof__(svt_hip_memset)      *memset_;
    __typeof__(svt_hip_stream_sync) *sync;
    __typeof__(svt_hip_last_error)  *last_error;
    int ok; /* every pointer above resolved */
} HipDev;
extern HipDev g_hd;

void        svt_hip_bind_dev_setup(void *(*sym)(const char *));
const char *hd_error(void);
int         hd_env_on(const char *name); /* getenv(name) is a non-zero number */

/* counted transfers (NULL stream = the calling thread's private stream; hd_sync waits for it) */
int hd_upload(void *d, const void *h, size_t n);
int hd_download(void *h, const void *d, size_t n);
int hd_sync(void);
/* device scratch from a recycling pool (no hipMalloc / hipFree on the hooks' paths once the sizes of a sequence have been seen) */
uint8_t *hd_alloc(size_t n);
void     hd_free(void *d);
/* page-locked host staging from a recycling pool (falls back to malloc when the library has no svt_hip_host_alloc) */
void *hd_host_alloc(size_t n);
void  hd_host_free(void *h);

/* ---- mirrors ---------------------------------------------------------------------------------------------------------- */
/* content tags: (picture number << 8) | stage.  A buffer's stage changes whenever somebody rewrites it. */
enum {
    HD_ST_SOURCE    = 1,  /* input picture planes as the picture-analysis stage sees them (before the temporal filter) */
    HD_ST_FILTERED  = 2,  /* after produce_temporally_filtered_pic (or pictures that are never filtered, once ME sees them) */
    HD_ST_RECON     = 3,  /* reconstruction after EncDec, before deblocking */
    HD_ST_DEBLOCKED = 4,
    HD_ST_CDEF      = 5,
    HD_ST_RESTORED  = 6,
    HD_ST_TPL_RECON = 7,  /* mc_flow_rec_picture_buffer of a picture, after its dispenser */
    HD_ST_MI_LF     = 8,  /* gathered SvtHipLfMi grid of a picture */
    HD_ST_MI_SKIP   = 9,  /* gathered 8x8 skip bitmap (CDEF) */
    HD_ST_SOURCE16  = 10, /* pcs->input_frame16bit as the CDEF stage sees it */
    HD_ST_CDEF_EXT  = 11, /* reconstruction after CDEF with the borders the restoration search extended (restoration_pick.c:1511) */
    HD_ST_SOURCE16_LR = 12, /* pcs->input_frame16bit after set_unscaled_input_16bit (cdef_process.c:418) */
};
#define HD_TAG(picture_number, stage) (((uint64_t)(picture_number) << 8) | (uint64_t)(stage))

/* Device copy of host[0 .. bytes) whose content is `tag`; uploaded if the cache holds none.  The entry is PINNED (never evicted,
 * never dropped under the caller) until hd_mirror_unpin(host).  NULL on failure (hd_error()). */
uint8_t *hd_mirror_get(const void *host, size_t bytes, uint64_t tag);
/* A device buffer of `bytes` bytes the caller will fill on the device and that then holds what host will hold under `tag`
 * (the caller downloads it into host, or knows host already equals it).  Replaces any other entry of `host`.  Pinned. */
uint8_t *hd_mirror_new(const void *host, size_t bytes, uint64_t tag);
void     hd_mirror_unpin(const void *host);
/* The host buffer is about to change (or was released): forget its mirror (deferred until unpinned). */
void hd_mirror_drop(const void *host);
/* Re-tag: the entry of `host` (if any, with tag `from`) now describes content `to` — the caller knows both are the same bytes. */
void hd_mirror_retag(const void *host, uint64_t from, uint64_t to);

/* ---- one scope per hook call ---------------------------------------------------------------------------------------------
 * A hook puts an HdCall on its stack and acquires everything through it: mirror pins, device scratch, pinned staging, plain host
 * memory.  The scope owns all of it until hd_call_end.  Its status is STICKY: once a step has failed, every later step made through
 * the scope does nothing (no device call is issued) and returns NULL / non-zero, so a hook is straight-line code with one
 * hd_call_sync test in front of the place where it copies its results into the encoder's buffers.  hd_call_end synchronises the
 * calling thread's stream BEFORE it releases anything, also after a failure.  The arrays are sized for the largest user (the temporal
 * filter: 5 planes / 3 scratch planes per window picture); one acquisition too many makes the call fail. */
#define HD_CALL_PINS 168
#define HD_CALL_BLOCKS 112
typedef struct HdCall {
    const char *timer; /* hook name of the "ms per call" lines at exit, or NULL */
    uint64_t    t0;
    int         failed, used, n_pins, n_blocks;
    const void *pin[HD_CALL_PINS];
    void       *block[HD_CALL_BLOCKS];
    uint8_t     pin_new[HD_CALL_PINS], block_kind[HD_CALL_BLOCKS];
} HdCall;
void     hd_call_begin(HdCall *c, const char *timer_name);
uint8_t *hd_call_mirror(HdCall *c, const void *host, size_t bytes, uint64_t tag);     /* hd_mirror_get, pinned until the end */
uint8_t *hd_call_mirror_new(HdCall *c, const void *host, size_t bytes, uint64_t tag); /* hd_mirror_new; dropped if the call fails */
void     hd_call_unpin(HdCall *c, const void *host);     /* early release of one pin (after hd_call_sync): the caller is done with it */
uint8_t *hd_call_dev(HdCall *c, size_t bytes);           /* device scratch of >= bytes + 256, 256-aligned */
uint8_t *hd_call_dev_put(HdCall *c, const void *host, size_t bytes); /* the same + upload */
void    *hd_call_pinned(HdCall *c, size_t bytes);        /* page-locked staging */
void    *hd_call_host(HdCall *c, size_t bytes);          /* zeroed */
int      hd_call_upload(HdCall *c, void *d, const void *h, size_t n);
int      hd_call_download(HdCall *c, void *h, const void *d, size_t n);
int      hd_call_memset(HdCall *c, void *d, int value, size_t n);
int      hd_call_ok(const HdCall *c);
void     hd_call_fail(HdCall *c);
int      hd_call_check(HdCall *c, int rc);               /* folds a return code into the status; non-zero when the scope has failed */
/* a library call through the scope: not made once the scope has failed */
#define HD_CALL(c, call) (hd_call_ok(c) ? hd_call_check(c, (call)) : 1)
int      hd_call_sync(HdCall *c);                        /* 0: everything so far has succeeded and arrived: results may be committed */
/* Syncs (unless nothing was done since a successful hd_call_sync), unpins, frees, adds the timer; after a failure prints "<fmt ...> (<hd_error()>)" once (fmt NULL:
 * nothing).  Returns 0 = the GPU did it, 1 = the caller runs the CPU code. */
int      hd_call_end(HdCall *c, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int      hd_call_decline(HdCall *c);                     /* not a case for the GPU: hd_call_end without a message, returns 1 */
/* for the tests: what is pinned / handed out right now */
void     hd_debug_in_use(int *pins, int *dev_blocks, int *host_blocks);

static inline size_t hd_al256(size_t v) { return (v + 255) & ~(size_t)255; }
/* one pool block cut into 256-aligned regions: *cursor walks through it (NULL stays NULL) */
static inline uint8_t *hd_carve(uint8_t **cursor, size_t n) {
    uint8_t *r = *cursor;
    if (r)
        *cursor = r + hd_al256(n);
    return r;
}
/* bytes of a padded luma plane; d: const EbPictureBufferDesc * (a macro: this header stays free of the reference's types) */
#define hd_luma_bytes(d) ((size_t)(d)->stride_y * ((d)->height + 2u * (d)->org_y))

/* ---- "the first caller computes the picture, the others wait" ----------------------------------------------------------
 * The reference's kernels are called per segment / block from several threads; a whole-picture entry point runs once.  An
 * entry is identified by (owner, key); `total` calls are expected per entry, after which it is recycled.  Never full: entries
 * are allocated on demand. */
typedef struct HdOnce HdOnce;
typedef struct HdOnceTable {
    HdOnce *head;
} HdOnceTable;
/* Exactly one caller of an entry runs compute(arg, &payload) (non-zero = ok); every other caller blocks until it has finished.
 * When it was ok, every caller gets take(arg, payload) to copy its share out; the last of the `total` callers frees the payload
 * with free_payload.  take / free_payload may be NULL.  Returns 0 = ok, 1 = not ok, -1 = no entry (out of memory). */
int hd_once_run(HdOnceTable *t, const void *owner, uint64_t key, uint32_t total, int (*compute)(void *arg, void **payload),
                void (*take)(void *arg, const void *payload), void (*free_payload)(void *), void *arg);

/* wall-clock spent inside each hook (summed over threads and calls; printed at exit): an HdCall adds its own; a hook's sub-steps use
 * hd_timer_add(name, hd_now_ns() - t0) */
uint64_t hd_now_ns(void);
void     hd_timer_add(const char *name, uint64_t ns);

/* statistics line of the glue at exit (svt_hip_bind_dev.c prints the PCIe totals and the mirror hit rate) */
void hd_count_picture(void);

#endif
