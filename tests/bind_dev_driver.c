/*
 * Driver of tests/test_bind_dev.py: tools/e2e/svt_hip_bind_dev.c (call scopes, "first caller computes", mirrors, pools) against a
 * fake device in host memory.  Every fake device call is counted, and the one with index FAIL_AT fails.
 *     bind_dev_driver script FAIL_AT | overflow | once | mirrors
 * A violated expectation ends the process with a message and status 1; the Python side also reads stdout / stderr.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "svt_hip_bind_dev.h"

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

/* ---- the fake device ------------------------------------------------------------------------------------------------------ */
static int g_calls, g_fail_at = -1, g_uploads, g_syncs;
static int tick(void) { return g_calls++ == g_fail_at ? -1 : 0; }

static int32_t fake_malloc(void **p, size_t n) { return tick() ? -1 : (*p = malloc(n)) ? 0 : -1; }
static int32_t fake_free(void *p) {
    if (tick())
        return -1;
    free(p);
    return 0;
}
static int32_t fake_upload(void *d, const void *h, size_t n, void *stream) {
    (void)stream;
    if (tick())
        return -1;
    g_uploads++;
    memcpy(d, h, n);
    return 0;
}
static int32_t fake_download(void *h, const void *d, size_t n, void *stream) {
    (void)stream;
    if (tick())
        return -1;
    memcpy(h, d, n);
    return 0;
}
static int32_t fake_memset(void *d, int v, size_t n, void *stream) {
    (void)stream;
    if (tick())
        return -1;
    memset(d, v, n);
    return 0;
}
static int32_t fake_sync(void *stream) {
    (void)stream;
    g_syncs++;
    return tick();
}
static const char *fake_last_error(void) { return "fake device error"; }
/* a "kernel": a library call that writes a pattern */
static int32_t fake_kernel(uint8_t *d, size_t n) {
    if (tick())
        return -1;
    for (size_t i = 0; i < n; i++) d[i] = (uint8_t)(i * 7 + 3);
    return 0;
}
static void *fake_sym(const char *name) {
    static const struct {
        const char *name;
        void       *fn;
    } tab[] = {{"svt_hip_malloc", (void *)fake_malloc},     {"svt_hip_free", (void *)fake_free},          {"svt_hip_upload", (void *)fake_upload},
               {"svt_hip_download", (void *)fake_download}, {"svt_hip_memset", (void *)fake_memset},      {"svt_hip_stream_sync", (void *)fake_sync},
               {"svt_hip_last_error", (void *)fake_last_error}}; /* no svt_hip_host_alloc: staging falls back to malloc */
    for (size_t i = 0; i < sizeof(tab) / sizeof(tab[0]); i++)
        if (strcmp(tab[i].name, name) == 0)
            return tab[i].fn;
    return NULL;
}
static void expect_nothing_in_use(void) {
    int pins, dev, host;
    hd_debug_in_use(&pins, &dev, &host);
    EXPECT(pins == 0 && dev == 0 && host == 0);
}

/* ---- the scripted call ---------------------------------------------------------------------------------------------------- */
#define N_RES 256
static void scripted_call(void) {
    static uint8_t plane[4][4096], params[512];
    uint8_t        dst[N_RES], pattern[N_RES];
    memset(dst, 0xEE, sizeof(dst));
    for (int i = 0; i < N_RES; i++) pattern[i] = (uint8_t)(i * 7 + 3);
    for (int k = 0; k < 4; k++) memset(plane[k], k + 1, sizeof(plane[k]));
    HdCall c;
    hd_call_begin(&c, "test_hook");
    for (int k = 0; k < 3; k++) hd_call_mirror(&c, plane[k], sizeof(plane[k]), HD_TAG(1, HD_ST_SOURCE));
    uint8_t *d_new = hd_call_mirror_new(&c, plane[3], sizeof(plane[3]), HD_TAG(1, HD_ST_SOURCE));
    uint8_t *d_out = hd_call_dev(&c, 1000), *d_tmp = hd_call_dev(&c, 70000);
    uint8_t *d_prm = hd_call_dev_put(&c, params, sizeof(params));
    uint8_t *h_out = (uint8_t *)hd_call_pinned(&c, N_RES);
    uint8_t *h_tmp = (uint8_t *)hd_call_host(&c, 100);
    if (hd_call_ok(&c)) {
        EXPECT(d_new && d_tmp && d_prm && ((uintptr_t)d_out & 255) == 0 && h_tmp[0] == 0 && h_tmp[99] == 0);
        int pins, dev, host;
        hd_debug_in_use(&pins, &dev, &host);
        EXPECT(pins == 4 && dev == 3 && host == 1);
        memcpy(d_new, plane[3], sizeof(plane[3])); /* "filled on the device" */
    }
    HD_CALL(&c, fake_kernel(d_out, N_RES));
    hd_call_download(&c, h_out, d_out, N_RES);
    for (int i = 0; i < N_RES; i++) EXPECT(dst[i] == 0xEE); /* nothing reaches the destination before the commit step */
    int committed = 0;
    if (hd_call_sync(&c) == 0) {
        memcpy(dst, h_out, N_RES);
        committed = 1;
    }
    const int failing = g_fail_at, calls_at_fail = failing + 1;
    const int ret = hd_call_end(&c, "bind_dev_driver: scripted call %d stays on the CPU", 7);
    const int total = g_calls;
    expect_nothing_in_use();
    if (failing < 0) {
        EXPECT(ret == 0 && committed && memcmp(dst, pattern, N_RES) == 0);
    } else {
        EXPECT(ret == 1 && !committed);
        for (int i = 0; i < N_RES; i++) EXPECT(dst[i] == 0xEE);
        /* sticky: after the failing call nothing but the final sync went to the device */
        EXPECT(total - calls_at_fail == 1 && g_syncs >= 1);
    }
    /* the mirror born in the call: resident after a success, dropped after a failure */
    const int up0 = g_uploads;
    HdCall    again;
    hd_call_begin(&again, NULL);
    EXPECT(hd_call_mirror(&again, plane[3], sizeof(plane[3]), HD_TAG(1, HD_ST_SOURCE)) != NULL);
    EXPECT(hd_call_end(&again, NULL) == 0);
    EXPECT(g_uploads - up0 == (failing < 0 ? 0 : 1));
    expect_nothing_in_use();
    printf("calls %d ret %d\n", total, ret);
}

/* ---- one acquisition more than the scope has room for --------------------------------------------------------------------- */
static void overflow(void) {
    static uint8_t hosts[(HD_CALL_PINS + 1) * 64];
    HdCall         c;
    hd_call_begin(&c, NULL);
    for (int i = 0; i < HD_CALL_PINS; i++) EXPECT(hd_call_mirror(&c, hosts + i * 64, 64, HD_TAG(2, HD_ST_SOURCE)) != NULL);
    EXPECT(hd_call_ok(&c));
    EXPECT(hd_call_mirror(&c, hosts + HD_CALL_PINS * 64, 64, HD_TAG(2, HD_ST_SOURCE)) == NULL && !hd_call_ok(&c));
    EXPECT(hd_call_end(&c, "bind_dev_driver: too many pins") == 1);
    expect_nothing_in_use();
    hd_call_begin(&c, NULL);
    for (int i = 0; i < HD_CALL_BLOCKS; i++) EXPECT(hd_call_host(&c, 8) != NULL);
    EXPECT(hd_call_dev(&c, 8) == NULL && hd_call_pinned(&c, 8) == NULL && hd_call_host(&c, 8) == NULL && !hd_call_ok(&c));
    EXPECT(hd_call_end(&c, "bind_dev_driver: too many blocks") == 1);
    expect_nothing_in_use();
}

/* ---- hd_once_run ---------------------------------------------------------------------------------------------------------- */
#define N_THREADS 8
static HdOnceTable g_tab;
static int         g_computed, g_freed, g_compute_ok;
typedef struct Caller {
    pthread_t th;
    int       rc, seen;
} Caller;
static int compute(void *arg, void **payload) {
    (void)arg;
    __atomic_add_fetch(&g_computed, 1, __ATOMIC_RELAXED);
    usleep(20000); /* the others arrive while the first one computes */
    int *p = (int *)malloc(sizeof(*p));
    *p = 42, *payload = p;
    return g_compute_ok;
}
static void take(void *arg, const void *payload) { ((Caller *)arg)->seen = *(const int *)payload; }
static void free_payload(void *p) {
    __atomic_add_fetch(&g_freed, 1, __ATOMIC_RELAXED);
    free(p);
}
static void *caller(void *arg) {
    Caller *c = (Caller *)arg;
    c->rc     = hd_once_run(&g_tab, &g_tab, 77, N_THREADS, compute, take, free_payload, c);
    return NULL;
}
static void once(int ok) {
    Caller c[N_THREADS];
    g_computed = g_freed = 0, g_compute_ok = ok;
    memset(c, 0, sizeof(c));
    for (int i = 0; i < N_THREADS; i++) pthread_create(&c[i].th, NULL, caller, &c[i]);
    for (int i = 0; i < N_THREADS; i++) pthread_join(c[i].th, NULL);
    EXPECT(g_computed == 1 && g_freed == 1 && g_tab.head == NULL);
    for (int i = 0; i < N_THREADS; i++) EXPECT(c[i].rc == (ok ? 0 : 1) && c[i].seen == (ok ? 42 : 0));
}

/* ---- mirrors under the scope ---------------------------------------------------------------------------------------------- */
static void mirrors(void) {
    static uint8_t host[8192];
    const char    *mb = getenv("SVTAV1_HIP_MIRROR_MB");
    const int      caching = !(mb && atoi(mb) == 0);
    int            pins, dev, blocks;
    HdCall         c;
    hd_call_begin(&c, NULL);
    uint8_t *a = hd_call_mirror(&c, host, sizeof(host), HD_TAG(3, HD_ST_SOURCE));
    uint8_t *b = hd_call_mirror(&c, host, sizeof(host), HD_TAG(3, HD_ST_SOURCE));
    EXPECT(a && a == b && g_uploads == 1); /* the same (host, tag) twice: one upload */
    EXPECT(hd_call_end(&c, NULL) == 0);
    hd_call_begin(&c, NULL);
    EXPECT(hd_call_mirror(&c, host, sizeof(host), HD_TAG(3, HD_ST_SOURCE)) != NULL);
    EXPECT(g_uploads == (caching ? 1 : 2)); /* budget 0: every call uploads */
    EXPECT(hd_call_end(&c, NULL) == 0);
    if (!caching)
        return;
    hd_call_begin(&c, NULL);
    EXPECT(hd_call_mirror(&c, host, sizeof(host), HD_TAG(3, HD_ST_FILTERED)) != NULL && g_uploads == 2); /* a new tag uploads again */
    hd_mirror_drop(host); /* pinned: deferred until the scope ends */
    hd_debug_in_use(&pins, &dev, &blocks);
    EXPECT(pins == 1);
    EXPECT(hd_call_end(&c, NULL) == 0);
    expect_nothing_in_use();
    hd_call_begin(&c, NULL);
    EXPECT(hd_call_mirror(&c, host, sizeof(host), HD_TAG(3, HD_ST_FILTERED)) != NULL && g_uploads == 3); /* it is gone now */
    EXPECT(hd_call_end(&c, NULL) == 0);
    expect_nothing_in_use();
}

int main(int argc, char **argv) {
    if (argc < 2)
        return 2;
    svt_hip_bind_dev_setup(fake_sym);
    EXPECT(g_hd.ok);
    if (strcmp(argv[1], "script") == 0 && argc > 2) {
        g_fail_at = atoi(argv[2]);
        scripted_call();
    } else if (strcmp(argv[1], "overflow") == 0)
        overflow();
    else if (strcmp(argv[1], "once") == 0)
        once(1), once(0);
    else if (strcmp(argv[1], "mirrors") == 0)
        mirrors();
    else
        return 2;
    return 0;
}
