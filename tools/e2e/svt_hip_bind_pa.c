/*
 * svt_hip_bind_pa.c — OUR glue compiled into the reference encoder by tools/reference_hip.patch (Step 2a of INTEGRATION.md): the
 * picture-analysis kernel's per-picture luma work through the batched entry points of include/svt_hip_me.h:
 *
 *   svt_hip_bind_pa_pyramid    in front of the body of svt_aom_downsample_filtering_input_picture (pic_analysis_process.c:1922-1979,
 *                              called at :2126) -> svt_hip_pyramid_frame: 1/4 and 1/16 decimation with their padding, one call.
 *   svt_hip_bind_pa_variance   in front of the b64 loop of compute_picture_spatial_statistics (:1532-1553, called through
 *                              svt_aom_gathering_picture_statistics at :2137) -> svt_hip_variance_frame: the 85 block variances of
 *                              every 64x64 block.
 *
 * The picture is uploaded ONCE here, into the device-resident mirrors of svt_hip_bind_dev.h; the two decimated planes are born
 * on the device and become the mirrors of the host planes they are downloaded into — the open-loop ME of this picture and of
 * every picture that references it, the temporal filter and the TPL dispenser then find all of it resident (no further upload).
 * Returns 0 when the GPU did the work, 1 when the caller must run the reference's code.  Active with `--asm hip` and
 * SVTAV1_HIP_TIERB_PA=1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "definitions.h"
#include "me_context.h"
#include "pcs.h"
#include "sequence_control_set.h"

#include "svt_hip.h"
#include "svt_hip_me.h"
#include "svt_hip_bind.h"
#include "svt_hip_bind_dev.h"

HD_FN(svt_hip_pyramid_frame);
HD_FN(svt_hip_variance_frame);
static int           g_active;
static unsigned long g_n_pyr, g_n_var;

static void report(void) {
    fprintf(stderr, "svt_hip_bind_pa: %lu pyramids, %lu variance maps through svt_hip_pyramid_frame / svt_hip_variance_frame\n", g_n_pyr, g_n_var);
}

void svt_hip_bind_pa_setup(void *(*sym)(const char *)) {
    HD_SYM(sym, svt_hip_pyramid_frame), HD_SYM(sym, svt_hip_variance_frame);
    g_active = hd_env_on("SVTAV1_HIP_TIERB_PA") && g_hd.ok && p_svt_hip_pyramid_frame && p_svt_hip_variance_frame;
    if (g_active)
        atexit(report);
}

static void plane_of(SvtHipPlane8 *p, const EbPictureBufferDesc *d, uint8_t *dev) {
    p->buf = dev, p->stride = d->stride_y, p->org_x = d->org_x, p->org_y = d->org_y, p->width = d->width, p->height = d->height;
}
/* paddings the library asks for (include/svt_hip_me.h: >= 64 / 32 / 16, the decimated planes exactly half / a quarter) */
static int geometry_ok(const EbPictureBufferDesc *f, const EbPictureBufferDesc *q, const EbPictureBufferDesc *s) {
    return f->org_x >= 64 && f->org_y >= 64 && q->org_x >= 32 && q->org_y >= 32 && s->org_x >= 16 && s->org_y >= 16 && q->org_x == q->org_y &&
        s->org_x == s->org_y /* the reference's destination offset uses org_x twice (:1934, :1953) */ && q->width == f->width >> 1 &&
        q->height == f->height >> 1 && s->width == f->width >> 2 && s->height == f->height >> 2;
}

int svt_hip_bind_pa_pyramid(PictureParentControlSet *pcs, EbPictureBufferDesc *full, EbPictureBufferDesc *quarter, EbPictureBufferDesc *sixteenth) {
    if (!g_active)
        return 1;
    HdCall c;
    hd_call_begin(&c, "pa_pyramid");
    if (!(pcs->enable_hme_flag || pcs->tf_enable_hme_flag) || !(pcs->enable_hme_level0_flag || pcs->tf_enable_hme_level0_flag) ||
        !geometry_ok(full, quarter, sixteenth))
        return hd_call_decline(&c);
    const int      level1 = pcs->enable_hme_level1_flag || pcs->tf_enable_hme_level1_flag;
    const uint64_t tag    = HD_TAG(pcs->picture_number, HD_ST_FILTERED);
    const size_t   nq = hd_luma_bytes(quarter), ns = hd_luma_bytes(sixteenth);
    const uint64_t t_a = hd_now_ns();
    uint8_t       *d_f = hd_call_mirror(&c, full->buffer_y, hd_luma_bytes(full), tag);
    hd_timer_add("pa_pyramid.1_source_mirror", hd_now_ns() - t_a);
    const uint64_t t_b = hd_now_ns();
    /* the decimated planes are produced on the device: their buffers become the mirrors of the host planes (a failed call drops them) */
    uint8_t *d_q = level1 ? hd_call_mirror_new(&c, quarter->buffer_y, nq, tag) : hd_call_dev(&c, nq);
    uint8_t *d_s = hd_call_mirror_new(&c, sixteenth->buffer_y, ns, tag);
    uint8_t *h_q = level1 ? (uint8_t *)hd_call_pinned(&c, nq) : NULL, *h_s = (uint8_t *)hd_call_pinned(&c, ns);
    hd_timer_add("pa_pyramid.2_alloc", hd_now_ns() - t_b);
    const uint64_t t_c = hd_now_ns();
    SvtHipPlane8   pf, pq, ps;
    plane_of(&pf, full, d_f), plane_of(&pq, quarter, d_q), plane_of(&ps, sixteenth, d_s);
    /* a plane keeps the bytes the kernel does not write (row tails behind the padding): start from the host's */
    if (level1)
        hd_call_upload(&c, d_q, quarter->buffer_y, nq);
    hd_call_upload(&c, d_s, sixteenth->buffer_y, ns);
    HD_CALL(&c, p_svt_hip_pyramid_frame(&pf, &pq, &ps, level1, NULL));
    if (level1)
        hd_call_download(&c, h_q, d_q, nq);
    hd_call_download(&c, h_s, d_s, ns);
    const int arrived = hd_call_sync(&c) == 0;
    hd_timer_add("pa_pyramid.3_upload_kernel_download", hd_now_ns() - t_c);
    const uint64_t t_d = hd_now_ns();
    if (arrived) {
        if (level1)
            memcpy(quarter->buffer_y, h_q, nq);
        memcpy(sixteenth->buffer_y, h_s, ns);
    }
    hd_timer_add("pa_pyramid.4_copy_out", hd_now_ns() - t_d);
    if (hd_call_end(&c, "svt_hip_bind_pa: pyramid of picture %llu stays on the CPU", (unsigned long long)pcs->picture_number))
        return 1;
    __atomic_add_fetch(&g_n_pyr, 1, __ATOMIC_RELAXED);
    hd_count_picture();
    return 0;
}

int svt_hip_bind_pa_variance(SequenceControlSet *scs, PictureParentControlSet *pcs, EbPictureBufferDesc *full) {
    if (!g_active)
        return 1;
    HdCall c;
    hd_call_begin(&c, "pa_variance");
    const uint32_t nb = pcs->b64_total_count;
    if (full->org_x < 64 || full->org_y < 64 || nb != ((uint32_t)(pcs->aligned_width + 63) / 64) * ((uint32_t)(pcs->aligned_height + 63) / 64))
        return hd_call_decline(&c);
    const size_t n   = (size_t)nb * 85 * sizeof(uint16_t);
    uint8_t     *d_f = hd_call_mirror(&c, full->buffer_y, hd_luma_bytes(full), HD_TAG(pcs->picture_number, HD_ST_FILTERED));
    uint8_t     *dev = hd_call_dev(&c, n);
    uint16_t    *h   = (uint16_t *)hd_call_host(&c, n);
    SvtHipPlane8 pf;
    plane_of(&pf, full, d_f);
    pf.width = pcs->aligned_width, pf.height = pcs->aligned_height; /* the b64 grid of the reference's loop (b64_geom) */
    HD_CALL(&c, p_svt_hip_variance_frame(&pf, (uint16_t *)dev, NULL, scs->block_mean_calc_prec == BLOCK_MEAN_PREC_FULL, NULL));
    hd_call_download(&c, h, dev, n);
    if (hd_call_sync(&c) == 0) {
        /* what compute_block_mean_compute_variance stores (:1111-1380): all 85 with adaptive quantisation 1 or variance_octile, else
         * only the 64x64 entry; then the picture average (:1547-1550) */
        const int all       = scs->static_config.enable_adaptive_quantization == 1 || scs->static_config.variance_octile;
        uint64_t  pic_total = 0;
        for (uint32_t b = 0; b < nb; b++) {
            if (all)
                memcpy(pcs->variance[b], h + (size_t)b * 85, 85 * sizeof(uint16_t));
            else
                pcs->variance[b][ME_TIER_ZERO_PU_64x64] = h[(size_t)b * 85 + ME_TIER_ZERO_PU_64x64];
            pic_total += pcs->variance[b][RASTER_SCAN_CU_INDEX_64x64];
        }
        pcs->pic_avg_variance = (uint16_t)(pic_total / nb);
    }
    if (hd_call_end(&c, "svt_hip_bind_pa: variance of picture %llu stays on the CPU", (unsigned long long)pcs->picture_number))
        return 1;
    __atomic_add_fetch(&g_n_var, 1, __ATOMIC_RELAXED);
    return 0;
}
