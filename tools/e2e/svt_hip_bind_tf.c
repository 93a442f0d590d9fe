/*
 * svt_hip_bind_tf.c — OUR glue compiled into the reference encoder by tools/reference_hip.patch (Step 6b of INTEGRATION.md):
 * the block loop of produce_temporally_filtered_pic (Source/Lib/Codec/temporal_filtering.c:2752-3308) through the BATCHED entry
 * point svt_hip_tf_filter_picture.  The patch puts `if (svt_hip_bind_tf_picture(...))` in front of the reference's block loop:
 * the first temporal-filter segment of a picture that arrives here runs the WHOLE picture on the GPU (window pictures from the
 * device-resident picture mirrors of svt_hip_bind_dev.h, one call, the filtered centre picture downloaded into host staging and
 * copied into the planes the reference's loop would have written only once everything has succeeded — a failure half-way leaves
 * the picture untouched for the reference's own loop); the other segments of that picture wait for it and return.  What stays in the reference: which pictures are in the window and the
 * outlier tests (re-evaluated here exactly as at :3002-3030, they are scalar), the decay factors (computed by the reference
 * right before the hook), 10-bit packing before / unpacking after, padding + decimation of the filtered picture.
 * Active with `--asm hip` and SVTAV1_HIP_TIERB_TF=1; a picture this path does not cover (8x8 prediction, sub-64 pictures ...)
 * returns 1 and the reference's own loop runs.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "definitions.h"
#include "me_context.h"
#include "pcs.h"
#include "reference_object.h"
#include "sequence_control_set.h"

#include "svt_hip.h"
#include "svt_hip_tf.h"
#include "svt_hip_bind.h"
#include "svt_hip_bind_dev.h"

HD_FN(svt_hip_tf_filter_picture);
HD_FN(svt_hip_tf_workspace_bytes);
static int           g_active;
static unsigned long g_pictures, g_pictures_ld;
static __thread int  t_low_delay; /* the variant the calling thread is in (svt_hip_bind_tf_picture_ld) */

void svt_hip_bind_me_params(SvtHipMeParams *out, const PictureParentControlSet *pcs, const MeContext *me); /* svt_hip_bind_me.c */

static void report(void) {
    fprintf(stderr, "svt_hip_bind_tf: %lu pictures through svt_hip_tf_filter_picture (%lu of them the low-delay variant)\n", g_pictures, g_pictures_ld);
}

void svt_hip_bind_tf_setup(void *(*sym)(const char *)) {
    HD_SYM(sym, svt_hip_tf_filter_picture), HD_SYM(sym, svt_hip_tf_workspace_bytes);
    g_active = hd_env_on("SVTAV1_HIP_TIERB_TF") && g_hd.ok && p_svt_hip_tf_filter_picture && p_svt_hip_tf_workspace_bytes;
    if (g_active)
        atexit(report);
}

static HdOnceTable g_tab;

/* device copies of one picture of the window */
typedef struct DevPic {
    SvtHipTfPic pic;
    uint8_t    *d_hbd[3]; /* scratch; the 8-bit planes are mirrors */
    size_t      n_luma8, n_c8, n_hbd_y, n_hbd_c;
} DevPic;

/* 8-bit luma pyramid (the picture + its pa reference object's decimations) and 8-bit chroma from the mirrors -- "FILTERED" stands
 * for "what the buffer holds until this picture's own temporal filter rewrites it" (drop_picture_mirrors); the packed 16-bit
 * planes are per-call temporaries of the reference (altref_buffer_highbd) and go through scratch memory. */
static void put_picture(HdCall *c, DevPic *dp, PictureParentControlSet *pcs, EbPictureBufferDesc *pic, int is_highbd, int chroma, int scratch_8bit) {
    EbPaReferenceObject *pa = (EbPaReferenceObject *)pcs->pa_ref_pic_wrapper->object_ptr;
    EbPictureBufferDesc *pl[3] = {pic, pa->quarter_downsampled_picture_ptr, pa->sixteenth_downsampled_picture_ptr};
    SvtHipPlane8        *dst[3] = {&dp->pic.pyr.full, &dp->pic.pyr.quarter, &dp->pic.pyr.sixteenth};
    const uint64_t       tag = HD_TAG(pcs->picture_number, HD_ST_FILTERED);
    memset(dp, 0, sizeof(*dp));
    for (int k = 0; k < 3; k++) {
        dst[k]->stride = pl[k]->stride_y, dst[k]->org_x = pl[k]->org_x, dst[k]->org_y = pl[k]->org_y;
        dst[k]->width = pl[k]->width, dst[k]->height = pl[k]->height;
        if (k == 0 && scratch_8bit) /* the centre picture of an 8-bit filter: the caller supplies a scratch copy (filtered in place) */
            continue;
        dst[k]->buf = hd_call_mirror(c, pl[k]->buffer_y, hd_luma_bytes(pl[k]), tag);
    }
    dp->n_luma8            = hd_luma_bytes(pic);
    dp->pic.chroma8_stride = pic->stride_cb;
    dp->n_c8               = (size_t)pic->stride_cb * ((pic->height + 2u * pic->org_y) >> 1);
    if (chroma && !is_highbd && !scratch_8bit)
        for (int k = 0; k < 2; k++) dp->pic.chroma8[k] = hd_call_mirror(c, k ? pic->buffer_cr : pic->buffer_cb, dp->n_c8, tag);
    if (is_highbd) {
        dp->n_hbd_y = dp->n_luma8 * 2, dp->n_hbd_c = dp->n_c8 * 2;
        for (int k = 0; k < (chroma ? 3 : 1); k++)
            dp->pic.hbd[k] = (uint16_t *)(dp->d_hbd[k] = hd_call_dev_put(c, pcs->altref_buffer_highbd[k], k ? dp->n_hbd_c : dp->n_hbd_y));
    }
    dp->pic.picture_number = pcs->picture_number;
}

/* The temporal filter is about to rewrite (or has rewritten) the centre picture: its source planes and, right behind the block
 * loop, the pa reference object's padded copy and decimations (temporal_filtering.c: pad + decimate of the filtered picture). */
static void drop_picture_mirrors(PictureParentControlSet *pcs, EbPictureBufferDesc *pic) {
    EbPaReferenceObject *pa = (EbPaReferenceObject *)pcs->pa_ref_pic_wrapper->object_ptr;
    hd_mirror_drop(pic->buffer_y), hd_mirror_drop(pic->buffer_cb), hd_mirror_drop(pic->buffer_cr);
    if (pa->input_padded_pic)
        hd_mirror_drop(pa->input_padded_pic->buffer_y);
    hd_mirror_drop(pa->quarter_downsampled_picture_ptr->buffer_y), hd_mirror_drop(pa->sixteenth_downsampled_picture_ptr->buffer_y);
}

static int run_picture(PictureParentControlSet **pcs_list, EbPictureBufferDesc **pics, int index_center, MeContext *ctx, int is_highbd, uint32_t tot[2]) {
    PictureParentControlSet *centre = pcs_list[index_center];
    SequenceControlSet      *scs    = centre->scs;
    EbPictureBufferDesc     *cpic   = pics[index_center];
    const TfControls        *tc     = &ctx->tf_ctrls;
    HdCall                   c;
    hd_call_begin(&c, "tf_picture");
    if ((tc->enable_8x8_pred && !centre->enable_me_8x8) /* tf_8x8_sub_pel_search starts from the ME's 8x8 vectors */ || scs->subsampling_x != 1 || scs->subsampling_y != 1 || cpic->width < 64 || cpic->height < 64 || cpic->org_x < 68 ||
        cpic->org_y < 68 || cpic->stride_cb * 2 != cpic->stride_y || (is_highbd && scs->static_config.encoder_bit_depth != 10))
        return hd_call_decline(&c);
    /* the pictures filtered against, in the reference's order, with its outlier tests (temporal_filtering.c:2990-3030) */
    int       idx[ALTREF_MAX_NFRAMES], n = 0;
    const int start[3] = {0, centre->past_altref_nframes, centre->past_altref_nframes + 1};
    const int end[3]   = {centre->past_altref_nframes - 1, centre->past_altref_nframes, centre->past_altref_nframes + centre->future_altref_nframes};
    for (int seg = 0; seg < 3; seg++)
        for (int fi = start[seg]; fi <= end[seg]; fi += tc->ref_frame_factor) {
            if (fi == index_center)
                continue;
            const uint32_t low_ahd_err = centre->aligned_width * centre->aligned_height;
            const uint8_t  th          = (centre->slice_type == I_SLICE) ? 20 : 40;
            if (pcs_list[fi]->tf_ahd_error_to_central > low_ahd_err &&
                ((int)(((int)pcs_list[fi]->tf_ahd_error_to_central - (int)centre->tf_avg_ahd_error) * 100)) > (th * (int)centre->tf_avg_ahd_error))
                continue;
            uint32_t bright = 0;
            for (uint32_t w = 0; w < scs->picture_analysis_number_of_regions_per_width; w++)
                for (uint32_t h = 0; h < scs->picture_analysis_number_of_regions_per_height; h++)
                    if (abs((int)pcs_list[fi]->average_intensity_per_region[w][h] - (int)centre->average_intensity_per_region[w][h]) > 2 &&
                        pcs_list[fi]->avg_luma != centre->tf_avg_luma)
                        bright++;
            if (bright >= ((14 * scs->picture_analysis_number_of_regions_per_width * scs->picture_analysis_number_of_regions_per_height) / 16))
                continue;
            idx[n++] = fi;
        }
    if (n == 0 || n > SVT_HIP_TF_MAX_REFS)
        return hd_call_decline(&c); /* nothing to filter against: the reference's loop does central + normalise, which leaves the picture as it is */
    SvtHipTfPictureJob *job = (SvtHipTfPictureJob *)hd_call_host(&c, sizeof(*job));
    if (!job)
        return hd_call_end(&c, "svt_hip_bind_tf: picture %llu stays on the CPU", (unsigned long long)centre->picture_number);
    /* ME parameters: the MeContext as svt_aom_sig_deriv_me_tf left it + what create_me_context_and_picture_control and the frame loop set */
    svt_hip_bind_me_params(&job->me, centre, ctx);
    job->me.me_mctf = 1, job->me.hme_search_method = 1, job->me.tf_me_exit_th = (uint16_t)tc->me_exit_th;
    job->me.hme_l0_sa_min.width = ctx->hme_l0_sa_default_tf.sa_min.width, job->me.hme_l0_sa_min.height = ctx->hme_l0_sa_default_tf.sa_min.height;
    job->me.hme_l0_sa_max.width = ctx->hme_l0_sa_default_tf.sa_max.width, job->me.hme_l0_sa_max.height = ctx->hme_l0_sa_default_tf.sa_max.height;
    job->me.num_of_list_to_search = 1, job->me.num_of_ref_pic_to_search[0] = 1, job->me.num_of_ref_pic_to_search[1] = 0;
    job->me.temporal_layer_index = centre->temporal_layer_index, job->me.is_ref = centre->is_ref;
    if (!job->me.max_refs)
        job->me.max_refs = 1;
    if (!job->me.max_cand)
        job->me.max_cand = 1;
    job->ctrls.half_pel_mode = tc->half_pel_mode, job->ctrls.quarter_pel_mode = tc->quarter_pel_mode, job->ctrls.eight_pel_mode = tc->eight_pel_mode;
    job->ctrls.use_2tap = tc->use_2tap, job->ctrls.sub_sampling_shift = tc->sub_sampling_shift;
    job->ctrls.use_pred_64x64_only_th = tc->use_pred_64x64_only_th, job->ctrls.subpel_early_exit_th = tc->subpel_early_exit_th;
    job->ctrls.use_8bit_subpel = tc->use_8bit_subpel, job->ctrls.use_zz_based_filter = tc->use_zz_based_filter;
    job->ctrls.pred_error_32x32_th = tc->pred_error_32x32_th;
    job->ctrls.low_delay           = (uint8_t)t_low_delay;
    job->ctrls.enable_8x8_pred     = tc->enable_8x8_pred ? 1 : 0;
    for (int p = 0; p < 3; p++) job->decay_factor_fp16[p] = ctx->tf_decay_factor_fp16[p];
    job->mv_dist_th = ctx->tf_mv_dist_th, job->chroma = ctx->tf_chroma, job->bit_depth = is_highbd ? 10 : 8;
    job->mi_rows = (uint32_t)centre->av1_cm->mi_rows, job->mi_cols = (uint32_t)centre->av1_cm->mi_cols, job->n_refs = (uint32_t)n;

    const uint64_t wsb = p_svt_hip_tf_workspace_bytes(cpic->width, cpic->height, (uint32_t)n);
    uint8_t       *ws  = hd_call_dev(&c, hd_al256(wsb));
    DevPic         dc, dr;
    put_picture(&c, &dc, centre, cpic, is_highbd, job->chroma, !is_highbd);
    job->centre = dc.pic;
    for (int k = 0; k < n; k++) {
        put_picture(&c, &dr, pcs_list[idx[k]], pics[idx[k]], is_highbd, job->chroma, 0);
        job->ref[k] = dr.pic;
    }
    /* the kernel filters the centre picture IN PLACE on the device: it must not do that to the cached mirror (a later window may
     * ask for the unfiltered picture again if this call fails) -- the centre's 8-bit planes are fresh scratch copies (uploaded from
     * the host: the same bytes the mirror holds); the 16-bit planes already are scratch (dc.d_hbd) */
    const int np       = job->chroma ? 3 : 1;
    uint8_t  *d_out[3] = {NULL, NULL, NULL}, *h_out[3] = {NULL, NULL, NULL};
    size_t    n_out[3] = {0, 0, 0};
    for (int k = 0; k < np; k++) {
        const uint8_t *hsrc[3] = {cpic->buffer_y, cpic->buffer_cb, cpic->buffer_cr};
        n_out[k] = is_highbd ? (k ? dc.n_hbd_c : dc.n_hbd_y) : (k ? dc.n_c8 : dc.n_luma8);
        d_out[k] = is_highbd ? dc.d_hbd[k] : hd_call_dev_put(&c, hsrc[k], n_out[k]);
    }
    if (!is_highbd) {
        job->centre.pyr.full.buf = d_out[0];
        if (job->chroma)
            job->centre.chroma8[0] = d_out[1], job->centre.chroma8[1] = d_out[2];
    }
    uint32_t *d_tot = ws ? (uint32_t *)(ws + hd_al256(wsb)) : NULL;
    job->workspace = ws, job->workspace_bytes = wsb, job->tot_blks = d_tot;
    hd_call_memset(&c, d_tot, 0, 8);
    HD_CALL(&c, p_svt_hip_tf_filter_picture(job, NULL));
    /* the filtered centre picture into host staging; into the encoder's planes only when all of it has arrived */
    for (int k = 0; k < np; k++) {
        h_out[k] = (uint8_t *)hd_call_pinned(&c, n_out[k]);
        hd_call_download(&c, h_out[k], d_out[k], n_out[k]);
    }
    hd_call_download(&c, tot, d_tot, 8);
    if (hd_call_sync(&c) == 0) {
        uint8_t *hdst[3] = {cpic->buffer_y, cpic->buffer_cb, cpic->buffer_cr};
        for (int k = 0; k < np; k++) memcpy(is_highbd ? (uint8_t *)centre->altref_buffer_highbd[k] : hdst[k], h_out[k], n_out[k]);
    }
    if (hd_call_end(&c, "svt_hip_bind_tf: picture %llu stays on the CPU", (unsigned long long)centre->picture_number))
        return 1;
    hd_count_picture();
    return 0;
}

/* Returns 0 when the picture has been filtered on the GPU (the caller skips its block loop), 1 when the caller must run it. */
typedef struct TfArgs {
    PictureParentControlSet **pcs_list;
    EbPictureBufferDesc     **pics;
    int                       index_center, is_highbd;
    MeContext                *ctx;
} TfArgs;
/* the first temporal-filter segment of a picture that arrives filters all of it (hd_once_run) */
static int tf_first(void *arg, void **payload) {
    (void)payload;
    const TfArgs            *a      = (const TfArgs *)arg;
    PictureParentControlSet *centre = a->pcs_list[a->index_center];
    uint32_t                 tot[2] = {0, 0};
    const int                rc     = run_picture(a->pcs_list, a->pics, a->index_center, a->ctx, a->is_highbd, tot);
    /* either way the centre picture changes now: here (GPU) or in the reference's loop right behind this call (CPU) */
    drop_picture_mirrors(centre, a->pics[a->index_center]);
    if (rc == 0) {
        /* tf_tot_*_blks of the whole picture go to this segment's context (the caller adds every segment's into the pcs) */
        a->ctx->tf_tot_horz_blks += tot[0], a->ctx->tf_tot_vert_blks += tot[1];
        __atomic_add_fetch(&g_pictures, 1, __ATOMIC_RELAXED);
        if (t_low_delay)
            __atomic_add_fetch(&g_pictures_ld, 1, __ATOMIC_RELAXED);
    }
    return rc == 0;
}
static int tf_picture(PictureParentControlSet **pcs_list, EbPictureBufferDesc **pics, int index_center, MeContext *ctx, int is_highbd) {
    PictureParentControlSet *centre = pcs_list[index_center];
    TfArgs                   a      = {pcs_list, pics, index_center, is_highbd, ctx};
    const int rc = g_active ? hd_once_run(&g_tab, centre, centre->picture_number, centre->tf_segments_total_count, tf_first, NULL, NULL, &a) : -1;
    if (rc < 0 && g_hd.ok)
        drop_picture_mirrors(centre, pics[index_center]); /* not through the table: other hooks may hold mirrors of the picture this loop rewrites */
    return rc != 0;
}
int svt_hip_bind_tf_picture(PictureParentControlSet **pcs_list, EbPictureBufferDesc **pics, int index_center, MeContext *ctx, int is_highbd) {
    t_low_delay = 0;
    return tf_picture(pcs_list, pics, index_center, ctx, is_highbd);
}
/* the same in front of the block loop of produce_temporally_filtered_pic_ld (pred_structure LOW_DELAY_B): co-located predictions, no search */
int svt_hip_bind_tf_picture_ld(PictureParentControlSet **pcs_list, EbPictureBufferDesc **pics, int index_center, MeContext *ctx, int is_highbd) {
    static int traced = -1; /* SVTAV1_E2E_TRACE_TF_LD=1: says once that the encoder reached this variant (tests, also without a GPU) */
    if (traced < 0)
        traced = getenv("SVTAV1_E2E_TRACE_TF_LD") != NULL;
    if (traced == 1 && __atomic_exchange_n(&traced, 2, __ATOMIC_RELAXED) == 1)
        fprintf(stderr, "svt_hip_bind_tf: produce_temporally_filtered_pic_ld reached (picture %llu)\n", (unsigned long long)pcs_list[index_center]->picture_number);
    t_low_delay = 1;
    const int rc = tf_picture(pcs_list, pics, index_center, ctx, is_highbd);
    t_low_delay  = 0;
    return rc;
}
