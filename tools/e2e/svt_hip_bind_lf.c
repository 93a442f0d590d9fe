/*
 * svt_hip_bind_lf.c — OUR glue compiled into the reference encoder by tools/reference_hip.patch (Step 4 of INTEGRATION.md): the
 * in-loop filters of a whole picture through the batched entry points of include/svt_hip_lf.h, called from the reference's own
 * kernels (dlf_process.c, cdef_process.c, rest_process.c and the functions they call):
 *
 *   svt_hip_bind_dlf_frame      in front of the SB loop of svt_av1_loop_filter_frame (deblocking_filter.c:624-653): covers the final
 *                               frame filter of dlf_process.c:106 AND every trial of the level search (try_filter_frame, :872)
 *                               -> svt_hip_loop_filter_frame.  With SB-based deblocking (presets M6+, coding_loop.c:2260-2281) the
 *                               per-SB call is skipped when svt_hip_bind_dlf_deferred() and dlf_process.c makes ONE frame call
 *                               instead (the frame order is equivalent to the SB schedule: tests/test_gpu_lf.py proves it against
 *                               the real function), so the deferral is correct whether that call then runs on the GPU or not.
 *   svt_hip_bind_cdef_seg       in front of cdef_seg_search (cdef_process.c:106-349): the first segment of a picture searches ALL
 *                               filter blocks of all planes -> svt_hip_cdef_search_plane x 3; results into pcs->mse_seg /
 *                               cdef_dir_data / skip_cdef_seg exactly where the reference's loop stores them.
 *   svt_hip_bind_cdef_frame     in front of svt_av1_cdef_frame (enc_cdef.c:284-610) -> svt_hip_cdef_apply_frame.
 *   svt_hip_bind_wiener_stats   in front of svt_av1_compute_stats(_highbd) in search_wiener_seg (restoration_pick.c:1322-1346):
 *                               the first unit of a plane that asks computes M / H of ALL units of the plane ->
 *                               svt_hip_wiener_stats; every unit then copies its own.
 *   svt_hip_bind_lr_frame       in front of svt_av1_loop_restoration_filter_frame (restoration.c:1179-1248) ->
 *                               svt_hip_restoration_filter_frame.
 *
 * Every hook returns 0 when the GPU did the work and 1 when the caller must run the reference's own code (feature off,
 * configuration not covered, any failure: results reach the encoder's buffers only after everything has succeeded).
 * Pictures travel through the device-resident mirrors of svt_hip_bind_dev.h: one upload per stage input (reconstruction before
 * deblocking / after deblocking / after CDEF, the source picture), shared by the calls of that stage (all trials of the
 * deblocking level search, CDEF search + apply, Wiener statistics + final restoration).
 * Active with `--asm hip` and SVTAV1_HIP_TIERB_DLF / _CDEF / _LR = 1.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "definitions.h"
#include "av1_common.h"
#include "cdef.h"
#include "deblocking_common.h"
#include "deblocking_filter.h"
#include "pcs.h"
#include "restoration.h"
#include "sequence_control_set.h"
#include "utility.h"

#include "svt_hip.h"
#include "svt_hip_lf.h"
#include "svt_hip_txfm.h" /* svt_hip_plane_sse */
#include "svt_hip_bind.h"
#include "svt_hip_bind_dev.h"

void svt_aom_get_recon_pic(PictureControlSet *pcs, EbPictureBufferDesc **recon_ptr, Bool is_highbd);

HD_FN(svt_hip_loop_filter_frame);
HD_FN(svt_hip_cdef_search_plane);
HD_FN(svt_hip_cdef_apply_frame);
HD_FN(svt_hip_wiener_stats);
HD_FN(svt_hip_restoration_filter_frame);
HD_FN(svt_hip_copy);
HD_FN(svt_hip_plane_sse);
HD_FN(svt_hip_download_2d);
static int g_dlf, g_cdef, g_lr;
static unsigned long g_n_dlf, g_n_dlf_trials, g_n_cdef_search, g_n_cdef_apply, g_n_wiener, g_n_lr;

static void report(void) {
    fprintf(stderr,
            "svt_hip_bind_lf: %lu frame deblocking calls, %lu CDEF searches, %lu CDEF applications, %lu Wiener statistics planes, %lu restoration "
            "frames on the GPU; %lu trials of the deblocking level search filtered and measured on the device\n",
            g_n_dlf, g_n_cdef_search, g_n_cdef_apply, g_n_wiener, g_n_lr, g_n_dlf_trials);
}

void svt_hip_bind_lf_setup(void *(*sym)(const char *)) {
    HD_SYM(sym, svt_hip_loop_filter_frame), HD_SYM(sym, svt_hip_cdef_search_plane), HD_SYM(sym, svt_hip_cdef_apply_frame);
    HD_SYM(sym, svt_hip_wiener_stats), HD_SYM(sym, svt_hip_restoration_filter_frame);
    HD_SYM(sym, svt_hip_copy), HD_SYM(sym, svt_hip_plane_sse), HD_SYM(sym, svt_hip_download_2d);
    const int base = g_hd.ok && p_svt_hip_copy && p_svt_hip_download_2d;
    g_dlf          = base && hd_env_on("SVTAV1_HIP_TIERB_DLF") && p_svt_hip_loop_filter_frame;
    g_cdef         = base && hd_env_on("SVTAV1_HIP_TIERB_CDEF") && p_svt_hip_cdef_search_plane && p_svt_hip_cdef_apply_frame;
    g_lr           = base && hd_env_on("SVTAV1_HIP_TIERB_LR") && p_svt_hip_wiener_stats && p_svt_hip_restoration_filter_frame;
    if (g_dlf || g_cdef || g_lr)
        atexit(report);
}

/* ---- picture planes --------------------------------------------------------------------------------------------------- */
typedef struct PlaneRef {
    uint8_t *host;   /* start of the allocation (padding included) */
    size_t   bytes;  /* of the allocation */
    size_t   origin; /* byte offset of sample (0, 0) */
    uint32_t stride; /* samples */
} PlaneRef;

static void picture_planes(const EbPictureBufferDesc *pic, int is16, PlaneRef out[3]) {
    out[0].host = pic->buffer_y, out[0].bytes = (size_t)pic->luma_size << is16, out[0].stride = pic->stride_y;
    out[0].origin = ((size_t)pic->org_y * pic->stride_y + pic->org_x) << is16;
    out[1].host = pic->buffer_cb, out[1].bytes = (size_t)pic->chroma_size << is16, out[1].stride = pic->stride_cb;
    out[1].origin = ((size_t)(pic->org_y >> 1) * pic->stride_cb + (pic->org_x >> 1)) << is16;
    out[2].host = pic->buffer_cr, out[2].bytes = (size_t)pic->chroma_size << is16, out[2].stride = pic->stride_cr;
    out[2].origin = ((size_t)(pic->org_y >> 1) * pic->stride_cr + (pic->org_x >> 1)) << is16;
}

static int covered(const PictureControlSet *pcs) {
    const SequenceControlSet *scs = pcs->scs;
    return scs->subsampling_x == 1 && scs->subsampling_y == 1 && scs->sb_size == 64 && !pcs->ppcs->frame_superres_enabled &&
        !pcs->ppcs->frame_resize_enabled && scs->static_config.resize_mode == RESIZE_NONE &&
        (scs->static_config.encoder_bit_depth == 8 || scs->static_config.encoder_bit_depth == 10);
}

/* ============================================================ deblocking ================================================== */
/* SVTAV1_HIP_DLF_DEFER_TEST=1 defers also without a device (the frame call then runs the reference's own loops): the CPU test of
 * the claim that one frame call behind EncDec equals the per-SB calls inside it (tests/test_e2e.py) */
int svt_hip_bind_dlf_deferred(void) {
    static int forced = -1;
    if (forced < 0)
        forced = hd_env_on("SVTAV1_HIP_DLF_DEFER_TEST");
    return g_dlf || forced;
}

/* the mode-info records of a picture, gathered once per picture (the level search calls the frame filter up to ~20 times) */
typedef struct MiGather {
    const void *grid; /* pcs->mi_grid_base */
    uint64_t    picture_number;
    SvtHipLfMi *mi;
    size_t      n;
} MiGather;
#define N_GATHER 8
static MiGather        g_gather[N_GATHER];
static unsigned        g_gather_next;
static pthread_mutex_t g_gather_mu = PTHREAD_MUTEX_INITIALIZER;

/* one 8-byte record per 4x4 from the fields set_lpf_parameters reads (deblocking_filter.c:162-282) */
static const SvtHipLfMi *gather_mi(PictureControlSet *pcs, size_t *bytes) {
    const Av1Common *cm = pcs->ppcs->av1_cm;
    const size_t     n  = (size_t)cm->mi_rows * pcs->mi_stride;
    pthread_mutex_lock(&g_gather_mu);
    for (int i = 0; i < N_GATHER; i++)
        if (g_gather[i].mi && g_gather[i].grid == pcs->mi_grid_base && g_gather[i].picture_number == pcs->picture_number && g_gather[i].n == n) {
            *bytes = n * sizeof(SvtHipLfMi);
            pthread_mutex_unlock(&g_gather_mu);
            return g_gather[i].mi;
        }
    MiGather *g = &g_gather[g_gather_next++ % N_GATHER];
    if (g->mi)
        hd_mirror_drop(g->mi);
    SvtHipLfMi *mi = (SvtHipLfMi *)realloc(g->mi, n * sizeof(*mi));
    if (!mi) {
        free(g->mi), g->mi = NULL;
        pthread_mutex_unlock(&g_gather_mu);
        return NULL;
    }
    for (int32_t r = 0; r < cm->mi_rows; r++)
        for (int32_t c = 0; c < pcs->mi_stride; c++) {
            SvtHipLfMi     *o = &mi[(size_t)r * pcs->mi_stride + c];
            const ModeInfo *p = pcs->mi_grid_base[(size_t)r * pcs->mi_stride + c];
            memset(o, 0, sizeof(*o));
            if (!p || c >= cm->mi_cols)
                continue;
            const BlockModeInfoEnc *b          = &p->mbmi.block_mi;
            const int               skip_inter = b->skip && is_inter_block_no_intrabc(b->ref_frame[0]);
            o->bsize                           = (uint8_t)b->bsize;
            o->tx_size_y                       = (uint8_t)tx_depth_to_tx_size[skip_inter ? 0 : b->tx_depth][b->bsize];
            o->tx_size_uv                      = (uint8_t)av1_get_max_uv_txsize(b->bsize, 1, 1);
            o->skip_inter                      = (uint8_t)skip_inter;
            o->segment_id                      = b->segment_id;
            o->ref_frame0                      = (uint8_t)b->ref_frame[0];
            o->mode_lf                         = (uint8_t)mode_lf_lut[b->mode];
        }
    g->mi = mi, g->grid = pcs->mi_grid_base, g->picture_number = pcs->picture_number, g->n = n;
    *bytes = n * sizeof(SvtHipLfMi);
    pthread_mutex_unlock(&g_gather_mu);
    return mi;
}

/* The frame filter (trial_sse == NULL: the filtered planes go back into the encoder's buffer) or one trial of the level search (the
 * filtered plane is only measured against the source picture, on the device). */
static int deblock(EbPictureBufferDesc *frame_buffer, PictureControlSet *pcs, int32_t plane_start, int32_t plane_end, int64_t *trial_sse) {
    HdCall c;
    hd_call_begin(&c, trial_sse ? "dlf_trial" : "dlf_frame");
    if (!covered(pcs) || pcs->ppcs->frm_hdr.delta_lf_params.delta_lf_present || plane_start < 0 || plane_end > 3 || plane_start >= plane_end)
        return hd_call_decline(&c);
    SequenceControlSet      *scs  = pcs->scs;
    PictureParentControlSet *ppcs = pcs->ppcs;
    const Av1Common         *cm   = ppcs->av1_cm;
    const int                is16 = scs->is_16bit_pipeline;
    /* what svt_av1_loop_filter_frame does first (:640) */
    svt_av1_loop_filter_frame_init(&ppcs->frm_hdr, &ppcs->lf_info, plane_start, plane_end);
    PlaneRef pl[3];
    picture_planes(frame_buffer, is16, pl);
    size_t            mi_bytes = 0;
    const SvtHipLfMi *h_mi     = gather_mi(pcs, &mi_bytes);
    if (!h_mi)
        return hd_call_decline(&c);
    uint8_t *d_mi = hd_call_mirror(&c, h_mi, mi_bytes, HD_TAG(pcs->picture_number, HD_ST_MI_LF));
    /* the planes to filter: a scratch copy of the mirror of the picture as EncDec left it (the level search filters that same
     * picture again and again: the reference restores it after every trial, the mirror never changed) */
    uint8_t *d_work[3] = {NULL, NULL, NULL};
    for (int p = plane_start; p < plane_end; p++) {
        uint8_t *d_src = hd_call_mirror(&c, pl[p].host, pl[p].bytes, HD_TAG(pcs->picture_number, HD_ST_RECON));
        d_work[p]      = hd_call_dev(&c, pl[p].bytes);
        HD_CALL(&c, p_svt_hip_copy(d_work[p], d_src, pl[p].bytes, NULL));
        hd_call_sync(&c); /* the copy has read the mirror before it is unpinned (the final filter below replaces that mirror) */
        hd_call_unpin(&c, pl[p].host);
    }
    if (hd_call_ok(&c)) {
        SvtHipLfFrame f;
        memset(&f, 0, sizeof(f));
        for (int p = 0; p < 3; p++) f.plane[p] = d_work[p] ? d_work[p] + pl[p].origin : NULL, f.stride[p] = pl[p].stride;
        _Static_assert(sizeof(f.lvl) == sizeof(ppcs->lf_info.lvl), "LoopFilterInfoN.lvl layout");
        f.width = frame_buffer->width, f.height = frame_buffer->height;
        f.mi = (const SvtHipLfMi *)d_mi, f.mi_stride = (uint32_t)pcs->mi_stride, f.mi_rows = (uint32_t)cm->mi_rows, f.mi_cols = (uint32_t)cm->mi_cols;
        memcpy(f.lvl, ppcs->lf_info.lvl, sizeof(f.lvl));
        const struct LoopFilter *lf = &ppcs->frm_hdr.loop_filter_params;
        f.filter_level[0] = (uint8_t)lf->filter_level[0], f.filter_level[1] = (uint8_t)lf->filter_level[1];
        f.filter_level_u = (uint8_t)lf->filter_level_u, f.filter_level_v = (uint8_t)lf->filter_level_v;
        f.sharpness_level = (uint8_t)lf->sharpness_level;
        f.bit_depth = (uint8_t)scs->static_config.encoder_bit_depth, f.is_16bit = (uint8_t)is16;
        f.plane_start = (uint8_t)plane_start, f.plane_end = (uint8_t)plane_end;
        hd_call_check(&c, p_svt_hip_loop_filter_frame(&f, NULL));
    }
    if (trial_sse) {
        /* picture_sse_calculations: against the source picture over the aligned size (8 bit) / the picture size (16 bit) */
        const int            p     = plane_start, ss = p ? 1 : 0;
        EbPictureBufferDesc *input = is16 ? pcs->input_frame16bit : ppcs->enhanced_pic;
        PlaneRef             sp[3];
        picture_planes(input, is16, sp);
        const uint32_t w = is16 ? (uint32_t)(input->width + ss) >> ss : (uint32_t)ppcs->aligned_width >> ss;
        const uint32_t h = is16 ? (uint32_t)(input->height + ss) >> ss : (uint32_t)ppcs->aligned_height >> ss;
        uint8_t       *d_src = hd_call_mirror(&c, sp[p].host, sp[p].bytes, HD_TAG(pcs->picture_number, is16 ? HD_ST_SOURCE16 : HD_ST_FILTERED));
        uint8_t       *d_sum = hd_call_dev(&c, 0);
        uint64_t       sum   = 0;
        HD_CALL(&c, p_svt_hip_plane_sse(d_src + sp[p].origin, sp[p].stride, d_work[p] + pl[p].origin, pl[p].stride, w, h, is16, (uint64_t *)d_sum, NULL));
        hd_call_download(&c, &sum, d_sum, 8);
        if (hd_call_sync(&c) == 0)
            *trial_sse = (int64_t)sum;
    } else {
        uint8_t *h_out[3] = {NULL, NULL, NULL};
        for (int p = plane_start; p < plane_end; p++) {
            h_out[p] = (uint8_t *)hd_call_pinned(&c, pl[p].bytes);
            hd_call_download(&c, h_out[p], d_work[p], pl[p].bytes);
        }
        if (hd_call_sync(&c) == 0) {
            for (int p = plane_start; p < plane_end; p++) memcpy(pl[p].host, h_out[p], pl[p].bytes);
            /* the picture's final deblocking (all planes; a trial filters one): the filtered planes become the mirrors of the host planes they
             * were just downloaded into, so that the CDEF search finds its input resident instead of uploading it again.  The picture is
             * committed: a plane that cannot be adopted (a scope of its own) is simply uploaded again later */
            for (int p = 0; plane_start == 0 && plane_end == 3 && p < 3; p++) {
                HdCall a;
                hd_call_begin(&a, NULL);
                uint8_t *d_new = hd_call_mirror_new(&a, pl[p].host, pl[p].bytes, HD_TAG(pcs->picture_number, HD_ST_DEBLOCKED));
                HD_CALL(&a, p_svt_hip_copy(d_new, d_work[p], pl[p].bytes, NULL));
                hd_call_end(&a, NULL);
            }
        }
    }
    if (hd_call_end(&c, "svt_hip_bind_lf: deblocking of picture %llu stays on the CPU", (unsigned long long)pcs->picture_number))
        return 1;
    __atomic_add_fetch(trial_sse ? &g_n_dlf_trials : &g_n_dlf, 1, __ATOMIC_RELAXED);
    return 0;
}
int svt_hip_bind_dlf_frame(EbPictureBufferDesc *frame_buffer, PictureControlSet *pcs, int32_t plane_start, int32_t plane_end) {
    return g_dlf ? deblock(frame_buffer, pcs, plane_start, plane_end, NULL) : 1;
}
/* One trial of the deblocking level search (try_filter_frame, deblocking_filter.c:842-882) entirely on the device: the plane is filtered in a
 * scratch copy of the mirror of the un-filtered reconstruction and compared with the source picture's mirror there (picture_sse_calculations,
 * :716-834); 8 bytes come back instead of the filtered plane, and the encoder's buffer is never touched (the reference filters it, measures
 * and restores it).  Returns 0 with *filt_err set, 1 when the caller must run the reference's sequence. */
int svt_hip_bind_dlf_try(EbPictureBufferDesc *frame_buffer, PictureControlSet *pcs, int32_t plane, int64_t *filt_err) {
    if (!g_dlf || !p_svt_hip_plane_sse || plane < 0 || plane > 2)
        return 1;
    return deblock(frame_buffer, pcs, plane, plane + 1, filt_err);
}

/* ================================================================ CDEF ==================================================== */
static HdOnceTable g_cdef_tab;

/* filt8x8[r][c] != 0: the 8x8 luma block (r, c) is filtered = not all four of its 4x4 units are skipped (svt_sb_compute_cdef_list,
 * enc_cdef.c:238-276) */
static uint8_t *skip_bitmap(HdCall *c, const PictureControlSet *pcs, uint32_t *w8, uint32_t *h8) {
    const Av1Common *cm = pcs->ppcs->av1_cm;
    *w8 = (uint32_t)(cm->mi_cols + 1) >> 1, *h8 = (uint32_t)(cm->mi_rows + 1) >> 1;
    uint8_t *m = (uint8_t *)hd_call_host(c, (size_t)*w8 * *h8);
    if (!m)
        return NULL;
    ModeInfo **grid = pcs->mi_grid_base;
    const int  ms   = pcs->mi_stride;
    for (int32_t r = 0; r + 1 < cm->mi_rows + (cm->mi_rows & 1); r += 2)
        for (int32_t c4 = 0; c4 + 1 < cm->mi_cols + (cm->mi_cols & 1); c4 += 2) {
            const int r1 = r + 1 < cm->mi_rows ? r + 1 : r, c1 = c4 + 1 < cm->mi_cols ? c4 + 1 : c4;
            m[(size_t)(r >> 1) * *w8 + (c4 >> 1)] = !grid[r * ms + c4]->mbmi.block_mi.skip || !grid[r * ms + c1]->mbmi.block_mi.skip ||
                !grid[r1 * ms + c4]->mbmi.block_mi.skip || !grid[r1 * ms + c1]->mbmi.block_mi.skip;
        }
    return m;
}

/* recon (after deblocking) and the second plane of every SvtHipCdefPlane: the source picture (search) or NULL (apply: set by the caller) */
static void cdef_planes(HdCall *c, SvtHipCdefPlane pl[3], PictureControlSet *pcs, int with_source) {
    const SequenceControlSet *scs  = pcs->scs;
    const Av1Common          *cm   = pcs->ppcs->av1_cm;
    const int                 is16 = scs->is_16bit_pipeline;
    EbPictureBufferDesc      *recon, *input = is16 ? pcs->input_frame16bit : pcs->ppcs->enhanced_pic;
    svt_aom_get_recon_pic(pcs, &recon, is16);
    PlaneRef rp[3], sp[3];
    picture_planes(recon, is16, rp), picture_planes(input, is16, sp);
    memset(pl, 0, 3 * sizeof(*pl));
    for (int p = 0; p < 3; p++) {
        SvtHipCdefPlane *o = &pl[p];
        uint8_t         *d = hd_call_mirror(c, rp[p].host, rp[p].bytes, HD_TAG(pcs->picture_number, HD_ST_DEBLOCKED));
        o->recon = d ? d + rp[p].origin : NULL, o->recon_stride = rp[p].stride;
        if (with_source) {
            uint8_t *s = hd_call_mirror(c, sp[p].host, sp[p].bytes, HD_TAG(pcs->picture_number, is16 ? HD_ST_SOURCE16 : HD_ST_FILTERED));
            o->source = s ? s + sp[p].origin : NULL, o->source_stride = sp[p].stride;
        }
        o->width = (uint32_t)(cm->mi_cols * 4) >> (p ? 1 : 0), o->height = (uint32_t)(cm->mi_rows * 4) >> (p ? 1 : 0);
        o->is_16bit = (uint8_t)is16, o->xdec = o->ydec = p ? 1 : 0, o->pli = (uint8_t)p;
    }
}

#define CDEF_DEFAULT_MSE_UV ((uint64_t)1040400 * 64) /* default_mse_uv * 64, cdef_process.c:78, :251 */

/* the first segment of a picture searches all of it (hd_once_run) */
static int cdef_search_picture(void *arg, void **payload) {
    (void)payload;
    PictureControlSet        *pcs  = (PictureControlSet *)arg;
    const SequenceControlSet *scs  = pcs->scs;
    PictureParentControlSet  *ppcs = pcs->ppcs;
    const Av1Common          *cm   = ppcs->av1_cm;
    const CdefControls       *cc   = &ppcs->cdef_ctrls;
    const int                 n1 = cc->first_pass_fs_num, n2 = cc->default_second_pass_fs_num, n = n1 + n2;
    HdCall                    c;
    hd_call_begin(&c, "cdef_search");
    if (n < 1 || n > SVT_HIP_CDEF_MAX_STRENGTHS)
        return !hd_call_decline(&c);
    const int32_t nvfb = (cm->mi_rows + MI_SIZE_64X64 - 1) / MI_SIZE_64X64, nhfb = (cm->mi_cols + MI_SIZE_64X64 - 1) / MI_SIZE_64X64;
    const size_t  nfb  = (size_t)nvfb * nhfb;
    uint32_t      w8, h8;
    uint8_t      *filt = skip_bitmap(&c, pcs, &w8, &h8);
    SvtHipCdefSearchParams prm[2]; /* luma, chroma */
    memset(prm, 0, sizeof(prm));
    for (int k = 0; k < 2; k++) {
        prm[k].n_strengths = n;
        for (int gi = 0; gi < n; gi++) {
            const int first = gi < n1;
            const int fs    = first ? cc->default_first_pass_fs[gi] : cc->default_second_pass_fs[gi - n1];
            const int uv    = first ? cc->default_first_pass_fs_uv[gi] : cc->default_second_pass_fs_uv[gi - n1];
            prm[k].strengths[gi] = (int8_t)((k && uv == -1) ? -1 : fs);
        }
        prm[k].pri_damping = prm[k].sec_damping = 3 + (ppcs->frm_hdr.quantization_params.base_q_idx >> 6);
        prm[k].coeff_shift        = AOMMAX(scs->static_config.encoder_bit_depth - 8, 0);
        prm[k].subsampling_factor = cc->subsampling_factor;
    }
    SvtHipCdefPlane pl[3];
    cdef_planes(&c, pl, pcs, 1);
    const size_t n_mse = nfb * n * sizeof(uint64_t), n_dir = nfb * 64, n_var = nfb * 64 * sizeof(int32_t), n_filt = (size_t)w8 * h8;
    uint8_t     *dev   = hd_call_dev(&c, hd_al256(3 * n_mse) + hd_al256(n_dir) + hd_al256(n_var) + n_filt);
    uint8_t     *d_mse = hd_carve(&dev, 3 * n_mse), *d_dir = hd_carve(&dev, n_dir), *d_var = hd_carve(&dev, n_var), *d_filt = dev;
    uint64_t    *h_mse = (uint64_t *)hd_call_host(&c, 3 * n_mse);
    uint8_t     *h_dir = (uint8_t *)hd_call_host(&c, n_dir);
    int32_t     *h_var = (int32_t *)hd_call_host(&c, n_var);
    hd_call_upload(&c, d_filt, filt, n_filt);
    hd_call_memset(&c, d_mse, 0, 3 * n_mse);
    for (int p = 0; p < 3; p++) /* luma first: it writes the directions the chroma planes read */
        HD_CALL(&c, p_svt_hip_cdef_search_plane(&pl[p], d_filt, &prm[p ? 1 : 0], (uint64_t *)(d_mse + p * n_mse), d_dir, (int32_t *)d_var, NULL));
    hd_call_download(&c, h_mse, d_mse, 3 * n_mse);
    hd_call_download(&c, h_dir, d_dir, n_dir);
    hd_call_download(&c, h_var, d_var, n_var);
    if (hd_call_sync(&c) == 0)
        for (int32_t fbr = 0; fbr < nvfb; fbr++)
            for (int32_t fbc = 0; fbc < nhfb; fbc++) {
                const size_t fb = (size_t)fbr * nhfb + fbc;
                /* cdef_count == 0 <=> no 8x8 of the filter block is filtered (:197-202) */
                int any = 0;
                for (uint32_t r = fbr * 8u; r < fbr * 8u + 8 && r < h8 && !any; r++)
                    for (uint32_t c8 = fbc * 8u; c8 < fbc * 8u + 8 && c8 < w8; c8++)
                        if (filt[(size_t)r * w8 + c8]) {
                            any = 1;
                            break;
                        }
                pcs->skip_cdef_seg[fb] = !any;
                if (!any)
                    continue;
                memcpy(pcs->cdef_dir_data[fb].dir, h_dir + fb * 64, 64);
                memcpy(pcs->cdef_dir_data[fb].var, h_var + fb * 64, 64 * sizeof(int32_t));
                for (int gi = 0; gi < n; gi++) {
                    pcs->mse_seg[0][fb][gi] = h_mse[fb * n + gi];
                    pcs->mse_seg[1][fb][gi] = prm[1].strengths[gi] == -1 ? CDEF_DEFAULT_MSE_UV : h_mse[(nfb + fb) * n + gi] + h_mse[(2 * nfb + fb) * n + gi];
                }
            }
    if (hd_call_end(&c, "svt_hip_bind_lf: CDEF search of picture %llu stays on the CPU", (unsigned long long)pcs->picture_number))
        return 0;
    __atomic_add_fetch(&g_n_cdef_search, 1, __ATOMIC_RELAXED);
    return 1;
}

int svt_hip_bind_cdef_seg(PictureControlSet *pcs, SequenceControlSet *scs, uint32_t segment_index) {
    (void)scs, (void)segment_index;
    if (!g_cdef || !covered(pcs))
        return 1;
    return hd_once_run(&g_cdef_tab, pcs, pcs->picture_number, pcs->cdef_segments_total_count, cdef_search_picture, NULL, NULL, pcs) != 0;
}

int svt_hip_bind_cdef_frame(SequenceControlSet *scs, PictureControlSet *pcs) {
    if (!g_cdef)
        return 1;
    HdCall c;
    hd_call_begin(&c, "cdef_apply");
    if (!covered(pcs) || pcs->ppcs->cdef_ctrls.use_reference_cdef_fs)
        return hd_call_decline(&c);
    PictureParentControlSet *ppcs    = pcs->ppcs;
    const Av1Common         *cm      = ppcs->av1_cm;
    const FrameHeader       *frm_hdr = &ppcs->frm_hdr;
    const int                is16    = scs->is_16bit_pipeline;
    const int32_t nvfb = (cm->mi_rows + MI_SIZE_64X64 - 1) / MI_SIZE_64X64, nhfb = (cm->mi_cols + MI_SIZE_64X64 - 1) / MI_SIZE_64X64;
    const size_t  nfb  = (size_t)nvfb * nhfb;
    const size_t  n_dir = nfb * 64, n_var = nfb * 64 * sizeof(int32_t);
    uint32_t      w8, h8;
    uint8_t      *filt  = skip_bitmap(&c, pcs, &w8, &h8);
    uint8_t      *fbs   = (uint8_t *)hd_call_host(&c, 2 * nfb);
    uint8_t      *h_dir = (uint8_t *)hd_call_host(&c, n_dir);
    int32_t      *h_var = (int32_t *)hd_call_host(&c, n_var);
    for (int32_t fbr = 0; hd_call_ok(&c) && fbr < nvfb; fbr++)
        for (int32_t fbc = 0; fbc < nhfb; fbc++) {
            const size_t  fb  = (size_t)fbr * nhfb + fbc;
            const int32_t idx = pcs->mi_grid_base[MI_SIZE_64X64 * fbr * cm->mi_stride + MI_SIZE_64X64 * fbc]->mbmi.cdef_strength;
            if (idx < 0 || idx >= CDEF_MAX_STRENGTHS) {
                hd_call_fail(&c);
                break;
            }
            fbs[fb] = (uint8_t)frm_hdr->cdef_params.cdef_y_strength[idx], fbs[nfb + fb] = (uint8_t)frm_hdr->cdef_params.cdef_uv_strength[idx];
            /* all four strengths zero: the reference leaves the filter block alone (:398-404) = not filtered for us */
            if (fbs[fb] == 0 && fbs[nfb + fb] == 0)
                for (uint32_t r = fbr * 8u; r < fbr * 8u + 8 && r < h8; r++)
                    for (uint32_t c8 = fbc * 8u; c8 < fbc * 8u + 8 && c8 < w8; c8++) filt[(size_t)r * w8 + c8] = 0;
            memcpy(h_dir + fb * 64, pcs->cdef_dir_data[fb].dir, 64);
            memcpy(h_var + fb * 64, pcs->cdef_dir_data[fb].var, 64 * sizeof(int32_t));
        }
    SvtHipCdefPlane pl[3];
    cdef_planes(&c, pl, pcs, 0);
    EbPictureBufferDesc *recon;
    svt_aom_get_recon_pic(pcs, &recon, is16);
    PlaneRef rp[3];
    picture_planes(recon, is16, rp);
    const size_t n_filt = (size_t)w8 * h8;
    uint8_t     *dev    = hd_call_dev(&c, hd_al256(n_dir) + hd_al256(n_var) + hd_al256(n_filt) + 2 * nfb);
    uint8_t     *d_dir = hd_carve(&dev, n_dir), *d_var = hd_carve(&dev, n_var), *d_filt = hd_carve(&dev, n_filt), *d_fbs = dev;
    uint8_t     *d_out[3] = {NULL, NULL, NULL}, *h_out[3] = {NULL, NULL, NULL};
    hd_call_upload(&c, d_dir, h_dir, n_dir);
    hd_call_upload(&c, d_var, h_var, n_var);
    hd_call_upload(&c, d_filt, filt, n_filt);
    hd_call_upload(&c, d_fbs, fbs, 2 * nfb);
    for (int p = 0; p < 3; p++) {
        /* the output plane starts as a copy of the input: the kernel writes the picture area, the padding stays what it was */
        d_out[p] = hd_call_dev(&c, rp[p].bytes);
        HD_CALL(&c, p_svt_hip_copy(d_out[p], (const uint8_t *)pl[p].recon - rp[p].origin, rp[p].bytes, NULL));
        pl[p].source = d_out[p] ? d_out[p] + rp[p].origin : NULL, pl[p].source_stride = rp[p].stride;
    }
    const uint8_t *strength[3] = {d_fbs, d_fbs + nfb, d_fbs + nfb};
    HD_CALL(&c, p_svt_hip_cdef_apply_frame(pl, 3, d_filt, strength, frm_hdr->cdef_params.cdef_damping, AOMMAX(scs->static_config.encoder_bit_depth - 8, 0),
                                          d_dir, (const int32_t *)d_var, NULL));
    for (int p = 0; p < 3; p++) {
        h_out[p] = (uint8_t *)hd_call_pinned(&c, rp[p].bytes);
        hd_call_download(&c, h_out[p], d_out[p], rp[p].bytes);
    }
    if (hd_call_sync(&c) == 0)
        for (int p = 0; p < 3; p++) memcpy(rp[p].host, h_out[p], rp[p].bytes);
    if (hd_call_end(&c, "svt_hip_bind_lf: CDEF of picture %llu stays on the CPU", (unsigned long long)pcs->picture_number))
        return 1;
    __atomic_add_fetch(&g_n_cdef_apply, 1, __ATOMIC_RELAXED);
    return 0;
}

/* ============================================================ restoration ================================================= */
/* the limits of every restoration unit of a plane in the order of foreach_rest_unit_in_tile (restoration.c:1250-1293; one tile) */
static int unit_limits(int W, int H, int unit_size, int ss_y, int horz_units, int vert_units, RestorationTileLimits *out) {
    const int ext = unit_size * 3 / 2, voff = RESTORATION_UNIT_OFFSET >> ss_y;
    int       y0 = 0, i = 0;
    while (y0 < H) {
        const int rem_h = H - y0, h = rem_h < ext ? rem_h : unit_size;
        int       x0 = 0, j = 0;
        if (i >= vert_units)
            return -1;
        while (x0 < W) {
            const int rem_w = W - x0, w = rem_w < ext ? rem_w : unit_size;
            if (j >= horz_units)
                return -1;
            RestorationTileLimits *l = &out[i * horz_units + j];
            l->v_start = y0 - voff > 0 ? y0 - voff : 0, l->v_end = y0 + h < H ? y0 + h - voff : y0 + h;
            l->h_start = x0, l->h_end = x0 + w;
            x0 += w, j++;
        }
        y0 += h, i++;
    }
    return 0;
}

typedef struct WienerPlaneStats {
    int                    n_units, win;
    int64_t               *M, *H; /* [n][49], [n][49 * 49] */
    RestorationTileLimits *lim;   /* [n]: the unit geometry the statistics were computed for */
} WienerPlaneStats;
static void wiener_stats_free(WienerPlaneStats *s) {
    if (s)
        free(s->M), free(s->H), free(s->lim), free(s);
}
/* statistics of the planes in flight: (pcs, picture number, plane) -> WienerPlaneStats.  Units that reuse the previous picture's
 * coefficients never ask (search_wiener_seg :1312-1318), so an entry cannot count its callers: it is replaced when its slot is
 * needed again (oldest first); readers copy their unit's share under the lock. */
typedef struct WienerSlot {
    const void       *pcs;
    uint64_t          picture_number;
    int               plane, state; /* 0 free, 1 being computed, 2 ready, 3 failed */
    uint64_t          stamp;
    WienerPlaneStats *st;
} WienerSlot;
#define N_WIENER 24
static WienerSlot      g_wiener[N_WIENER];
static uint64_t        g_wiener_clock;
static pthread_mutex_t g_wiener_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t  g_wiener_cv = PTHREAD_COND_INITIALIZER;

/* plane sample (0,0) pointers as the search sees them (init_rsc_seg: dgd = org_fts, src = cpi_source) against our PlaneRefs */
static WienerPlaneStats *wiener_plane(PictureControlSet *pcs, int plane, int wiener_win, const uint8_t *dgd, const uint8_t *src, int dgd_stride,
                                      int src_stride, int highbd, int bit_depth) {
    const SequenceControlSet *scs  = pcs->scs;
    const Av1Common          *cm   = pcs->ppcs->av1_cm;
    const int                 is16 = scs->is_16bit_pipeline;
    const RestorationInfo    *rsi  = &pcs->rst_info[plane];
    EbPictureBufferDesc      *recon, *input = is16 ? pcs->input_frame16bit : pcs->ppcs->enhanced_unscaled_pic;
    svt_aom_get_recon_pic(pcs, &recon, is16);
    PlaneRef rp[3], sp[3];
    picture_planes(recon, is16, rp), picture_planes(input, is16, sp);
    const uint8_t *dgd_raw = highbd ? (const uint8_t *)CONVERT_TO_SHORTPTR(dgd) : dgd, *src_raw = highbd ? (const uint8_t *)CONVERT_TO_SHORTPTR(src) : src;
    const int      ss = plane > 0, W = (cm->frm_size.superres_upscaled_width + ss) >> ss, H = (cm->frm_size.frame_height + ss) >> ss;
    const int      n  = rsi->horz_units_per_tile * rsi->vert_units_per_tile;
    HdCall         c;
    hd_call_begin(&c, "wiener_plane");
    /* the second line: not the buffers this hook knows how to mirror (scaled source, a private copy of the reconstruction) */
    if (scs->use_boundaries_in_rest_search || highbd != is16 || n < 1 ||
        dgd_raw != rp[plane].host + rp[plane].origin || src_raw != sp[plane].host + sp[plane].origin || (uint32_t)dgd_stride != rp[plane].stride ||
        (uint32_t)src_stride != sp[plane].stride) {
        hd_call_decline(&c);
        return NULL;
    }
    const size_t      n_m = (size_t)n * 49 * 8, n_h = (size_t)n * 49 * 49 * 8;
    WienerPlaneStats *st  = (WienerPlaneStats *)calloc(1, sizeof(*st)); /* outlives the call: plain heap (wiener_stats_free) */
    if (st)
        st->lim = (RestorationTileLimits *)calloc(n, sizeof(*st->lim)), st->M = (int64_t *)malloc(n_m), st->H = (int64_t *)malloc(n_h);
    if (!st || !st->lim || !st->M || !st->H || unit_limits(W, H, rsi->restoration_unit_size, ss, rsi->horz_units_per_tile, rsi->vert_units_per_tile, st->lim) != 0)
        hd_call_fail(&c);
    SvtHipWienerUnit *u = (SvtHipWienerUnit *)hd_call_host(&c, (size_t)n * sizeof(*u));
    /* the reconstruction after CDEF with the borders restoration_seg_search extended (svt_extend_frame, restoration_pick.c:1511: the
     * statistics read 3 samples beyond the picture) and the source as cdef_process.c left it */
    uint8_t *d_dgd = hd_call_mirror(&c, rp[plane].host, rp[plane].bytes, HD_TAG(pcs->picture_number, HD_ST_CDEF_EXT));
    uint8_t *d_src = hd_call_mirror(&c, sp[plane].host, sp[plane].bytes, HD_TAG(pcs->picture_number, is16 ? HD_ST_SOURCE16_LR : HD_ST_FILTERED));
    uint8_t *dev   = hd_call_dev(&c, hd_al256(n_m) + n_h);
    uint8_t *d_M = hd_carve(&dev, n_m), *d_H = dev;
    if (hd_call_ok(&c)) {
        for (int i = 0; i < n; i++) {
            const RestorationTileLimits *l = &st->lim[i];
            u[i].dgd = d_dgd + rp[plane].origin, u[i].src = d_src + sp[plane].origin, u[i].dgd_stride = rp[plane].stride, u[i].src_stride = sp[plane].stride;
            u[i].h_start = l->h_start, u[i].h_end = l->h_end, u[i].v_start = l->v_start, u[i].v_end = l->v_end;
        }
        st->n_units = n, st->win = wiener_win;
        hd_call_check(&c, p_svt_hip_wiener_stats(u, (uint32_t)n, wiener_win, is16, bit_depth, (int64_t *)d_M, (int64_t *)d_H, NULL));
        hd_call_download(&c, st->M, d_M, n_m);
        hd_call_download(&c, st->H, d_H, n_h);
    }
    hd_call_sync(&c);
    if (hd_call_end(&c, "svt_hip_bind_lf: Wiener statistics of picture %llu plane %d stay on the CPU", (unsigned long long)pcs->picture_number, plane)) {
        wiener_stats_free(st);
        return NULL;
    }
    __atomic_add_fetch(&g_n_wiener, 1, __ATOMIC_RELAXED);
    return st;
}

int svt_hip_bind_wiener_stats(PictureControlSet *pcs, int plane, int rest_unit_idx, int wiener_win, const uint8_t *dgd, const uint8_t *src,
                              const RestorationTileLimits *limits, int dgd_stride, int src_stride, int highbd, int bit_depth, int64_t *M, int64_t *H) {
    if (!g_lr || !covered(pcs) || plane < 0 || plane > 2)
        return 1;
    const RestorationInfo *rsi = &pcs->rst_info[plane];
    const int              n   = rsi->horz_units_per_tile * rsi->vert_units_per_tile;
    if (rest_unit_idx < 0 || rest_unit_idx >= n)
        return 1;
    pthread_mutex_lock(&g_wiener_mu);
    WienerSlot *e = NULL;
    for (;;) {
        e = NULL;
        for (int i = 0; i < N_WIENER; i++)
            if (g_wiener[i].state && g_wiener[i].pcs == pcs && g_wiener[i].picture_number == pcs->picture_number && g_wiener[i].plane == plane)
                e = &g_wiener[i];
        if (!e || e->state != 1)
            break;
        pthread_cond_wait(&g_wiener_cv, &g_wiener_mu);
    }
    if (!e) { /* first unit of this plane: take the free or the oldest settled slot and compute the whole plane */
        for (int i = 0; i < N_WIENER && (!e || e->state != 0); i++) {
            WienerSlot *c = &g_wiener[i];
            if (c->state == 1)
                continue;
            if (c->state == 0 || !e || c->stamp < e->stamp)
                e = c;
        }
        if (!e) {
            pthread_mutex_unlock(&g_wiener_mu);
            return 1;
        }
        wiener_stats_free(e->st);
        e->st = NULL, e->pcs = pcs, e->picture_number = pcs->picture_number, e->plane = plane, e->state = 1, e->stamp = ++g_wiener_clock;
        pthread_mutex_unlock(&g_wiener_mu);
        WienerPlaneStats *st = wiener_plane(pcs, plane, wiener_win, dgd, src, dgd_stride, src_stride, highbd, bit_depth);
        pthread_mutex_lock(&g_wiener_mu);
        e->st = st, e->state = st ? 2 : 3;
        pthread_cond_broadcast(&g_wiener_cv);
    }
    int rc = 1;
    if (e->state == 2) {
        const WienerPlaneStats *st = e->st;
        /* only for the unit geometry this hook derived itself; anything else the reference computes */
        if (st->win == wiener_win && rest_unit_idx < st->n_units && memcmp(&st->lim[rest_unit_idx], limits, sizeof(*limits)) == 0) {
            memcpy(M, st->M + (size_t)rest_unit_idx * 49, 49 * 8);
            memcpy(H, st->H + (size_t)rest_unit_idx * 49 * 49, 49 * 49 * 8);
            rc = 0;
        }
    }
    pthread_mutex_unlock(&g_wiener_mu);
    return rc;
}

int svt_hip_bind_lr_frame(Yv12BufferConfig *frame, Av1Common *cm, int32_t optimized_lr) {
    if (!g_lr)
        return 1;
    PictureControlSet *pcs = cm->child_pcs;
    HdCall             c;
    hd_call_begin(&c, "lr_frame");
    if (!pcs || !covered(pcs) || cm->use_highbitdepth != pcs->scs->is_16bit_pipeline)
        return hd_call_decline(&c);
    const int            is16 = pcs->scs->is_16bit_pipeline;
    EbPictureBufferDesc *recon;
    svt_aom_get_recon_pic(pcs, &recon, is16);
    PlaneRef rp[3];
    picture_planes(recon, is16, rp);
    SvtHipLrPlane pl[3];
    int           plane_of[3], n_pl = 0;
    uint8_t      *h_out[3] = {NULL, NULL, NULL};
    memset(pl, 0, sizeof(pl));
    for (int plane = 0; hd_call_ok(&c) && plane < 3; plane++) {
        RestorationInfo *rsi = &pcs->rst_info[plane];
        rsi->optimized_lr    = optimized_lr; /* what the reference's loop sets for every plane (:1207) */
        if (rsi->frame_restoration_type == RESTORE_NONE)
            continue;
        const int      is_uv = plane > 0;
        const uint8_t *buf   = is16 ? (const uint8_t *)CONVERT_TO_SHORTPTR(frame->buffers[plane]) : frame->buffers[plane];
        if (buf != rp[plane].host + rp[plane].origin || (uint32_t)frame->strides[is_uv] != rp[plane].stride) {
            hd_call_fail(&c); /* not the picture's reconstruction buffer */
            break;
        }
        SvtHipLrPlane *o     = &pl[n_pl];
        const int      n     = rsi->horz_units_per_tile * rsi->vert_units_per_tile;
        uint8_t       *d     = hd_call_mirror(&c, rp[plane].host, rp[plane].bytes, HD_TAG(pcs->picture_number, HD_ST_CDEF_EXT));
        SvtHipLrUnit  *hu    = (SvtHipLrUnit *)hd_call_host(&c, (size_t)n * sizeof(*hu));
        uint8_t       *d_out = hd_call_dev(&c, rp[plane].bytes);
        if (!hd_call_ok(&c))
            break;
        for (int i = 0; i < n; i++) {
            const RestorationUnitInfo *ui = &rsi->unit_info[i];
            hu[i].restoration_type       = (uint8_t)ui->restoration_type;
            hu[i].ep = (uint8_t)ui->sgrproj_info.ep, hu[i].xqd[0] = ui->sgrproj_info.xqd[0], hu[i].xqd[1] = ui->sgrproj_info.xqd[1];
            memcpy(hu[i].hfilter, ui->wiener_info.hfilter, sizeof(hu[i].hfilter));
            memcpy(hu[i].vfilter, ui->wiener_info.vfilter, sizeof(hu[i].vfilter));
        }
        o->units = (const SvtHipLrUnit *)hd_call_dev_put(&c, hu, (size_t)n * sizeof(*hu));
        if (!optimized_lr) {
            const size_t nb    = (size_t)rsi->boundaries.stripe_boundary_size;
            uint8_t     *d_bnd = hd_call_dev(&c, 2 * hd_al256(nb));
            o->boundary_above = hd_carve(&d_bnd, nb), o->boundary_below = d_bnd;
            hd_call_upload(&c, (void *)o->boundary_above, rsi->boundaries.stripe_boundary_above, nb);
            hd_call_upload(&c, (void *)o->boundary_below, rsi->boundaries.stripe_boundary_below, nb);
            o->boundary_stride = (uint32_t)rsi->boundaries.stripe_boundary_stride;
        }
        o->src = d + rp[plane].origin, o->dst = d_out + rp[plane].origin, o->src_stride = o->dst_stride = rp[plane].stride;
        o->width = (uint32_t)frame->crop_widths[is_uv], o->height = (uint32_t)frame->crop_heights[is_uv];
        o->ss_x = o->ss_y = (uint8_t)is_uv, o->is_16bit = (uint8_t)is16, o->bit_depth = (uint8_t)cm->bit_depth;
        o->unit_size = (uint32_t)rsi->restoration_unit_size, o->horz_units = (uint32_t)rsi->horz_units_per_tile, o->vert_units = (uint32_t)rsi->vert_units_per_tile;
        o->optimized_lr = (uint32_t)optimized_lr;
        plane_of[n_pl++] = plane;
    }
    if (n_pl)
        HD_CALL(&c, p_svt_hip_restoration_filter_frame(pl, (uint32_t)n_pl, NULL));
    /* only the picture area comes back (copy_funs[plane](dst, frame) copies the cropped plane, :1243) */
    for (int k = 0; k < n_pl; k++) {
        const size_t row = (size_t)pl[k].width << is16;
        h_out[k]         = (uint8_t *)hd_call_pinned(&c, row * pl[k].height);
        HD_CALL(&c, p_svt_hip_download_2d(h_out[k], row, pl[k].dst, (size_t)pl[k].dst_stride << is16, row, pl[k].height, NULL));
    }
    if (hd_call_sync(&c) == 0)
        for (int k = 0; k < n_pl; k++) {
            const PlaneRef *r   = &rp[plane_of[k]];
            const size_t    row = (size_t)pl[k].width << is16;
            for (uint32_t y = 0; y < pl[k].height; y++) memcpy(r->host + r->origin + (((size_t)y * r->stride) << is16), h_out[k] + y * row, row);
        }
    if (hd_call_end(&c, "svt_hip_bind_lf: restoration of picture %llu stays on the CPU", (unsigned long long)pcs->picture_number))
        return 1;
    __atomic_add_fetch(&g_n_lr, 1, __ATOMIC_RELAXED);
    return 0;
}
