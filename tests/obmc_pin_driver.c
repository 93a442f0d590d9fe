/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/obmc_cases.py against the reference's own OBMC
 * motion refinement.
 *
 * pin_target: the static calc_target_weighted_pred (enc_inter_prediction.c:1767-1827; this file includes that source to reach it) on a
 * fabricated xd->mi grid, so foreach_overlappable_nb_above / _left, the pairing of 4-wide blocks, nb_max and the clip at mi_cols / mi_rows
 * are the reference's own, and the visitors are whatever the RTCD pointers hold.  ModeDecisionContext and PictureControlSet are zeroed and
 * carry only what the function reads.
 *
 * pin_search: single_motion_search (mode_decision.c:2425-2533) itself on zeroed contexts wherever its hard-wired controls (8 taps,
 * forced_stop 0, two iterations per step, the three refinement combinations refine_level reaches) are the case's: that gives best_mv and
 * rate_mv.  Every case also goes through the two stage functions single_motion_search calls, svt_av1_obmc_full_pixel_search and
 * svt_av1_find_best_obmc_sub_pixel_tree_up, behind the same set-up lines: that reaches the other controls and the values
 * single_motion_search drops (the tree's return value, dis, sse1, the full-pel vector).  How many full-pel rounds moved is read off the
 * reference too: the full-pel stage is run with search ranges 0 .. R and the vectors are compared.
 *
 * Built by tests/test_obmc_abi.py (and by tests/golden/make_golden_obmc.py) into a temporary directory with the include paths and defines
 * of oracle/Makefile, asserts on, and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include <limits.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>

#include "enc_inter_prediction.c"

#include "av1me.h"
#include "md_process.h"
#include "mode_decision.h"
#include "rd_cost.h"

void ref_init(void);
void init_fn_ptr(void);
void svt_av1_init_me_luts(void);
void single_motion_search(PictureControlSet *pcs, ModeDecisionContext *ctx, ModeDecisionCandidate *cand, IntMv best_pred_mv, IntraBcContext *x,
                          BlockSize bsize, MV *ref_mv, int *rate_mv, int refine_level);
int  svt_av1_find_best_obmc_sub_pixel_tree_up(ModeDecisionContext *ctx, IntraBcContext *x, const AV1_COMMON *const cm, int mi_row, int mi_col,
                                              MV *bestmv, const MV *ref_mv, int allow_hp, int error_per_bit, const AomVarianceFnPtr *vfp,
                                              int forced_stop, int iters_per_step, int *mvjcost, int *mvcost[2], int *distortion,
                                              unsigned int *sse1, int is_second, int use_accurate_subpel_search);
int  svt_av1_obmc_full_pixel_search(ModeDecisionContext *ctx, IntraBcContext *x, MV *mvp_full, int sadpb, const AomVarianceFnPtr *fn_ptr,
                                    const MV *ref_mv, MV *dst_mv, int is_second);

static void pin_init(void) {
    static int done;
    if (!done)
        ref_init(), init_fn_ptr(), svt_av1_init_me_luts(), done = 1;
}

static BlockSize bsize_of(int w, int h) {
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == w && block_size_high[b] == h)
            return (BlockSize)b;
    return BLOCK_INVALID;
}

typedef struct PinTarget {
    int32_t w, h, mi_row, mi_col, mi_rows, mi_cols, up_available, left_available, src_stride, above_stride, left_stride;
} PinTarget;

/* above_w / above_inter: per mode-info column of the picture, the width in mode-info units and the inter flag of the block that covers it in
 * the row above the block; left_h / left_inter: the same per mode-info row in the column to its left.  wsrc, mask: w * h each. */
static double now_ns(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e9 + t.tv_nsec;
}

/* calc_target_weighted_pred `repeats` times on one fabricated grid; *best_ns (where given): the least time of one call */
static void target_run(const PinTarget *a, uint8_t *src, const uint8_t *above, const uint8_t *left, const uint8_t *above_w, const uint8_t *above_inter,
                       const uint8_t *left_h, const uint8_t *left_inter, int32_t *wsrc, int32_t *mask, int repeats, double *best_ns) {
    pin_init();
    const int  stride = a->mi_cols + 2, rows = a->mi_rows + 2;
    ModeInfo  *cells  = calloc((size_t)stride * rows, sizeof(*cells));
    ModeInfo **grid   = calloc((size_t)stride * rows, sizeof(*grid));
    for (int i = 0; i < stride * rows; i++) {
        cells[i].mbmi.block_mi.bsize = BLOCK_4X4, cells[i].mbmi.block_mi.ref_frame[0] = INTRA_FRAME;
        grid[i] = &cells[i];
    }
#define CELL(r, c) cells[((r) + 1) * stride + (c) + 1]
    if (a->mi_row > 0)
        for (int c = 0; c < a->mi_cols; c++) {
            CELL(a->mi_row - 1, c).mbmi.block_mi.bsize        = bsize_of(above_w[c] * 4, above_w[c] * 4);
            CELL(a->mi_row - 1, c).mbmi.block_mi.ref_frame[0] = above_inter[c] ? LAST_FRAME : INTRA_FRAME;
        }
    if (a->mi_col > 0)
        for (int r = 0; r < a->mi_rows; r++) {
            CELL(r, a->mi_col - 1).mbmi.block_mi.bsize        = bsize_of(left_h[r] * 4, left_h[r] * 4);
            CELL(r, a->mi_col - 1).mbmi.block_mi.ref_frame[0] = left_inter[r] ? LAST_FRAME : INTRA_FRAME;
        }
    MacroBlockD *xd = calloc(1, sizeof(*xd));
    xd->n4_w = (uint8_t)(a->w / 4), xd->n4_h = (uint8_t)(a->h / 4), xd->mi_stride = stride;
    xd->mi = grid + (a->mi_row + 1) * stride + a->mi_col + 1;
    xd->up_available = a->up_available != 0, xd->left_available = a->left_available != 0;
    AV1_COMMON *cm = calloc(1, sizeof(*cm));
    cm->mi_rows = a->mi_rows, cm->mi_cols = a->mi_cols;
    BlockGeom geom;
    memset(&geom, 0, sizeof(geom));
    geom.bsize = bsize_of(a->w, a->h);
    ModeDecisionContext *ctx = calloc(1, sizeof(*ctx));
    ctx->blk_geom = &geom, ctx->obmc_ctrls.max_blk_size_to_refine = 128, ctx->wsrc_buf = wsrc, ctx->mask_buf = mask;
    PictureControlSet       *pcs  = calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    EbPictureBufferDesc      pic;
    memset(&pic, 0, sizeof(pic));
    pic.buffer_y = src, pic.stride_y = (uint16_t)a->src_stride; /* blk_org and org are 0: src is the block's first sample */
    ppcs->enhanced_pic = &pic, pcs->ppcs = ppcs;
    for (int k = 0; k < repeats; k++) {
        const double t0 = now_ns();
        calc_target_weighted_pred(pcs, ctx, cm, xd, a->mi_row, a->mi_col, above, a->above_stride, left, a->left_stride);
        const double t1 = now_ns();
        if (best_ns && (k == 0 || t1 - t0 < *best_ns))
            *best_ns = t1 - t0;
    }
    free(ppcs), free(pcs), free(ctx), free(cm), free(xd), free(grid), free(cells);
#undef CELL
}

void pin_target(const PinTarget *a, uint8_t *src, const uint8_t *above, const uint8_t *left, const uint8_t *above_w, const uint8_t *above_inter,
                const uint8_t *left_h, const uint8_t *left_inter, int32_t *wsrc, int32_t *mask) {
    target_run(a, src, above, left, above_w, above_inter, left_h, left_inter, wsrc, mask, 1, NULL);
}

typedef struct PinSearch {
    int32_t w, h, ref_stride, start_row, start_col, ref_row, ref_col, mi_row, mi_col, mi_rows, mi_cols;
    int32_t do_full_refine, do_frac_refine, fpel_search_range, fpel_search_diag, qindex, full_lambda, approx_inter_rate, allow_hp;
    int32_t subpel_search_type, forced_stop, iters_per_step;
} PinSearch;

typedef struct PinState {
    PictureControlSet       *pcs;
    PictureParentControlSet *ppcs;
    AV1_COMMON              *cm;
    ModeDecisionContext     *ctx;
    MdRateEstimationContext *rate;
    BlkStruct               *blk;
    MacroBlockD             *xd;
    ModeDecisionCandidate   *cand;
    IntraBcContext          *x;
    BlockGeom                geom;
} PinState;

static void state_make(PinState *s, const PinSearch *a, int32_t *wsrc, int32_t *mask, uint8_t *ref, const int *mvjcost, int *mvcost_row,
                       int *mvcost_col) {
    s->pcs = calloc(1, sizeof(*s->pcs)), s->ppcs = calloc(1, sizeof(*s->ppcs)), s->cm = calloc(1, sizeof(*s->cm));
    s->ctx = calloc(1, sizeof(*s->ctx)), s->rate = calloc(1, sizeof(*s->rate)), s->blk = calloc(1, sizeof(*s->blk));
    s->xd = calloc(1, sizeof(*s->xd)), s->cand = calloc(1, sizeof(*s->cand)), s->x = calloc(1, sizeof(*s->x));
    memset(&s->geom, 0, sizeof(s->geom));
    s->geom.bsize = bsize_of(a->w, a->h);
    s->cm->mi_rows = a->mi_rows, s->cm->mi_cols = a->mi_cols;
    s->ppcs->av1_cm = s->cm, s->pcs->ppcs = s->ppcs;
    s->ppcs->frm_hdr.quantization_params.base_q_idx = (uint8_t)a->qindex, s->ppcs->frm_hdr.allow_high_precision_mv = a->allow_hp != 0;
    s->xd->mb_to_top_edge = -(a->mi_row * MI_SIZE * 8), s->xd->mb_to_left_edge = -(a->mi_col * MI_SIZE * 8);
    s->blk->av1xd = s->xd;
    memcpy(s->rate->nmv_vec_cost, mvjcost, sizeof(s->rate->nmv_vec_cost));
    s->rate->nmvcoststack[0] = mvcost_row, s->rate->nmvcoststack[1] = mvcost_col;
    s->ctx->full_lambda_md[EB_8_BIT_MD] = (uint32_t)a->full_lambda, s->ctx->blk_ptr = s->blk, s->ctx->md_rate_est_ctx = s->rate;
    s->ctx->blk_geom = &s->geom, s->ctx->wsrc_buf = wsrc, s->ctx->mask_buf = mask, s->ctx->approx_inter_rate = (uint8_t)a->approx_inter_rate;
    s->ctx->obmc_ctrls.fpel_search_range = (uint8_t)a->fpel_search_range, s->ctx->obmc_ctrls.fpel_search_diag = (uint8_t)a->fpel_search_diag;
    s->cand->motion_mode           = OBMC_CAUSAL;
    s->x->xdplane[0].pre[0].buf    = ref; /* the block's co-located first sample */
    s->x->xdplane[0].pre[0].stride = a->ref_stride;
}

static void state_free(PinState *s) {
    free(s->pcs), free(s->ppcs), free(s->cm), free(s->ctx), free(s->rate), free(s->blk), free(s->xd), free(s->cand), free(s->x);
}

/* the set-up lines of single_motion_search (mode_decision.c:2449-2466) and its full-pel branch, with the search range given */
static void stage_full(PinState *s, const PinSearch *a, MV *ref_mv, int range, int *sadpb_out) {
    IntraBcContext *x    = s->x;
    const BlockSize bsize = s->geom.bsize;
    x->xd                = s->xd;
    x->nmv_vec_cost      = s->rate->nmv_vec_cost;
    x->mv_cost_stack     = s->rate->nmvcoststack;
    x->mv_limits.row_min = -(((a->mi_row + mi_size_high[bsize]) * MI_SIZE) + AOM_INTERP_EXTEND);
    x->mv_limits.col_min = -(((a->mi_col + mi_size_wide[bsize]) * MI_SIZE) + AOM_INTERP_EXTEND);
    x->mv_limits.row_max = (a->mi_rows - a->mi_row) * MI_SIZE + AOM_INTERP_EXTEND;
    x->mv_limits.col_max = (a->mi_cols - a->mi_col) * MI_SIZE + AOM_INTERP_EXTEND;
    x->sadperbit16       = svt_aom_get_sad_per_bit(a->qindex, 0);
    x->errorperbit       = (uint32_t)a->full_lambda >> RD_EPB_SHIFT;
    x->errorperbit += (x->errorperbit == 0);
    *sadpb_out = x->sadperbit16;
    MV start   = {(int16_t)a->start_row, (int16_t)a->start_col};
    if (a->do_full_refine) {
        const MvLimits tmp = x->mv_limits;
        svt_av1_set_mv_search_range(&x->mv_limits, ref_mv);
        MV mvp_full = {start.row >> 3, start.col >> 3};
        x->best_mv.as_int = x->second_best_mv.as_int = INVALID_MV;
        s->ctx->obmc_ctrls.fpel_search_range         = (uint8_t)range;
        svt_av1_obmc_full_pixel_search(s->ctx, x, &mvp_full, x->sadperbit16, &svt_aom_mefn_ptr[bsize], ref_mv, &x->best_mv.as_mv, 0);
        s->ctx->obmc_ctrls.fpel_search_range = (uint8_t)a->fpel_search_range;
        x->mv_limits                         = tmp;
    } else {
        x->best_mv.as_mv.col = start.col >> 3;
        x->best_mv.as_mv.row = start.row >> 3;
    }
}

/* out[0 .. 8]: through the stage functions: best_mv.row, .col, the full-pel vector's row, col, the tree's return value, dis, sse1, rate_mv,
 * full-pel rounds that moved.  out[9 .. 11]: best_mv.row, .col and rate_mv of single_motion_search itself, INT_MIN where its hard-wired
 * controls are not the case's.  out[12]: sadperbit16.  out[13 .. 20]: the limits before and after svt_av1_set_mv_search_range (col_min,
 * col_max, row_min, row_max each). */
void pin_search(const PinSearch *a, int32_t *wsrc, int32_t *mask, uint8_t *ref, const int *mvjcost, int *mvcost_row, int *mvcost_col, int64_t *out) {
    pin_init();
    PinState s;
    state_make(&s, a, wsrc, mask, ref, mvjcost, mvcost_row, mvcost_col);
    MV  ref_mv = {(int16_t)a->ref_row, (int16_t)a->ref_col};
    int sadpb;
    /* rounds that moved: the vector after k rounds, k = 0 .. R */
    int rounds = 0;
    if (a->do_full_refine) {
        MV prev;
        for (int k = 0; k <= a->fpel_search_range; k++) {
            stage_full(&s, a, &ref_mv, k, &sadpb);
            if (k > 0 && (prev.row != s.x->best_mv.as_mv.row || prev.col != s.x->best_mv.as_mv.col))
                rounds++;
            prev = s.x->best_mv.as_mv;
        }
    }
    stage_full(&s, a, &ref_mv, a->fpel_search_range, &sadpb);
    IntraBcContext *x = s.x;
    out[2] = x->best_mv.as_mv.row, out[3] = x->best_mv.as_mv.col, out[8] = rounds, out[12] = sadpb;
    out[13] = x->mv_limits.col_min, out[14] = x->mv_limits.col_max, out[15] = x->mv_limits.row_min, out[16] = x->mv_limits.row_max;
    MvLimits fp = x->mv_limits;
    svt_av1_set_mv_search_range(&fp, &ref_mv);
    out[17] = fp.col_min, out[18] = fp.col_max, out[19] = fp.row_min, out[20] = fp.row_max;
    int          dis  = 0, besterr = 0;
    unsigned int sse1 = 0;
    if (a->do_frac_refine) {
        besterr = svt_av1_find_best_obmc_sub_pixel_tree_up(s.ctx, x, s.cm, a->mi_row, a->mi_col, &x->best_mv.as_mv, &ref_mv, a->allow_hp,
                                                           x->errorperbit, &svt_aom_mefn_ptr[s.geom.bsize], a->forced_stop, a->iters_per_step,
                                                           x->nmv_vec_cost, x->mv_cost_stack, &dis, &sse1, 0, a->subpel_search_type);
    } else {
        x->best_mv.as_mv.col <<= 3;
        x->best_mv.as_mv.row <<= 3;
    }
    int rate_mv;
    if (s.ctx->approx_inter_rate)
        rate_mv = svt_av1_mv_bit_cost_light(&x->best_mv.as_mv, &ref_mv);
    else
        rate_mv = svt_av1_mv_bit_cost(&x->best_mv.as_mv, &ref_mv, x->nmv_vec_cost, x->mv_cost_stack, 108 /* MV_COST_WEIGHT */);
    out[0] = x->best_mv.as_mv.row, out[1] = x->best_mv.as_mv.col, out[4] = besterr, out[5] = dis, out[6] = sse1, out[7] = rate_mv;
    state_free(&s);
    /* the function itself */
    out[9] = out[10] = out[11] = INT_MIN;
    const int reachable = a->subpel_search_type == USE_8_TAPS && a->forced_stop == 0 && a->iters_per_step == 2 &&
        (a->do_frac_refine || !a->do_full_refine);
    if (reachable) {
        state_make(&s, a, wsrc, mask, ref, mvjcost, mvcost_row, mvcost_col);
        IntMv start;
        start.as_mv.row = (int16_t)a->start_row, start.as_mv.col = (int16_t)a->start_col;
        /* refine_level: 0 full + fractional, 2 fractional only, 5 neither (mode_decision.c:2430-2443) */
        const int refine_level = a->do_full_refine ? 0 : a->do_frac_refine ? 2 : 5;
        int       rate         = 0;
        single_motion_search(s.pcs, s.ctx, s.cand, start, s.x, s.geom.bsize, &ref_mv, &rate, refine_level);
        out[9] = s.x->best_mv.as_mv.row, out[10] = s.x->best_mv.as_mv.col, out[11] = rate;
        state_free(&s);
    }
}

/* tools/obmc_time.py: nanoseconds of one call of calc_target_weighted_pred and of single_motion_search (refine_level 0: both stages) on
 * contexts made beforehand, each the least of `repeats` runs */
void pin_time(const PinTarget *t, const PinSearch *a, uint8_t *src, const uint8_t *above, const uint8_t *left, const uint8_t *above_w,
              const uint8_t *above_inter, const uint8_t *left_h, const uint8_t *left_inter, int32_t *wsrc, int32_t *mask, uint8_t *ref, const int *mvjcost,
              int *mvcost_row, int *mvcost_col, int repeats, double *ns) {
    target_run(t, src, above, left, above_w, above_inter, left_h, left_inter, wsrc, mask, repeats, &ns[0]);
    for (int k = 0; k < repeats; k++) {
        PinState s;
        state_make(&s, a, wsrc, mask, ref, mvjcost, mvcost_row, mvcost_col);
        MV    ref_mv = {(int16_t)a->ref_row, (int16_t)a->ref_col};
        IntMv start;
        start.as_mv.row = (int16_t)a->start_row, start.as_mv.col = (int16_t)a->start_col;
        int          rate = 0;
        const double t0   = now_ns();
        single_motion_search(s.pcs, s.ctx, s.cand, start, s.x, s.geom.bsize, &ref_mv, &rate, 0);
        const double t1 = now_ns();
        if (k == 0 || t1 - t0 < ns[1])
            ns[1] = t1 - t0;
        state_free(&s);
    }
}

/* the ramps and the constants the header and the restatement state */
void pin_constants(int32_t *out) {
    const int32_t v[12] = {USE_2_TAPS, USE_4_TAPS, USE_8_TAPS, MV_LOW, MV_UPP, MAX_FULL_PEL_VAL, MI_SIZE, AOM_INTERP_EXTEND,
                           AOM_BLEND_A64_MAX_ALPHA, AOM_BLEND_A64_ROUND_BITS, AV1_PROB_COST_SHIFT, RD_EPB_SHIFT};
    memcpy(out, v, sizeof(v));
    int n = 12;
    for (int len = 1; len <= 32; len *= 2) {
        const uint8_t *m = svt_av1_get_obmc_mask(len);
        for (int i = 0; i < len; i++) out[n++] = m[i];
    }
}
