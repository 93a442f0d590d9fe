/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/subpel_cases.py against the reference's own
 * svt_av1_find_best_sub_pixel_tree and svt_av1_find_best_sub_pixel_tree_pruned (mcomp.c:609-775), called the way md_subpel_search
 * (product_coding_loop.c:2502-2614) calls them: the variance functions are svt_aom_mefn_ptr[bsize] as init_fn_ptr filled it, ictx is
 * NULL, or, for the cases of the mvp_th rule, a zeroed ModeDecisionContext that carries only pd_pass, md_subpel_me_ctrls.mvp_th /
 * hp_mv_th, best_fp_mvp_dist, best_fp_mvp_idx and mvp_array.  The limits are those of svt_av1_set_mv_search_range and
 * svt_av1_set_subpel_mv_search_range.  Built by tests/test_subpel_abi.py (and by tests/golden/make_golden_subpel.py) into a temporary
 * directory with the include paths and defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is
 * committed. */
#include <stdlib.h>
#include <string.h>

#include "definitions.h"
#include "md_process.h"
#include "mcomp.h"
#include "av1me.h"

void ref_init(void);
void init_fn_ptr(void);

typedef struct PinSubpel {
    int32_t w, h, src_stride, ref_stride, start_row, start_col, ref_row, ref_col, col_min, col_max, row_min, row_max;
    int32_t method, search_type, iters_per_step, forced_stop, allow_hp, bias_fp, skip_diag_refinement, pred_variance_th, abs_th_mult, round_dev_th, qp;
    int32_t mv_cost_type, error_per_bit, early_exit_th, early_exit;
    int32_t mvp_th, hp_mv_th, best_mvp_dist, best_mvp_row, best_mvp_col;
} PinSubpel;

static void pin_init(void) {
    static int done;
    if (!done)
        ref_init(), init_fn_ptr(), done = 1;
}

/* out: best_mv.row, best_mv.col, the return value, *distortion, *sse1 (0 going in), the centre's error (ctx->fp_me_dist where there is a
 * context; otherwise the same sum from the same functions: vf at the start plus svt_aom_fp_mv_err_cost) */
void pin_subpel(const PinSubpel *a, uint8_t *src, uint8_t *ref, const int *mvjcost, const int *mvcost_row, const int *mvcost_col, int64_t *out) {
    pin_init();
    BlockSize bsize = BLOCK_INVALID;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == a->w && block_size_high[b] == a->h)
            bsize = (BlockSize)b;
    MacroBlockD *xd = calloc(1, sizeof(*xd));
    SUBPEL_MOTION_SEARCH_PARAMS ms;
    memset(&ms, 0, sizeof(ms));
    MV ref_mv = {(int16_t)a->ref_row, (int16_t)a->ref_col}, start = {(int16_t)a->start_row, (int16_t)a->start_col}, best = {0, 0};
    ms.search_stage = SPEL_ME, ms.list_idx = 0, ms.ref_idx = 0;
    ms.allow_hp = a->allow_hp, ms.forced_stop = (SUBPEL_FORCE_STOP)a->forced_stop, ms.iters_per_step = a->iters_per_step;
    ms.pred_variance_th = a->pred_variance_th, ms.abs_th_mult = (uint8_t)a->abs_th_mult, ms.round_dev_th = a->round_dev_th;
    ms.skip_diag_refinement = (uint8_t)a->skip_diag_refinement;
    ms.mv_limits.col_min = a->col_min, ms.mv_limits.col_max = a->col_max, ms.mv_limits.row_min = a->row_min, ms.mv_limits.row_max = a->row_max;
    MV_COST_PARAMS *cp = &ms.mv_cost_params;
    cp->ref_mv = &ref_mv, cp->mv_cost_type = (MV_COST_TYPE)a->mv_cost_type, cp->mvjcost = mvjcost, cp->mvcost[0] = mvcost_row, cp->mvcost[1] = mvcost_col;
    cp->error_per_bit = a->error_per_bit, cp->early_exit_th = a->early_exit_th;
    struct svt_buf_2d src_buf = {src, a->w, a->h, a->src_stride}, ref_buf = {ref, a->w, a->h, a->ref_stride};
    ms.var_params.vfp = &svt_aom_mefn_ptr[bsize], ms.var_params.subpel_search_type = (SUBPEL_SEARCH_TYPE)a->search_type;
    ms.var_params.w = a->w, ms.var_params.h = a->h, ms.var_params.bias_fp = a->bias_fp != 0;
    ms.var_params.ms_buffers.src = &src_buf, ms.var_params.ms_buffers.ref = &ref_buf;
    ModeDecisionContext *ctx = NULL;
    if (a->mvp_th > 0) {
        ctx = calloc(1, sizeof(*ctx));
        ctx->pd_pass = PD_PASS_1, ctx->md_subpel_me_ctrls.mvp_th = (uint8_t)a->mvp_th, ctx->md_subpel_me_ctrls.hp_mv_th = a->hp_mv_th;
        ctx->best_fp_mvp_dist[0][0] = (uint32_t)a->best_mvp_dist, ctx->best_fp_mvp_idx[0][0] = 1;
        ctx->mvp_array[0][0][1].row = (int16_t)a->best_mvp_row, ctx->mvp_array[0][0][1].col = (int16_t)a->best_mvp_col;
    }
    int          distortion = 0;
    unsigned int sse1 = 0;
    fractional_mv_step_fp *fn = a->method == SUBPEL_TREE ? svt_av1_find_best_sub_pixel_tree : svt_av1_find_best_sub_pixel_tree_pruned;
    const int besterr = fn(ctx, xd, NULL, &ms, start, &best, &distortion, &sse1, a->qp, bsize, (uint8_t)a->early_exit);
    unsigned int centre_sse;
    const uint8_t *at = ref + (start.row >> 3) * a->ref_stride + (start.col >> 3);
    const unsigned int centre = ms.var_params.vfp->vf(at, a->ref_stride, src, a->src_stride, &centre_sse) + svt_aom_fp_mv_err_cost(&start, cp);
    out[0] = best.row, out[1] = best.col, out[2] = besterr, out[3] = distortion, out[4] = sse1;
    out[5] = ctx ? ctx->fp_me_dist[0][0] : centre;
    if (ctx && ctx->fp_me_dist[0][0] != centre)
        out[5] = -1;
    free(ctx), free(xd);
}

/* product_coding_loop.c:2527-2537 with the reference's two range functions; out: col_min, col_max, row_min, row_max */
void pin_limits(int32_t mi_row, int32_t mi_col, int32_t mi_width, int32_t mi_height, int32_t mi_rows, int32_t mi_cols, int32_t ref_row, int32_t ref_col,
                int32_t *out) {
    MV       ref_mv = {(int16_t)ref_row, (int16_t)ref_col};
    MvLimits mv_limits;
    mv_limits.row_min = -(((mi_row + mi_height) * MI_SIZE) + AOM_INTERP_EXTEND);
    mv_limits.col_min = -(((mi_col + mi_width) * MI_SIZE) + AOM_INTERP_EXTEND);
    mv_limits.row_max = (mi_rows - mi_row) * MI_SIZE + AOM_INTERP_EXTEND;
    mv_limits.col_max = (mi_cols - mi_col) * MI_SIZE + AOM_INTERP_EXTEND;
    svt_av1_set_mv_search_range(&mv_limits, &ref_mv);
    SubpelMvLimits s;
    svt_av1_set_subpel_mv_search_range(&s, (FullMvLimits *)&mv_limits, &ref_mv);
    out[0] = s.col_min, out[1] = s.col_max, out[2] = s.row_min, out[3] = s.row_max;
}

/* the constants the header and the restatement state */
void pin_constants(int32_t *out) {
    const int32_t v[16] = {SUBPEL_TREE, SUBPEL_TREE_PRUNED, USE_2_TAPS, USE_4_TAPS, USE_8_TAPS, MV_COST_ENTROPY, MV_COST_L1_LOWRES, MV_COST_L1_MIDRES,
                           MV_COST_L1_HDRES, MV_COST_OPT, MV_COST_NONE, FULL_PEL, MV_LOW, MV_UPP, MAX_FULL_PEL_VAL, QUARTER_PEL};
    memcpy(out, v, sizeof(v));
}
