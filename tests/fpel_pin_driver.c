/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/fpel_cases.py against the reference's own static
 * functions of product_coding_loop.c, which this file includes for them:
 *   md_sq_motion_search (:2314-2498) and md_nsq_motion_search (:2075-2241) themselves, on zeroed, fabricated PictureControlSet /
 *     PictureParentControlSet / ModeDecisionContext / EbReferenceObject objects that carry only what the two functions read.  The
 *     reference is a KEY_FRAME, so search_area_multiplier comes from check_spatial_mv_size and is dialled through mvp_array; the MVC
 *     list of the NSQ search is the one :2079-2140 derive from a fabricated MeSbResults (pin_pu_tables gives the tables the Python
 *     side needs to say which list that is).
 *   md_full_pel_search (:1918-2046) for single stages with any incoming best and level-0 state (PIN_STAGE), which is also how the
 *     full-pel call of pme_search (:3263-3280) is pinned: pme_search itself needs the MVP machinery around it and is restated only.
 *   The MVP scoring of :3087-3108 sits in the middle of a function that builds the MVP list first; its loop is restated here over
 *     svt_aom_mefn_ptr[bsize].vf (PIN_MVP) and is restated only.
 *   svt_init_mv_cost_params lets md_full_pel_search reach MV_COST_ENTROPY and MV_COST_OPT only; the other cost types are pinned on
 *     svt_pme_sad_loop_kernel_c (pin_psad) and svt_aom_fp_mv_err_cost (pin_mv_cost), which take any MV_COST_PARAMS.
 * Built by tests/test_fpel_abi.py (and by tests/golden/make_golden_fpel.py) into a temporary directory with the include paths and
 * defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include "product_coding_loop.c"

void ref_init(void);
void init_fn_ptr(void);

enum { PIN_MVP, PIN_SQ, PIN_NSQ, PIN_STAGE };

typedef struct PinFpel {
    int32_t mode, w, h, sq_size, stride, pic_width;             /* both pictures: stride, width */
    int32_t blk_org_x, blk_org_y, org_x, org_y, max_width, max_height;
    int32_t ref_row, ref_col, cost_opt, error_per_bit, dist_type, enable_psad;
    int32_t n_mv, mv[12];                                       /* (row, col) pairs */
    /* SQ */
    int32_t pame_distortion_th, multiplier_dial, poc_distance;  /* dial 0 .. 3: the search_area_multiplier check_spatial_mv_size is to give */
    int32_t lev_enabled[3], lev_step[3], lev_w[3], lev_h[3], lev_max_w[3], lev_max_h[3], lev_multiplier[3];
    /* NSQ */
    int32_t nsq_width, nsq_height, blk_geom_org_x, blk_geom_org_y, sub_mv[2 * 85]; /* ME vectors (x, y, full-pel) of the 85 square PUs; 0x7fff: absent */
    /* STAGE */
    int32_t start_x, end_x, start_y, end_y, step, lev0_performed, lev0[4], best_mvx, best_mvy;
    uint32_t best_cost;
} PinFpel;

static void pin_init(void) {
    static int done;
    if (!done)
        ref_init(), init_fn_ptr(), done = 1;
}

/* out: best_mvx, best_mvy, best_cost, aux, flag, ctx->sprs_lev0_start_x, _end_x, _start_y, _end_y
 *   MVP:   the winner's col, row, best_fp_mvp_dist, best_fp_mvp_idx
 *   SQ:    *me_mv_x, *me_mv_y; best_cost is not observable (a local) and comes back 0; aux = 0
 *   NSQ:   *me_mv_x, *me_mv_y
 *   STAGE: *best_mvx, *best_mvy, *best_cost */
void pin_fpel(const PinFpel *a, uint8_t *src_pic, uint8_t *ref_pic_buf, const int *mvjcost, const int *mvcost_row, const int *mvcost_col, int64_t *out) {
    pin_init();
    PictureControlSet       *pcs = calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    ModeDecisionContext     *ctx = calloc(1, sizeof(*ctx));
    MdRateEstimationContext *rate = calloc(1, sizeof(*rate));
    EbReferenceObject       *ref_obj = calloc(1, sizeof(*ref_obj));
    MotionEstimationData    *me_data = calloc(1, sizeof(*me_data));
    EbObjectWrapper          wrapper;
    EbPictureBufferDesc      input_pic, ref_pic;
    BlockGeom                geom;
    memset(&wrapper, 0, sizeof(wrapper)), memset(&input_pic, 0, sizeof(input_pic)), memset(&ref_pic, 0, sizeof(ref_pic)), memset(&geom, 0, sizeof(geom));
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == a->w && block_size_high[b] == a->h)
            geom.bsize = (BlockSize)b;
    geom.bwidth = a->w, geom.bheight = a->h, geom.sq_size = a->sq_size, geom.org_x = a->blk_geom_org_x, geom.org_y = a->blk_geom_org_y;
    ref_pic.buffer_y = ref_pic_buf, ref_pic.stride_y = a->stride, ref_pic.org_x = a->org_x, ref_pic.org_y = a->org_y;
    ref_pic.max_width = a->max_width, ref_pic.max_height = a->max_height, ref_pic.width = a->pic_width;
    input_pic = ref_pic, input_pic.buffer_y = src_pic;
    ref_obj->reference_picture = &ref_pic, ref_obj->frame_type = KEY_FRAME;
    wrapper.object_ptr = ref_obj;
    pcs->ref_pic_ptr_array[0][0] = &wrapper, pcs->ppcs = ppcs;
    pcs->picture_number = 100 + a->poc_distance, ppcs->ref_pic_poc_array[0][0] = 100;
    ppcs->pa_me_data = me_data, me_data->max_refs = 1, me_data->max_l0 = 1, me_data->max_cand = 1;
    ppcs->enable_me_16x16 = 1, ppcs->enable_me_8x8 = 1, ppcs->max_number_of_pus_per_sb = SQUARE_PU_COUNT;
    memcpy(rate->nmv_vec_cost, mvjcost, sizeof(rate->nmv_vec_cost));
    rate->nmvcoststack[0] = (int32_t *)mvcost_row, rate->nmvcoststack[1] = (int32_t *)mvcost_col;
    ctx->md_rate_est_ctx = rate, ctx->blk_geom = &geom, ctx->blk_org_x = a->blk_org_x, ctx->blk_org_y = a->blk_org_y;
    ctx->ref_mv.row = (int16_t)a->ref_row, ctx->ref_mv.col = (int16_t)a->ref_col;
    ctx->md_subpel_me_ctrls.skip_diag_refinement = a->cost_opt ? 3 : 0;
    ctx->full_lambda_md[EB_8_BIT_MD] = ctx->fast_lambda_md[EB_8_BIT_MD] = (uint32_t)a->error_per_bit << RD_EPB_SHIFT;
    const uint32_t input_origin_index = (a->blk_org_y + a->org_y) * a->stride + (a->blk_org_x + a->org_x);
    int16_t        mvx = (int16_t)a->mv[1], mvy = (int16_t)a->mv[0];
    memset(out, 0, 9 * sizeof(*out));
    if (a->mode == PIN_MVP) { /* :3087-3108 */
        uint32_t best_mvp_cost = (int32_t)~0;
        for (int8_t mvp_index = 0; mvp_index < a->n_mv; mvp_index++) {
            int32_t ref_origin_index = ref_pic.org_x + (ctx->blk_org_x + ((int16_t)a->mv[2 * mvp_index + 1] >> 3)) +
                (ctx->blk_org_y + ((int16_t)a->mv[2 * mvp_index] >> 3) + ref_pic.org_y) * ref_pic.stride_y;
            const AomVarianceFnPtr *fn_ptr = &svt_aom_mefn_ptr[ctx->blk_geom->bsize];
            unsigned int            sse;
            uint32_t mvp_cost = fn_ptr->vf(ref_pic.buffer_y + ref_origin_index, ref_pic.stride_y, input_pic.buffer_y + input_origin_index, input_pic.stride_y, &sse);
            if (mvp_cost < best_mvp_cost)
                out[3] = mvp_index, out[2] = mvp_cost, best_mvp_cost = mvp_cost, out[0] = a->mv[2 * mvp_index + 1], out[1] = a->mv[2 * mvp_index];
        }
        if (best_mvp_cost == (uint32_t)~0)
            out[2] = best_mvp_cost;
    } else if (a->mode == PIN_SQ) {
        MdSqMotionSearchCtrls *c = &ctx->md_sq_me_ctrls;
        c->enabled = 1, c->dist_type = (DistortionType)a->dist_type, c->pame_distortion_th = a->pame_distortion_th, c->enable_psad = a->enable_psad;
        c->sprs_lev0_enabled = a->lev_enabled[0], c->sprs_lev0_step = a->lev_step[0], c->sprs_lev0_w = a->lev_w[0], c->sprs_lev0_h = a->lev_h[0];
        c->max_sprs_lev0_w = a->lev_max_w[0], c->max_sprs_lev0_h = a->lev_max_h[0], c->sprs_lev0_multiplier = a->lev_multiplier[0];
        c->sprs_lev1_enabled = a->lev_enabled[1], c->sprs_lev1_step = a->lev_step[1], c->sprs_lev1_w = a->lev_w[1], c->sprs_lev1_h = a->lev_h[1];
        c->max_sprs_lev1_w = a->lev_max_w[1], c->max_sprs_lev1_h = a->lev_max_h[1], c->sprs_lev1_multiplier = a->lev_multiplier[1];
        c->sprs_lev2_enabled = a->lev_enabled[2], c->sprs_lev2_step = a->lev_step[2], c->sprs_lev2_w = a->lev_w[2], c->sprs_lev2_h = a->lev_h[2];
        /* check_spatial_mv_size: one MVP whose column lies above the threshold of the wanted category */
        static const int16_t dial[4] = {0, LOW_SPATIAL_MV_TH + 1, MEDIUM_SPATIAL_MV_TH + 1, HIGH_SPATIAL_MV_TH + 1};
        ctx->mvp_count[0][0] = a->multiplier_dial ? 1 : 0, ctx->mvp_array[0][0][0].col = dial[a->multiplier_dial];
        md_sq_motion_search(pcs, ctx, &input_pic, input_origin_index, 0, 0, &mvx, &mvy);
        out[0] = mvx, out[1] = mvy;
        out[5] = ctx->sprs_lev0_start_x, out[6] = ctx->sprs_lev0_end_x, out[7] = ctx->sprs_lev0_start_y, out[8] = ctx->sprs_lev0_end_y;
    } else if (a->mode == PIN_NSQ) {
        MdNsqMotionSearchCtrls *c = &ctx->md_nsq_me_ctrls;
        c->enabled = 1, c->dist_type = (DistortionType)a->dist_type, c->enable_psad = a->enable_psad;
        c->full_pel_search_width = a->nsq_width, c->full_pel_search_height = a->nsq_height;
        MeSbResults me;
        memset(&me, 0, sizeof(me));
        me.total_me_candidate_index = calloc(SQUARE_PU_COUNT, 1), me.me_mv_array = calloc(SQUARE_PU_COUNT, sizeof(MvCandidate));
        me.me_candidate_array = calloc(SQUARE_PU_COUNT, sizeof(MeCandidate));
        for (int i = 0; i < SQUARE_PU_COUNT; i++)
            if (a->sub_mv[2 * i] != 0x7fff) /* a list-0, reference-0 unipred candidate */
                me.total_me_candidate_index[i] = 1, me.me_mv_array[i].x_mv = (int16_t)a->sub_mv[2 * i], me.me_mv_array[i].y_mv = (int16_t)a->sub_mv[2 * i + 1];
        md_nsq_motion_search(pcs, ctx, &input_pic, input_origin_index, 0, 0, &me, &mvx, &mvy);
        out[0] = mvx, out[1] = mvy;
        free(me.total_me_candidate_index), free(me.me_mv_array), free(me.me_candidate_array);
    } else {
        int16_t  best_mvx = (int16_t)a->best_mvx, best_mvy = (int16_t)a->best_mvy;
        uint32_t best_cost = a->best_cost;
        ctx->enable_psad = a->enable_psad;
        ctx->sprs_lev0_start_x = a->lev0[0], ctx->sprs_lev0_end_x = a->lev0[1], ctx->sprs_lev0_start_y = a->lev0[2], ctx->sprs_lev0_end_y = a->lev0[3];
        md_full_pel_search(pcs, ctx, &input_pic, &ref_pic, input_origin_index, (DistortionType)a->dist_type, mvx, mvy, a->start_x, a->end_x, a->start_y,
                           a->end_y, a->step, a->lev0_performed, &best_mvx, &best_mvy, &best_cost, EB_8_BIT_MD);
        out[0] = best_mvx, out[1] = best_mvy, out[2] = best_cost;
    }
    free(pcs), free(ppcs), free(ctx), free(rate), free(ref_obj), free(me_data);
}

/* svt_pme_sad_loop_kernel_c under any cost type; best: mvx, mvy, cost in and out */
void pin_psad(int32_t cost_type, int32_t error_per_bit, int32_t ref_row, int32_t ref_col, const int *mvjcost, const int *mvcost_row, const int *mvcost_col,
              uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride, uint32_t h, uint32_t w, int32_t start_x, int32_t start_y, int32_t area_w,
              int32_t area_h, int32_t step, int32_t mvx, int32_t mvy, int64_t *best) {
    MV             ref_mv = {(int16_t)ref_row, (int16_t)ref_col};
    MV_COST_PARAMS p;
    memset(&p, 0, sizeof(p));
    p.ref_mv = &ref_mv, p.mv_cost_type = (MV_COST_TYPE)cost_type, p.error_per_bit = error_per_bit, p.mvjcost = mvjcost, p.mvcost[0] = mvcost_row, p.mvcost[1] = mvcost_col;
    uint32_t cost = (uint32_t)best[2];
    int16_t  bx = (int16_t)best[0], by = (int16_t)best[1];
    svt_pme_sad_loop_kernel_c(&p, src, src_stride, ref, ref_stride, h, w, &cost, &bx, &by, start_x, start_y, area_w, area_h, step, mvx, mvy);
    best[0] = bx, best[1] = by, best[2] = cost;
}

int32_t pin_mv_cost(int32_t cost_type, int32_t error_per_bit, int32_t ref_row, int32_t ref_col, int32_t row, int32_t col, const int *mvjcost,
                    const int *mvcost_row, const int *mvcost_col) {
    MV             ref_mv = {(int16_t)ref_row, (int16_t)ref_col}, mv = {(int16_t)row, (int16_t)col};
    MV_COST_PARAMS p;
    memset(&p, 0, sizeof(p));
    p.ref_mv = &ref_mv, p.mv_cost_type = (MV_COST_TYPE)cost_type, p.error_per_bit = error_per_bit, p.mvjcost = mvjcost, p.mvcost[0] = mvcost_row, p.mvcost[1] = mvcost_col;
    return svt_aom_fp_mv_err_cost(&mv, &p);
}

/* x, y, width, height of the 85 square PUs, as :2096-2103 read them */
void pin_pu_tables(int32_t *out) {
    for (int i = 0; i < SQUARE_PU_COUNT; i++)
        out[4 * i] = pu_search_index_map[i][0], out[4 * i + 1] = pu_search_index_map[i][1], out[4 * i + 2] = partition_width[i], out[4 * i + 3] = partition_height[i];
}

uint16_t pin_scaled_distance(uint16_t dist) { return svt_aom_get_scaled_picture_distance(dist); }

/* the constants the header and the restatement state */
void pin_constants(int32_t *out) {
    const int32_t v[16] = {SAD, VAR, SSD, MV_COST_ENTROPY, MV_COST_L1_LOWRES, MV_COST_L1_MIDRES, MV_COST_L1_HDRES, MV_COST_OPT, MV_COST_NONE,
                           MAX_MD_NSQ_SARCH_MVC_CNT, MAX_MVP_CANIDATES, SQUARE_PU_COUNT, LOW_SPATIAL_MV_TH, MEDIUM_SPATIAL_MV_TH, HIGH_SPATIAL_MV_TH, RD_EPB_SHIFT};
    memcpy(out, v, sizeof(v));
}
