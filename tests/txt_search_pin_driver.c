/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/txt_search_cases.py against the reference's own
 * static tx_type_search (product_coding_loop.c:4458-4940): the candidate order from tx_type_group[_sc], only_dct_dct and
 * av1_ext_tx_used, the rate-cost threshold, the SATD early exit, the quantiser with its RDOQ stage, the inverse transform and the
 * spatial or transform-domain distortion, the early_cost skip, the coefficient rate, the cost comparison, the coefficient-count /
 * cost exit and copy_txt_data.  The reference's product_coding_loop.c is included from where it lies (nothing is copied).  The control
 * structures are zeroed and only what the call reads is set; update_skip_ctx_dc_sign_ctx stays off, so both contexts are 0.  Built by
 * tests/test_txt_search_abi.py (and by tests/golden/make_golden_txt_search.py) into a temporary directory with the include paths and
 * defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include "product_coding_loop.c"

#include "md_config_process.h"

typedef struct PinTables {
    MdRateEstimationContext rate;
    FRAME_CONTEXT           fc;
} PinTables;

void *pin_tables_new(int32_t base_qindex) {
    PinTables *t = calloc(1, sizeof(*t));
    svt_av1_default_coef_probs(&t->fc, base_qindex);
    svt_aom_init_mode_probs(&t->fc);
    svt_aom_estimate_syntax_rate(&t->rate, 1, 1, 0, 1, 0, &t->fc);
    svt_aom_estimate_coefficients_rate(&t->rate, &t->fc);
    return t;
}

/* what one call of tx_type_search depends on besides the pixels */
typedef struct PinTxt {
    int32_t  bit_depth, qindex, tx_size, w, h, is_inter, pred_mode, spatial_sse, rdoq_level, sc_class1, n_groups;
    uint32_t lambda;
    int32_t  satd_th, rate_th, coeff_th, dist_th, crop_w, crop_h;
    int32_t  residual_stride, pred_stride, src_stride, recon_stride; /* in samples */
} PinTxt;

/* the reference's loop order for a block: tx_type_group[_sc] rows 0 .. n_groups - 1 without the types av1_ext_tx_used refuses; returns
 * the count, group_start gets bit k where candidate k is the first its row visits */
int32_t pin_candidate_order(int32_t tx_size, int32_t is_inter, int32_t reduced_tx_set, int32_t sc, int32_t n_groups, uint8_t *types, uint32_t *group_start) {
    const TxSetType set = get_ext_tx_set_type((TxSize)tx_size, is_inter, reduced_tx_set);
    int32_t         n = 0;
    *group_start = 0;
    for (int g = 0; g < n_groups; g++) {
        int first = 1;
        for (int i = 0; i < TX_TYPES; i++) {
            const int t = sc ? tx_type_group_sc[g][i] : tx_type_group[g][i];
            if (t == INVALID_TX_TYPE)
                break;
            if (t != DCT_DCT && !av1_ext_tx_used[set][t])
                continue;
            if (first)
                *group_start |= 1u << n, first = 0;
            types[n++] = (uint8_t)t;
        }
    }
    return n;
}

static EbPictureBufferDesc *pin_buffer(void *data, uint32_t stride) {
    EbPictureBufferDesc *d = calloc(1, sizeof(*d));
    d->buffer_y = data, d->stride_y = (uint16_t)stride;
    return d;
}

/* tx_type_search on one transform block at the origin of its superblock.  residual: int16 [h][residual_stride]; pred, src: samples
 * (uint8, or uint16 above 8 bits).  Leaves cand_bf's quant and rec_coeff blocks (w * h int32 each; zero-filled before the call) and
 * recon block ([h][recon_stride] samples, as handed in) in the caller's arrays and
 * out = {transform_type, y_coeff_bits, y_full_distortion[DIST_SSD][RESIDUAL], [PREDICTION], eob.y, y_has_coeff}. */
void pin_tx_type_search(void *tables, const PinTxt *a, int16_t *residual, void *pred, void *src, int32_t *quant, int32_t *rec_coeff, void *recon,
                        uint64_t *out) {
    EncodeContext           *enc = calloc(1, sizeof(*enc));
    SequenceControlSet      *scs = calloc(1, sizeof(*scs));
    PictureControlSet       *pcs = calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    ModeDecisionContext     *ctx = calloc(1, sizeof(*ctx));
    BlockGeom               *geom = calloc(1, sizeof(*geom));
    SuperBlock              *sb = calloc(1, sizeof(*sb));
    BlkStruct               *blk = calloc(1, sizeof(*blk));
    ModeDecisionCandidateBuffer *cand_bf = calloc(1, sizeof(*cand_bf));
    ModeDecisionCandidate       *cand = calloc(1, sizeof(*cand));
    const size_t n = (size_t)a->w * a->h, px = a->bit_depth > 8 ? 2 : 1, recon_bytes = (size_t)a->h * a->recon_stride * px;
    void        *scratch[3 * TX_TYPES + 1];
    int          n_scratch = 0;

    svt_av1_build_quantizer(EB_EIGHT_BIT, 0, 0, 0, 0, 0, &enc->quants_8bit, &enc->deq_8bit);
    svt_av1_build_quantizer(EB_TEN_BIT, 0, 0, 0, 0, 0, &enc->quants_bd, &enc->deq_bd);
    scs->enc_ctx = enc, pcs->scs = scs, pcs->ppcs = ppcs, ppcs->scs = scs;
    svt_av1_qm_init(ppcs);
    for (int p = 0; p < 3; p++) ppcs->frm_hdr.quantization_params.qm[p] = NUM_QM_LEVELS - 1;
    ppcs->frm_hdr.quantization_params.base_q_idx = (uint8_t)a->qindex;
    ppcs->frm_hdr.delta_q_params.delta_q_present = 1;
    ppcs->sc_class1 = (uint8_t)a->sc_class1;
    ppcs->aligned_width = (uint16_t)a->crop_w, ppcs->aligned_height = (uint16_t)a->crop_h; /* cropped_tx_width / cropped_tx_height */
    EbPictureBufferDesc *input = pin_buffer(src, a->src_stride);
    input->bit_depth = (EbBitDepth)a->bit_depth;
    ppcs->enhanced_pic = input, pcs->input_frame16bit = input;
    sb->qindex = 255;

    geom->txsize[0] = geom->txsize_uv[0] = (TxSize)a->tx_size;
    geom->tx_width[0] = geom->bwidth = (uint8_t)a->w, geom->tx_height[0] = geom->bheight = (uint8_t)a->h;
    geom->sq_size = 16, geom->bsize = BLOCK_16X16;
    ctx->sb_ptr = sb, ctx->blk_geom = geom, ctx->blk_ptr = blk;
    ctx->md_rate_est_ctx = &((PinTables *)tables)->rate;
    ctx->hbd_md = a->bit_depth > 8;
    ctx->full_lambda_md[EB_8_BIT_MD] = ctx->full_lambda_md[EB_10_BIT_MD] = a->lambda;
    ctx->mds_txt_level = 1, ctx->mds_fast_coeff_est_level = 1, ctx->rate_est_ctrls.coeff_rate_est_lvl = 1;
    ctx->mds_spatial_sse = (uint8_t)a->spatial_sse;
    ctx->rdoq_level = (uint8_t)a->rdoq_level;
    RdoqCtrls *r = &ctx->rdoq_ctrls;
    r->fp_q_y = r->fp_q_uv = 1, r->satd_factor = r->eob_th = r->eob_fast_th = 255;
    TxtControls *t = &ctx->txt_ctrls;
    t->txt_group_inter_lt_16x16 = t->txt_group_inter_gt_eq_16x16 = t->txt_group_intra_lt_16x16 = t->txt_group_intra_gt_eq_16x16 = (uint8_t)a->n_groups;
    t->satd_early_exit_th_inter = t->satd_early_exit_th_intra = (uint16_t)a->satd_th, t->satd_th_q_weight = (uint16_t)~0;
    t->txt_rate_cost_th = (uint16_t)a->rate_th, t->early_exit_coeff_th = (uint32_t)a->coeff_th, t->early_exit_dist_th = (uint32_t)a->dist_th;

    cand->pred_mode = (PredictionMode)a->pred_mode, cand->filter_intra_mode = FILTER_INTRA_MODES;
    cand_bf->cand = cand;
    cand_bf->residual = pin_buffer(residual, a->residual_stride), cand_bf->pred = pin_buffer(pred, a->pred_stride);
    cand_bf->recon = pin_buffer(recon, a->recon_stride);
    memset(quant, 0, n * 4), memset(rec_coeff, 0, n * 4);
    cand_bf->quant = pin_buffer(quant, 0), cand_bf->rec_coeff = pin_buffer(rec_coeff, 0);
    ctx->tx_coeffs = pin_buffer(scratch[n_scratch++] = calloc(n, 4), 0);
    for (int k = 0; k < TX_TYPES; k++) {
        ctx->recon_coeff_ptr[k] = pin_buffer(scratch[n_scratch++] = calloc(n, 4), 0);
        ctx->quant_coeff_ptr[k] = pin_buffer(scratch[n_scratch++] = calloc(n, 4), 0);
        ctx->recon_ptr[k] = pin_buffer(scratch[n_scratch++] = calloc(1, recon_bytes), a->recon_stride);
    }

    uint64_t bits = 0, dist[DIST_TOTAL][DIST_CALC_TOTAL] = {{0}};
    tx_type_search(pcs, ctx, cand_bf, (uint32_t)a->qindex, 0, &bits, dist);
    out[0] = cand->transform_type[0], out[1] = bits, out[2] = dist[DIST_SSD][DIST_CALC_RESIDUAL], out[3] = dist[DIST_SSD][DIST_CALC_PREDICTION];
    out[4] = cand_bf->eob.y[0], out[5] = cand_bf->y_has_coeff;

    for (int k = 0; k < n_scratch; k++) free(scratch[k]);
    free(ctx->tx_coeffs);
    for (int k = 0; k < TX_TYPES; k++) free(ctx->recon_coeff_ptr[k]), free(ctx->quant_coeff_ptr[k]), free(ctx->recon_ptr[k]);
    free(cand_bf->residual), free(cand_bf->pred), free(cand_bf->recon), free(cand_bf->quant), free(cand_bf->rec_coeff), free(input);
    free(cand), free(cand_bf), free(blk), free(sb), free(geom), free(ctx), free(ppcs), free(pcs), free(scs), free(enc);
}
