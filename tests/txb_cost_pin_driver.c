/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/txb_cost_cases.py against the reference's own
 * rate estimation.  The tables are the ones the encoder builds for a picture (default CDFs of a base qindex -> svt_aom_estimate_syntax_rate
 * + svt_aom_estimate_coefficients_rate); the bits are what svt_av1_cost_coeffs_txb returns, taken either directly or through its caller
 * svt_aom_txb_estimate_coeff_bits, which shifts the luma rate by mds_subres_step and returns the skip cost for eob 0.  The
 * ModeDecisionContext, the picture control sets and the candidate are zeroed; only what the call reads is set.  Built by tests/test_txb_cost_abi.py (and by
 * tests/golden/make_golden_txb_cost.py) into a temporary directory with the include paths and defines of oracle/Makefile and linked
 * against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include <stdlib.h>
#include <string.h>

#include "definitions.h"
#include "pcs.h"
#include "md_process.h"
#include "mode_decision.h"
#include "md_rate_estimation.h"
#include "rd_cost.h"
#include "coefficients.h"
#include "full_loop.h"

#include "svt_hip_txfm.h"

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

void pin_tables_free(void *t) { free(t); }

/* fills an SvtHipRateTables the way a caller of svt_hip_txb_cost_batch does (include/svt_hip_txfm.h); eob_extra_cost has
 * EOB_COEF_CONTEXTS = 22 rows in the reference, of which get_eob_cost reaches the first 9 (eob_pt - 3) */
size_t pin_tables_export(const void *tables, SvtHipRateTables *out) {
    const MdRateEstimationContext *r = &((const PinTables *)tables)->rate;
    for (int s = 0; s < TX_SIZES; s++)
        for (int p = 0; p < PLANE_TYPES; p++) {
            const LvMapCoeffCost *c = &r->coeff_fac_bits[s][p];
            SvtHipCoeffCost      *o = &out->coeff[s][p];
            memcpy(o->txb_skip, c->txb_skip_cost, sizeof(o->txb_skip));
            memcpy(o->base_eob, c->base_eob_cost, sizeof(o->base_eob));
            memcpy(o->base, c->base_cost, sizeof(o->base));
            memcpy(o->eob_extra, c->eob_extra_cost, sizeof(o->eob_extra));
            memcpy(o->dc_sign, c->dc_sign_cost, sizeof(o->dc_sign));
            memcpy(o->lps, c->lps_cost, sizeof(o->lps));
        }
    memcpy(out->eob, r->eob_frac_bits, sizeof(out->eob));
    memcpy(out->intra_tx_type, r->intra_tx_type_fac_bits, sizeof(out->intra_tx_type));
    memcpy(out->inter_tx_type, r->inter_tx_type_fac_bits, sizeof(out->inter_tx_type));
    /* every array but eob_extra has the reference's own size */
    return sizeof(out->eob) == sizeof(r->eob_frac_bits) && sizeof(out->intra_tx_type) == sizeof(r->intra_tx_type_fac_bits) &&
            sizeof(out->inter_tx_type) == sizeof(r->inter_tx_type_fac_bits) && sizeof(out->coeff[0][0].lps) == sizeof(r->coeff_fac_bits[0][0].lps_cost) &&
            sizeof(out->coeff[0][0].base) == sizeof(r->coeff_fac_bits[0][0].base_cost) && sizeof(out->coeff) / sizeof(out->coeff[0][0]) == TX_SIZES * PLANE_TYPES
        ? sizeof(*out)
        : 0;
}

/* iscan of av1_scan_orders[tx_size][tx_type]: n = retained coefficients */
int32_t pin_iscan(int32_t tx_size, int32_t tx_type, int16_t *iscan) {
    const int32_t n = get_txb_wide_tab[tx_size] * get_txb_high_tab[tx_size];
    memcpy(iscan, av1_scan_orders[tx_size][tx_type].iscan, n * sizeof(int16_t));
    return n;
}

int32_t pin_tx_type_allowed(int32_t tx_size, int32_t tx_type, int32_t is_inter, int32_t reduced_tx_set) {
    return av1_ext_tx_used[get_ext_tx_set_type((TxSize)tx_size, is_inter, reduced_tx_set)][tx_type];
}

/* the enumerators the descriptor's ranges rest on: NEARESTMV, MB_MODE_COUNT, FILTER_INTRA_MODES, D157_PRED, TX_SIZES_ALL */
int32_t pin_enum(int32_t which) {
    const int32_t v[5] = {NEARESTMV, MB_MODE_COUNT, FILTER_INTRA_MODES, D157_PRED, TX_SIZES_ALL};
    return v[which];
}

/* svt_av1_cost_coeffs_txb itself (eob > 0), not shifted */
static uint64_t pin_cost_coeffs_txb(ModeDecisionContext *ctx, ModeDecisionCandidateBuffer *cand_bf, const int32_t *qcoeff, uint32_t eob,
                                    int32_t plane_type, int32_t tx_size, int32_t tx_type, int32_t txb_skip_ctx, int32_t dc_sign_ctx,
                                    int32_t reduced_tx_set) {
    return svt_av1_cost_coeffs_txb(ctx, 0, NULL, cand_bf, qcoeff, (uint16_t)eob, (PlaneType)plane_type, (TxSize)tx_size, (TxType)tx_type,
                                   (int16_t)txb_skip_ctx, (int16_t)dc_sign_ctx, (Bool)reduced_tx_set);
}

/* direct != 0 and eob > 0: the return value of svt_av1_cost_coeffs_txb; otherwise what svt_aom_txb_estimate_coeff_bits hands to mode
 * decision for the luma block (shifted by mds_subres_step) or the Cb block (not shifted) */
uint64_t pin_txb_bits(void *tables, const int32_t *qcoeff, uint32_t eob, int32_t plane_type, int32_t tx_size, int32_t tx_type,
                      int32_t txb_skip_ctx, int32_t dc_sign_ctx, int32_t reduced_tx_set, int32_t pred_mode, int32_t filter_intra_mode,
                      int32_t fast_coeff_est_level, int32_t subres_step, int32_t direct) {
    static ModeDecisionContext     *ctx;
    static PictureControlSet       *pcs;
    static PictureParentControlSet *ppcs;
    if (!ctx)
        ctx = calloc(1, sizeof(*ctx)), pcs = calloc(1, sizeof(*pcs)), ppcs = calloc(1, sizeof(*ppcs));
    memset(ctx, 0, sizeof(*ctx));
    memset(ppcs, 0, sizeof(*ppcs));
    memset(pcs, 0, sizeof(*pcs));
    ModeDecisionCandidateBuffer cand_bf;
    ModeDecisionCandidate       cand;
    EbPictureBufferDesc         coeffs;
    memset(&cand_bf, 0, sizeof(cand_bf));
    memset(&cand, 0, sizeof(cand));
    memset(&coeffs, 0, sizeof(coeffs));
    pcs->ppcs                    = ppcs;
    ppcs->frm_hdr.reduced_tx_set = (uint8_t)reduced_tx_set;
    ctx->md_rate_est_ctx         = &((PinTables *)tables)->rate;
    ctx->mds_fast_coeff_est_level = (uint8_t)fast_coeff_est_level;
    ctx->mds_subres_step          = (uint8_t)subres_step;
    cand.pred_mode                = (PredictionMode)pred_mode;
    cand.filter_intra_mode        = (uint8_t)filter_intra_mode;
    cand_bf.cand                  = &cand;
    uint64_t bits[3] = {0, 0, 0};
    if (direct && eob)
        return pin_cost_coeffs_txb(ctx, &cand_bf, qcoeff, eob, plane_type, tx_size, tx_type, txb_skip_ctx, dc_sign_ctx, reduced_tx_set);
    if (plane_type == 0) {
        ctx->luma_txb_skip_context = (int16_t)txb_skip_ctx, ctx->luma_dc_sign_context = (int16_t)dc_sign_ctx;
        coeffs.buffer_y = (uint8_t *)qcoeff;
        svt_aom_txb_estimate_coeff_bits(ctx, 0, NULL, pcs, &cand_bf, 0, 0, &coeffs, eob, 0, 0, &bits[0], &bits[1], &bits[2], (TxSize)tx_size,
                                        (TxSize)tx_size, (TxType)tx_type, (TxType)tx_type, COMPONENT_LUMA);
        return bits[0];
    }
    ctx->cb_txb_skip_context = (int16_t)txb_skip_ctx, ctx->cb_dc_sign_context = (int16_t)dc_sign_ctx;
    coeffs.buffer_cb = (uint8_t *)qcoeff;
    svt_aom_txb_estimate_coeff_bits(ctx, 0, NULL, pcs, &cand_bf, 0, 0, &coeffs, 0, eob, 0, &bits[0], &bits[1], &bits[2], (TxSize)tx_size,
                                    (TxSize)tx_size, (TxType)tx_type, (TxType)tx_type, COMPONENT_CHROMA_CB);
    return bits[1];
}
