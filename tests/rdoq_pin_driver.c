/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/rdoq_cases.py against the reference's own
 * svt_aom_quantize_inv_quantize (full_loop.c:1462-1686): first quantiser, SATD gate, eob thresholds, svt_fast_optimize_b,
 * svt_av1_optimize_b and svt_av1_compute_cul_level, exactly as mode decision calls it (is_encode_pass = 0).  The quantiser tables
 * are svt_av1_build_quantizer's, the quantisation matrices svt_av1_qm_init's, the rate tables those of
 * tests/txb_cost_pin_driver.c::pin_tables_new.  PictureControlSet, PictureParentControlSet, SequenceControlSet, EncodeContext and
 * ModeDecisionContext are zeroed; only what the call reads is set.  Built by tests/test_rdoq_abi.py (and by
 * tests/golden/make_golden_rdoq.py) into a temporary directory with the include paths and defines of oracle/Makefile and linked
 * against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include <stdlib.h>
#include <string.h>

#include "definitions.h"
#include "pcs.h"
#include "sequence_control_set.h"
#include "encode_context.h"
#include "md_process.h"
#include "mode_decision.h"
#include "md_rate_estimation.h"
#include "md_config_process.h"
#include "rd_cost.h"
#include "coefficients.h"
#include "full_loop.h"

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

/* what one call of svt_aom_quantize_inv_quantize depends on besides the coefficients */
typedef struct PinRdoq {
    int32_t  bit_depth, qindex, plane, tx_size, tx_type, txb_skip_ctx, dc_sign_ctx, is_inter;
    uint32_t lambda;
    int32_t  rdoq_level, fast_mode, sharpness, eob_th, eob_fast_th, satd_factor, early_exit_th, sq_size;
    int32_t  qm_level; /* NUM_QM_LEVELS - 1 = 15: no matrices */
    int32_t  fp_q;     /* rdoq_ctrls.fp_q_y / fp_q_uv */
    int32_t  pic_bd;   /* enhanced_pic->bit_depth; mode decision runs at bit_depth (hbd_md = bit_depth > 8) */
} PinRdoq;

static EncodeContext           *enc;
static SequenceControlSet      *scs;
static PictureControlSet       *pcs;
static PictureParentControlSet *ppcs;
static ModeDecisionContext     *ctx;

static void pin_init(void) {
    if (enc)
        return;
    enc = calloc(1, sizeof(*enc)), scs = calloc(1, sizeof(*scs)), pcs = calloc(1, sizeof(*pcs)), ppcs = calloc(1, sizeof(*ppcs));
    ctx = calloc(1, sizeof(*ctx));
    svt_av1_build_quantizer(EB_EIGHT_BIT, 0, 0, 0, 0, 0, &enc->quants_8bit, &enc->deq_8bit);
    svt_av1_build_quantizer(EB_TEN_BIT, 0, 0, 0, 0, 0, &enc->quants_bd, &enc->deq_bd);
}

/* [7][2]: zbin, round, quant, quant_shift, round_fp, quant_fp, dequant of the luma plane (all deltas are 0: chroma has the same) */
void pin_quant_tables(int32_t bit_depth, int32_t q, int16_t *out) {
    pin_init();
    const Quants   *qt = bit_depth == 8 ? &enc->quants_8bit : &enc->quants_bd;
    const Dequants *dq = bit_depth == 8 ? &enc->deq_8bit : &enc->deq_bd;
    const int16_t  *src[7] = {qt->y_zbin[q], qt->y_round[q], qt->y_quant[q], qt->y_quant_shift[q], qt->y_round_fp[q], qt->y_quant_fp[q], dq->y_dequant_qtx[q]};
    for (int i = 0; i < 7; i++) out[2 * i] = src[i][0], out[2 * i + 1] = src[i][1];
}

/* the matrices svt_av1_qm_init hands out for (level, plane, size); returns their length, 0 where there are none */
int32_t pin_qm(int32_t level, int32_t plane, int32_t tx_size, uint8_t *qm, uint8_t *iqm) {
    pin_init();
    memset(ppcs, 0, sizeof(*ppcs));
    svt_av1_qm_init(ppcs);
    const TxSize adj = tx_size == TX_64X64 || tx_size == TX_64X32 || tx_size == TX_32X64 ? TX_32X32
        : tx_size == TX_64X16                                                            ? TX_32X16
        : tx_size == TX_16X64                                                            ? TX_16X32
                                                                                         : (TxSize)tx_size;
    if (!ppcs->gqmatrix[level][plane][adj])
        return 0;
    const int32_t n = tx_size_2d[adj];
    memcpy(qm, ppcs->gqmatrix[level][plane][adj], n), memcpy(iqm, ppcs->giqmatrix[level][plane][adj], n);
    return n;
}

int32_t pin_iscan(int32_t tx_size, int32_t tx_type, int16_t *iscan) {
    const int32_t n = get_txb_wide_tab[tx_size] * get_txb_high_tab[tx_size];
    memcpy(iscan, av1_scan_orders[tx_size][tx_type].iscan, n * sizeof(int16_t));
    return n;
}

static EbPictureBufferDesc pic;
static BlockGeom           geom;
static SuperBlock          sb;

/* everything svt_aom_quantize_inv_quantize reads; clean: zero the structures first (every field set here is set on every call) */
static void pin_setup(void *tables, const PinRdoq *a, int clean) {
    pin_init();
    if (clean) {
        memset(scs, 0, sizeof(*scs)), memset(pcs, 0, sizeof(*pcs)), memset(ppcs, 0, sizeof(*ppcs)), memset(ctx, 0, sizeof(*ctx));
        memset(&pic, 0, sizeof(pic)), memset(&geom, 0, sizeof(geom)), memset(&sb, 0, sizeof(sb));
        scs->enc_ctx = enc, pcs->scs = scs, pcs->ppcs = ppcs, ppcs->scs = scs;
        svt_av1_qm_init(ppcs);
    }
    ppcs->frm_hdr.quantization_params.using_qmatrix = a->qm_level < NUM_QM_LEVELS - 1;
    for (int p = 0; p < 3; p++) ppcs->frm_hdr.quantization_params.qm[p] = (uint8_t)a->qm_level;
    ppcs->frm_hdr.quantization_params.base_q_idx = (uint8_t)a->qindex;
    ppcs->frm_hdr.delta_q_params.delta_q_present = 1;
    ppcs->enhanced_pic = &pic, pic.bit_depth = (EbBitDepth)a->pic_bd;
    /* the sharpness case: the superblock's qindex below the picture's */
    scs->vq_ctrls.sharpness_ctrls.rdoq = (uint8_t)a->sharpness;
    pcs->picture_qp = a->sharpness ? 63 : 0, sb.qindex = a->sharpness ? 0 : 255;
    ctx->sb_ptr = &sb, ctx->blk_geom = &geom, geom.sq_size = (uint8_t)a->sq_size;
    ctx->md_rate_est_ctx = &((PinTables *)tables)->rate;
    ctx->mds_skip_rdoq = 0, ctx->rdoq_level = (uint8_t)a->rdoq_level, ctx->hbd_md = a->bit_depth > 8;
    ctx->rate_est_ctrls.update_skip_ctx_dc_sign_ctx = 1;
    RdoqCtrls *r = &ctx->rdoq_ctrls;
    r->eob_fast_y_inter = r->eob_fast_y_intra = r->eob_fast_uv_inter = r->eob_fast_uv_intra = (uint8_t)a->fast_mode;
    r->fp_q_y = r->fp_q_uv = (uint8_t)a->fp_q;
    r->satd_factor = (uint8_t)a->satd_factor, r->early_exit_th = (uint8_t)a->early_exit_th;
    r->eob_th = (uint8_t)a->eob_th, r->eob_fast_th = (uint8_t)a->eob_fast_th;
}

static int32_t pin_call(const PinRdoq *a, int32_t *coeff, int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob) {
    return svt_aom_quantize_inv_quantize(pcs, ctx, coeff, qcoeff, dqcoeff, (uint32_t)a->qindex, 0, (TxSize)a->tx_size, eob,
                                         a->plane ? COMPONENT_CHROMA_CB : COMPONENT_LUMA, (uint32_t)a->bit_depth, (TxType)a->tx_type,
                                         (int16_t)a->txb_skip_ctx, (int16_t)a->dc_sign_ctx, a->is_inter ? NEARESTMV : DC_PRED, a->lambda, 0);
}

/* svt_aom_quantize_inv_quantize on coeff: fills qcoeff, dqcoeff and *eob, returns cul_level */
int32_t pin_rdoq(void *tables, const PinRdoq *a, int32_t *coeff, int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob) {
    pin_setup(tables, a, 1);
    return pin_call(a, coeff, qcoeff, dqcoeff, eob);
}

/* the same over n_blocks blocks of n coefficients with their own arguments, for tools/rdoq_time.py: one call, the structures zeroed once */
void pin_rdoq_many(void *tables, const PinRdoq *a, int32_t *coeff, int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob, int32_t n_blocks, int32_t n) {
    for (int32_t i = 0; i < n_blocks; i++) {
        pin_setup(tables, &a[i], i == 0);
        pin_call(&a[i], coeff + (size_t)i * n, qcoeff + (size_t)i * n, dqcoeff + (size_t)i * n, &eob[i]);
    }
}

/* the constants the restatement states: COEFF_CONTEXT_BITS, MAX_TX_SCALE, AOM_QM_BITS, NUM_QM_LEVELS */
int32_t pin_enum(int32_t which) {
    const int32_t v[4] = {COEFF_CONTEXT_BITS, MAX_TX_SCALE, AOM_QM_BITS, NUM_QM_LEVELS};
    return v[which];
}
