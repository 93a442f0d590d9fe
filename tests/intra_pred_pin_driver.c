/* TEST INFRASTRUCTURE — pins the Python restatement of tests/intra_pred_cases.py against the reference's two static functions.
 * The reference's enc_intra_prediction.c is included from where it lies (nothing is copied), so that build_intra_predictors and
 * build_intra_predictors_high can be called with flat arguments.  filt_type reaches them the way the encoder passes it: through
 * xd->above_mbmi, a block whose luma mode is SMOOTH_PRED.  Built by tests/test_intra_pred_abi.py into a temporary directory with
 * the include paths and defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include "enc_intra_prediction.c"

static const MacroBlockD *pin_xd(MacroBlockD *xd, MbModeInfo *mi, int filt_type) {
    memset(xd, 0, sizeof(*xd));
    memset(mi, 0, sizeof(*mi));
    mi->block_mi.mode = SMOOTH_PRED;
    xd->above_mbmi    = filt_type ? mi : NULL;
    return xd;
}

void pin_build_intra_predictors(uint8_t *above_ref, uint8_t *left_ref, uint8_t *dst, int32_t dst_stride, int32_t mode, int32_t angle_delta,
                                int32_t filter_intra_mode, int32_t tx_size, int32_t disable_edge_filter, int32_t n_top_px,
                                int32_t n_topright_px, int32_t n_left_px, int32_t n_bottomleft_px, int32_t filt_type) {
    MacroBlockD xd;
    MbModeInfo  mi;
    build_intra_predictors(pin_xd(&xd, &mi, filt_type), above_ref, left_ref, dst, dst_stride, (PredictionMode)mode, angle_delta,
                           (FilterIntraMode)filter_intra_mode, (TxSize)tx_size, disable_edge_filter, n_top_px, n_topright_px, n_left_px,
                           n_bottomleft_px, 0);
}

void pin_build_intra_predictors_high(uint16_t *above_ref, uint16_t *left_ref, uint16_t *dst, int32_t dst_stride, int32_t mode,
                                     int32_t angle_delta, int32_t filter_intra_mode, int32_t tx_size, int32_t disable_edge_filter,
                                     int32_t n_top_px, int32_t n_topright_px, int32_t n_left_px, int32_t n_bottomleft_px, int32_t filt_type,
                                     int32_t bd) {
    MacroBlockD xd;
    MbModeInfo  mi;
    build_intra_predictors_high(pin_xd(&xd, &mi, filt_type), above_ref, left_ref, dst, dst_stride, (PredictionMode)mode, angle_delta,
                                (FilterIntraMode)filter_intra_mode, (TxSize)tx_size, disable_edge_filter, n_top_px, n_topright_px,
                                n_left_px, n_bottomleft_px, 0, bd);
}
