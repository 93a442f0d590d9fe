/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/scale_cases.py against two functions of the reference
 * that cannot be called through oracle/_ref/libsvtref.so as they stand: svt_av1_upscale_normative_rows (super_res.c:214) wants an
 * Av1Common, and compute_subpel_params (enc_inter_prediction.c:3126) is static.  It also hands out the reference's own filter banks, one
 * of which (av1_resize_filter_normative, super_res.h) is static too.  The reference's enc_inter_prediction.c is included from where it
 * lies (nothing is copied).  Built by tests/test_scale_abi.py (and by tests/golden/make_golden_scale.py) into a temporary directory
 * with the include paths and defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include "enc_inter_prediction.c"

#include "resize.h"
#include "super_res.h"

extern const int16_t av1_down2_symodd_half_filter[4];

/* banks: [5][64][8] in the order 1000, 875, 750, 625, 500; half: svt_aom_av1_down2_symeven_half_filter, av1_down2_symodd_half_filter */
void pin_filter_banks(int16_t *banks, int16_t *half) {
    const void *src[5] = {av1_resize_filter_normative, svt_aom_av1_filteredinterp_filters875, svt_aom_av1_filteredinterp_filters750,
                          svt_aom_av1_filteredinterp_filters625, svt_aom_av1_filteredinterp_filters500};
    for (int b = 0; b < 5; b++) memcpy(banks + b * 64 * 8, src[b], 64 * 8 * sizeof(int16_t));
    memcpy(half, svt_aom_av1_down2_symeven_half_filter, 4 * sizeof(int16_t));
    memcpy(half + 4, av1_down2_symodd_half_filter, 4 * sizeof(int16_t));
}

/* src: column 0 of the first row, with at least five samples the function may overwrite and restore on either side of each row.
 * starts: tile_cols + 1 entries, the last one is mi_cols. */
void pin_upscale_rows(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t rows, int32_t sub_x, int32_t bd, int32_t is_16bit,
                      int32_t frame_width, int32_t upscaled_width, int32_t denom, int32_t tile_cols, const uint16_t *starts) {
    Av1Common *cm = calloc(1, sizeof(*cm));
    cm->frm_size.frame_width             = (uint16_t)frame_width;
    cm->frm_size.superres_upscaled_width = (uint16_t)upscaled_width;
    cm->frm_size.superres_denominator    = (uint8_t)denom;
    cm->tiles_info.tile_cols             = (uint8_t)tile_cols;
    for (int j = 0; j <= tile_cols; j++) cm->tiles_info.tile_col_start_mi[j] = starts[j];
    cm->mi_cols = starts[tile_cols];
    svt_av1_upscale_normative_rows(cm, src, src_stride, dst, dst_stride, rows, sub_x, bd, (Bool)is_16bit);
    free(cm);
}

/* out: pos_x, pos_y, subpel_x, subpel_y, xs, ys.  Returns av1_is_scaled of the factors: 0 means the un-scaled branch ran (not what
 * svt_hip_scaled_block_position stands for). */
int32_t pin_subpel_params(int32_t other_w, int32_t other_h, int32_t this_w, int32_t this_h, int32_t sb_size, int32_t pre_x, int32_t pre_y, int32_t mv_col,
                          int32_t mv_row, int32_t ss_x, int32_t ss_y, int32_t frame_width, int32_t frame_height, int32_t *out) {
    ScaleFactors sf;
    svt_av1_setup_scale_factors_for_frame(&sf, other_w, other_h, this_w, this_h);
    if (!av1_is_scaled(&sf))
        return 0;
    SequenceControlSet *scs = calloc(1, sizeof(*scs));
    scs->super_block_size   = (uint8_t)sb_size;
    SubpelParams sp;
    MV           mv;
    mv.col = (int16_t)mv_col, mv.row = (int16_t)mv_row;
    compute_subpel_params(scs, (int16_t)pre_y, (int16_t)pre_x, mv, &sf, (uint16_t)frame_width, (uint16_t)frame_height, 0, 0, NULL, (uint32_t)ss_y,
                          (uint32_t)ss_x, &sp, &out[1], &out[0]);
    out[2] = sp.subpel_x, out[3] = sp.subpel_y, out[4] = sp.xs, out[5] = sp.ys;
    free(scs);
    return 1;
}
