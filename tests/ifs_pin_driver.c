/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/ifs_cases.py against the reference's own functions:
 * interpolation_filter_search (enc_inter_prediction.c:2413-2543) wants a PictureControlSet, a ModeDecisionContext and a candidate buffer, and
 * model_rd_for_sb (:2277) reads its pictures and its quantizer through them, so the loop of :2458-2533 is driven here on a case's buffers
 * with the functions it ends in: svt_inter_predictor / svt_highbd_inter_predictor (what svt_aom_enc_make_inter_predictor calls on the
 * un-scaled path, with the ConvolveParams of :4147 and :4207-4213), svt_spatial_full_distortion_kernel_c / svt_full_distortion_kernel16_bits_c
 * with the strides and the shift of :2302-2318, model_rd_from_sse (:2255, :2341-2360) and RDCOST (:2520-2525).  It also hands out the five filter
 * banks.  The reference's enc_inter_prediction.c is included from where it lies (nothing is copied).  Built by tests/test_ifs_abi.py (and by
 * tests/golden/make_golden_ifs.py) into a temporary directory with the include paths and defines of oracle/Makefile and linked against
 * oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include "enc_inter_prediction.c"

/* banks: [5][16][8]: EIGHTTAP_REGULAR, EIGHTTAP_SMOOTH, MULTITAP_SHARP as av1_get_interp_filter_params_with_block_size hands them out for a
 * side above 4, then av1_interp_4tap[0] and [1] */
void pin_ifs_filter_banks(int16_t *banks) {
    for (int f = 0; f < 3; f++) {
        InterpFilterParams p = av1_get_interp_filter_params_with_block_size((InterpFilter)f, 8);
        memcpy(banks + f * 16 * 8, p.filter_ptr, 16 * 8 * sizeof(int16_t));
    }
    for (int f = 0; f < 2; f++) memcpy(banks + (3 + f) * 16 * 8, av1_interp_4tap[f].filter_ptr, 16 * 8 * sizeof(int16_t));
}

typedef struct PinIfsCase {
    const void    *src, *ref0, *ref1; /* samples of bd 8: uint8, of bd 10: uint16; the block's first sample / what (0,0) maps to */
    int32_t        src_stride, ref0_stride, ref1_stride;
    int32_t        w, h, bd;
    int32_t        phase[4]; /* x0, y0, x1, y1 */
    int32_t        compound, fwd_offset, bck_offset;
    int32_t        ctx[2];
    const int32_t *rates;    /* [16][3] */
    uint32_t       full_lambda;
    int32_t        quantizer, dual, subsampled, skip_model, bias;
} PinIfsCase;

static void pin_predict(const PinIfsCase *c, uint32_t interp_filters, uint8_t *pred, int32_t pred_stride, ConvBufType *tmp) {
    const int      is_compound = c->compound != 0;
    ScaleFactors   sf;
    ConvolveParams cp = get_conv_params_no_round(0, 0, 0, tmp, 128, is_compound, c->bd);
    svt_av1_setup_scale_factors_for_frame(&sf, 64, 64, 64, 64);
    svt_aom_asm_set_convolve_asm_table(); /* the dispatch tables of svt_inter_predictor, from the RTCD pointers the library's ref_init() set */
    svt_aom_asm_set_convolve_hbd_asm_table();
    for (int r = 0; r < 1 + is_compound; r++) {
        SubpelParams sp;
        sp.xs = sp.ys = SCALE_SUBPEL_SHIFTS;
        sp.subpel_x   = c->phase[2 * r] << SCALE_EXTRA_BITS;
        sp.subpel_y   = c->phase[2 * r + 1] << SCALE_EXTRA_BITS;
        if (r) {
            cp.do_average            = 1;
            cp.fwd_offset            = c->fwd_offset;
            cp.bck_offset            = c->bck_offset;
            cp.use_dist_wtd_comp_avg = c->compound == 3;
            cp.use_jnt_comp_avg      = cp.use_dist_wtd_comp_avg;
        }
        const void *ref    = r ? c->ref1 : c->ref0;
        const int   stride = r ? c->ref1_stride : c->ref0_stride;
        if (c->bd > 8)
            svt_highbd_inter_predictor((const uint16_t *)ref, stride, (uint16_t *)pred, pred_stride, &sp, &sf, c->w, c->h, &cp, interp_filters, 0, c->bd);
        else
            svt_inter_predictor((const uint8_t *)ref, stride, pred, pred_stride, &sp, &sf, c->w, c->h, &cp, interp_filters, 0);
    }
}

/* sse, rd: [9], all ones where a pair is not tested; record: best index, interp_filters, switchable_rate; winner_pred: w x h samples, packed.
 * Returns the winner's rd. */
uint64_t pin_ifs_search(const PinIfsCase *c, uint64_t *sse_out, uint64_t *rd_out, int32_t *record, void *winner_pred) {
    const int    px = c->bd > 8 ? 2 : 1, pred_stride = 128;
    uint8_t     *pred = malloc((size_t)128 * 128 * px);
    ConvBufType *tmp = malloc(sizeof(ConvBufType) * 128 * 128);
    BlockSize    bsize = BLOCK_INVALID;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == c->w && block_size_high[b] == c->h)
            bsize = (BlockSize)b;
    const uint8_t shift = (c->subsampled && c->h > 16) ? 1 : 0;
    uint64_t      rd = (uint64_t)~0;
    int32_t       switchable_rate = 0;
    uint32_t      best_filters = 0;
    record[0] = -1;
    for (unsigned int i = 0; i < DUAL_FILTER_SET_SIZE; i++) {
        sse_out[i] = rd_out[i] = (uint64_t)~0;
        if (c->dual == 0 && (filter_sets[i][0] != filter_sets[i][1]))
            continue;
        const uint32_t interp_filters = av1_make_interp_filters((InterpFilter)filter_sets[i][0], (InterpFilter)filter_sets[i][1]);
        /* svt_av1_get_switchable_rate with the contexts handed in */
        int32_t tmp_rs = 0;
        for (int dir = 0; dir < (c->dual ? 2 : 1); ++dir) tmp_rs += c->rates[c->ctx[dir] * 3 + av1_extract_interp_filter(interp_filters, dir)];
        pin_predict(c, interp_filters, pred, pred_stride, tmp);
        /* model_rd_for_sb, plane 0 */
        uint64_t sse = (c->bd > 8 ? svt_full_distortion_kernel16_bits_c : svt_spatial_full_distortion_kernel_c)(
                           (uint8_t *)c->src, 0, c->src_stride << shift, pred, 0, pred_stride << shift, c->w, c->h >> shift)
            << shift;
        uint64_t rate_sum = 0, dist_sum = 0;
        if (c->skip_model) {
            dist_sum += sse * 10;
        } else {
            uint32_t rate;
            uint64_t dist;
            model_rd_from_sse(bsize, (int16_t)c->quantizer, (uint8_t)c->bd, ROUND_POWER_OF_TWO(sse, 2 * (c->bd - 8)), &rate, &dist, 0);
            rate_sum += rate;
            dist_sum += dist;
        }
        const int32_t tmp_rate = (int32_t)rate_sum;
        const int64_t tmp_dist = dist_sum;
        uint64_t      tmp_rd = RDCOST(c->full_lambda, tmp_rs + tmp_rate, tmp_dist);
        if (c->bias) {
            if (filter_sets[i][0] == 1 || filter_sets[i][1] == 1)
                tmp_rd = (tmp_rd * (uint64_t)c->bias) / 100;
        }
        sse_out[i] = sse, rd_out[i] = tmp_rd;
        if (tmp_rd < rd) {
            rd              = tmp_rd;
            switchable_rate = tmp_rs;
            best_filters    = interp_filters;
            record[0]       = (int32_t)i;
        }
    }
    record[1] = (int32_t)best_filters, record[2] = switchable_rate;
    /* the luma compensation the reference repeats with the chosen filters */
    pin_predict(c, best_filters, pred, pred_stride, tmp);
    for (int y = 0; y < c->h; y++) memcpy((uint8_t *)winner_pred + (size_t)y * c->w * px, pred + (size_t)y * pred_stride * px, (size_t)c->w * px);
    free(pred);
    free(tmp);
    return rd;
}
