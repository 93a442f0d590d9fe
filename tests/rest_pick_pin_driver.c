/* TEST INFRASTRUCTURE — pins the Python restatement of tests/rest_pick_cases.py against the reference's own static functions of
 * restoration_pick.c, which this file includes for them: encode_xq (:508), finer_search_pixel_proj_error (:320-411),
 * count_sgrproj_bits (:655), and the finish visitors search_norestore_finish, search_wiener_finish (:1380), search_sgrproj_finish
 * (:1267) and search_switchable (:1148), called in raster order, pass after pass, as search_rest_type_finish (:1456) does through
 * svt_aom_foreach_rest_unit_in_frame.  Built by tests/test_rest_pick_abi.py into a temporary directory with the include paths and
 * defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include "restoration_pick.c"

void pin_encode_xq(int32_t *xq, int32_t *xqd, int32_t ep) { encode_xq(xq, xqd, &svt_aom_eb_sgr_params[ep]); }

int32_t pin_count_sgrproj_bits(int32_t ep, const int32_t *xqd, const int32_t *ref) {
    SgrprojInfo a, r;
    a.ep = ep, a.xqd[0] = xqd[0], a.xqd[1] = xqd[1];
    r.ep = 0, r.xqd[0] = ref[0], r.xqd[1] = ref[1];
    return count_sgrproj_bits(&a, &r);
}

int64_t pin_finer_search(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8, int32_t dat_stride,
                         int32_t highbd, int32_t *flt0, int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride, int32_t *xqd, int32_t do_refine,
                         int32_t ep) {
    return finer_search_pixel_proj_error(src8, width, height, src_stride, dat8, dat_stride, highbd, flt0, flt0_stride, flt1, flt1_stride, 2, xqd,
                                         (int8_t)do_refine, &svt_aom_eb_sgr_params[ep]);
}

/* sse[n][3]; taps[n][2][8] = vfilter, hfilter; costs = wiener_restore_cost[2], sgrproj_restore_cost[2], switchable_restore_cost[3];
 * win 7 runs the visitors as a luma plane, win 5 as a chroma plane (so that search_wiener_finish and search_switchable count the
 * same window); tested: bit r = run the pass of type r.  Out: best_rtype[n][3] and per type rsc.sse, rsc.bits, the RDCOST_DBL. */
void pin_finish(int32_t n, const int64_t *sse, const int16_t *taps, const int32_t *ep, const int32_t *xqd, int32_t rdmult, const int32_t *costs,
                int32_t win, int32_t tested, int32_t *best_rtype, int64_t *out_sse, int64_t *out_bits, double *out_cost) {
    static Macroblock   x;
    static Av1Common    cm;
    RestSearchCtxt      rsc;
    RestUnitSearchInfo *pic = (RestUnitSearchInfo *)calloc(n, sizeof(*pic)), *rusi = (RestUnitSearchInfo *)calloc(n, sizeof(*rusi));
    static const RestUnitVisitor funs[RESTORE_TYPES] = {search_norestore_finish, search_wiener_finish, search_sgrproj_finish, search_switchable};
    memset(&x, 0, sizeof(x)), memset(&cm, 0, sizeof(cm)), memset(&rsc, 0, sizeof(rsc));
    x.rdmult = rdmult;
    for (int i = 0; i < 2; i++) x.wiener_restore_cost[i] = costs[i], x.sgrproj_restore_cost[i] = costs[2 + i];
    for (int i = 0; i < 3; i++) x.switchable_restore_cost[i] = costs[4 + i];
    cm.wn_filter_ctrls.filter_tap_lvl = 1;
    rsc.cm = &cm, rsc.x = &x, rsc.plane = win == 7 ? AOM_PLANE_Y : AOM_PLANE_U, rsc.rusi = rusi, rsc.rusi_pic = pic;
    for (int k = 0; k < n; k++) {
        for (int r = 0; r < 3; r++) pic[k].sse[r] = sse[3 * k + r];
        memcpy(pic[k].wiener.vfilter, taps + 16 * k, 16), memcpy(pic[k].wiener.hfilter, taps + 16 * k + 8, 16);
        pic[k].sgrproj.ep = ep[k], pic[k].sgrproj.xqd[0] = xqd[2 * k], pic[k].sgrproj.xqd[1] = xqd[2 * k + 1];
    }
    for (int r = 0; r < RESTORE_TYPES; r++) {
        out_sse[r] = out_bits[r] = 0, out_cost[r] = 0;
        if (!((tested >> r) & 1))
            continue;
        reset_rsc(&rsc);
        rsc_on_tile(0, 0, &rsc);
        for (int k = 0; k < n; k++) funs[r](NULL, NULL, k, &rsc);
        out_sse[r] = rsc.sse, out_bits[r] = rsc.bits, out_cost[r] = RDCOST_DBL(x.rdmult, rsc.bits >> 4, rsc.sse);
    }
    for (int k = 0; k < n; k++)
        for (int r = 0; r < 3; r++) best_rtype[3 * k + r] = rusi[k].best_rtype[r];
    free(pic), free(rusi);
}

/* SGRPROJ_PRJ_MIN0 / MAX0 / MIN1 / MAX1, SGRPROJ_PRJ_BITS, SGRPROJ_PARAMS_BITS, SGRPROJ_PRJ_SUBEXP_K, the default xqd,
 * RESTORATION_PROC_UNIT_SIZE, RESTORATION_UNIT_OFFSET, RESTORATION_UNITSIZE_MAX * 3 / 2 */
void pin_rest_constants(int64_t *out) {
    SgrprojInfo d;
    set_default_sgrproj(&d);
    const int64_t v[] = {SGRPROJ_PRJ_MIN0, SGRPROJ_PRJ_MAX0, SGRPROJ_PRJ_MIN1, SGRPROJ_PRJ_MAX1, SGRPROJ_PRJ_BITS, SGRPROJ_PARAMS_BITS, SGRPROJ_PRJ_SUBEXP_K,
                         d.xqd[0], d.xqd[1], RESTORATION_PROC_UNIT_SIZE, RESTORATION_UNIT_OFFSET, RESTORATION_UNITSIZE_MAX * 3 / 2};
    memcpy(out, v, sizeof(v));
}
