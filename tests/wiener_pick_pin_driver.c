/* TEST INFRASTRUCTURE — pins the Python restatement of tests/wiener_pick_cases.py against the reference's own static functions of
 * restoration_pick.c, which this file includes for them: wiener_decompose_sep_sym (:906-936) with update_a_sep_sym, update_b_sep_sym
 * and linsolve_wiener, finalize_sym_filter (:977-1006), compute_score (:937-975), count_wiener_bits (:1008-1037), and the
 * RDCOST_DBL macro (restoration.h:346).  Built by tests/test_wiener_pick_abi.py into a temporary directory with the include paths
 * and defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include "restoration_pick.c"

/* out: vfilter[8], hfilter[8] after finalize_sym_filter; taps: the solver's vfilterd[7], hfilterd[7]; returns compute_score */
int64_t pin_wiener_solve(int32_t wiener_win, int64_t *M, int64_t *H, int16_t *out, int32_t *taps) {
    int32_t    vfilterd[WIENER_WIN], hfilterd[WIENER_WIN];
    WienerInfo info;
    memset(&info, 0, sizeof(info));
    memset(vfilterd, 0, sizeof(vfilterd)), memset(hfilterd, 0, sizeof(hfilterd));
    wiener_decompose_sep_sym(wiener_win, M, H, vfilterd, hfilterd);
    finalize_sym_filter(wiener_win, vfilterd, info.vfilter);
    finalize_sym_filter(wiener_win, hfilterd, info.hfilter);
    memcpy(out, info.vfilter, 16), memcpy(out + 8, info.hfilter, 16);
    memcpy(taps, vfilterd, sizeof(vfilterd)), memcpy(taps + WIENER_WIN, hfilterd, sizeof(hfilterd));
    return compute_score(wiener_win, M, H, info.vfilter, info.hfilter);
}

int32_t pin_count_wiener_bits(int32_t wiener_win, const int16_t *v, const int16_t *h, const int16_t *ref_v, const int16_t *ref_h) {
    WienerInfo a, r;
    memcpy(a.vfilter, v, 16), memcpy(a.hfilter, h, 16), memcpy(r.vfilter, ref_v, 16), memcpy(r.hfilter, ref_h, 16);
    return count_wiener_bits(wiener_win, &a, &r);
}

double pin_rdcost_dbl(int32_t rdmult, int64_t rate, int64_t dist) { return RDCOST_DBL(rdmult, rate, dist); }

/* WIENER_FILT_TAPn_MINV / _MAXV / _MIDV, NUM_WIENER_ITERS, WIENER_TAP_SCALE_FACTOR, RESTORATION_UNIT_OFFSET */
void pin_constants(int64_t *out) {
    const int64_t v[] = {WIENER_FILT_TAP0_MINV, WIENER_FILT_TAP1_MINV, WIENER_FILT_TAP2_MINV, WIENER_FILT_TAP0_MAXV, WIENER_FILT_TAP1_MAXV,
                         WIENER_FILT_TAP2_MAXV, WIENER_FILT_TAP0_MIDV, WIENER_FILT_TAP1_MIDV, WIENER_FILT_TAP2_MIDV, WIENER_FILT_TAP3_MIDV,
                         NUM_WIENER_ITERS, WIENER_TAP_SCALE_FACTOR, WIENER_FILT_STEP, RESTORATION_UNIT_OFFSET, AV1_PROB_COST_SHIFT};
    memcpy(out, v, sizeof(v));
}
