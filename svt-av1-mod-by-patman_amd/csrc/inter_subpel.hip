// inter_subpel.hip — the sub-pel motion search of mode decision on gfx950: svt_av1_find_best_sub_pixel_tree and
// svt_av1_find_best_sub_pixel_tree_pruned (mcomp.c:609-775) as md_subpel_search (product_coding_loop.c:2502-2614) calls them,
// bit-exact, one descriptor per luma block of one (list, reference).
//
// One workgroup per descriptor.  Two instantiations of one kernel share a call: a single wave takes the blocks of up to 256
// samples (and every bad descriptor), four waves take the larger ones; each walks all descriptors and skips the other's.  With
// two iterations per step a round of step s moves the centre by up to 2 s per component, so a candidate lies up to
// 2 (4 + 2 + 1) = 14 eighths from start_mv: full-pel offsets -2 .. +1, and with the taps 1 .. 6 that the filter tables use the
// (w + 8) x (h + 8) reference window from 4 above and 4 left of start_mv holds every sample any candidate reads.  It is staged in
// LDS once.  A candidate is two separable passes over it (subpel_device.hpp, shared with inter_obmc.hip) with a uint8 intermediate in LDS, clipped between the passes as
// svt_aom_convolve8_horiz_c / svt_aom_convolve8_vert_c leave it; a direction without a sub-pel offset filters with the identity kernel, which is exact, so
// the four cases of svt_aom_upsampled_pred_c are one path.  The bilinear svf of the pruned search is the same path with the
// bilinear table (its uint16 intermediate never exceeds 255, so the clip changes nothing).  The variance sums cross the lanes
// by shuffles and the waves through LDS; the search itself is replayed by every lane on those uniform values.
#include "common.hpp"
#include "subpel_device.hpp"

using namespace svthip;
using namespace svthip::subpel;

namespace {

__device__ int subpel_status(const SvtHipSubpelDesc &d, const SvtHipSubpelJob &job) {
    if (!is_block_size(d.w, d.h))
        return SVT_HIP_SUBPEL_BAD_SIZE;
    if (!d.src || !d.ref)
        return SVT_HIP_SUBPEL_BAD_POINTER;
    if ((d.start_mv.row & 7) || (d.start_mv.col & 7) || abs((int)d.start_mv.row) >= MV_UPP || abs((int)d.start_mv.col) >= MV_UPP)
        return SVT_HIP_SUBPEL_BAD_START_MV;  // (inside MV_LOW .. MV_UPP no candidate leaves int16, so none leaves the window)
    if (d.method > SVT_HIP_SUBPEL_TREE_PRUNED)
        return SVT_HIP_SUBPEL_BAD_METHOD;
    if (d.subpel_search_type < SVT_HIP_SUBPEL_USE_2_TAPS || d.subpel_search_type > SVT_HIP_SUBPEL_USE_8_TAPS)
        return SVT_HIP_SUBPEL_BAD_FILTER;
    if (d.mv_cost_type > 5 || (d.mv_cost_type == 0 && (!job.mvcost[0] || !job.mvcost[1])))
        return SVT_HIP_SUBPEL_BAD_COST;
    return SVT_HIP_SUBPEL_OK;
}

// svt_mv_err_cost_ (mcomp.c:70-78): mv_cost_device.hpp, shared with inter_fpel.hip
__device__ __forceinline__ int mv_err_cost(SvtHipMv mv, const SvtHipSubpelDesc &d, const SvtHipSubpelJob &job) {
    return subpel::mv_err_cost(mv, d.ref_mv, d.mv_cost_type, d.error_per_bit, job);
}

struct Block : Window {  // what a candidate's error is computed from: the window from 4 above and 4 left of start_mv, and the source
    const uint8_t *src;  // global
    int            src_stride;
};

// vf(prediction at mv, src): the variance and the sum of squares.  against_128: vf(.., svt_aom_eb_av1_var_offs, 0, ..) instead.
template <int NT> __device__ __forceinline__ Error candidate_error(const Block &b, SvtHipMv mv, bool against_128) {
    return predicted_error<NT>(b, mv, [&](int, int r, int c, int pre) { return pre - (against_128 ? 128 : (int)b.src[r * b.src_stride + c]); });
}

struct Search {  // the running best of one search and what the checks need
    const SvtHipSubpelDesc &d;
    const SvtHipSubpelJob  &job;
    const Block            &b;
    SvtHipMv                best_mv;
    uint32_t                besterr, sse1;
    int                     distortion;

    __device__ bool in_range(SvtHipMv mv) const {
        return mv.col >= d.col_min && mv.col <= d.col_max && mv.row >= d.row_min && mv.row <= d.row_max;
    }
    // the comparison both checks end in; returns whether mv won
    __device__ bool take_if_better(SvtHipMv mv, uint32_t cost, int thismse, uint32_t sse) {
        const uint32_t weight = d.bias_fp && best_mv.col % 8 == 0 && best_mv.row % 8 == 0 ? 110 : 100;  // BIAS_FP_WEIGHT
        if ((cost * weight) / 100 >= besterr)                                                              // wraps mod 2^32
            return false;
        besterr = cost, best_mv = mv, distortion = thismse, sse1 = sse;
        return true;
    }
    // svt_check_better (mcomp.c:226-253)
    template <int NT> __device__ uint32_t check(SvtHipMv mv, bool *better = nullptr) {
        if (!in_range(mv))
            return 0x7FFFFFFFu;
        const Error    e = candidate_error<NT>(b, mv, false);
        const int      thismse = (int)e.var;
        const uint32_t cost = (uint32_t)mv_err_cost(mv, d, job) + (uint32_t)thismse;
        if (take_if_better(mv, cost, thismse, e.sse) && better)
            *better = true;
        return cost;
    }
    // svt_check_better_fast (mcomp.c:184-222)
    template <int NT> __device__ uint32_t check_fast(SvtHipMv mv) {
        if (!in_range(mv))
            return 0x7FFFFFFFu;
        uint32_t cost = (uint32_t)mv_err_cost(mv, d, job);
        if (d.mv_cost_type == 4) {  // MV_COST_OPT
            const int64_t bestcost = (int64_t)((uint32_t)distortion + cost);
            if (bestcost > ((int64_t)besterr * (int64_t)d.early_exit_th) / 1000)
                return (uint32_t)bestcost;
        }
        const Error e = candidate_error<NT>(b, mv, false);
        const int   thismse = (int)e.var;
        cost += (uint32_t)thismse;
        take_if_better(mv, cost, thismse, e.sse);
        return cost;
    }
};

// svt_av1_find_best_sub_pixel_tree behind the centre and the exits (mcomp.c:749-772)
template <int NT> __device__ void tree_rounds(Search &s, int round, int iters_per_step) {
    int hstep = 4;
    for (int iter = 0; iter < round; iter++, hstep >>= 1) {
        const SvtHipMv c = s.best_mv;
        // svt_first_level_check
        const uint32_t left = s.check<NT>(mv_of(c.row, c.col - hstep)), right = s.check<NT>(mv_of(c.row, c.col + hstep));
        const uint32_t up = s.check<NT>(mv_of(c.row - hstep, c.col)), down = s.check<NT>(mv_of(c.row + hstep, c.col));
        int            step_row = up <= down ? -hstep : hstep, step_col = left <= right ? -hstep : hstep;
        s.check<NT>(mv_of(c.row + step_row, c.col + step_col));
        if ((c.row == s.best_mv.row && c.col == s.best_mv.col) || iters_per_step <= 1)
            continue;
        // svt_second_level_check_v2
        if (c.row == s.best_mv.row)
            step_row = -step_row;
        else if (c.col == s.best_mv.col)
            step_col = -step_col;
        const SvtHipMv m = s.best_mv;
        bool           better = false;
        s.check<NT>(mv_of(m.row + step_row, m.col), &better);
        s.check<NT>(mv_of(m.row, m.col + step_col), &better);
        if (better)
            s.check<NT>(mv_of(m.row + step_row, m.col + step_col));
    }
}

// two_level_checks_fast (mcomp.c:378-607)
template <int NT> __device__ void two_level_checks_fast(Search &s, SvtHipMv t, int hstep, uint32_t orgerr, int iters) {
    const uint32_t left = s.check_fast<NT>(mv_of(t.row, t.col - hstep)), right = s.check_fast<NT>(mv_of(t.row, t.col + hstep));
    const uint32_t up = s.check_fast<NT>(mv_of(t.row - hstep, t.col)), down = s.check_fast<NT>(mv_of(t.row + hstep, t.col));
    const int      step_row = up <= down ? -hstep : hstep, step_col = left <= right ? -hstep : hstep;
    if (s.besterr >= orgerr)
        return;
    s.check_fast<NT>(mv_of(t.row + step_row, t.col + step_col));
    if (s.besterr >= orgerr || iters <= 1)
        return;
    // second_level_check_fast
    const int br = s.best_mv.row, bc = s.best_mv.col;
    if (t.row != br && t.col != bc) {
        s.check_fast<NT>(mv_of(br, bc + step_col));
        s.check_fast<NT>(mv_of(br + step_row, bc));
    } else if (t.row == br && t.col != bc) {
        s.check_fast<NT>(mv_of(br + hstep, bc + step_col));
        s.check_fast<NT>(mv_of(br - hstep, bc + step_col));
        s.check_fast<NT>(mv_of(br - step_row, bc));
    } else if (t.row != br && t.col == bc) {
        s.check_fast<NT>(mv_of(br + step_row, bc + hstep));
        s.check_fast<NT>(mv_of(br + step_row, bc - hstep));
        s.check_fast<NT>(mv_of(br, bc - step_col));
    }
}

template <int NT> __device__ int search_block(Search &s) {
    const SvtHipSubpelDesc &d = s.d;
    const Block            &b = s.b;
    const bool              pruned = d.method == SVT_HIP_SUBPEL_TREE_PRUNED;
    int                     round = min(3 - (int)d.forced_stop, 3 - !d.allow_hp);
    if (!pruned && d.mvp_th > 0) {  // mcomp.c:715-729; int arithmetic that wraps where the reference's would overflow
        const int mvp_err = (int)(d.best_mvp_dist + 1u), me_err = (int)(s.besterr + 1u);
        const int deviation = me_err ? (int)((uint32_t)(me_err - mvp_err) * 100u) / me_err : 0;
        if (deviation >= d.mvp_th)
            round = 1;
        else if (abs(s.best_mv.col - d.best_mvp.col) > d.hp_mv_th || abs(s.best_mv.row - d.best_mvp.row) > d.hp_mv_th)
            round = min(round, 2);
    }
    if (d.early_exit)
        return SVT_HIP_SUBPEL_EXIT_EARLY;
    const uint64_t th_normalizer = (uint64_t)(int64_t)(((b.w * b.h) >> (pruned ? 3 : 2)) * (int)d.abs_th_mult * (d.qp >> 1));
    if (pruned) {
        if (s.besterr < th_normalizer)
            return SVT_HIP_SUBPEL_EXIT_ABS_TH;
        if (!round)
            return SVT_HIP_SUBPEL_EXIT_NO_ROUND;
    }
    const uint32_t var = candidate_error<NT>(b, s.best_mv, true).var;
    const int      block_var = (int)((var + ((1u << b.log2_area) >> 1)) >> b.log2_area);
    if (block_var < d.pred_variance_th)
        return SVT_HIP_SUBPEL_EXIT_VARIANCE;
    if (!pruned) {
        if (s.besterr < th_normalizer)
            return SVT_HIP_SUBPEL_EXIT_ABS_TH;
        if (!round)
            return SVT_HIP_SUBPEL_EXIT_NO_ROUND;
        tree_rounds<NT>(s, round, d.iters_per_step);
        return SVT_HIP_SUBPEL_EXIT_END;
    }
    uint32_t org_error = 0;
    if (d.skip_diag_refinement < 4) {
        const uint32_t demo = d.skip_diag_refinement >= 2 && (b.w >= 64 || b.h >= 64) ? 2 : 1;
        org_error = d.skip_diag_refinement ? s.besterr / demo : 0x7FFFFFFFu;
    }
    SvtHipMv start = s.best_mv;
    int      hstep = 4;
    for (int iter = 0; iter < round; iter++) {
        const uint32_t prev = s.besterr;
        two_level_checks_fast<NT>(s, start, hstep, org_error, d.iters_per_step);
        hstep >>= 1, start = s.best_mv;
        if (d.skip_diag_refinement && iter < 1)  // QUARTER_PEL
            org_error = min(org_error, s.besterr);
        const int64_t p = max(prev, 1u);
        if ((int32_t)((((int64_t)max(s.besterr, 1u) - p) * 100) / p) >= d.round_dev_th)
            return SVT_HIP_SUBPEL_EXIT_ROUND_DEV;
    }
    return SVT_HIP_SUBPEL_EXIT_END;
}

template <int NT, int WIN_BYTES, int TMP_BYTES, bool LARGE>
__global__ __launch_bounds__(NT) void subpel_kernel(const SvtHipSubpelJob job, const SvtHipSubpelDesc *__restrict__ d_desc,
                                                    SvtHipSubpelResult *__restrict__ d_result, uint32_t n) {
    __shared__ uint8_t win[WIN_BYTES];
    __shared__ uint8_t tmp[TMP_BYTES];
    __shared__ int32_t red[2 * (NT / 64)];
    const auto         status_of = [&](const SvtHipSubpelDesc &d) { return subpel_status(d, job); };
    for_each_descriptor<LARGE>(d_desc, d_result, n, status_of, ByArea(), [&](const SvtHipSubpelDesc &d, SvtHipSubpelResult &r) {
        Block b;
        b.win = win, b.tmp = tmp, b.red = red, b.src = d.src, b.src_stride = (int)d.src_stride, b.w = d.w, b.h = d.h;
        b.lw = log2_pow2(d.w), b.win_stride = d.w + 8, b.log2_area = b.lw + log2_pow2(d.h);
        b.base_row = d.start_mv.row >> 3, b.base_col = d.start_mv.col >> 3, b.margin = 4;
        b.table = d.method == SVT_HIP_SUBPEL_TREE_PRUNED ? 0 : d.subpel_search_type - SVT_HIP_SUBPEL_USE_2_TAPS;
        __syncthreads();  // the previous block's last candidate has read win
        const uint8_t *ref = d.ref + ((int64_t)b.base_row - 4) * (int64_t)d.ref_stride + (b.base_col - 4);
        // not stage_rows: with it the single-wave kernel comes out at 64 VGPRs instead of 65, another occupancy step than it was measured at
        for (int k = threadIdx.x; k < (d.w + 8) * (d.h + 8); k += NT) {
            const int y = k / b.win_stride, x = k - y * b.win_stride;
            win[k] = ref[(int64_t)y * d.ref_stride + x];
        }
        Search s = {d, job, b, d.start_mv, 0, 0, 0};
        // svt_upsampled_setup_center_error: the variance lands in *distortion, *sse1 is not written
        s.distortion = (int)candidate_error<NT>(b, d.start_mv, false).var;
        s.besterr = (uint32_t)s.distortion + (uint32_t)mv_err_cost(d.start_mv, d, job);
        r.fullpel_err = s.besterr;
        r.exit = (uint8_t)search_block<NT>(s);
        r.best_mv = s.best_mv, r.besterr = (int32_t)s.besterr, r.distortion = s.distortion, r.sse = s.sse1;
    });
}

}  // namespace

extern "C" int32_t svt_hip_subpel_search_batch(const SvtHipSubpelJob *job, const SvtHipSubpelDesc *d_desc, SvtHipSubpelResult *d_result,
                                               uint32_t n, void *stream) {
    return launch_two_classes("svt_hip_subpel_search_batch", job && d_desc && d_result, n, stream, subpel_kernel<64, 640, 480, false>, 64, 32,
                              subpel_kernel<256, 136 * 136, 135 * 128, true>, 256, 8, job ? *job : SvtHipSubpelJob{}, d_desc, d_result, n);
}

extern "C" int32_t svt_hip_subpel_mv_limits(int32_t mi_row, int32_t mi_col, int32_t mi_width, int32_t mi_height, int32_t mi_rows,
                                            int32_t mi_cols, const SvtHipMv *ref_mv, int32_t limits[4]) {
    if (!ref_mv || !limits)
        return refuse("svt_hip_subpel_mv_limits: bad argument");
    // product_coding_loop.c:2532-2535 (MI_SIZE 4, AOM_INTERP_EXTEND 4)
    int32_t fp[4] = {-(((mi_col + mi_width) * 4) + 4), (mi_cols - mi_col) * 4 + 4, -(((mi_row + mi_height) * 4) + 4), (mi_rows - mi_row) * 4 + 4};
    set_mv_search_range(fp, *ref_mv);
    set_subpel_mv_search_range(limits, fp, *ref_mv);
    return SVT_HIP_OK;
}

SVT_HIP_MODULE_WARMUP(inter_subpel)
