// inter_obmc.hip — OBMC motion refinement on gfx950: the weighted target of calc_target_weighted_pred
// (enc_inter_prediction.c:1767-1827) and single_motion_search (mode_decision.c:2425-2533) for OBMC_CAUSAL, bit-exact, one
// descriptor per luma block (of one reference).
//
// Target: one thread per sample; every step of the reference touches a sample on its own, so the above pass, the scaling, the
// left pass and the subtraction from the source run in registers and wsrc / mask are written once.
//
// Search: one workgroup per descriptor, two instantiations by area as in inter_subpel.hip.  With R = fpel_search_range the
// full-pel stage stays within R samples of the clamped start and the tree within 14 eighths of where that ends, so the
// (w + 2 R + 8) x (h + 2 R + 8) reference window from R + 4 above and left of the clamped start holds every sample any candidate
// reads; it is staged in LDS once (at most 168 x 168 bytes).  wsrc and mask are 8 bytes per sample, up to 128 KB per block: they
// stay in global memory and every pass streams them once, coalesced; one full-pel round is ONE such pass that sums the weighted
// SAD of all 4 / 8 neighbours at once from the window (the comparisons then run on the sums in the reference's order, and a
// neighbour that is_mv_in refuses is simply not looked at).  A sub-pel candidate is the two-pass prediction of subpel_device.hpp
// with the weighted variance as its per-sample step.  Every lane replays the search on the wave-uniform sums.
#include "common.hpp"
#include "subpel_device.hpp"

using namespace svthip;
using namespace svthip::subpel;

namespace {

// svt_av1_get_obmc_mask(1 .. 32) (the AV1 specification's Obmc_Mask_*): the ramp of length L starts at L - 1
__constant__ const uint8_t OBMC_RAMPS[63] = {64, 45, 64, 39, 50, 59, 64, 36, 42, 48, 53, 57, 61, 64, 64, 34, 37, 40, 43, 46, 49,
                                             52, 54, 56, 58, 60, 61, 64, 64, 64, 64, 33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48,
                                             50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64};

// the neighbours of obmc_refining_search_sad (av1me.c:724), in its order; the first four without fpel_search_diag
__constant__ const int8_t SITE_ROW[8] = {-1, 0, 0, 1, -1, 1, 1, -1}, SITE_COL[8] = {0, -1, 1, 0, 1, 1, -1, -1};

__device__ __forceinline__ bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

// ---- the weighted target ---------------------------------------------------------------------------------------------------------
__device__ bool segments_ok(const SvtHipObmcNeighbour *nb, int n, int mi_units) {
    if (n > SVT_HIP_OBMC_MAX_NEIGHBOURS)
        return false;
    int  end = 0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < SVT_HIP_OBMC_MAX_NEIGHBOURS; k++)
        if (k < n) {
            ok = ok && nb[k].mi_len != 0 && nb[k].rel_mi >= end && nb[k].rel_mi + nb[k].mi_len <= mi_units;
            end = nb[k].rel_mi + nb[k].mi_len;
        }
    return ok;
}

__device__ int target_status(const SvtHipObmcTargetDesc &d) {
    if (!is_block_size(d.w, d.h))
        return SVT_HIP_OBMC_BAD_SIZE;
    if (!d.src || !d.wsrc || !d.mask || !aligned4(d.wsrc) || !aligned4(d.mask))
        return SVT_HIP_OBMC_BAD_POINTER;
    if ((d.up_available && d.n_above && !d.above) || (d.left_available && d.n_left && !d.left))
        return SVT_HIP_OBMC_BAD_POINTER;
    if ((d.up_available && !segments_ok(d.above_nb, d.n_above, d.w >> 2)) || (d.left_available && !segments_ok(d.left_nb, d.n_left, d.h >> 2)))
        return SVT_HIP_OBMC_BAD_SEGMENT;
    return SVT_HIP_OBMC_OK;
}

__device__ __forceinline__ bool in_segments(const SvtHipObmcNeighbour *nb, int n, int mi) {
    bool in = false;
#pragma unroll
    for (int k = 0; k < SVT_HIP_OBMC_MAX_NEIGHBOURS; k++) in = in || (k < n && mi >= nb[k].rel_mi && mi < nb[k].rel_mi + nb[k].mi_len);
    return in;
}

template <int NT, bool LARGE>
__global__ __launch_bounds__(NT) void obmc_target_kernel(const SvtHipObmcTargetDesc *__restrict__ d_desc, uint32_t *__restrict__ d_status, uint32_t n) {
    const int tid = threadIdx.x;
    // a bad descriptor whose outputs can be addressed gets them zeroed
    const auto zero_outputs = [&](const SvtHipObmcTargetDesc &d) {
        if (is_block_size(d.w, d.h) && d.wsrc && d.mask && aligned4(d.wsrc) && aligned4(d.mask))
            for (int k = tid; k < d.w * d.h; k += NT) d.wsrc[k] = 0, d.mask[k] = 0;
    };
    const auto status_of = [](const SvtHipObmcTargetDesc &d) { return target_status(d); };
    for_each_descriptor<LARGE>(d_desc, d_status, n, status_of, ByArea(), [&](const SvtHipObmcTargetDesc &d, uint32_t &) {
        const int      w = d.w, h = d.h, lw = log2_pow2(w);
        const int      n_above = d.up_available ? d.n_above : 0, n_left = d.left_available ? d.n_left : 0;
        const int      ov_above = min(h, 64) >> 1, ov_left = min(w, 64) >> 1;
        const uint8_t *ramp_above = OBMC_RAMPS + ov_above - 1, *ramp_left = OBMC_RAMPS + ov_left - 1;
        for (int k = tid; k < (h << lw); k += NT) {
            const int r = k >> lw, c = k & (w - 1);
            int       ws = 0, m = 64;
            if (r < ov_above && in_segments(d.above_nb, n_above, c >> 2)) {  // svt_av1_calc_target_weighted_pred_above_c
                const int m0 = ramp_above[r];
                ws = (64 - m0) * d.above[(int64_t)r * d.above_stride + c], m = m0;
            }
            ws *= 64, m *= 64;
            if (c < ov_left && in_segments(d.left_nb, n_left, r >> 2)) {  // svt_av1_calc_target_weighted_pred_left_c
                const int m0 = ramp_left[c];
                ws = (ws >> 6) * m0 + ((int)d.left[(int64_t)r * d.left_stride + c] << 6) * (64 - m0), m = (m >> 6) * m0;
            }
            d.wsrc[k] = (int)d.src[(int64_t)r * d.src_stride + c] * 4096 - ws, d.mask[k] = m;
        }
    }, zero_outputs);
}

// ---- the search ------------------------------------------------------------------------------------------------------------------
__device__ int search_status(const SvtHipObmcSearchDesc &d, const SvtHipSubpelJob &job) {
    if (!is_block_size(d.w, d.h))
        return SVT_HIP_OBMC_BAD_SIZE;
    if (!d.wsrc || !d.mask || !d.ref || !aligned4(d.wsrc) || !aligned4(d.mask))
        return SVT_HIP_OBMC_BAD_POINTER;
    if (d.fpel_search_range > 16)
        return SVT_HIP_OBMC_BAD_RANGE;
    if (abs((int)d.start_mv.row) >= MV_UPP || abs((int)d.start_mv.col) >= MV_UPP)
        return SVT_HIP_OBMC_BAD_START_MV;  // (inside MV_LOW .. MV_UPP no candidate leaves int16)
    for (int k = 0; k < 4; k += 2) {
        if (d.raw_limits[k] > d.raw_limits[k + 1] || d.fp_limits[k] > d.fp_limits[k + 1])
            return SVT_HIP_OBMC_BAD_LIMITS;
        if (d.fp_limits[k] < -2048 || d.fp_limits[k + 1] > 2048 || d.raw_limits[k] < -(1 << 20) || d.raw_limits[k + 1] > (1 << 20))
            return SVT_HIP_OBMC_BAD_LIMITS;  // (a clamped start times 8 stays an int16; the raw limits times 8 an int)
    }
    if (d.subpel_search_type < SVT_HIP_SUBPEL_USE_2_TAPS || d.subpel_search_type > SVT_HIP_SUBPEL_USE_8_TAPS)
        return SVT_HIP_OBMC_BAD_FILTER;
    if (!d.approx_inter_rate && (!job.mvcost[0] || !job.mvcost[1]))
        return SVT_HIP_OBMC_BAD_COST;
    return SVT_HIP_OBMC_OK;
}

// mvsad_err_cost / mvsad_err_cost_light (av1me.c:237-261) of the full-pel vector (row, col) against ref_mv >> 3
__device__ uint32_t mvsad_err_cost(int row, int col, const SvtHipObmcSearchDesc &d, const SvtHipSubpelJob &job) {
    const int dr = row - (d.ref_mv.row >> 3), dc = col - (d.ref_mv.col >> 3);
    if (d.approx_inter_rate)
        return 1296u + 50u * ((uint32_t)(abs(dc) * 8) + (uint32_t)(abs(dr) * 8));
    return ((uint32_t)mv_rate((int16_t)(dr * 8), (int16_t)(dc * 8), job) * (uint32_t)d.sad_per_bit + 256u) >> 9;  // AV1_PROB_COST_SHIFT
}

// svt_aom_mv_err_cost / svt_aom_mv_err_cost_light (av1me.c:229-252) of the vector (row, col) in 1/8 units
__device__ uint32_t mv_err_cost(int row, int col, const SvtHipObmcSearchDesc &d, const SvtHipSubpelJob &job) {
    const int dr = (int16_t)row - d.ref_mv.row, dc = (int16_t)col - d.ref_mv.col;
    if (d.approx_inter_rate)
        return 1296u + 50u * ((uint32_t)abs(dc) + (uint32_t)abs(dr));
    return (uint32_t)mv_entropy_cost(mv_rate((int16_t)dr, (int16_t)dc, job), d.error_per_bit);
}

struct Block : Window {
    const int32_t *wsrc, *mask;  // global, [h][w]
};

// svt_aom_obmc_sad* of the (up to) 8 neighbours of the full-pel vector (row, col) at once, or with n_sites == 1 of the vector itself:
// site j is (row, col) + SITES[j].  One pass over wsrc and mask.  red: 8 words per wave.
template <int NT> __device__ __forceinline__ void weighted_sads(const Block &b, int row, int col, int n_sites, bool centre, uint32_t (&sad)[8]) {
    const int     tid = threadIdx.x, w = b.w, lw = b.lw, ws = b.win_stride;
    const int     oy = row - b.base_row + b.margin, ox = col - b.base_col + b.margin;
    if (NT > 64)
        __syncthreads();  // the previous pass's sums have been read from red
#pragma unroll
    for (int j = 0; j < 8; j++) sad[j] = 0;
    for (int i = tid; i < (b.h << lw); i += NT) {
        const int      r = i >> lw, c = i & (w - 1);
        const int      t = b.wsrc[i], m = b.mask[i];
        const uint8_t *p = b.win + (r + oy) * ws + c + ox;
        if (centre) {
            sad[0] += (uint32_t)(abs(t - (int)p[0] * m) + 2048) >> 12;
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j < n_sites)
                    sad[j] += (uint32_t)(abs(t - (int)p[SITE_ROW[j] * ws + SITE_COL[j]] * m) + 2048) >> 12;
        }
    }
    block_sums<NT>(b.red, sad);
}

// upsampled_obmc_pref_error (av1me.c:901-938): svt_aom_upsampled_pred_c, then svt_aom_obmc_variance* (variance.c:347-373)
template <int NT> __device__ __forceinline__ Error weighted_variance(const Block &b, int row, int col) {
    return predicted_error<NT>(b, mv_of(row, col), [&](int i, int, int, int pre) {
        const int v = b.wsrc[i] - pre * b.mask[i];
        return v < 0 ? -((-v + 2048) >> 12) : (v + 2048) >> 12;  // ROUND_POWER_OF_TWO_SIGNED
    });
}

struct Tree {  // svt_av1_find_best_obmc_sub_pixel_tree_up's running best
    const SvtHipObmcSearchDesc &d;
    const SvtHipSubpelJob      &job;
    const Block                &b;
    int32_t                     lim[4];  // col_min, col_max, row_min, row_max
    int                         br, bc;
    uint32_t                    besterr, sse1;
    int                         distortion;

    // the body of CHECK_BETTER1 and of the loop's own checks: the cost of (r, c), INT_MAX outside the limits; *won: it is the new best
    template <int NT> __device__ uint32_t check(int r, int c, bool *won) {
        *won = false;
        if (!(c >= lim[0] && c <= lim[1] && r >= lim[2] && r <= lim[3]))
            return 0x7FFFFFFFu;
        const Error    e = weighted_variance<NT>(b, r, c);
        const uint32_t cost = e.var + mv_err_cost(r, c, d, job);
        if (cost < besterr)
            besterr = cost, distortion = (int)e.var, sse1 = e.sse, *won = true;
        return cost;
    }
};

template <int NT> __device__ void tree_search(Tree &s) {
    const SvtHipObmcSearchDesc &d = s.d;
    int                         round = 3 - (int)d.forced_stop;
    if (!d.allow_hp && round == 3)
        round = 2;
    // upsampled_setup_obmc_center_error
    const Error e = weighted_variance<NT>(s.b, s.br, s.bc);
    s.distortion = (int)e.var, s.sse1 = e.sse, s.besterr = e.var + mv_err_cost(s.br, s.bc, d, s.job);
    int hstep = 4;
    for (int iter = 0; iter < round; iter++, hstep >>= 1) {
        // search_step_table: left, right, up, down
        uint32_t cost[4];
        int      best_idx = -1;
        bool     won;
        for (int idx = 0; idx < 4; idx++) {
            const int tr = s.br + (idx == 2 ? -hstep : idx == 3 ? hstep : 0), tc = s.bc + (idx == 0 ? -hstep : idx == 1 ? hstep : 0);
            cost[idx] = s.check<NT>(tr, tc, &won);
            if (won)
                best_idx = idx;
        }
        int       kc = cost[0] <= cost[1] ? -hstep : hstep, kr = cost[2] <= cost[3] ? -hstep : hstep;
        const int tc = s.bc + kc, tr = s.br + kr;
        s.check<NT>(tr, tc, &won);
        if (won)
            best_idx = 4;
        if (best_idx == 4)
            s.br = tr, s.bc = tc;
        else if (best_idx >= 0)
            s.br += best_idx == 2 ? -hstep : best_idx == 3 ? hstep : 0, s.bc += best_idx == 0 ? -hstep : best_idx == 1 ? hstep : 0;
        if (d.iters_per_step > 1 && best_idx != -1) {  // SECOND_LEVEL_CHECKS_BEST(1)
            const int br0 = s.br, bc0 = s.bc;
            if (tr == s.br && tc != s.bc)
                kc = s.bc - tc;
            else if (tr != s.br && tc == s.bc)
                kr = s.br - tr;
            bool moved = false;
            s.check<NT>(br0 + kr, bc0, &won);
            if (won)
                s.br = br0 + kr, s.bc = bc0, moved = true;
            s.check<NT>(br0, bc0 + kc, &won);
            if (won)
                s.br = br0, s.bc = bc0 + kc, moved = true;
            if (moved) {
                s.check<NT>(br0 + kr, bc0 + kc, &won);
                if (won)
                    s.br = br0 + kr, s.bc = bc0 + kc;
            }
        }
    }
}

template <int NT, int WIN_BYTES, int TMP_BYTES, bool LARGE>
__global__ __launch_bounds__(NT) void obmc_search_kernel(const SvtHipSubpelJob job, const SvtHipObmcSearchDesc *__restrict__ d_desc,
                                                         SvtHipObmcSearchResult *__restrict__ d_result, uint32_t n) {
    __shared__ uint8_t win[WIN_BYTES];
    __shared__ uint8_t tmp[TMP_BYTES];
    __shared__ int32_t red[8 * (NT / 64)];
    const int          tid = threadIdx.x;
    // for_each_descriptor written out and, below, not stage_rows: with them the search measured 1 to 4 % slower
    // (profiles/md_search_refactor_ab.json)
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const SvtHipObmcSearchDesc d = d_desc[i];
        const int                  status = search_status(d, job);
        if (!takes(LARGE, status, [&] { return ByArea()(d); }))
            continue;
        SvtHipObmcSearchResult r = {};
        r.status = (uint8_t)status;
        if (status != SVT_HIP_OBMC_OK) {
            if (tid == 0)
                d_result[i] = r;
            continue;
        }
        // mvp_full, clamped as svt_av1_obmc_full_pixel_search clamps it
        int row = d.start_mv.row >> 3, col = d.start_mv.col >> 3;
        if (d.do_full_refine)
            col = min(max(col, d.fp_limits[0]), d.fp_limits[1]), row = min(max(row, d.fp_limits[2]), d.fp_limits[3]);
        const int range = d.do_full_refine ? d.fpel_search_range : 0;
        Block     b;
        b.win = win, b.tmp = tmp, b.red = red, b.wsrc = d.wsrc, b.mask = d.mask, b.w = d.w, b.h = d.h;
        b.lw = log2_pow2(d.w), b.log2_area = b.lw + log2_pow2(d.h);
        b.margin = range + 4, b.win_stride = d.w + 2 * b.margin, b.base_row = row, b.base_col = col;
        b.table = d.subpel_search_type - SVT_HIP_SUBPEL_USE_2_TAPS;
        __syncthreads();  // the previous block's last candidate has read win
        const uint8_t *ref = d.ref + ((int64_t)row - b.margin) * (int64_t)d.ref_stride + (col - b.margin);
        for (int k = tid; k < b.win_stride * (d.h + 2 * b.margin); k += NT) {
            const int y = k / b.win_stride, x = k - y * b.win_stride;
            win[k] = ref[(int64_t)y * d.ref_stride + x];
        }
        __syncthreads();
        if (d.do_full_refine) {  // obmc_refining_search_sad
            const int n_sites = d.fpel_search_diag ? 8 : 4;
            uint32_t  sad[8];
            weighted_sads<NT>(b, row, col, 1, true, sad);
            uint32_t best_sad = sad[0] + mvsad_err_cost(row, col, d, job);
            int      rounds = 0;
            for (int it = 0; it < range; it++) {
                weighted_sads<NT>(b, row, col, n_sites, false, sad);
                int best_site = -1;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int mr = row + SITE_ROW[j], mc = col + SITE_COL[j];
                    if (j >= n_sites || mc < d.fp_limits[0] || mc > d.fp_limits[1] || mr < d.fp_limits[2] || mr > d.fp_limits[3])  // is_mv_in
                        continue;
                    uint32_t s = sad[j];
                    if (s < best_sad) {
                        s += mvsad_err_cost(mr, mc, d, job);
                        if (s < best_sad)
                            best_sad = s, best_site = j;
                    }
                }
                if (best_site < 0)
                    break;
                row += SITE_ROW[best_site], col += SITE_COL[best_site], rounds++;
            }
            r.fullpel_rounds = (uint8_t)rounds;
        }
        r.fullpel_mv = mv_of(row, col);
        int br = row * 8, bc = col * 8;
        if (d.do_frac_refine) {
            Tree s = {d, job, b};
            set_subpel_mv_search_range(s.lim, d.raw_limits, d.ref_mv);  // on the limits from before the full-pel narrowing
            s.br = br, s.bc = bc;
            tree_search<NT>(s);
            br = s.br, bc = s.bc;
            r.besterr = (int32_t)s.besterr, r.distortion = s.distortion, r.sse = s.sse1;
        }
        r.best_mv = mv_of(br, bc);
        const int dr = (int16_t)br - d.ref_mv.row, dc = (int16_t)bc - d.ref_mv.col;
        if (d.approx_inter_rate)  // svt_av1_mv_bit_cost_light, svt_av1_mv_bit_cost with MV_COST_WEIGHT (rd_cost.c:67-87)
            r.rate_mv = (int32_t)(1296u + 50u * ((uint32_t)abs(dc) + (uint32_t)abs(dr)));
        else
            r.rate_mv = (mv_rate((int16_t)dr, (int16_t)dc, job) * 108 + 64) >> 7;
        if (tid == 0)
            d_result[i] = r;
    }
}

}  // namespace

extern "C" int32_t svt_hip_obmc_target_batch(const SvtHipObmcTargetDesc *d_desc, uint32_t *d_status, uint32_t n, void *stream) {
    return launch_two_classes("svt_hip_obmc_target_batch", d_desc && d_status, n, stream, obmc_target_kernel<64, false>, 64, 32, obmc_target_kernel<256, true>,
                              256, 8, d_desc, d_status, n);
}

extern "C" int32_t svt_hip_obmc_search_batch(const SvtHipSubpelJob *job, const SvtHipObmcSearchDesc *d_desc, SvtHipObmcSearchResult *d_result,
                                             uint32_t n, void *stream) {
    // The windows: 16 x 16, 8 x 32 and 32 x 8 at R = 16 are the largest of the single-wave sizes (72 x 48 bytes), 128 x 128 of the others (168 x 168)
    return launch_two_classes("svt_hip_obmc_search_batch", job && d_desc && d_result, n, stream, obmc_search_kernel<64, 72 * 48, 480, false>, 64, 32,
                              obmc_search_kernel<256, 168 * 168, 135 * 128, true>, 256, 8, job ? *job : SvtHipSubpelJob{}, d_desc, d_result, n);
}

extern "C" int32_t svt_hip_obmc_mv_limits(int32_t mi_row, int32_t mi_col, int32_t mi_width, int32_t mi_height, int32_t mi_rows,
                                          int32_t mi_cols, const SvtHipMv *ref_mv, int32_t raw_limits[4], int32_t fp_limits[4]) {
    if (!ref_mv || !raw_limits || !fp_limits)
        return refuse("svt_hip_obmc_mv_limits: bad argument");
    // mode_decision.c:2459-2462 (MI_SIZE 4, AOM_INTERP_EXTEND 4)
    raw_limits[0] = -(((mi_col + mi_width) * 4) + 4), raw_limits[1] = (mi_cols - mi_col) * 4 + 4;
    raw_limits[2] = -(((mi_row + mi_height) * 4) + 4), raw_limits[3] = (mi_rows - mi_row) * 4 + 4;
    for (int k = 0; k < 4; k++) fp_limits[k] = raw_limits[k];
    set_mv_search_range(fp_limits, *ref_mv);
    return SVT_HIP_OK;
}

SVT_HIP_MODULE_WARMUP(inter_obmc)
