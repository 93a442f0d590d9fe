// inter_fpel.hip — the full-pel motion search of mode decision on gfx950: md_full_pel_search (product_coding_loop.c:1918-2046) with
// md_full_pel_search_large_lbd / svt_pme_sad_loop_kernel_c (:1781-1904) behind it, chained as md_sq_motion_search (:2314-2498),
// md_nsq_motion_search (:2141-2241), the full-pel call of pme_search (:3263) and the MVP scoring of :3087-3108 chain it, bit-exact,
// one descriptor per luma block of one (list, reference).
//
// One workgroup of four waves per descriptor; a workgroup strides over the descriptors when there are more than the grid holds.  Two
// instantiations of one kernel share a call: one sized for blocks with sides up to 32 (8 KB of LDS; it also takes every bad descriptor),
// one for the larger ones (45 KB); each walks all descriptors and skips the other's.  The descriptor and the source block are staged in
// LDS once.  A stage (one md_full_pel_search call) walks its window in tiles of
// SVT_HIP_FPEL_TILE x SVT_HIP_FPEL_TILE search positions: per tile the rectangle of the reference that the tile's visited positions span
// (at most (TILE - 1 + w) x (TILE - 1 + h) samples) is staged in LDS, whatever the window's size.  A position is scored by a group of
// L = min(64, w * h) lanes, so a wave scores 64 / L positions at a time and the workgroup 256 / L; the sums cross the group's lanes by
// shuffles.  Every group's first lane keeps its best (cost << 32 | scan-order number) over all tiles of the stage; the stage ends with
// one minimum over the groups through LDS.  The order number is the position's 1-based place in the reference's scan (column-major in the
// generic loop, row-major on the psad path) and the incoming best enters with order 0: the winner is the one the reference's sequential
// `cost < *best_cost` finds.  The stages of a descriptor run back to back in the workgroup, replayed by every lane on uniform values,
// because a stage's centre is the previous stage's winner.
#include "common.hpp"
#include "subpel_device.hpp"

#include <algorithm>

using namespace svthip;
using namespace svthip::subpel;

namespace {

constexpr int NT = 256;
constexpr int TILE = SVT_HIP_FPEL_TILE;

__device__ int fpel_status(const SvtHipFpelDesc &d, const SvtHipSubpelJob &job) {
    if (!is_block_size(d.w, d.h))
        return SVT_HIP_FPEL_BAD_SIZE;
    if (!d.src || !d.ref)
        return SVT_HIP_FPEL_BAD_POINTER;
    if (d.mode > SVT_HIP_FPEL_PME)
        return SVT_HIP_FPEL_BAD_MODE;
    if (d.dist_type > SVT_HIP_FPEL_SSD)
        return SVT_HIP_FPEL_BAD_DIST;
    if (d.mode != SVT_HIP_FPEL_MVP && (d.mv_cost_type > 5 || (d.mv_cost_type == 0 && (!job.mvcost[0] || !job.mvcost[1]))))
        return SVT_HIP_FPEL_BAD_COST;
    if ((d.mode == SVT_HIP_FPEL_MVP && (d.n_mv < 1 || d.n_mv > SVT_HIP_FPEL_MAX_MVP)) ||
        (d.mode == SVT_HIP_FPEL_NSQ && (d.n_mv < 1 || d.n_mv > SVT_HIP_FPEL_MAX_MV)))
        return SVT_HIP_FPEL_BAD_COUNT;
    const int levels = d.mode == SVT_HIP_FPEL_SQ ? 3 : d.mode == SVT_HIP_FPEL_PME ? 1 : 0;
    for (int l = 0; l < levels; l++) {
        const SvtHipFpelLevel &v = d.level[l];
        if (d.mode == SVT_HIP_FPEL_SQ && !v.enabled)
            continue;
        if (d.mode == SVT_HIP_FPEL_SQ && v.step == 0)
            return SVT_HIP_FPEL_BAD_STEP;
        if ((int)v.end_x - v.start_x > SVT_HIP_FPEL_MAX_EXTENT || (int)v.end_y - v.start_y > SVT_HIP_FPEL_MAX_EXTENT)
            return SVT_HIP_FPEL_BAD_WINDOW;
    }
    return SVT_HIP_FPEL_OK;
}

template <int SIDE> struct Shared {  // LDS of one workgroup whose blocks have sides of at most SIDE
    SvtHipFpelDesc     d;
    unsigned long long key[NT];
    uint32_t           pos[NT];
    int32_t            row_rate[TILE], col_rate[TILE];  // MV_COST_ENTROPY: mvcost[0] / mvcost[1] at the tile's visited rows / columns
    uint8_t            src[SIDE * SIDE];
    uint8_t            tile[((TILE - 1 + SIDE) * (TILE - 1 + SIDE) + 15) / 16 * 16];  // a SIDE x SIDE block over a full tile
};

struct Best {  // *best_mvx, *best_mvy, *best_cost
    int16_t  mvx, mvy;
    uint32_t cost;
};

struct Stage {  // the arguments of one md_full_pel_search call that are not the descriptor's
    int  dist_type;
    int  mvx, mvy;                        // the centre, 1/8 units, not necessarily full-pel
    int  start_x, end_x, start_y, end_y;  // before the clip
    int  step;
    bool clip, cost;                      // false, false: the MVP scoring
    bool lev0_performed;
    int  lev0_start_x, lev0_end_x, lev0_start_y, lev0_end_y;  // ctx->sprs_lev0_*
};

// One md_full_pel_search call.  Every thread of the workgroup calls it with the same arguments and leaves with the same *best.
template <class Shared> __device__ __forceinline__ void full_pel_search(Shared &sh, const SvtHipSubpelJob &job, const Stage &s, Best &best) {
    const SvtHipFpelDesc &d = sh.d;
    const int tid = threadIdx.x, w = d.w, h = d.h, lw = log2_pow2(w), area = w * h, log2_area = lw + log2_pow2(h);
    const int L = min(64, area), groups = NT / L, g = tid / L, sub = tid & (L - 1);
    const int cx = s.mvx >> 3, cy = s.mvy >> 3;
    int       sx = s.start_x, ex = s.end_x, sy = s.start_y, ey = s.end_y;
    if (s.clip) {  // :1933-1947; the results land in int16_t variables
        const int bx = d.blk_org_x + cx, by = d.blk_org_y + cy;
        if (bx + sx < -(int)d.ref_org_x + 1)
            sx = (int16_t)((-(int)d.ref_org_x + 1) - bx);
        if (bx + w + ex > d.ref_org_x + d.ref_max_width - 1)
            ex = (int16_t)((d.ref_org_x + d.ref_max_width - 1) - (bx + w));
        if (by + sy < -(int)d.ref_org_y + 1)
            sy = (int16_t)((-(int)d.ref_org_y + 1) - by);
        if (by + h + ey > d.ref_org_y + d.ref_max_height - 1)
            ey = (int16_t)((d.ref_org_y + d.ref_max_height - 1) - (by + h));
    }
    const bool psad = s.dist_type == SVT_HIP_FPEL_SAD && d.enable_psad && ex - sx >= 7;
    const bool entropy = s.cost && d.mv_cost_type == 0;  // MV_COST_ENTROPY
    // offsets (xo, yo) from (sx, sy) over X x Y; generic: both multiples of step; psad: yo a multiple of step, xo the first eight
    // columns of every period of 7 + step that still has eight columns before X
    int X = ex - sx + 1;
    const int Y = ey - sy + 1, period = 7 + s.step;
    if (psad) {
        const int remain = 8 - ((ex - sx) % 8);
        X = ex - sx + (remain == 8 ? 0 : remain);  // search_area_width
    }
    unsigned long long key = (unsigned long long)best.cost << 32;  // the incoming best: order 0
    uint32_t           pos = 0;
    if (X > 0 && Y > 0) {
        for (int y0 = 0; y0 < Y; y0 += TILE) {
            // the tile's visited rows: multiples of step in [y0, y0 + TILE)
            const int fy = (y0 + s.step - 1) / s.step * s.step, y_end = min(y0 + TILE, Y);
            if (fy >= y_end)
                continue;
            const int ny = (y_end - 1 - fy) / s.step + 1, ly = fy + (ny - 1) * s.step;
            for (int x0 = 0; x0 < X; x0 += TILE) {
                const int x_end = min(x0 + TILE, X);
                int       fx, lx, nx;  // first and last visited column of the tile, and how many candidates the tile enumerates per row
                if (psad) {
                    fx = -1, lx = -1;
                    for (int xo = x0; xo < x_end; xo++) {
                        const int k = xo / period;
                        if (xo - k * period < 8 && k * period + 8 <= X)
                            fx = fx < 0 ? xo : fx, lx = xo;
                    }
                    nx = lx - fx + 1;
                } else {
                    fx = (x0 + s.step - 1) / s.step * s.step;
                    nx = fx < x_end ? (x_end - 1 - fx) / s.step + 1 : 0;
                    lx = fx + (nx - 1) * s.step;
                }
                if (fx < 0 || nx <= 0)
                    continue;
                // stage the rectangle the tile's visited positions span
                const int      tw = lx - fx + w, th = ly - fy + h;
                const uint8_t *ref = d.ref + ((int64_t)cy + sy + fy) * (int64_t)d.ref_stride + ((int64_t)cx + sx + fx);
                __syncthreads();  // the previous tile has been scored
                stage_rows<NT>(sh.tile, ref, d.ref_stride, tw, tw * th);
                if (entropy && tid < 2 * TILE) {  // the table entries the tile's positions need, one global load each instead of two per position
                    const int  t = tid & (TILE - 1);
                    const bool is_row = tid < TILE;
                    const int  pos1 = is_row ? sy + fy + t * s.step : sx + (psad ? fx + t : fx + t * s.step);
                    const int16_t v = (int16_t)((is_row ? s.mvy : s.mvx) + pos1 * 8);
                    const int16_t diff = (int16_t)(v - (is_row ? d.ref_mv.row : d.ref_mv.col));
                    if (t < (is_row ? ny : nx))
                        (is_row ? sh.row_rate : sh.col_rate)[t] = ((const __attribute__((address_space(1))) int32_t *)job.mvcost[is_row ? 0 : 1])[mv_table_index(diff)];
                }
                __syncthreads();
                for (int idx = g; idx < nx * ny; idx += groups) {
                    const int iy = idx / nx, ix = idx - iy * nx;
                    const int yo = fy + iy * s.step, xo = psad ? fx + ix : fx + ix * s.step;
                    const int px = sx + xo, py = sy + yo;  // refinement_pos_x / _y
                    if (psad) {
                        const int k = xo / period;
                        if (xo - k * period >= 8 || k * period + 8 > X)
                            continue;
                    } else if (s.step == 2 && s.lev0_performed) {  // :1973-1982
                        if (px + cx >= s.lev0_start_x && px + cx <= s.lev0_end_x && py + cy >= s.lev0_start_y && py + cy <= s.lev0_end_y &&
                            px % 4 == 0 && py % 4 == 0)
                            continue;
                    }
                    const uint8_t *t = sh.tile + (yo - fy) * tw + (xo - fx);
                    int            sum = 0;
                    uint32_t       acc = 0;
                    if (s.dist_type == SVT_HIP_FPEL_SAD) {
                        for (int i = sub; i < area; i += L) {
                            const int diff = (int)t[(i >> lw) * tw + (i & (w - 1))] - (int)sh.src[i];
                            acc += (uint32_t)abs(diff);
                        }
                    } else {
                        for (int i = sub; i < area; i += L) {
                            const int diff = (int)t[(i >> lw) * tw + (i & (w - 1))] - (int)sh.src[i];
                            sum += diff, acc += (uint32_t)(diff * diff);
                        }
                    }
                    for (int o = L >> 1; o > 0; o >>= 1) {
                        acc += (uint32_t)__shfl_xor((int)acc, o, 64);
                        sum += __shfl_xor(sum, o, 64);
                    }
                    if (sub == 0) {
                        uint32_t cost = acc;  // SAD, or svt_spatial_full_distortion_kernel cast to uint32_t
                        if (s.dist_type == SVT_HIP_FPEL_VAR)
                            cost = variance_of(sum, acc, log2_area).var;  // svt_aom_mefn_ptr[bsize].vf
                        const SvtHipMv mv = mv_of(s.mvy + py * 8, s.mvx + px * 8);  // stored into int16_t
                        if (entropy) {
                            const int16_t dr = (int16_t)(mv.row - d.ref_mv.row), dc = (int16_t)(mv.col - d.ref_mv.col);
                            cost += (uint32_t)mv_entropy_cost(mv_joint_cost(job, mv_joint(dr, dc)) + sh.row_rate[iy] + sh.col_rate[ix], d.error_per_bit);
                        } else if (s.cost) {
                            cost += (uint32_t)mv_err_cost<false>(mv, d.ref_mv, d.mv_cost_type, d.error_per_bit, job);
                        }
                        const uint32_t order = psad ? (uint32_t)(yo * X + xo + 1) : (uint32_t)(xo * Y + yo + 1);
                        const unsigned long long k = ((unsigned long long)cost << 32) | order;
                        if (k < key)
                            key = k, pos = ((uint32_t)(uint16_t)mv.row << 16) | (uint16_t)mv.col;
                    }
                }
            }
        }
    }
    // the smallest (cost, order) over the groups, in every thread
    __syncthreads();  // the previous stage's minimum has been read
    if (sub == 0)
        sh.key[g] = key, sh.pos[g] = pos;
    __syncthreads();
    unsigned long long win = (unsigned long long)best.cost << 32;
    uint32_t           win_pos = 0;
    for (int v = 0; v < groups; v++)
        if (sh.key[v] < win)
            win = sh.key[v], win_pos = sh.pos[v];
    if ((uint32_t)win) {  // a visited position beat the incoming cost
        best.cost = (uint32_t)(win >> 32);
        best.mvx = (int16_t)(win_pos & 0xffff), best.mvy = (int16_t)(win_pos >> 16);
    }
}

__device__ __forceinline__ Stage stage_of(const SvtHipFpelDesc &d, int mvx, int mvy, int sx, int ex, int sy, int ey, int step) {
    Stage s;
    s.dist_type = d.dist_type, s.mvx = mvx, s.mvy = mvy, s.start_x = sx, s.end_x = ex, s.start_y = sy, s.end_y = ey, s.step = step;
    s.clip = true, s.cost = true, s.lev0_performed = false;
    s.lev0_start_x = s.lev0_end_x = s.lev0_start_y = s.lev0_end_y = 0;
    return s;
}

// The chain of md_full_pel_search calls of one descriptor, as a loop over phases with one (inlined) call in it: a called function
// would cost a frame in scratch.  `a` is the running best of the probes (SQ: pa_me; NSQ: the search centre; MVP: the best MVP), `b`
// the best_search_* of the searches proper.
template <class Shared> __device__ __forceinline__ void search_desc(Shared &sh, const SvtHipSubpelJob &job, SvtHipFpelResult &r) {
    const SvtHipFpelDesc &d = sh.d;
    const int             mode = d.mode, n_mv = d.n_mv;
    Best                  a = {(int16_t)~0, (int16_t)~0, ~0u}, b = a;
    int                   me_x = d.mv[0].col, me_y = d.mv[0].row;  // SQ: *me_mv_x / _y
    int                   idx = 0, multiplier = 0;
    int                   l0_sx = 0, l0_ex = 0, l0_sy = 0, l0_ey = 0;  // ctx->sprs_lev0_*
    if (mode == SVT_HIP_FPEL_NSQ)
        a.mvx = d.mv[0].col, a.mvy = d.mv[0].row;  // search_center_mvx / _mvy start as the first MVC, not rounded
    const int phases = mode == SVT_HIP_FPEL_MVP ? n_mv : mode == SVT_HIP_FPEL_SQ ? 4 : mode == SVT_HIP_FPEL_NSQ ? n_mv + 3 : 1;
    for (int phase = 0; phase < phases; phase++) {
        Stage s = stage_of(d, 0, 0, 0, 0, 0, 0, 1);
        bool  into_b = true;
        if (mode == SVT_HIP_FPEL_MVP) {  // :3087-3108
            s.mvx = d.mv[phase].col, s.mvy = d.mv[phase].row;
            s.dist_type = SVT_HIP_FPEL_VAR, s.clip = false, s.cost = false, into_b = false;
        } else if (mode == SVT_HIP_FPEL_SQ) {  // md_sq_motion_search
            s.mvx = me_x, s.mvy = me_y;
            if (phase == 0) {
                into_b = false;
            } else {
                const SvtHipFpelLevel &v = d.level[phase - 1];
                if (!multiplier || !v.enabled)
                    continue;
                s.start_x = v.start_x, s.end_x = v.end_x, s.start_y = v.start_y, s.end_y = v.end_y, s.step = v.step;
                if (phase == 1) {  // int16_t, from the window before the clip
                    l0_sx = (int16_t)((me_x >> 3) + v.start_x), l0_ex = (int16_t)((me_x >> 3) + v.end_x);
                    l0_sy = (int16_t)((me_y >> 3) + v.start_y), l0_ey = (int16_t)((me_y >> 3) + v.end_y);
                }
                s.lev0_performed = phase == 2 && d.level[0].enabled && d.level[0].step == 4;
                s.lev0_start_x = l0_sx, s.lev0_end_x = l0_ex, s.lev0_start_y = l0_sy, s.lev0_end_y = l0_ey;
            }
        } else if (mode == SVT_HIP_FPEL_NSQ) {  // md_nsq_motion_search from :2141 on
            if (phase < n_mv) {
                s.mvx = (int16_t)((d.mv[phase].col + 4) & ~0x07), s.mvy = (int16_t)((d.mv[phase].row + 4) & ~0x07);
                into_b = false;
            } else {
                const int k = phase - n_mv;
                const int hw = k == 0 ? d.nsq_search_width >> 1 : k == 1 ? 2 : 1, hh = k == 0 ? d.nsq_search_height >> 1 : k == 1 ? 2 : 1;
                s.mvx = k == 0 ? a.mvx : b.mvx, s.mvy = k == 0 ? a.mvy : b.mvy;
                s.start_x = -hw, s.end_x = hw, s.start_y = -hh, s.end_y = hh, s.step = k == 0 ? 4 : k == 1 ? 2 : 1;
            }
        } else {  // pme_search :3263
            const SvtHipFpelLevel &v = d.level[0];
            s.mvx = d.mv[0].col, s.mvy = d.mv[0].row;
            s.start_x = v.start_x, s.end_x = v.end_x, s.start_y = v.start_y, s.end_y = v.end_y;
        }
        Best           cur = into_b ? b : a;
        const uint32_t before = cur.cost;
        full_pel_search(sh, job, s, cur);
        if (into_b)
            b = cur;
        else
            a = cur;
        if (mode == SVT_HIP_FPEL_MVP && cur.cost < before)
            idx = phase;
        if (mode == SVT_HIP_FPEL_SQ) {
            if (phase == 0)  // RDCOST(fast_lambda, 16, pa_me_cost) > RDCOST(fast_lambda, 16, th * bw * bh): the same rate term on both sides
                multiplier = d.gate_enabled && (int64_t)a.cost > (int64_t)(int32_t)d.gate_th ? d.search_area_multiplier : 0;
            else
                me_x = b.mvx, me_y = b.mvy;  // overwritten even if the level visited nothing
        }
    }
    if (mode == SVT_HIP_FPEL_MVP) {
        if (a.cost != ~0u)
            r.best_mv = d.mv[idx];
        r.best_cost = a.cost, r.mvp_idx = (uint8_t)idx;
    } else if (mode == SVT_HIP_FPEL_SQ) {
        r.best_mv = mv_of(me_y, me_x), r.best_cost = b.cost, r.aux_cost = a.cost, r.expanded = multiplier != 0;
    } else if (mode == SVT_HIP_FPEL_NSQ) {
        r.best_mv = b.cost < a.cost ? mv_of(b.mvy, b.mvx) : mv_of(a.mvy, a.mvx);
        r.best_cost = b.cost, r.aux_cost = a.cost;
    } else {
        r.best_mv = mv_of(b.mvy, b.mvx), r.best_cost = b.cost;
    }
}

// SIDE = SMALL_SIDE takes the blocks with sides up to it and every bad descriptor, SIDE = 128 the larger ones; each instantiation walks
// all descriptors and skips the other's.
template <int SIDE> __global__ __launch_bounds__(NT) void fpel_kernel(const SvtHipSubpelJob job, const SvtHipFpelDesc *__restrict__ d_desc,
                                                                     SvtHipFpelResult *__restrict__ d_result, uint32_t n) {
    __shared__ Shared<SIDE> sh;
    const int         tid = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        __syncthreads();  // the previous descriptor's last stage has read sh
        if (tid < (int)(sizeof(SvtHipFpelDesc) / 4))
            ((uint32_t *)&sh.d)[tid] = ((const uint32_t *)&d_desc[i])[tid];
        __syncthreads();
        SvtHipFpelResult r = {};
        r.status = (uint8_t)fpel_status(sh.d, job);
        // takes() of subpel_device.hpp spelt out, with a side above SMALL_SIDE as the large class: through any function the expression
        // compiles to a few other scalar instructions, and the kernel with them measured 0.7 to 1.4 % slower
        // (profiles/md_search_refactor_ab.json)
        const bool large = r.status == SVT_HIP_FPEL_OK && (sh.d.w > SMALL_SIDE || sh.d.h > SMALL_SIDE);
        if (large != (SIDE > SMALL_SIDE))
            continue;
        if (r.status == SVT_HIP_FPEL_OK) {
            stage_rows<NT>(sh.src, sh.d.src, sh.d.src_stride, sh.d.w, sh.d.w * sh.d.h);
            search_desc(sh, job, r);
        }
        if (tid == 0)
            d_result[i] = r;
    }
}

int16_t narrow(int32_t status) { return SVT_HIP_FPEL_STATUS(status); }

}  // namespace

extern "C" int16_t svt_hip_fpel_search_batch(const SvtHipSubpelJob *job, const SvtHipFpelDesc *d_desc, SvtHipFpelResult *d_result, uint32_t n,
                                             void *stream) {
    return narrow(launch_two_classes("svt_hip_fpel_search_batch", job && d_desc && d_result, n, stream, fpel_kernel<SMALL_SIDE>, NT, 8, fpel_kernel<128>, NT, 3,
                                     job ? *job : SvtHipSubpelJob{}, d_desc, d_result, n));
}

extern "C" void svt_hip_fpel_sq_windows(const SvtHipFpelSqCtrls *ctrls, uint8_t search_area_multiplier, uint16_t dist, SvtHipFpelLevel level[3]) {
    if (!ctrls || !level)
        return;
    for (int l = 0; l < 3; l++) {
        SvtHipFpelLevel &v = level[l];
        v = SvtHipFpelLevel{};
        v.enabled = ctrls->enabled[l], v.step = ctrls->step[l];
        const int step = v.step;
        if (!step)
            continue;
        // :2379-2386 / :2423-2430: int arithmetic stored into uint16_t; level 2 takes sprs_lev2_w / _h as they are
        const uint16_t sw = l == 2 ? ctrls->w[l]
                                   : (uint16_t)((ctrls->multiplier[l] * std::min(ctrls->w[l] * search_area_multiplier * dist, (int)ctrls->max_w[l])) / 100);
        const uint16_t sh = l == 2 ? ctrls->h[l]
                                   : (uint16_t)((ctrls->multiplier[l] * std::min(ctrls->h[l] * search_area_multiplier * dist, (int)ctrls->max_h[l])) / 100);
        v.start_x = (int16_t)-(((sw >> 1) / step) * step), v.end_x = (int16_t)(((sw >> 1) / step) * step);
        v.start_y = (int16_t)-(((sh >> 1) / step) * step), v.end_y = (int16_t)(((sh >> 1) / step) * step);
        if (l == 1) {  // :2439-2446
            v.start_x = (int16_t)(v.start_x % 4 == 0 ? v.start_x - 2 : v.start_x), v.end_x = (int16_t)(v.end_x % 4 == 0 ? v.end_x + 2 : v.end_x);
            v.start_y = (int16_t)(v.start_y % 4 == 0 ? v.start_y - 2 : v.start_y), v.end_y = (int16_t)(v.end_y % 4 == 0 ? v.end_y + 2 : v.end_y);
        }
    }
}

SVT_HIP_MODULE_WARMUP(inter_fpel)
