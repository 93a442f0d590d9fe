// loopfilter_dlf_pick.hip — svt_av1_pick_filter_level (deblocking_filter.c:1129) for the searched methods on the device:
// search_filter_level (:886-991) for up to three planes with no host step, and the frame call that reads the levels it picked.
// DESIGN.md section 4 ("Deblocking level search") has the chain, the tile shape and the measured time.
//
//   dlf_pick_plan    one wave, a lane per plane.  Round 0 starts the loops: the record is cleared and the trial at filt_mid is asked
//                    for.  Every later step takes the sums of the trials before it into ss_err and runs the reference's loop, in its
//                    integer types, through every iteration whose filt_low / filt_high are already measured; at the first iteration
//                    that needs an error it asks for the one or two trials (both are known before either is tried, :943-970) and
//                    stops.  The step after the last round asks for nothing: a plane that still needs a trial stays unfinished.
//   dlf_trial        grid (the tiles of each of the 6 trial slots, one slot after the other): one workgroup owns one TILE_W x TILE_H tile of one trial.  It
//                    loads the unfiltered tile plus halo into LDS, filters all vertical edges, then all horizontal edges there
//                    (loopfilter_dlf.hip has the ordering argument), sums the squared error against the source over the part of the
//                    tile inside the measured area and adds it to the slot's 64-bit sum with one atomicAdd.  The sums are integers,
//                    so the order of the additions does not matter.  The filtered samples never go to memory.  The workgroups of an
//                    inactive slot (level -1) return at once.
//   dlf_pass_picked  dlf_pass_kernel of loopfilter_dlf.hip with the level table built in LDS from the record's levels.
//
// The halo.  A final sample (x, y) is changed by at most one horizontal edge, the one at row ye with ye - M <= y <= ye + M - 1, where M
// is the most samples a filter changes on a side: 6 for luma (the 14-tap filter), 2 for chroma (its longest filter is 6).  That edge
// reads rows ye - R .. ye + R - 1 of the vertically filtered column x, R = 7 for luma and 3 for chroma.  So the output rows
// [y0, y0 + TILE_H) need the edges ye in [y0 - M + 1, y0 + TILE_H - 1 + M], which on the 4-sample grid of the edges is
// [y0 - BACK, y0 + TILE_H + BACK] with BACK = 4 (luma) / 0 (chroma), and those read rows [y0 - BACK - R, y0 + TILE_H + BACK + R - 1]: 11
// rows above and below for luma, 3 for chroma.  The horizontal pass works column by column, so vertically filtered samples are
// needed in the output COLUMNS only; each depends in the same way on one vertical edge xe in [x0 - BACK, x0 + TILE_W + BACK] that
// reads columns within 11 (3) of the tile.  Rounded up to whole 4x4 units: HALO = 12 samples on every side for luma, 4 for chroma.
// Only the edges of those two ranges are filtered, so no tap leaves the LDS tile and no edge that would need samples from outside
// it contributes to an output sample.
#include "common.hpp"
#include "dlf_device.hpp"

using namespace svthip;
using namespace svthip::dlf;

namespace {

constexpr int TILE_W = 64, TILE_H = 64;    // output samples of one workgroup
constexpr int HALO_Y = 12, HALO_UV = 4;    // samples loaded around the tile
constexpr int BACK_Y = 4, BACK_UV = 0;     // how far outside the tile an edge still changes or feeds an output sample
constexpr int LDS_W = TILE_W + 2 * HALO_Y; // pitch of the LDS tile (chroma uses the same pitch)
constexpr int LDS_H = TILE_H + 2 * HALO_Y;
constexpr int PAD_READ = 8;                // samples past the mi-aligned plane that SvtHipLfFrame promises to be readable
constexpr int SLOTS = 6;                   // trials of one round: low and high of three planes
constexpr int MAX_LEVEL = SVT_HIP_DLF_MAX_LEVEL;

enum Phase : int32_t { IDLE = 0, FIRST = 1, ITER = 2, DONE = 3 };  // not searched / waits for the trial at filt_mid / for an iteration's / ended
struct PlaneState {  // the locals of search_filter_level
    int64_t best_err;
    int32_t filt_mid, filter_step, filt_direction, filt_best, tot_convergence, phase;
};
struct Work {  // the workspace
    PlaneState         st[3];
    int32_t            slot_level[SLOTS];  // [2 * plane]: the low trial (or the first), [2 * plane + 1]: the high one; -1 = inactive
    unsigned long long sum[SLOTS];
};
constexpr size_t WS_BYTES = (sizeof(Work) + 255) / 256 * 256;

struct SegDeltas {  // the SEG_LVL_ALT_LF_* features
    uint8_t on, en[8][4];
    int16_t data[8][4];
};
struct PlanArgs {
    uint32_t plane_mask;
    uint8_t  start[3], only_4x4, host_level[4];  // host_level: frame.filter_level[0], [1], _u, _v
    int32_t  early_exit_convergence;
};
struct TrialArgs {
    LfGeom      g[3];
    const void *src[3];
    uint32_t    src_stride[3], sse_w[3], sse_h[3];
    uint32_t    tiles[3];  // 64x64 tiles of each plane
    SegDeltas   sd;
};
struct PickedArgs {
    LfGeom    g[3];
    SegDeltas sd;
    uint32_t  plane_mask;
    uint8_t   host_level[4], plane_start, plane_end;
};

// svt_av1_loop_filter_frame_init (deblocking_common.c:107-120) without mode_ref_delta: one plane's table from its two levels.
__device__ __forceinline__ void build_levels(LfLevels &L, const SegDeltas &sd, int plane, int lvl_v, int lvl_h, int tid) {
    if (tid < 16) {
        const int seg = tid >> 1, dir = tid & 1, feat = plane ? plane + 1 : dir;  // seg_lvl_lf_lut
        int       v = dir ? lvl_h : lvl_v;
        if (sd.on && sd.en[seg][feat])
            v = clampi(v + sd.data[seg][feat], 0, MAX_LEVEL);
        for (int i = 0; i < 16; i++) (&L.lvl[seg][dir][0][0])[i] = (uint8_t)v;
    }
}

__global__ __launch_bounds__(64) void dlf_pick_plan(PlanArgs a, int round, int last, Work *w, SvtHipDlfPickResult *res) {
    const int p = threadIdx.x;
    if (p < 3) {
        PlaneState &s  = w->st[p];
        int64_t    *ss = res->ss_err[p];
        int32_t    *lo_slot = &w->slot_level[2 * p], *hi_slot = lo_slot + 1;
        if (round == 0) {
            const bool searched = (a.plane_mask >> p) & 1;
            const int  mid = a.start[p];
            for (int i = 0; i <= MAX_LEVEL; i++) ss[i] = -1;
            s.best_err = 0, s.filt_mid = s.filt_best = searched ? mid : 0, s.filter_step = mid < 16 ? 4 : mid / 4;
            s.filt_direction = 0, s.tot_convergence = 0, s.phase = searched ? FIRST : IDLE;
            *lo_slot = searched ? mid : -1, *hi_slot = -1;
            w->sum[2 * p] = w->sum[2 * p + 1] = 0;
            res->rounds[p] = res->trials[p] = searched;
        } else if (s.phase == FIRST || s.phase == ITER) {
            if (*lo_slot >= 0)
                ss[*lo_slot] = (int64_t)w->sum[2 * p];
            if (*hi_slot >= 0)
                ss[*hi_slot] = (int64_t)w->sum[2 * p + 1];
            *lo_slot = *hi_slot = -1;
            if (s.phase == FIRST)
                s.best_err = ss[s.filt_mid];
            s.phase = ITER;
            while (s.filter_step > 0) {
                const int  mid = s.filt_mid, step = s.filter_step;
                const int  filt_high = mid + step < MAX_LEVEL ? mid + step : MAX_LEVEL, filt_low = mid - step > 0 ? mid - step : 0;
                const bool look_low = s.filt_direction <= 0 && filt_low != mid, look_high = s.filt_direction >= 0 && filt_high != mid;
                const bool need_low = look_low && ss[filt_low] < 0, need_high = look_high && ss[filt_high] < 0;
                if (need_low || need_high) {
                    if (!last) {
                        *lo_slot = need_low ? filt_low : -1, *hi_slot = need_high ? filt_high : -1;
                        w->sum[2 * p] = w->sum[2 * p + 1] = 0;
                        res->rounds[p] += 1, res->trials[p] += (int)need_low + (int)need_high;
                    }
                    break;
                }
                int64_t bias = (s.best_err >> (15 - (mid / 8))) * step;  // against raising the level (:937)
                if (!a.only_4x4)
                    bias >>= 1;
                if (look_low && ss[filt_low] < s.best_err + bias) {
                    if (ss[filt_low] < s.best_err)
                        s.best_err = ss[filt_low];
                    s.filt_best = filt_low;
                }
                if (look_high && ss[filt_high] < s.best_err - bias)
                    s.best_err = ss[filt_high], s.filt_best = filt_high;
                if (s.filt_best == mid) {  // halve the step when the best level stays
                    s.tot_convergence++;
                    s.filter_step    = s.tot_convergence == a.early_exit_convergence ? 0 : step / 2;
                    s.filt_direction = 0;
                } else {
                    s.filt_direction = s.filt_best < mid ? -1 : 1;
                    s.filt_mid       = s.filt_best;
                }
            }
            if (s.filter_step == 0)
                s.phase = DONE, s.best_err = ss[s.filt_best];  // :986
        }
        res->level[p] = s.filt_best, res->best_err[p] = s.best_err;
    }
    __syncthreads();
    if (p == 0) {
        uint32_t fin = 0;
        for (int q = 0; q < 3; q++) fin |= (uint32_t)(w->st[q].phase == DONE) << q;
        res->finished = fin, res->pad_ = 0;
        for (int k = 0; k < 4; k++) {  // filter_level[0], [1], _u, _v of the frame header
            const int q       = k < 2 ? 0 : k - 1;
            res->hdr_level[k] = ((a.plane_mask >> q) & 1) ? (uint8_t)w->st[q].filt_best : a.host_level[k];
        }
    }
}

// Loads, filters and measures one tile; HALO / BACK of the plane kind.  Returns this thread's part of the squared error.
template <typename T, int HALO, int BACK>
__device__ __forceinline__ unsigned long long trial_tile(const LfGeom &g, const LfLevels &L, uint16_t *tile, const T *src, uint32_t src_stride,
                                                         int x0, int y0, int ow, int oh, int bd) {
    constexpr int RW = TILE_W + 2 * HALO, RH = TILE_H + 2 * HALO;  // loaded region; its sample (0, 0) is picture (x0 - HALO, y0 - HALO)
    const int     tid = threadIdx.x;
    const T      *plane = (const T *)g.plane;
    const int     lim_x = (int)g.units_x * 4 + PAD_READ, lim_y = (int)g.units_y * 4 + PAD_READ;
    // one sample per lane and load (not tuned: no wide loads); RW is a constant, so the division is a multiplication
    for (int i = tid; i < RW * RH; i += 256) {
        const int r = i / RW, c = i - r * RW, x = x0 - HALO + c, y = y0 - HALO + r;
        tile[r * LDS_W + c] = (x >= 0 && y >= 0 && x < lim_x && y < lim_y) ? (uint16_t)plane[(size_t)y * g.stride + x] : (uint16_t)0;
    }
    __syncthreads();
    {   // vertical edges xe = x0 - BACK + 4 i of every unit row of the region
        constexpr int NE = (TILE_W + 2 * BACK) / 4 + 1, NU = RH / 4;
        for (int u = tid; u < NE * NU; u += 256) {
            const int j = u / NE, i = u - j * NE, x = x0 - BACK + 4 * i, y = y0 - HALO + 4 * j;
            if (x >= 0 && y >= 0)
                filter_unit<0>(g, L, (uint32_t)x >> 2, (uint32_t)y >> 2, [&](uint32_t ex, uint32_t ey, int len, int mblim, int lim, int hev) {
                    filter_segment(tile + (((int)ey - y0 + HALO) * LDS_W + ((int)ex - x0 + HALO)), 1, LDS_W, len, mblim, lim, hev, bd);
                });
        }
    }
    __syncthreads();
    {   // horizontal edges ye = y0 - BACK + 4 j of the output columns
        constexpr int NE = (TILE_H + 2 * BACK) / 4 + 1, NU = TILE_W / 4;
        for (int u = tid; u < NE * NU; u += 256) {
            const int j = u / NU, i = u - j * NU, x = x0 + 4 * i, y = y0 - BACK + 4 * j;
            if (y >= 0)
                filter_unit<1>(g, L, (uint32_t)x >> 2, (uint32_t)y >> 2, [&](uint32_t ex, uint32_t ey, int len, int mblim, int lim, int hev) {
                    filter_segment(tile + (((int)ey - y0 + HALO) * LDS_W + ((int)ex - x0 + HALO)), LDS_W, 1, len, mblim, lim, hev, bd);
                });
        }
    }
    __syncthreads();
    unsigned long long sum = 0;
    const int          c = tid & 63;
    if (c < ow)
        for (int r = tid >> 6; r < oh; r += 4) {
            const int d = (int)tile[(r + HALO) * LDS_W + HALO + c] - (int)src[(size_t)(y0 + r) * src_stride + x0 + c];
            sum += (unsigned long long)((long long)d * d);
        }
    return sum;
}

// A trial at level 0: the unfiltered plane's error, straight from memory.
template <typename T>
__device__ __forceinline__ unsigned long long plain_tile(const LfGeom &g, const T *src, uint32_t src_stride, int x0, int y0, int ow, int oh) {
    unsigned long long sum = 0;
    const T           *plane = (const T *)g.plane;
    const int          tid = threadIdx.x, c = tid & 63;
    if (c < ow)
        for (int r = tid >> 6; r < oh; r += 4) {
            const int d = (int)plane[(size_t)(y0 + r) * g.stride + x0 + c] - (int)src[(size_t)(y0 + r) * src_stride + x0 + c];
            sum += (unsigned long long)((long long)d * d);
        }
    return sum;
}

__global__ __launch_bounds__(256) void dlf_trial(TrialArgs a, Work *w) {
    __shared__ uint16_t           s_tile[LDS_H * LDS_W];
    __shared__ LfLevels           s_L;
    __shared__ unsigned long long s_sum[4];
    // the grid is every slot's tiles one after the other: 2 x luma, 2 x U, 2 x V
    const int t0 = (int)a.tiles[0], t1 = (int)a.tiles[1], t2 = (int)a.tiles[2];
    int       tile = (int)blockIdx.x, slot;
    if (tile < 2 * t0)
        slot = tile >= t0, tile -= slot * t0;
    else if ((tile -= 2 * t0) < 2 * t1)
        slot = 2 + (tile >= t1), tile -= (slot - 2) * t1;
    else
        tile -= 2 * t1, slot = 4 + (tile >= t2), tile -= (slot - 4) * t2;
    const int level = w->slot_level[slot];
    if (level < 0)
        return;
    const int     p = slot >> 1;
    const LfGeom &g = a.g[p];
    const int     tiles_x = ((int)g.units_x * 4 + TILE_W - 1) / TILE_W;
    const int     ty = tile / tiles_x, tx = tile - ty * tiles_x, x0 = tx * TILE_W, y0 = ty * TILE_H;
    const int     mw = (int)a.sse_w[p], mh = (int)a.sse_h[p];  // at most the mi-aligned plane (checked on the host)
    if (x0 >= mw || y0 >= mh)
        return;  // nothing of the tile is measured
    const int ow = mw - x0 < TILE_W ? mw - x0 : TILE_W, oh = mh - y0 < TILE_H ? mh - y0 : TILE_H;
    unsigned long long sum;
    if (level == 0) {
        sum = g.is_16bit ? plain_tile(g, (const uint16_t *)a.src[p], a.src_stride[p], x0, y0, ow, oh)
                         : plain_tile(g, (const uint8_t *)a.src[p], a.src_stride[p], x0, y0, ow, oh);
    } else {
        build_levels(s_L, a.sd, p, level, level, threadIdx.x);  // trial_tile's first barrier orders it before the first edge
        if (g.is_16bit)
            sum = p ? trial_tile<uint16_t, HALO_UV, BACK_UV>(g, s_L, s_tile, (const uint16_t *)a.src[p], a.src_stride[p], x0, y0, ow, oh, g.bit_depth)
                    : trial_tile<uint16_t, HALO_Y, BACK_Y>(g, s_L, s_tile, (const uint16_t *)a.src[p], a.src_stride[p], x0, y0, ow, oh, g.bit_depth);
        else
            sum = p ? trial_tile<uint8_t, HALO_UV, BACK_UV>(g, s_L, s_tile, (const uint8_t *)a.src[p], a.src_stride[p], x0, y0, ow, oh, 8)
                    : trial_tile<uint8_t, HALO_Y, BACK_Y>(g, s_L, s_tile, (const uint8_t *)a.src[p], a.src_stride[p], x0, y0, ow, oh, 8);
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63) == 0)
        s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(&w->sum[slot], s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
}

template <int DIR>
__global__ __launch_bounds__(256) void dlf_pass_picked(PickedArgs a, const SvtHipDlfPickResult *res) {
    __shared__ LfLevels s_L;
    const int p = blockIdx.z;
    if (p < a.plane_start || p >= a.plane_end)
        return;
    const bool luma_searched = a.plane_mask & 1;
    const int  y_v = luma_searched ? res->level[0] : a.host_level[0], y_h = luma_searched ? res->level[0] : a.host_level[1];
    if (a.plane_start == 0 && !y_v && !y_h)
        return;  // deblocking_filter.c:570-572: nothing at all
    const int uv = p ? (((a.plane_mask >> p) & 1) ? res->level[p] : a.host_level[p + 1]) : 0;
    if (p && !uv)
        return;
    build_levels(s_L, a.sd, p, p ? uv : y_v, p ? uv : y_h, threadIdx.x);
    __syncthreads();
    const LfGeom  &g = a.g[p];
    const uint32_t ux = blockIdx.x * 64 + (threadIdx.x & 63), uy = blockIdx.y * 4 + (threadIdx.x >> 6);  // as dlf_pass_kernel
    filter_unit_in_plane<DIR>(g, s_L, ux, uy);
}

// What both entry points refuse; NULL when the call is good.
const char *bad_params(const SvtHipDlfPickParams *prm, const void *d_result, bool search) {
    if (!prm || !d_result)
        return "NULL argument";
    if ((uintptr_t)d_result & 7)
        return "d_result is not 8-byte aligned";
    const SvtHipLfFrame *f = &prm->frame;
    if (!frame_ok(f))
        return "bad frame";
    if (prm->plane_mask == 0 || prm->plane_mask > 7)
        return "plane_mask is empty or names a plane above 2";
    if (f->filter_level[0] > MAX_LEVEL || f->filter_level[1] > MAX_LEVEL || f->filter_level_u > MAX_LEVEL || f->filter_level_v > MAX_LEVEL)
        return "a filter level above 63";
    for (int p = 0; p < 3; p++) {
        const bool searched = (prm->plane_mask >> p) & 1;
        if (((search && searched) || (p >= f->plane_start && p < f->plane_end)) && (!f->plane[p] || !f->stride[p]))
            return "missing plane";
        if (!search || !searched)
            continue;
        if (!prm->src[p] || !prm->src_stride[p])
            return "missing source plane";
        if (prm->start_level[p] > MAX_LEVEL)
            return "a start level above 63";
        if (!prm->sse_width[p] || !prm->sse_height[p])
            return "an empty measured area";
        if (prm->sse_width[p] > ((f->mi_cols * 4) >> (p > 0)) || prm->sse_height[p] > ((f->mi_rows * 4) >> (p > 0)))
            return "a measured area larger than the mi-aligned plane";
    }
    if (search && (prm->max_rounds < 1 || prm->max_rounds > 63))
        return "max_rounds outside 1..63";
    return nullptr;
}

// The entry points return the 32 bits of the SvtHipStatus that refuse() and TierBCall give as int32_t.
uint32_t status_bits(int32_t status) { return (uint32_t)status; }

SegDeltas seg_deltas(const SvtHipDlfPickParams *prm) {
    SegDeltas sd{};
    sd.on = prm->segmentation_enabled != 0;
    memcpy(sd.en, prm->seg_lf_enabled, sizeof(sd.en)), memcpy(sd.data, prm->seg_lf_data, sizeof(sd.data));
    return sd;
}

}  // namespace

extern "C" uint64_t svt_hip_dlf_pick_workspace_bytes(uint32_t width, uint32_t height, int32_t is_16bit) {
    (void)is_16bit;
    return width && height ? WS_BYTES : 0;
}

extern "C" uint32_t svt_hip_dlf_pick_levels(const SvtHipDlfPickParams *prm, SvtHipDlfPickResult *d_result, void *d_workspace,
                                            uint64_t workspace_bytes, void *stream) {
    if (const char *why = bad_params(prm, d_result, true))
        return status_bits(refuse("svt_hip_dlf_pick_levels: %s", why));
    if (!d_workspace || ((uintptr_t)d_workspace & 7))
        return status_bits(refuse("svt_hip_dlf_pick_levels: d_workspace is NULL or not 8-byte aligned"));
    if (workspace_bytes < WS_BYTES)
        return status_bits(refuse("svt_hip_dlf_pick_levels: workspace of %llu bytes, %llu needed", (unsigned long long)workspace_bytes, (unsigned long long)WS_BYTES));
    TierBCall c("svt_hip_dlf_pick_levels", stream);
    if (!c.ok())
        return status_bits(c.status());
    hipStream_t          st = c.stream();
    const SvtHipLfFrame *f = &prm->frame;
    PlanArgs             pa{};
    TrialArgs            ta{};
    pa.plane_mask = prm->plane_mask, pa.only_4x4 = prm->only_4x4 != 0, pa.early_exit_convergence = prm->early_exit_convergence;
    pa.host_level[0] = f->filter_level[0], pa.host_level[1] = f->filter_level[1], pa.host_level[2] = f->filter_level_u, pa.host_level[3] = f->filter_level_v;
    ta.sd = seg_deltas(prm);
    for (int p = 0; p < 3; p++) {
        pa.start[p] = prm->start_level[p];
        ta.g[p] = plane_geom(f, p);
        ta.tiles[p] = ((ta.g[p].units_x * 4 + TILE_W - 1) / TILE_W) * ((ta.g[p].units_y * 4 + TILE_H - 1) / TILE_H);
        ta.src[p] = prm->src[p], ta.src_stride[p] = prm->src_stride[p], ta.sse_w[p] = prm->sse_width[p], ta.sse_h[p] = prm->sse_height[p];
    }
    Work      *w = (Work *)d_workspace;
    const dim3 grid(2 * (ta.tiles[0] + ta.tiles[1] + ta.tiles[2]));
    for (int r = 0; r < prm->max_rounds; r++) {
        hipLaunchKernelGGL(dlf_pick_plan, dim3(1), dim3(64), 0, st, pa, r, 0, w, d_result);
        hipLaunchKernelGGL(dlf_trial, grid, dim3(256), 0, st, ta, w);
    }
    hipLaunchKernelGGL(dlf_pick_plan, dim3(1), dim3(64), 0, st, pa, (int)prm->max_rounds, 1, w, d_result);
    return status_bits(c.finish());
}

extern "C" uint32_t svt_hip_dlf_apply_picked(const SvtHipDlfPickParams *prm, const SvtHipDlfPickResult *d_result, void *stream) {
    if (const char *why = bad_params(prm, d_result, false))
        return status_bits(refuse("svt_hip_dlf_apply_picked: %s", why));
    TierBCall c("svt_hip_dlf_apply_picked", stream);
    if (!c.ok())
        return status_bits(c.status());
    const SvtHipLfFrame *f = &prm->frame;
    PickedArgs           a{};
    a.sd = seg_deltas(prm), a.plane_mask = prm->plane_mask, a.plane_start = f->plane_start, a.plane_end = f->plane_end;
    a.host_level[0] = f->filter_level[0], a.host_level[1] = f->filter_level[1], a.host_level[2] = f->filter_level_u, a.host_level[3] = f->filter_level_v;
    for (int p = 0; p < 3; p++) a.g[p] = plane_geom(f, p);
    if (f->plane_start < f->plane_end) {  // vertical edges of every plane, then horizontal edges of every plane
        const dim3 grid((f->mi_cols + 63) / 64, (f->mi_rows + 3) / 4, 3);
        hipLaunchKernelGGL(dlf_pass_picked<0>, grid, dim3(256), 0, c.stream(), a, d_result);
        hipLaunchKernelGGL(dlf_pass_picked<1>, grid, dim3(256), 0, c.stream(), a, d_result);
    }
    return status_bits(c.finish());
}

SVT_HIP_MODULE_WARMUP(loopfilter_dlf_pick)
