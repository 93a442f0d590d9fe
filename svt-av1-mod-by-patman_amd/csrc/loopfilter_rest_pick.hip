// loopfilter_rest_pick.hip — the restoration decision of one plane with the self-guided filter enabled (restoration_pick.c:
// search_sgrproj_seg :1220-1264, search_sgrproj_finish :1267, search_wiener_finish :1380, search_switchable :1148, rest_finish_search
// :1555-1625, copy_unit_info :1202), between svt_hip_wiener_pick_plane and svt_hip_restoration_filter_frame.  Four launches whatever
// the data, on one stream, nothing read back.  DESIGN.md section 4 has the design and why.
//
//   rpick_filter   workgroup per (processing-unit tile, ep candidate, unit): apply_sgr (:523-548) with the tile filter of
//                  lr_device.hpp; flt0 / flt1 go to the workspace, and the five sums of svt_get_proj_subspace are taken from the
//                  values while they are in registers (int64, exact; one 64-bit atomic add per sum and workgroup).
//   rpick_search   workgroup per (ep candidate, unit): the 2x2 solve in IEEE double, encode_xq (:508) and
//                  finer_search_pixel_proj_error (:320-411) with the reference's control flow, the loop inside the kernel, every
//                  pass over the unit a block reduction that yields the errors of up to four moves of a walk.  At most 135 trials:
//                  see below.
//   rpick_trial    workgroup per (stripe tile, unit): picks the unit's winner (first strictly smallest error in candidate order),
//                  runs svt_apply_selfguided_restoration with it in the tiling of svt_av1_loop_restoration_filter_unit (:1067-1135,
//                  need_boundaries == 0: the picture's own rows above and below a stripe) and sums the squared differences of the
//                  restored and of the unrestored samples against the source.  No picture is written.
//   rpick_decide   one workgroup: the unit records, the three raster-order chains, the RDCOST_DBL of every tested type, the choice,
//                  the histogram of ep and the units for svt_hip_restoration_filter_frame.
// Samples outside the cropped plane replicate its edge (svt_extend_frame): coordinates are clamped, nothing outside is read.
#include <vector>

#include "lr_pick.hpp"

using namespace svthip;
using namespace svthip::lr;

namespace {

constexpr int NT = 512;  // threads of the two filtering kernels: see SGR_NT in loopfilter_sgr.hip
// The longest finer search.  A trial is accepted on an equal error, so on a flat unit (every filtered value equals the sample, every
// error equals the first) every move ties and the walk at step 2 only ends at the clamp.  Per tap at step 2: either moves down
// (at most (PRJ_MAX - PRJ_MIN) / 2 = 63 accepted ones, after which `if (skip) break;` leaves the tap loop), or one refused move
// down, at most 63 moves up and one refused: 65 trials.  At step 1 nothing repeats: at most 2 per tap.  With the first
// error: 1 + 2 * 65 + 2 * 2 = 135 trials at the most.

struct PUnit {  // a unit as the kernels take it: the caller's record and where its filtered samples start in a workspace plane
    SvtHipWienerUnit   u;
    unsigned long long off;
};
struct Cand {  // workspace: one per (unit, candidate)
    long long sums[5];  // svt_get_proj_subspace: f1 * f1, f2 * f2, f1 * f2, f1 * s, f2 * s
    long long err;      // after the finer search
    int32_t   xqd[2], trials, pad_;
};
static_assert(sizeof(Cand) == 64, "workspace record stated in the header");
struct Acc {  // workspace: one per unit
    unsigned long long none, sgr;
};
struct PlanePrm {
    int                plane_w, plane_h, is16, bd, pu_w, pu_h, stripe_h, stripe_off, start_ep, ep_inc, n_ep, refine;
    unsigned long long plane_px;
};

__device__ __forceinline__ const void *px_at(const void *base, size_t idx, int is16) { return (const uint8_t *)base + (idx << (is16 ? 1 : 0)); }

// grid (tiles of the largest unit, candidates, units)
__global__ __launch_bounds__(NT) void rpick_filter(const PUnit *__restrict__ units, Cand *__restrict__ cands, int32_t *__restrict__ planes, PlanePrm p) {
    __shared__ alignas(4) uint16_t tile[70 * TP];
    __shared__ int32_t  Am[66 * AP], Bm[66 * AP];
    __shared__ long long s_sums[5];
    const int              tid = threadIdx.x, k = blockIdx.y, ep = p.start_ep + k * p.ep_inc;
    const SvtHipWienerUnit u   = units[blockIdx.z].u;
    const int uw = u.h_end - u.h_start, uh = u.v_end - u.v_start, gx = (uw + p.pu_w - 1) / p.pu_w, n_tiles = gx * ((uh + p.pu_h - 1) / p.pu_h);
    if ((int)blockIdx.x >= n_tiles)
        return;
    const int i0 = ((int)blockIdx.x / gx) * p.pu_h, j0 = ((int)blockIdx.x % gx) * p.pu_w, w = min(p.pu_w, uw - j0), h = min(p.pu_h, uh - i0);
    if (tid < 5)
        s_sums[tid] = 0;
    load_tile_clamped(tile, TP, u.dgd, u.dgd_stride, p.is16, p.plane_w, p.plane_h, u.v_start + i0 - 3, u.h_start + j0 - 3, h + 6, w + 6, NT);  // with the 3-sample border
    __syncthreads();
    int32_t  *f0p = planes + (size_t)(2 * k) * p.plane_px + units[blockIdx.z].off, *f1p = f0p + p.plane_px;
    const int r0 = SGR_PRM[ep][0], r1 = SGR_PRM[ep][1], is16 = p.is16;
    long long a[5] = {0, 0, 0, 0, 0};
    sgr_tile_filter_to<NT>(tile, Am, Bm, tid, w, h, ep, p.bd,
                              [&](int i, int j, int32_t x, int32_t f0, int32_t f1) {
                                  const size_t o = (size_t)(i0 + i) * uw + j0 + j;
                                  if (r0 > 0)
                                      f0p[o] = f0;
                                  if (r1 > 0)
                                      f1p[o] = f1;
                                  const long long uu = (long long)x << RST_BITS;
                                  const long long s  = ((long long)ldpx(u.src, (size_t)(u.v_start + i0 + i) * u.src_stride + u.h_start + j0 + j, is16) << RST_BITS) - uu;
                                  const long long d0 = r0 > 0 ? f0 - uu : 0, d1 = r1 > 0 ? f1 - uu : 0;
                                  a[0] += d0 * d0, a[1] += d1 * d1, a[2] += d0 * d1, a[3] += d0 * s, a[4] += d1 * s;
                              });
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const long long v = wave_sum64(a[q]);
        if ((tid & 63) == 0)
            lds_add(&s_sums[q], v);
    }
    __syncthreads();
    if (tid < 5)
        atomicAdd((unsigned long long *)&cands[(size_t)blockIdx.z * p.n_ep + k].sums[tid], (unsigned long long)s_sums[tid]);
}

constexpr int NB = 4;  // moves of a step-2 walk of the finer search (lr_device.hpp) that one pass over the unit evaluates

// grid (candidates, units)
__global__ __launch_bounds__(1024) void rpick_search(const PUnit *__restrict__ units, Cand *__restrict__ cands, const int32_t *__restrict__ planes, PlanePrm p) {
    __shared__ long long   scratch[16 * NB];
    const int              k = blockIdx.x, ep = p.start_ep + k * p.ep_inc;
    const SvtHipWienerUnit un = units[blockIdx.y].u;
    const uint32_t         uw = un.h_end - un.h_start, uh = un.v_end - un.v_start;
    const int32_t         *f0 = planes + (size_t)(2 * k) * p.plane_px + units[blockIdx.y].off, *f1 = f0 + p.plane_px;
    Cand                  &c  = cands[(size_t)blockIdx.y * p.n_ep + k];
    UnitData u{px_at(un.src, (size_t)un.v_start * un.src_stride + un.h_start, p.is16), px_at(un.dgd, (size_t)un.v_start * un.dgd_stride + un.h_start, p.is16),
               f0, f1, un.src_stride, un.dgd_stride, uw, uw, uw, uh, p.is16, SGR_PRM[ep][0], SGR_PRM[ep][1]};
    long long sums[5];
    for (int q = 0; q < 5; q++) sums[q] = c.sums[q];
    int exq[2], xqd[2], trials;
    solve_subspace(sums, (int)(uw * uh), u.r0, u.r1, exq);
    encode_xq(exq, xqd, u.r0, u.r1);
    const long long err = finer_search<NB>(u, xqd, p.refine, scratch, trials);
    if (threadIdx.x == 0)
        c.err = err, c.xqd[0] = xqd[0], c.xqd[1] = xqd[1], c.trials = trials, c.pad_ = 0;
}

// Stripe `sr` of a unit: stripes end at the picture rows k * stripe_h - stripe_off (restoration.c:1100-1113)
__device__ __host__ inline int first_stripe_end(int v_start, int stripe_h, int stripe_off) { return ((v_start + stripe_off) / stripe_h + 1) * stripe_h - stripe_off; }
__device__ __host__ inline int stripes_of(int v_start, int v_end, int stripe_h, int stripe_off) {
    const int e0 = first_stripe_end(v_start, stripe_h, stripe_off);
    return v_end <= e0 ? 1 : 1 + (v_end - e0 + stripe_h - 1) / stripe_h;
}

// grid (stripe tiles of the largest unit, units)
__global__ __launch_bounds__(NT) void rpick_trial(const PUnit *__restrict__ units, const Cand *__restrict__ cands, Acc *__restrict__ accs, PlanePrm p) {
    __shared__ alignas(4) uint16_t tile[70 * TP];
    __shared__ int32_t  Am[66 * AP], Bm[66 * AP];
    __shared__ long long s_sum[2];
    const int              tid = threadIdx.x;
    const SvtHipWienerUnit u   = units[blockIdx.y].u;
    const int uw = u.h_end - u.h_start, gx = (uw + p.pu_w - 1) / p.pu_w, n_tiles = gx * stripes_of(u.v_start, u.v_end, p.stripe_h, p.stripe_off);
    if ((int)blockIdx.x >= n_tiles)
        return;
    const int sr = (int)blockIdx.x / gx, j0 = ((int)blockIdx.x % gx) * p.pu_w, e0 = first_stripe_end(u.v_start, p.stripe_h, p.stripe_off);
    const int y0 = sr == 0 ? u.v_start : e0 + (sr - 1) * p.stripe_h, y1 = min(u.v_end, sr == 0 ? e0 : y0 + p.stripe_h);
    const int w = min(p.pu_w, uw - j0), h = y1 - y0;
    const Cand *cu = cands + (size_t)blockIdx.y * p.n_ep;
    const int   b = first_min(cu, p.n_ep), ep = p.start_ep + b * p.ep_inc, r0 = SGR_PRM[ep][0], r1 = SGR_PRM[ep][1], is16 = p.is16, bd = p.bd;
    int xqd[2] = {cu[b].xqd[0], cu[b].xqd[1]}, xq[2];
    decode_xq(xqd, xq, r0, r1);
    if (tid < 2)
        s_sum[tid] = 0;
    load_tile_clamped(tile, TP, u.dgd, u.dgd_stride, is16, p.plane_w, p.plane_h, y0 - 3, u.h_start + j0 - 3, h + 6, w + 6, NT);
    __syncthreads();
    long long acc = 0, accn = 0;
    sgr_tile_filter_to<NT>(tile, Am, Bm, tid, w, h, ep, bd,
                              [&](int i, int j, int32_t x, int32_t f0, int32_t f1) {
                                  const int32_t o = sgr_project(x, f0, f1, xq, r0, r1, bd);
                                  const int32_t s = ldpx(u.src, (size_t)(y0 + i) * u.src_stride + u.h_start + j0 + j, is16);
                                  acc += (long long)((o - s) * (o - s)), accn += (long long)((x - s) * (x - s));
                              });
    acc = wave_sum64(acc), accn = wave_sum64(accn);
    if ((tid & 63) == 0)
        lds_add(&s_sum[0], acc), lds_add(&s_sum[1], accn);
    __syncthreads();
    if (tid == 0)
        atomicAdd(&accs[blockIdx.y].sgr, (unsigned long long)s_sum[0]), atomicAdd(&accs[blockIdx.y].none, (unsigned long long)s_sum[1]);
}

struct DecidePrm {
    int n_units, n_ep, start_ep, ep_inc, win, rdmult, cost_w[2], cost_s[2], cost_sw[3];
};

// One thread walks the units in raster order; everything that does not depend on a `ref` is prepared beside it by 256 threads,
// 256 units at a time, in LDS (as wpick_decide does: a dependent read of device memory per unit costs more than the chains).
__global__ __launch_bounds__(256) void rpick_decide(const Cand *__restrict__ cands, const Acc *__restrict__ accs, const SvtHipWienerPickUnit *__restrict__ wrecs,
                                                    SvtHipRestPickUnit *__restrict__ recs, SvtHipRestPickResult *__restrict__ res,
                                                    SvtHipLrUnit *__restrict__ lr_units, DecidePrm p) {
    constexpr int CH = 256;
    __shared__ long long s_sse[3][CH];
    __shared__ int16_t   s_taps[CH][6];
    __shared__ int       s_ep[CH], s_xqd[CH][2], s_wbest[CH], s_best[3][CH], s_type, s_hist[16], s_count[3];
    const int  tid = threadIdx.x;
    const bool with_w = wrecs != nullptr, with_sw = with_w && p.n_units > 1;
    if (tid < 16)
        s_hist[tid] = 0;
    if (tid < 3)
        s_count[tid] = 0;
    // thread 0's alone: ref and totals of the passes WIENER, SGRPROJ, SWITCHABLE
    int ref_w[6], ref_s[2], sw_w[6], sw_s[2];
    set_default_wiener(ref_w), set_default_sgrproj(ref_s), set_default_wiener(sw_w), set_default_sgrproj(sw_s);
    long long sse[4] = {0, 0, 0, 0}, bits[4] = {0, 0, 0, 0};
    for (int base = 0; base < p.n_units; base += CH) {
        const int i = base + tid;
        __syncthreads();
        if (i < p.n_units) {
            const Cand *cu = cands + (size_t)i * p.n_ep;
            const int   b  = first_min(cu, p.n_ep), ep = p.start_ep + b * p.ep_inc;
            SvtHipRestPickUnit &r = recs[i];
            const long long     sse1 = with_w ? wrecs[i].sse[1] : SSE_REJECTED;
            r.sse[0] = (long long)accs[i].none, r.sse[1] = sse1, r.sse[2] = (long long)accs[i].sgr, r.search_err = cu[b].err;
            r.ep = ep, r.xqd[0] = cu[b].xqd[0], r.xqd[1] = cu[b].xqd[1], r.trials = cu[b].trials, r.pad_ = 0;
            s_sse[0][tid] = r.sse[0], s_sse[1][tid] = sse1, s_sse[2][tid] = r.sse[2];
            s_ep[tid] = ep, s_xqd[tid][0] = cu[b].xqd[0], s_xqd[tid][1] = cu[b].xqd[1];
            for (int t = 0; t < 3; t++) s_taps[tid][t] = with_w ? wrecs[i].vfilter[t] : (int16_t)0, s_taps[tid][3 + t] = with_w ? wrecs[i].hfilter[t] : (int16_t)0;
            s_wbest[tid] = with_w ? wrecs[i].best_rtype : 0;
            atomicAdd(&s_hist[ep], 1);
        }
        __syncthreads();
        if (tid == 0) {
            const int n = min(CH, p.n_units - base);
            for (int k = 0; k < n; k++) {
                const long long sse0 = s_sse[0][k], sse1 = s_sse[1][k], sse2 = s_sse[2][k];
                sse[RESTORE_NONE] += sse0;
                int bw = RESTORE_NONE;
                if (with_w) {  // search_wiener_finish (:1380-1431); the comparison of the two costs is the Wiener call's
                    if (sse1 == SSE_REJECTED)
                        bits[RESTORE_WIENER] += p.cost_w[0], sse[RESTORE_WIENER] += sse0;
                    else {
                        const long long bits_wiener = p.cost_w[1] + (count_wiener_bits(p.win, s_taps[k], ref_w, wiener_tap_bits) << 9);
                        bw = s_wbest[k] == RESTORE_WIENER ? RESTORE_WIENER : RESTORE_NONE;
                        sse[RESTORE_WIENER] += bw ? sse1 : sse0, bits[RESTORE_WIENER] += bw ? bits_wiener : (long long)p.cost_w[0];
                        if (bw)
                            for (int t = 0; t < 6; t++) ref_w[t] = s_taps[k][t];
                    }
                }
                int bs;
                {  // search_sgrproj_finish (:1267-1293)
                    const long long bits_none = p.cost_s[0], bits_sgr = p.cost_s[1] + (count_sgrproj_bits(s_ep[k], s_xqd[k], ref_s) << 9);
                    const double    cost_none = rdcost_dbl(p.rdmult, bits_none >> 4, sse0), cost_sgr = rdcost_dbl(p.rdmult, bits_sgr >> 4, sse2);
                    const bool      sgr       = cost_sgr < cost_none;
                    bs = sgr ? RESTORE_SGRPROJ : RESTORE_NONE;
                    sse[RESTORE_SGRPROJ] += sgr ? sse2 : sse0, bits[RESTORE_SGRPROJ] += sgr ? bits_sgr : bits_none;
                    if (sgr)
                        ref_s[0] = s_xqd[k][0], ref_s[1] = s_xqd[k][1];
                }
                int bsw = RESTORE_NONE;
                if (with_sw) {  // search_switchable (:1148-1200)
                    double    best_cost = 0;
                    long long best_bits = 0;
                    for (int r = 0; r < 3; r++) {
                        if (r > RESTORE_NONE && (r == RESTORE_WIENER ? bw : bs) == RESTORE_NONE)
                            continue;
                        const long long pcost = r == RESTORE_NONE ? 0 : (r == RESTORE_WIENER ? count_wiener_bits(p.win, s_taps[k], sw_w, wiener_tap_bits) : count_sgrproj_bits(s_ep[k], s_xqd[k], sw_s));
                        const long long b     = p.cost_sw[r] + (pcost << 9);
                        const double    cost  = rdcost_dbl(p.rdmult, b >> 4, s_sse[r][k]);
                        if (r == 0 || cost < best_cost)
                            best_cost = cost, best_bits = b, bsw = r;
                    }
                    sse[RESTORE_SWITCHABLE] += s_sse[bsw][k], bits[RESTORE_SWITCHABLE] += best_bits;
                    if (bsw == RESTORE_WIENER)
                        for (int t = 0; t < 6; t++) sw_w[t] = s_taps[k][t];
                    if (bsw == RESTORE_SGRPROJ)
                        sw_s[0] = s_xqd[k][0], sw_s[1] = s_xqd[k][1];
                }
                s_best[0][k] = bw, s_best[1][k] = bs, s_best[2][k] = bsw;
            }
        }
        __syncthreads();
        if (i < p.n_units)
            recs[i].best_rtype[0] = s_best[0][tid], recs[i].best_rtype[1] = s_best[1][tid], recs[i].best_rtype[2] = s_best[2][tid];
    }
    if (tid == 0) {  // rest_finish_search (:1592-1617)
        const int tested = 1 | (with_w ? 1 << RESTORE_WIENER : 0) | 1 << RESTORE_SGRPROJ | (with_sw ? 1 << RESTORE_SWITCHABLE : 0);
        double    best_cost = 0;
        int       type = RESTORE_NONE;
        for (int r = 0; r < 4; r++) {
            const bool   t    = (tested >> r) & 1;
            const double cost = t ? rdcost_dbl(p.rdmult, bits[r] >> 4, sse[r]) : 0.0;
            res->sse[r] = t ? sse[r] : 0, res->bits[r] = t ? bits[r] : 0, res->cost[r] = cost;
            if (t && (r == 0 || cost < best_cost))
                best_cost = cost, type = r;
        }
        res->frame_restoration_type = type, res->tested = tested, res->pad_ = 0;
        s_type = type;
    }
    __syncthreads();
    for (int i = tid; i < p.n_units; i += 256) {  // copy_unit_info (:1202); a thread reads back what it wrote itself
        const SvtHipRestPickUnit &r = recs[i];
        const int                 t = s_type >= 1 ? r.best_rtype[s_type - 1] : RESTORE_NONE;
        SvtHipLrUnit              o{};
        o.restoration_type = (uint8_t)t;
        if (t == RESTORE_WIENER)
            for (int k = 0; k < 8; k++) o.hfilter[k] = wrecs[i].hfilter[k], o.vfilter[k] = wrecs[i].vfilter[k];
        if (t == RESTORE_SGRPROJ)
            o.ep = (uint8_t)r.ep, o.xqd[0] = r.xqd[0], o.xqd[1] = r.xqd[1];
        lr_units[i] = o;
        atomicAdd(&s_count[t], 1);
    }
    __syncthreads();
    if (tid < 16)
        res->sg_frame_ep_cnt[tid] = s_hist[tid];
    if (tid < 3)
        res->n_units_of_type[tid] = s_count[tid];
}

int    n_ep_of(const SvtHipRestPickParams *prm) { return (prm->sg_end_ep - prm->sg_start_ep + prm->sg_ep_inc - 1) / prm->sg_ep_inc; }
size_t head_bytes(size_t n_units, size_t n_ep) { return up256(n_units * n_ep * sizeof(Cand)) + up256(n_units * sizeof(Acc)); }

}  // namespace

extern "C" uint64_t svt_hip_rest_pick_workspace_bytes(uint32_t n_units, uint32_t plane_width, uint32_t plane_height, int32_t n_ep) {
    if (!n_units || !plane_width || !plane_height || n_ep < 1)
        return 0;
    return head_bytes(n_units, (size_t)n_ep) + up256((uint64_t)n_ep * 2 * plane_width * plane_height * sizeof(int32_t));
}

extern "C" int64_t svt_hip_rest_pick_plane(const SvtHipRestPickParams *prm, const SvtHipWienerUnit *units, uint32_t n_units,
                                           const SvtHipWienerPickUnit *d_wiener_records, SvtHipRestPickUnit *d_unit_records,
                                           SvtHipRestPickResult *d_result, SvtHipLrUnit *d_lr_units, void *d_workspace, uint64_t workspace_bytes,
                                           void *stream) {
    static_assert(sizeof(SvtHipRestPickUnit) == SVT_HIP_REST_PICK_UNIT_BYTES && sizeof(SvtHipRestPickResult) == SVT_HIP_REST_PICK_RESULT_BYTES,
                  "record sizes stated in the header");
    if (!prm || !units || !d_unit_records || !d_result || !d_lr_units || !d_workspace)
        return refuse("svt_hip_rest_pick_plane: NULL argument");
    if (n_units == 0 || n_units > 65535)
        return refuse("svt_hip_rest_pick_plane: %u units (1..65535)", n_units);
    if (const int32_t rc = pick_plane_ok("svt_hip_rest_pick_plane", prm->bit_depth, prm->is_16bit, prm->plane_width, prm->plane_height); rc != SVT_HIP_OK)
        return rc;
    if ((prm->ss_x | prm->ss_y) & ~1)
        return refuse("svt_hip_rest_pick_plane: subsampling %d, %d (0 or 1)", prm->ss_x, prm->ss_y);
    if (prm->sg_start_ep < 0 || prm->sg_end_ep > 16 || prm->sg_start_ep >= prm->sg_end_ep || prm->sg_ep_inc < 1)
        return refuse("svt_hip_rest_pick_plane: ep from %d to %d in steps of %d", prm->sg_start_ep, prm->sg_end_ep, prm->sg_ep_inc);
    if (d_wiener_records && prm->wiener_win != 7 && prm->wiener_win != 5)
        return refuse("svt_hip_rest_pick_plane: wiener_win %d is neither 7 nor 5", prm->wiener_win);
    PlanePrm p{(int)prm->plane_width, (int)prm->plane_height, prm->is_16bit ? 1 : 0, prm->bit_depth, 64 >> prm->ss_x, 64 >> prm->ss_y, 64 >> prm->ss_y,
               8 >> prm->ss_y, prm->sg_start_ep, prm->sg_ep_inc, n_ep_of(prm), prm->sg_refine ? 1 : 0, (unsigned long long)prm->plane_width * prm->plane_height};
    static thread_local std::vector<PUnit> staged;
    staged.resize(n_units);
    unsigned long long off = 0;
    int                max_tiles = 0, max_stripe_tiles = 0;
    if (const int32_t rc = pick_units_ok("svt_hip_rest_pick_plane", units, n_units, prm->plane_width, prm->plane_height, 384,
                                         [&](uint32_t i, const SvtHipWienerUnit &u, int uw, int uh) {
                                             staged[i] = PUnit{u, off};
                                             off += (unsigned long long)uw * uh;
                                             const int gx = (uw + p.pu_w - 1) / p.pu_w;
                                             max_tiles        = std::max(max_tiles, gx * ((uh + p.pu_h - 1) / p.pu_h));
                                             max_stripe_tiles = std::max(max_stripe_tiles, gx * stripes_of(u.v_start, u.v_end, p.stripe_h, p.stripe_off));
                                         });
        rc != SVT_HIP_OK)
        return rc;
    if (off > p.plane_px)
        return refuse("svt_hip_rest_pick_plane: the units hold %llu samples, the plane %llu", off, p.plane_px);
    const uint64_t need = svt_hip_rest_pick_workspace_bytes(n_units, prm->plane_width, prm->plane_height, p.n_ep);
    if (workspace_bytes < need || ((uintptr_t)d_workspace & 7) || ((uintptr_t)d_result & 7) || ((uintptr_t)d_unit_records & 7) || ((uintptr_t)d_lr_units & 7))
        return refuse("svt_hip_rest_pick_plane: workspace of %llu bytes, %llu needed (workspace, records, result and units 8-byte aligned)",
                      (unsigned long long)workspace_bytes, (unsigned long long)need);
    TierBCall    c("svt_hip_rest_pick_plane", stream);
    const PUnit *d_units = (const PUnit *)c.stage(staged.data(), sizeof(PUnit) * n_units);
    if (!c.ok())
        return c.status();
    hipStream_t  st    = c.stream();
    const size_t head  = head_bytes(n_units, (size_t)p.n_ep);
    Cand        *cands = (Cand *)d_workspace;
    Acc         *accs  = (Acc *)((uint8_t *)d_workspace + up256((size_t)n_units * p.n_ep * sizeof(Cand)));
    int32_t     *planes = (int32_t *)((uint8_t *)d_workspace + head);
    if (!c.check(hipMemsetAsync(d_workspace, 0, head, st), "hipMemsetAsync"))  // the sums start from zero in every call
        return c.status();
    hipLaunchKernelGGL(rpick_filter, dim3((unsigned)max_tiles, (unsigned)p.n_ep, n_units), dim3(NT), 0, st, d_units, cands, planes, p);
    hipLaunchKernelGGL(rpick_search, dim3((unsigned)p.n_ep, n_units), dim3(1024), 0, st, d_units, cands, (const int32_t *)planes, p);
    hipLaunchKernelGGL(rpick_trial, dim3((unsigned)max_stripe_tiles, n_units), dim3(NT), 0, st, d_units, (const Cand *)cands, accs, p);
    const DecidePrm dp{(int)n_units, p.n_ep, p.start_ep, p.ep_inc, prm->wiener_win, prm->rdmult,
                       {prm->wiener_restore_cost[0], prm->wiener_restore_cost[1]}, {prm->sgrproj_restore_cost[0], prm->sgrproj_restore_cost[1]},
                       {prm->switchable_restore_cost[0], prm->switchable_restore_cost[1], prm->switchable_restore_cost[2]}};
    hipLaunchKernelGGL(rpick_decide, dim3(1), dim3(256), 0, st, (const Cand *)cands, (const Acc *)accs, d_wiener_records, d_unit_records, d_result, d_lr_units,
                       dp);
    const int32_t rc = c.finish();
    return rc == SVT_HIP_OK ? 4 : (int64_t)rc;
}

SVT_HIP_MODULE_WARMUP(loopfilter_rest_pick)
