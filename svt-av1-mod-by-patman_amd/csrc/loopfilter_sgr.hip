// loopfilter_sgr.hip — AV1 self-guided restoration on gfx950.
// Replaces svt_av1_selfguided_restoration_c and its two internal filters (restoration.c:468-955),
// svt_apply_selfguided_restoration_c (:957-992), svt_av1_{lowbd,highbd}_pixel_proj_error_c and
// svt_get_proj_subspace_c (restoration_pick.c:167-303, 417-506) and, as one device-side pipeline, apply_sgr +
// search_selfguided_restoration + finer_search_pixel_proj_error (restoration_pick.c:320-411, 523-652).
//
// Filter: one workgroup per 64x64 (or 32x32) processing unit.  The unit + its 3-sample border is staged once in LDS
// as uint16; the (2r+1)^2 box sums are taken straight from that tile for every position of the (w+2) x (h+2) A/B maps
// (odd rows only for the r = 2 "fast" filter), the maps stay in LDS, and every output sample reads its 6 or 9
// neighbours from there.  Nothing but the final flt0 / flt1 (or the projected samples, in the fused apply) goes back
// to memory.  Search: one workgroup per epsilon candidate owns the whole decision chain of that candidate — the five
// second-moment sums (exact in int64; the reference's double sums are exact too), the 2x2 solve in IEEE double
// (-ffp-contract=off), encode_xq and the data-dependent finer search, each error evaluation being a block reduction
// over the unit — so the host sees one readback per restoration unit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/svt_hip_lf.h"
#include "common.hpp"
#include "lr_device.hpp"

using namespace svthip;
using namespace svthip::lr;

namespace {

struct SgrGeom {
    const void *dat;
    uint32_t    dat_stride, width, height;
    uint8_t     is16, bit_depth, pu_w, pu_h;
};

// MODE 0: write flt0 / flt1.  MODE 1: fused svt_apply_selfguided_restoration (sgr_project with xq, store samples).
// SGR_NT threads share one 64x64 unit's 45 KB of LDS: three workgroups fit a CU, so the thread count sets the number of
// waves that can cover each other's barrier phases
constexpr int SGR_NT = 512;
template <int MODE>
__global__ __launch_bounds__(SGR_NT) void sgr_filter_kernel(SgrGeom g, int ep, int32_t *__restrict__ flt0, int32_t *__restrict__ flt1,
                                                         uint32_t flt_stride, void *__restrict__ dst, uint32_t dst_stride, int xq0, int xq1) {
    __shared__ alignas(4) uint16_t tile[70 * TP];
    __shared__ int32_t  Am[66 * AP], Bm[66 * AP];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * g.pu_w, i0 = blockIdx.y * g.pu_h;
    const int w = min((int)g.pu_w, (int)g.width - j0), h = min((int)g.pu_h, (int)g.height - i0);
    for (int idx = tid; idx < (h + 6) * (w + 6); idx += SGR_NT) {
        const int r = idx / (w + 6), c = idx - r * (w + 6);
        tile[r * TP + c] = (uint16_t)ldpx(g.dat, (size_t)((ptrdiff_t)(i0 + r - 3) * g.dat_stride + (j0 + c - 3)), g.is16);
    }
    __syncthreads();
    const int r0 = SGR_PRM[ep][0], r1 = SGR_PRM[ep][1], xq[2] = {xq0, xq1};
    sgr_tile_filter_to<SGR_NT>(tile, Am, Bm, tid, w, h, ep, g.bit_depth, [&](int i, int j, int32_t x, int32_t f0, int32_t f1) {
        if (MODE == 0) {
            const size_t o = (size_t)(i0 + i) * flt_stride + j0 + j;
            if (r0 > 0)
                flt0[o] = f0;
            if (r1 > 0)
                flt1[o] = f1;
        } else
            stpx(dst, (size_t)(i0 + i) * dst_stride + j0 + j, g.is16, sgr_project(x, f0, f1, xq, r0, r1, g.bit_depth));
    });
}

struct EpResult {
    long long err;
    int32_t   ep, xqd[2], pad;
};

// One workgroup per epsilon candidate: get_proj_subspace + encode_xq + finer_search_pixel_proj_error.  All threads run
// the (uniform) control flow; every error of the finer search (lr_device.hpp, one trial a pass) is a block reduction whose result all threads see.
__global__ __launch_bounds__(1024) void sgr_search_ep_kernel(SvtHipSgrUnit un, const int32_t *__restrict__ work, uint32_t flt_stride,
                                                             int start_ep, int ep_inc, int do_refine, EpResult *__restrict__ res) {
    __shared__ long long scratch[17];
    const int      ep = start_ep + blockIdx.x * ep_inc;
    const size_t   plane = (size_t)flt_stride * un.height;
    const int32_t *f0 = work + (size_t)blockIdx.x * 2 * plane, *f1 = f0 + plane;
    UnitData       u{un.src, un.dat, f0, f1, un.src_stride, un.dat_stride, flt_stride, flt_stride, un.width, un.height, un.is_16bit,
               SGR_PRM[ep][0], SGR_PRM[ep][1]};
    long long sums[5];
    unit_sums(u, sums, scratch);
    int exq[2], xqd[2];
    solve_subspace(sums, (int)(un.width * un.height), u.r0, u.r1, exq);
    encode_xq(exq, xqd, u.r0, u.r1);
    int       trials;
    long long err = finer_search<1>(u, xqd, do_refine, scratch, trials);
    if (threadIdx.x == 0)
        res[blockIdx.x] = EpResult{err, ep, {xqd[0], xqd[1]}, 0};
}
__global__ void sgr_pick_kernel(const EpResult *res, int n, EpResult *best) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        *best = res[first_min(res, n)];
}

// Tier A reductions over host-staged data: out[0..4] = subspace sums, out[5] = projection error for (xq0, xq1)
__global__ __launch_bounds__(1024) void sgr_stats_kernel(UnitData u, int xq0, int xq1, int want_sums, long long *out) {
    __shared__ long long scratch[17];
    if (want_sums) {
        long long s[5];
        unit_sums(u, s, scratch);
        if (threadIdx.x == 0)
            for (int k = 0; k < 5; k++) out[k] = s[k];
    } else {
        const int xq[1][2] = {{xq0, xq1}};
        long long e;
        unit_errors<1>(u, xq, &e, scratch);
        if (threadIdx.x == 0)
            out[5] = e;
    }
}
__global__ void sgr_solve_kernel(const long long *sums, int size, int r0, int r1, int32_t *xq) {
    if (threadIdx.x == 0) {
        int x[2];
        solve_subspace(sums, size, r0, r1, x);
        xq[0] = x[0], xq[1] = x[1];
    }
}

// The search works on one restoration unit (<= 384 x 384, restoration.h:80-84); filter / apply accept any region whose
// origin lies on the processing-unit grid, e.g. a whole plane in one launch.
bool unit_ok(const SvtHipSgrUnit *u, bool need_src) {
    const uint32_t lim = need_src ? 384u : 16384u;
    return u && u->dat && (!need_src || u->src) && u->width && u->height && u->width <= lim && u->height <= lim &&
        (u->pu_w == 64 || u->pu_w == 32) && (u->pu_h == 64 || u->pu_h == 32) && (u->bit_depth == 8 || u->bit_depth == 10 || u->bit_depth == 12) &&
        (u->bit_depth == 8 || u->is_16bit);
}
SgrGeom geom_of(const SvtHipSgrUnit *u) {
    return SgrGeom{u->dat, u->dat_stride, u->width, u->height, u->is_16bit, u->bit_depth, u->pu_w, u->pu_h};
}
template <typename T> const T *decode_ptr(const uint8_t *p, int highbd) {
    return highbd ? (const T *)((uintptr_t)p << 1) : (const T *)p;  // CONVERT_TO_SHORTPTR (definitions.h:953)
}

}  // namespace

// ------------------------------------------------------------------------------------------------ Tier B
extern "C" int32_t svt_hip_sgr_filter_unit(const SvtHipSgrUnit *unit, int32_t ep, int32_t *d_flt0, int32_t *d_flt1, uint32_t flt_stride,
                                           void *stream) {
    if (!unit_ok(unit, false) || ep < 0 || ep > 15 || !d_flt0 || !d_flt1 || flt_stride < unit->width)
        return refuse("svt_hip_sgr_filter_unit: bad argument");
    TierBCall c("svt_hip_sgr_filter_unit", stream);
    if (!c.ok())
        return c.status();
    const dim3 grid((unit->width + unit->pu_w - 1) / unit->pu_w, (unit->height + unit->pu_h - 1) / unit->pu_h);
    hipLaunchKernelGGL(sgr_filter_kernel<0>, grid, dim3(SGR_NT), 0, c.stream(), geom_of(unit), ep, d_flt0, d_flt1, flt_stride,
                       (void *)nullptr, 0u, 0, 0);
    return c.finish();
}

extern "C" int32_t svt_hip_sgr_apply_unit(const SvtHipSgrUnit *unit, int32_t ep, const int32_t xqd[2], void *d_dst, uint32_t dst_stride,
                                          void *stream) {
    if (!unit_ok(unit, false) || ep < 0 || ep > 15 || !xqd || !d_dst || dst_stride < unit->width || d_dst == unit->dat)
        return refuse("svt_hip_sgr_apply_unit: bad argument (output must not alias the input)");
    TierBCall c("svt_hip_sgr_apply_unit", stream);
    if (!c.ok())
        return c.status();
    int xq[2];
    decode_xq(xqd, xq, SGR_PRM[ep][0], SGR_PRM[ep][1]);
    const dim3 grid((unit->width + unit->pu_w - 1) / unit->pu_w, (unit->height + unit->pu_h - 1) / unit->pu_h);
    hipLaunchKernelGGL(sgr_filter_kernel<1>, grid, dim3(SGR_NT), 0, c.stream(), geom_of(unit), ep, (int32_t *)nullptr,
                       (int32_t *)nullptr, 0u, d_dst, dst_stride, xq[0], xq[1]);
    return c.finish();
}

static uint32_t search_flt_stride(uint32_t width) { return ((width + 7) & ~7u) + 8; }  // restoration_pick.c:561
extern "C" size_t svt_hip_sgr_search_work_bytes(uint32_t width, uint32_t height, int32_t n_ep) {
    if (n_ep < 1)
        n_ep = 1;
    return (size_t)n_ep * 2 * search_flt_stride(width) * height * sizeof(int32_t) + (size_t)(n_ep + 1) * sizeof(EpResult) + 256;
}

extern "C" int32_t svt_hip_sgr_search_unit(const SvtHipSgrUnit *unit, int32_t start_ep, int32_t end_ep, int32_t ep_inc, int32_t do_refine,
                                           void *d_work, int32_t out[3], int64_t *best_err, void *stream) {
    if (!unit_ok(unit, true) || start_ep < 0 || end_ep > 16 || ep_inc < 1 || start_ep >= end_ep || !d_work || !out)
        return refuse("svt_hip_sgr_search_unit: bad argument");
    TierBCall c("svt_hip_sgr_search_unit", stream);
    if (!c.ok())
        return c.status();
    hipStream_t    st    = c.stream();
    const int      n_ep  = (end_ep - start_ep + ep_inc - 1) / ep_inc;
    const uint32_t fs    = search_flt_stride(unit->width);
    const size_t   plane = (size_t)fs * unit->height;
    int32_t       *work  = (int32_t *)d_work;
    EpResult      *res   = (EpResult *)((uint8_t *)d_work + up256((size_t)n_ep * 2 * plane * sizeof(int32_t)));
    const dim3     grid((unit->width + unit->pu_w - 1) / unit->pu_w, (unit->height + unit->pu_h - 1) / unit->pu_h);
    for (int k = 0; k < n_ep; k++)
        hipLaunchKernelGGL(sgr_filter_kernel<0>, grid, dim3(SGR_NT), 0, st, geom_of(unit), start_ep + k * ep_inc, work + (size_t)k * 2 * plane,
                           work + (size_t)k * 2 * plane + plane, fs, (void *)nullptr, 0u, 0, 0);
    hipLaunchKernelGGL(sgr_search_ep_kernel, dim3(n_ep), dim3(1024), 0, st, *unit, (const int32_t *)work, fs, start_ep, ep_inc, do_refine,
                       res);
    hipLaunchKernelGGL(sgr_pick_kernel, dim3(1), dim3(64), 0, st, (const EpResult *)res, n_ep, res + n_ep);
    EpResult best;
    if (!c.check(hipGetLastError(), "launch") || !c.check(hipMemcpyAsync(&best, res + n_ep, sizeof(best), hipMemcpyDeviceToHost, st), "hipMemcpyAsync") ||
        !c.check(hipStreamSynchronize(st), "hipStreamSynchronize"))
        return c.status();
    out[0] = best.ep, out[1] = best.xqd[0], out[2] = best.xqd[1];
    if (best_err)
        *best_err = best.err;
    return c.finish();
}

// ------------------------------------------------------------------------------------------------ Tier A
// Stage a w x h region (+border) of host samples as a packed plane; returns the offset of the plane (pitch w + 2 * border).
static size_t stage_region(TierAStage &s, const uint8_t *p8, int highbd, int w, int hh, int stride, int border) {
    const size_t   px = highbd ? 2 : 1, pitch = ((size_t)w + 2 * border) * px;
    const uint8_t *p  = highbd ? (const uint8_t *)decode_ptr<uint16_t>(p8, 1) : p8;
    return s.in_rows(p - ((ptrdiff_t)border * stride + border) * (ptrdiff_t)px, (size_t)stride * px, (size_t)hh + 2 * border, pitch);
}

TIER_A_LEAF(void, svt_av1_selfguided_restoration,
            (const uint8_t *dgd8, int32_t width, int32_t height, int32_t dgd_stride, int32_t *flt0, int32_t *flt1, int32_t
             flt_stride, int32_t ep, int32_t bit_depth, int32_t highbd),
            (dgd8, width, height, dgd_stride, flt0, flt1, flt_stride, ep, bit_depth, highbd)) {
    if (width <= 0 || height <= 0 || width > 384 || height > 384 || ep < 0 || ep > 15) {
        set_error("svt_av1_selfguided_restoration_hip: unsupported size %dx%d / ep %d", width, height, ep);
        fatal("selfguided_restoration");
    }
    TierAStage   s("selfguided_restoration");
    const size_t px = highbd ? 2 : 1, pitch = (size_t)width + 6, fl_bytes = (size_t)width * height * 4;
    const size_t o_in = stage_region(s, dgd8, highbd, width, height, dgd_stride, 3), o_f0 = s.out(fl_bytes), o_f1 = s.out(fl_bytes);
    s.upload();
    SvtHipSgrUnit u{s.dev(o_in) + (3 * pitch + 3) * px, nullptr, (uint32_t)pitch, 0, (uint32_t)width, (uint32_t)height, (uint8_t)(highbd != 0),
                    (uint8_t)bit_depth, 64, 64};
    const dim3    grid((width + 63) / 64, (height + 63) / 64);
    hipLaunchKernelGGL(sgr_filter_kernel<0>, grid, dim3(SGR_NT), 0, s.stream(), geom_of(&u), ep, s.dev<int32_t>(o_f0), s.dev<int32_t>(o_f1),
                       (uint32_t)width, (void *)nullptr, 0u, 0, 0);
    s.finish(o_f0, o_f1 + fl_bytes - o_f0);  // adjacent: one copy brings both back
    if (SGR_PRM[ep][0] > 0)
        s.out_rows(flt0, (size_t)flt_stride * 4, o_f0, height, (size_t)width * 4);
    if (SGR_PRM[ep][1] > 0)
        s.out_rows(flt1, (size_t)flt_stride * 4, o_f1, height, (size_t)width * 4);
}

TIER_A_LEAF(void, svt_apply_selfguided_restoration,
            (const uint8_t *dat, int32_t width, int32_t height, int32_t stride, int32_t eps, const int32_t *xqd, uint8_t *dst,
             int32_t dst_stride, int32_t *tmpbuf, int32_t bit_depth, int32_t highbd),
            (dat, width, height, stride, eps, xqd, dst, dst_stride, tmpbuf, bit_depth, highbd)) {
    (void)tmpbuf;
    if (width <= 0 || height <= 0 || width > 384 || height > 384 || eps < 0 || eps > 15) {
        set_error("svt_apply_selfguided_restoration_hip: unsupported size %dx%d / eps %d", width, height, eps);
        fatal("apply_selfguided_restoration");
    }
    TierAStage   s("apply_selfguided_restoration");
    const size_t px = highbd ? 2 : 1, pitch = (size_t)width + 6, out_bytes = (size_t)width * height * px;
    const size_t o_in = stage_region(s, dat, highbd, width, height, stride, 3), o_out = s.out(out_bytes);
    s.upload();
    SvtHipSgrUnit u{s.dev(o_in) + (3 * pitch + 3) * px, nullptr, (uint32_t)pitch, 0, (uint32_t)width, (uint32_t)height, (uint8_t)(highbd != 0),
                    (uint8_t)bit_depth, 64, 64};
    if (svt_hip_sgr_apply_unit(&u, eps, xqd, s.dev(o_out), (uint32_t)width, s.stream()) != SVT_HIP_OK)
        fatal("apply_selfguided_restoration");
    s.finish(o_out, out_bytes);
    s.out_rows(highbd ? (uint8_t *)((uintptr_t)dst << 1) : dst, (size_t)dst_stride * px, o_out, height, (size_t)width * px);
}

// Shared staging of (src, dat, flt0, flt1) for the two reductions
static void proj_tier_a(const uint8_t *src8, int width, int height, int src_stride, const uint8_t *dat8, int dat_stride, int highbd,
                        const int32_t *flt0, int flt0_stride, const int32_t *flt1, int flt1_stride, const SvtHipSgrParams *params, int xq0,
                        int xq1, int want_sums, long long out[6], int32_t *xq_solved) {
    if (width <= 0 || height <= 0 || (size_t)width * height > (size_t)1 << 20 || !params) {
        set_error("sgr projection: unsupported size %dx%d", width, height);
        fatal("sgr projection");
    }
    TierAStage     s("sgr projection");
    const size_t   px = highbd ? 2 : 1, row = (size_t)width * px, frow = (size_t)width * 4;
    const uint8_t *sb = highbd ? (const uint8_t *)((uintptr_t)src8 << 1) : src8, *db = highbd ? (const uint8_t *)((uintptr_t)dat8 << 1) : dat8;
    const int      r0 = params->r[0], r1 = params->r[1];
    const size_t   o_src = s.in_rows(sb, (size_t)src_stride * px, height, row), o_dat = s.in_rows(db, (size_t)dat_stride * px, height, row);
    // an unused filter plane (radius 0) is not read from the caller but keeps its place
    const size_t   o_f0 = r0 > 0 ? s.in_rows(flt0, (size_t)flt0_stride * 4, height, frow) : s.in(nullptr, height * frow);
    const size_t   o_f1 = r1 > 0 ? s.in_rows(flt1, (size_t)flt1_stride * 4, height, frow) : s.in(nullptr, height * frow);
    const size_t   o_res = s.out(80);
    s.upload();
    UnitData   u{s.dev(o_src), s.dev(o_dat), s.dev<const int32_t>(o_f0), s.dev<const int32_t>(o_f1), (uint32_t)width, (uint32_t)width,
               (uint32_t)width, (uint32_t)width, (uint32_t)width, (uint32_t)height, highbd != 0, r0, r1};
    long long *dres = s.dev<long long>(o_res);
    hipLaunchKernelGGL(sgr_stats_kernel, dim3(1), dim3(1024), 0, s.stream(), u, xq0, xq1, want_sums, dres);
    if (want_sums && xq_solved)
        hipLaunchKernelGGL(sgr_solve_kernel, dim3(1), dim3(64), 0, s.stream(), (const long long *)dres, width * height, r0, r1, (int32_t *)(dres + 8));
    s.finish(o_res, 80);
    memcpy(out, s.host(o_res), 6 * sizeof(long long));
    if (xq_solved)
        memcpy(xq_solved, s.host(o_res) + 64, 8);
}

TIER_A_LEAF(int64_t, svt_av1_lowbd_pixel_proj_error,
            (const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8, int32_t dat_stride,
             int32_t *flt0, int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride, int32_t xq[2], const SvtHipSgrParams *params),
            (src8, width, height, src_stride, dat8, dat_stride, flt0, flt0_stride, flt1, flt1_stride, xq, params)) {
    long long out[6];
    proj_tier_a(src8, width, height, src_stride, dat8, dat_stride, 0, flt0, flt0_stride, flt1, flt1_stride, params, xq[0], xq[1], 0, out, nullptr);
    return out[5];
}
TIER_A_LEAF(int64_t, svt_av1_highbd_pixel_proj_error,
            (const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8, int32_t dat_stride,
             int32_t *flt0, int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride, int32_t xq[2], const SvtHipSgrParams *params),
            (src8, width, height, src_stride, dat8, dat_stride, flt0, flt0_stride, flt1, flt1_stride, xq, params)) {
    long long out[6];
    proj_tier_a(src8, width, height, src_stride, dat8, dat_stride, 1, flt0, flt0_stride, flt1, flt1_stride, params, xq[0], xq[1], 0, out, nullptr);
    return out[5];
}
TIER_A_LEAF(void, svt_get_proj_subspace,
            (const uint8_t *src8, int width, int height, int src_stride, const uint8_t *dat8, int dat_stride, int use_highbitdepth,
             int32_t *flt0, int flt0_stride, int32_t *flt1, int flt1_stride, int *xq, const SvtHipSgrParams *params),
            (src8, width, height, src_stride, dat8, dat_stride, use_highbitdepth, flt0, flt0_stride, flt1, flt1_stride, xq, params)) {
    long long out[6];
    int32_t   solved[2] = {0, 0};
    proj_tier_a(src8, width, height, src_stride, dat8, dat_stride, use_highbitdepth, flt0, flt0_stride, flt1, flt1_stride, params, 0, 0, 1, out,
                solved);
    xq[0] = solved[0], xq[1] = solved[1];
}

SVT_HIP_MODULE_WARMUP(loopfilter_sgr)
