// loopfilter_dlf.hip — AV1 deblocking on gfx950.
// Replaces svt_av1_loop_filter_frame / svt_aom_loop_filter_sb / svt_av1_filter_block_plane_vert|horz /
// set_lpf_parameters (deblocking_filter.c:162-653) and the sixteen svt_aom_[highbd_]lpf_* leaves
// (deblocking_common.c:141-865).
//
// AV1 sizes every edge filter so that the samples one edge modifies are never read by another edge of the same
// direction, so a pass is embarrassingly parallel: one thread owns one 4-sample edge segment (one 4x4 unit),
// derives the edge decision from the two mode-info records either side of it and filters its four lines in
// registers.  The frame is two passes per plane — all vertical edges, then all horizontal edges — which is what
// the reference's superblock schedule (vert SB n, horz SB n-1) is equivalent to.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/svt_hip_lf.h"
#include "common.hpp"
#include "dlf_device.hpp"

using namespace svthip;
using namespace svthip::dlf;

namespace {

// All planes of a pass in one launch (blockIdx.z = plane): a pass over one 4K plane is a 10 - 15 us kernel, so six separate
// launches spend a good part of their time ramping up and draining.
struct LfPassArgs {
    LfGeom   g[3];
    LfLevels L[3];
};
template <int DIR>
__global__ __launch_bounds__(256) void dlf_pass_kernel(LfPassArgs a) {
    const LfGeom   &g = a.g[blockIdx.z];
    const LfLevels &L = a.L[blockIdx.z];
    // 64x4 thread tiles: consecutive lanes walk along x so that the horizontal-edge pass is fully coalesced
    const uint32_t ux = blockIdx.x * 64 + (threadIdx.x & 63), uy = blockIdx.y * 4 + (threadIdx.x >> 6);
    filter_unit_in_plane<DIR>(g, L, ux, uy);
}

template <typename T>
__global__ void lpf_leaf_kernel(T *s, int pitch, int vertical, int len, int blimit, int limit, int thresh, int bd) {
    if (threadIdx.x == 0)
        filter_segment(s, vertical ? (ptrdiff_t)1 : (ptrdiff_t)pitch, vertical ? (ptrdiff_t)pitch : (ptrdiff_t)1, len, blimit, limit, thresh, bd);
}

// Tier A: stage the samples the reference call touches (4 lines x 2*reach taps), run the leaf, copy them back.
template <typename T> void lpf_tier_a(T *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit, const uint8_t *thresh, int bd, int len, int vertical) {
    TierAStage      st("lpf");
    const int       reach = len == 4 ? 2 : (len == 6 ? 3 : (len == 8 ? 4 : 7));
    const ptrdiff_t first = vertical ? -reach : -(ptrdiff_t)reach * pitch;
    const ptrdiff_t last  = vertical ? 3 * (ptrdiff_t)pitch + reach : (ptrdiff_t)(reach - 1) * pitch + 4;  // one past
    const size_t    bytes = (size_t)(last - first) * sizeof(T), off = st.in(s + first, bytes);
    st.upload();
    hipLaunchKernelGGL(lpf_leaf_kernel<T>, dim3(1), dim3(64), 0, st.stream(), st.dev<T>(off) - first, (int)pitch, vertical, len, (int)*blimit,
                       (int)*limit, (int)*thresh, bd);
    st.finish(off, bytes);
    const T *h = st.host<T>(off);
    // write back only the taps of the four lines (the span in between belongs to the caller's other samples)
    for (int i = 0; i < 4; i++)
        for (int k = -reach; k < reach; k++) {
            const ptrdiff_t o = vertical ? i * (ptrdiff_t)pitch + k : k * (ptrdiff_t)pitch + i;
            s[o]              = h[o - first];
        }
}

}  // namespace

#define SVT_HIP_DEF_LPF(dir, n, vert)                                                                                              \
    extern "C" void svt_aom_lpf_##dir##_##n##_hip(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,          \
                                                  const uint8_t *thresh) {                                                         \
        TIER_A_CALL(svt_aom_lpf_##dir##_##n, lpf_tier_a<uint8_t>(s, pitch, blimit, limit, thresh, 8, n, vert), (s, pitch, blimit, limit, thresh)); \
    }                                                                                                                              \
    extern "C" void svt_aom_highbd_lpf_##dir##_##n##_hip(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,  \
                                                         const uint8_t *thresh, int32_t bd) {                                      \
        TIER_A_CALL(svt_aom_highbd_lpf_##dir##_##n, lpf_tier_a<uint16_t>(s, pitch, blimit, limit, thresh, bd, n, vert), (s, pitch, blimit, limit, thresh, bd)); \
    }
SVT_HIP_DEF_LPF(horizontal, 4, 0)
SVT_HIP_DEF_LPF(horizontal, 6, 0)
SVT_HIP_DEF_LPF(horizontal, 8, 0)
SVT_HIP_DEF_LPF(horizontal, 14, 0)
SVT_HIP_DEF_LPF(vertical, 4, 1)
SVT_HIP_DEF_LPF(vertical, 6, 1)
SVT_HIP_DEF_LPF(vertical, 8, 1)
SVT_HIP_DEF_LPF(vertical, 14, 1)

extern "C" int32_t svt_hip_loop_filter_frame(const SvtHipLfFrame *f, void *stream) {
    if (!frame_ok(f))
        return refuse("svt_hip_loop_filter_frame: bad argument");
    for (int p = f->plane_start; p < f->plane_end; p++)
        if (!f->plane[p] || !f->stride[p])
            return refuse("svt_hip_loop_filter_frame: missing plane");
    TierBCall c("svt_hip_loop_filter_frame", stream);
    if (!c.ok())
        return c.status();
    hipStream_t st = c.stream();
    LfPassArgs  a{};
    uint32_t    np = 0, gx = 0, gy = 0;
    for (int p = f->plane_start; p < f->plane_end; p++) {
        if (p == 0 && !f->filter_level[0] && !f->filter_level[1])
            break;  // deblocking_filter.c:570-572
        if ((p == 1 && !f->filter_level_u) || (p == 2 && !f->filter_level_v))
            continue;
        const LfGeom &g = a.g[np] = plane_geom(f, p);
        memcpy(a.L[np].lvl, f->lvl[p], sizeof(a.L[np].lvl));
        gx = (g.units_x + 63) / 64 > gx ? (g.units_x + 63) / 64 : gx;
        gy = (g.units_y + 3) / 4 > gy ? (g.units_y + 3) / 4 : gy;
        np++;
    }
    if (np) {  // vertical edges of every plane, then horizontal edges of every plane (the planes are independent)
        hipLaunchKernelGGL(dlf_pass_kernel<0>, dim3(gx, gy, np), dim3(256), 0, st, a);
        hipLaunchKernelGGL(dlf_pass_kernel<1>, dim3(gx, gy, np), dim3(256), 0, st, a);
    }
    return c.finish();
}

SVT_HIP_MODULE_WARMUP(loopfilter_dlf)
