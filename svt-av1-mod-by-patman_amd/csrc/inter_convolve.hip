// inter_convolve.hip — inter-prediction interpolation on gfx950: single-reference and compound.
// Replaces svt_av1_convolve_{2d_sr,x_sr,y_sr,2d_copy_sr}_c, svt_av1_jnt_convolve_{2d,x,y,2d_copy}_c and the highbd sets
// (inter_prediction.c:311-668, 670-1035).
// One workgroup per 64 x 64 tile of one predicted block: the tile and its filter margin are staged in LDS, the
// horizontal pass writes the int16 intermediate to LDS, the vertical pass writes the prediction.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/svt_hip_inter.h"
#include "common.hpp"
#include "convolve_device.hpp"

using namespace svthip;
using namespace svthip::conv;

namespace {

__global__ __launch_bounds__(256) void convolve_sr_kernel(const SvtHipConvolveDesc *__restrict__ descs) {
    __shared__ alignas(4) uint16_t in[(TILE + 7) * IP + CONV_IN_SLACK];
    __shared__ int16_t  im[(TILE + 7) * TILE];
    const SvtHipConvolveDesc d = descs[blockIdx.x];
    convolve_tile(d, (int)blockIdx.y, in, im);
}


// Tier A: stage the block and its margins, run the batch kernel on one descriptor, copy the prediction back.
void conv_tier_a(const void *src, int32_t src_stride, void *dst, int32_t dst_stride, int32_t w, int32_t h, const SvtHipInterpFilterParams *fx,
                 const SvtHipInterpFilterParams *fy, int32_t sx, int32_t sy, const SvtHipConvolveParams *cp, int use_x, int use_y, int is16, int bd,
                 int compound = 0) {
    TierAStage s("convolve_sr");
    if (w < 1 || h < 1 || w > 128 || h > 128 || (use_x && (!fx || fx->taps > 8 || (fx->taps & 1))) || (use_y && (!fy || fy->taps > 8 || (fy->taps & 1)))) {
        set_error("convolve_sr: unsupported block %dx%d / filter", w, h);
        fatal("convolve_sr");
    }
    const int    px = is16 ? 2 : 1, tx = use_x ? fx->taps : 0, ty = use_y ? fy->taps : 0;
    const int    fo_h = tx ? tx / 2 - 1 : 0, fo_v = ty ? ty / 2 - 1 : 0, ew = w + (tx ? tx - 1 : 0), eh = h + (ty ? ty - 1 : 0);
    // [block + filter margins, packed][prediction, packed][descriptor][compound buffer, packed]
    const size_t o_in = s.in_rows((const uint8_t *)src - ((ptrdiff_t)fo_v * src_stride + fo_h) * px, (size_t)src_stride * px, eh, (size_t)ew * px);
    const size_t o_out = s.out((size_t)w * h * px), o_desc = s.out(256), o_cb = s.out((size_t)w * h * 2);
    SvtHipConvolveDesc ds{};
    ds.src = s.dev(o_in) + ((size_t)fo_v * ew + fo_h) * px, ds.dst = s.dev(o_out), ds.src_stride = (uint32_t)ew, ds.dst_stride = (uint32_t)w;
    ds.w = (uint16_t)w, ds.h = (uint16_t)h, ds.taps_x = (uint8_t)tx, ds.taps_y = (uint8_t)ty;
    if (tx)
        memcpy(ds.filter_x, fx->filter_ptr + (size_t)fx->taps * (sx & 15), sizeof(int16_t) * tx);  // av1_get_interp_filter_subpel_kernel
    if (ty)
        memcpy(ds.filter_y, fy->filter_ptr + (size_t)fy->taps * (sy & 15), sizeof(int16_t) * ty);
    ds.round_0 = (uint8_t)cp->round_0, ds.round_1 = (uint8_t)cp->round_1, ds.bit_depth = (uint8_t)bd, ds.is_16bit = (uint8_t)is16;
    // compound: the ConvBufType block sits behind the descriptor in the same staging buffers
    uint16_t *cb_host = compound ? (uint16_t *)cp->dst : nullptr;
    if (compound) {
        if (!cb_host) {
            set_error("jnt_convolve: conv_params->dst is NULL");
            fatal("jnt_convolve");
        }
        ds.compound    = cp->do_average ? (cp->use_jnt_comp_avg ? 3 : 2) : 1;
        ds.fwd_offset  = (uint8_t)cp->fwd_offset, ds.bck_offset = (uint8_t)cp->bck_offset;
        ds.cbuf        = s.dev<uint16_t>(o_cb), ds.cbuf_stride = (uint32_t)w;
        if (cp->do_average)
            copy_rows(s.host(o_cb), (size_t)w * 2, cb_host, (size_t)cp->dst_stride * 2, h, (size_t)w * 2);
    }
    memcpy(s.host(o_desc), &ds, sizeof(ds));
    s.h2d(o_in, (size_t)ew * eh * px);
    s.h2d(o_desc, compound && cp->do_average ? o_cb + (size_t)w * h * 2 - o_desc : 256);
    if (svt_hip_convolve_batch(s.dev<const SvtHipConvolveDesc>(o_desc), 1, s.stream()) != SVT_HIP_OK)
        fatal("convolve");
    if (compound && !cp->do_average) {
        s.finish(o_cb, (size_t)w * h * 2);
        s.out_rows(cb_host, (size_t)cp->dst_stride * 2, o_cb, h, (size_t)w * 2);
        return;
    }
    s.finish(o_out, (size_t)w * h * px);
    s.out_rows(dst, (size_t)dst_stride * px, o_out, h, (size_t)w * px);
}

}  // namespace

extern "C" int32_t svt_hip_convolve_sr_batch(const SvtHipConvolveDesc *d_desc, uint32_t n, void *stream) {
    return svt_hip_convolve_batch(d_desc, n, stream);
}
extern "C" int32_t svt_hip_convolve_batch(const SvtHipConvolveDesc *d_desc, uint32_t n, void *stream) {
    if (!d_desc || n == 0)
        return refuse("svt_hip_convolve_batch: bad argument");
    TierBCall c("svt_hip_convolve_batch", stream);
    if (!c.ok())
        return c.status();
    hipLaunchKernelGGL(convolve_sr_kernel, dim3(n, 4), dim3(256), 0, c.stream(), d_desc);
    return c.finish();
}

#define SVT_HIP_DEF_CONV(mode, UX, UY)                                                                                          \
    extern "C" void svt_av1_convolve_##mode##_hip(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride,      \
                                                  int32_t w, int32_t h, SvtHipInterpFilterParams *fx, SvtHipInterpFilterParams *fy, \
                                                  const int32_t sx, const int32_t sy, SvtHipConvolveParams *cp) {               \
        TIER_A_CALL(svt_av1_convolve_##mode, conv_tier_a(src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp, UX, UY, 0, 8), (src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp)); \
    }                                                                                                                            \
    extern "C" void svt_av1_highbd_convolve_##mode##_hip(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride, \
                                                         int32_t w, int32_t h, const SvtHipInterpFilterParams *fx,              \
                                                         const SvtHipInterpFilterParams *fy, const int32_t sx, const int32_t sy, \
                                                         SvtHipConvolveParams *cp, int32_t bd) {                                \
        TIER_A_CALL(svt_av1_highbd_convolve_##mode, conv_tier_a(src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp, UX, UY, 1, bd), (src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp, bd)); \
    }
SVT_HIP_DEF_CONV(2d_sr, 1, 1)
SVT_HIP_DEF_CONV(x_sr, 1, 0)
SVT_HIP_DEF_CONV(y_sr, 0, 1)
SVT_HIP_DEF_CONV(2d_copy_sr, 0, 0)


#define SVT_HIP_DEF_JNT(mode, UX, UY)                                                                                           \
    extern "C" void svt_av1_jnt_convolve_##mode##_hip(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride,  \
                                                      int32_t w, int32_t h, SvtHipInterpFilterParams *fx, SvtHipInterpFilterParams *fy, \
                                                      const int32_t sx, const int32_t sy, SvtHipConvolveParams *cp) {           \
        TIER_A_CALL(svt_av1_jnt_convolve_##mode, conv_tier_a(src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp, UX, UY, 0, 8, 1), (src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp)); \
    }                                                                                                                            \
    extern "C" void svt_av1_highbd_jnt_convolve_##mode##_hip(const uint16_t *src, int32_t src_stride, uint16_t *dst,            \
                                                             int32_t dst_stride, int32_t w, int32_t h,                          \
                                                             const SvtHipInterpFilterParams *fx, const SvtHipInterpFilterParams *fy, \
                                                             const int32_t sx, const int32_t sy, SvtHipConvolveParams *cp, int32_t bd) { \
        TIER_A_CALL(svt_av1_highbd_jnt_convolve_##mode, conv_tier_a(src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp, UX, UY, 1, bd, 1), (src, src_stride, dst, dst_stride, w, h, fx, fy, sx, sy, cp, bd)); \
    }
SVT_HIP_DEF_JNT(2d, 1, 1)
SVT_HIP_DEF_JNT(x, 1, 0)
SVT_HIP_DEF_JNT(y, 0, 1)
SVT_HIP_DEF_JNT(2d_copy, 0, 0)

SVT_HIP_MODULE_WARMUP(inter_convolve)
