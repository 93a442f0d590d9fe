// inter_scale.hip — inter prediction from a reference of another size on gfx950 (include/svt_hip_scale.h).
// Replaces svt_av1_convolve_2d_scale_c and svt_av1_highbd_convolve_2d_scale_c (inter_prediction.c:420-492, 779-850), and holds the
// host arithmetic around them: svt_av1_setup_scale_factors_for_frame, the scaled branch of compute_subpel_params and
// calculate_scaled_size_helper.
// Tiled as inter_convolve.hip: one workgroup per 64 x 64 output tile, 2 x 2 tiles per block.  A tile's rows reach over up to
// ((63 * 2048 + 1023) >> 10) + 8 = 134 rows of the horizontal pass at the largest step; that intermediate sits in LDS (17 KB).  The
// horizontal pass reads the reference plane itself: neighbouring lanes are x_step_qn / 1024 <= 2 samples apart, so a wave's eight taps
// fall into the same few cache lines, and a staged copy of the up to 134 x 134 source samples would take the LDS of two more workgroups.
// Both filter tables sit in LDS as [16][8], zero-padded: the phase differs per sample.
#include "../../include/svt_hip_scale.h"
#include "common.hpp"
#include "convolve_device.hpp"

using namespace svthip;
using namespace svthip::conv;

namespace {

constexpr int SCALE_SUBPEL_BITS = 10, SCALE_SUBPEL_MASK = (1 << SCALE_SUBPEL_BITS) - 1, SCALE_EXTRA_BITS = 6, SUBPEL_SHIFTS = 16;
constexpr int IM_ROWS = (((TILE - 1) * 2048 + SCALE_SUBPEL_MASK) >> SCALE_SUBPEL_BITS) + 8;  // 134

__global__ __launch_bounds__(256) void convolve_scale_kernel(const SvtHipConvolveScaleDesc *__restrict__ descs) {
    __shared__ int16_t             im[IM_ROWS * TILE];
    __shared__ alignas(16) int16_t ftab[2][SUBPEL_SHIFTS * 8];
    const SvtHipConvolveScaleDesc  d = descs[blockIdx.x];
    if (d.w == 0 || d.h == 0)
        return;
    const int tiles_x = (d.w + TILE - 1) / TILE, tile = (int)blockIdx.y;
    const int x0 = (tile % tiles_x) * TILE, y0 = (tile / tiles_x) * TILE;
    if (y0 >= d.h)
        return;
    const int tw = min(TILE, d.w - x0), th = min(TILE, d.h - y0);
    const int tx = d.taps_x, ty = d.taps_y, is16 = d.is_16bit, bd = d.bit_depth, r0 = d.round_0, r1 = d.round_1;
    const int fo_h = tx / 2 - 1, fo_v = ty / 2 - 1, xs = d.x_step_qn, ys = d.y_step_qn;
    // rows of the horizontal pass this tile's outputs read: im_block rows first .. first + rows - 1 of the reference
    const int first = (d.subpel_y_qn + y0 * ys) >> SCALE_SUBPEL_BITS;
    const int rows  = ((d.subpel_y_qn + (y0 + th - 1) * ys) >> SCALE_SUBPEL_BITS) - first + ty;
    if (tx > 8 || ty > 8 || rows > IM_ROWS || rows < ty)  // descriptors are not validated: nothing outside the LDS arrays in any case
        return;
    {
        const int      t = threadIdx.x >> 7, i = threadIdx.x & 127, n = t ? ty : tx;  // 128 threads per table
        const int16_t *g = t ? d.filter_y : d.filter_x;
        ftab[t][i]       = (i & 7) < n ? g[(i >> 3) * n + (i & 7)] : (int16_t)0;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < rows * tw; idx += 256) {
        const int       r = idx / tw, c = idx - r * tw;
        const int       x_qn = d.subpel_x_qn + (x0 + c) * xs;
        const ptrdiff_t at0  = (ptrdiff_t)(first + r - fo_v) * d.src_stride + (x_qn >> SCALE_SUBPEL_BITS) - fo_h;
        const int32_t   sum  = tap_sum(&ftab[0][((x_qn & SCALE_SUBPEL_MASK) >> SCALE_EXTRA_BITS) * 8], tx, 1 << (bd + FILTER_BITS - 1),
                                       [&](int k) { return ldpx(d.src, at0 + k, is16); });
        im[r * TILE + c]     = (int16_t)rnd(sum, r0);
    }
    __syncthreads();
    const int     offset_bits = bd + 2 * FILTER_BITS - r0, bits = 2 * FILTER_BITS - r0 - r1;
    const int32_t round_offset = (1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1));
    for (int idx = threadIdx.x; idx < th * tw; idx += 256) {
        const int      r = idx / tw, c = idx - r * tw;
        const int      y_qn = d.subpel_y_qn + (y0 + r) * ys;
        const int16_t *col  = im + ((y_qn >> SCALE_SUBPEL_BITS) - first) * TILE + c;
        const int32_t  sum  = tap_sum(&ftab[1][((y_qn & SCALE_SUBPEL_MASK) >> SCALE_EXTRA_BITS) * 8], ty, 1 << offset_bits,
                                      [&](int k) { return (int32_t)col[k * TILE]; });
        const int32_t  res  = (uint16_t)rnd(sum, r1);  // ConvBufType
        if (d.compound)
            comp_out(d, y0 + r, x0 + c, res, round_offset, bits);
        else
            stpx(d.dst, (size_t)(y0 + r) * d.dst_stride + x0 + c, is16, rnd(res - round_offset, bits), bd);
    }
}

int32_t clamp32(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// scaled_x / scaled_y (inter_prediction.c:154-165): val in 1/16 sample, the result in 1/1024
int32_t scaled(int32_t val, int32_t scale_fp) {
    const int32_t off  = (scale_fp - (1 << 14)) * (1 << 3);
    const int64_t tval = (int64_t)val * scale_fp + off;
    return (int32_t)(tval < 0 ? -((-tval + (1 << 7)) >> 8) : (tval + (1 << 7)) >> 8);  // ROUND_POWER_OF_TWO_SIGNED_64(tval, 14 - 6)
}

}  // namespace

extern "C" intptr_t svt_hip_convolve_scale_batch(const SvtHipConvolveScaleDesc *d_desc, uint32_t n, void *stream) {
    if (!d_desc)
        return SVT_HIP_SCALE_STATUS(refuse("svt_hip_convolve_scale_batch: NULL argument"));
    if (n == 0)
        return SVT_HIP_SCALE_STATUS(SVT_HIP_OK);
    TierBCall c("svt_hip_convolve_scale_batch", stream);
    if (!c.ok())
        return SVT_HIP_SCALE_STATUS(c.status());
    hipLaunchKernelGGL(convolve_scale_kernel, dim3(n, 4), dim3(256), 0, c.stream(), d_desc);
    return SVT_HIP_SCALE_STATUS(c.finish());
}

extern "C" void svt_hip_scale_factors(int32_t other_w, int32_t other_h, int32_t this_w, int32_t this_h, SvtHipScaleFactors *out) {
    if (!out)
        return;
    // valid_ref_frame_size (inter_prediction.h:174); a size below 1 would divide by zero in the reference
    if (other_w < 1 || other_h < 1 || this_w < 1 || this_h < 1 || 2 * (int64_t)this_w < other_w || 2 * (int64_t)this_h < other_h ||
        this_w > 16 * (int64_t)other_w || this_h > 16 * (int64_t)other_h) {
        out->x_scale_fp = out->y_scale_fp = SVT_HIP_SCALE_INVALID;
        return;
    }
    out->x_scale_fp = (int32_t)((((int64_t)other_w << 14) + this_w / 2) / this_w);  // get_fixed_point_scale_factor
    out->y_scale_fp = (int32_t)((((int64_t)other_h << 14) + this_h / 2) / this_h);
    out->x_step_q4  = (out->x_scale_fp + (1 << 3)) >> 4;  // fixed_point_scale_to_coarse_point_scale
    out->y_step_q4  = (out->y_scale_fp + (1 << 3)) >> 4;
}

extern "C" void svt_hip_scaled_block_position(const SvtHipScaleFactors *sf, int32_t pre_x, int32_t pre_y, int32_t mv_col, int32_t mv_row, uint32_t ss_x,
                                              uint32_t ss_y, uint32_t frame_width, uint32_t frame_height, uint32_t sb_size, SvtHipScaledPosition *out) {
    if (!sf || !out)
        return;
    ss_x = ss_x ? 1 : 0, ss_y = ss_y ? 1 : 0;
    const int32_t orig_y = pre_y * 16 + mv_row * (1 << (1 - ss_y)), orig_x = pre_x * 16 + mv_col * (1 << (1 - ss_x));  // SUBPEL_BITS 4
    int32_t       pos_y = scaled(orig_y, sf->y_scale_fp) + 32, pos_x = scaled(orig_x, sf->x_scale_fp) + 32;             // SCALE_EXTRA_OFF
    // the padding of a scaled reference is 2 * sb_size + 32; INTERPOLATION_OFFSET 8 left and above, AOM_INTERP_EXTEND 4 right and below
    const int32_t border = (int32_t)sb_size * 2 + 32;
    const int32_t top = -(((border >> ss_y) - 8) << SCALE_SUBPEL_BITS), left = -(((border >> ss_x) - 8) << SCALE_SUBPEL_BITS);
    const int32_t bottom = (int32_t)((frame_height >> ss_y) + 4) << SCALE_SUBPEL_BITS, right = (int32_t)((frame_width >> ss_x) + 4) << SCALE_SUBPEL_BITS;
    pos_y         = clamp32(pos_y, top, bottom);
    pos_x         = clamp32(pos_x, left, right);
    out->subpel_x = pos_x & SCALE_SUBPEL_MASK, out->subpel_y = pos_y & SCALE_SUBPEL_MASK;
    out->xs = sf->x_step_q4, out->ys = sf->y_step_q4;
    out->pos_x = pos_x >> SCALE_SUBPEL_BITS, out->pos_y = pos_y >> SCALE_SUBPEL_BITS;
}

extern "C" void svt_hip_scaled_size(uint16_t *dim, uint8_t denom) {
    if (!dim)
        return;
    if (denom != 8 && denom <= 16 && denom) {  // SCALE_NUMERATOR, SCALE_DENOMINATOR_MAX; 0 would divide by zero in the reference
        const int min_dim = *dim < 16 ? *dim : 16;
        const int scaled  = (uint16_t)((*dim * 8 + denom / 2) / denom);
        *dim              = (uint16_t)(scaled > min_dim ? scaled : min_dim);
    } else if (denom == 17) {  // SCALE_THREE_QUATER
        *dim = (uint16_t)((3 + *dim * 3) >> 2);
    }
}

SVT_HIP_MODULE_WARMUP(inter_scale)
