// loopfilter_resize.hip — picture resizing and the normative super-res upscaler on gfx950 (include/svt_hip_scale.h).
// Replaces svt_av1_resize_plane_c / svt_av1_resize_plane_horizontal with their highbd twins (resize.c:399-460, 679-760) and
// svt_av1_upscale_normative_rows (super_res.c:214) for device-resident planes.
//
// Resizing is resize_multistep along the rows and then along the columns of the clipped intermediate: one launch per direction, all
// planes of a call in both.  One lane computes one output sample; lanes run along the memory rows in both passes, so in the column
// pass a wave's loads and stores are contiguous too.  The chosen bank sits in LDS (the phase differs per lane in the row pass).
//
// ONE CLAMPED FORM.  The reference writes every filter three times: an initial part that clamps the tap index at 0, a middle part
// that clamps nothing and an end part that clamps at length - 1, and beside them a "short input" form that clamps at both ends.  Here
// every tap index is clamped to [0, length - 1].  That is the same sum because the parts are split where the clamp they leave out
// cannot act:
//   svt_av1_interpolate_core_c: x1 is the first output whose leftmost tap (int_pel - 3) is >= 0, x2 the last whose rightmost tap
//   (int_pel + 4) is < in_length, and int_pel never decreases with x.  The three-part form runs only when x1 <= x2: an initial
//   output x < x1 <= x2 has int_pel(x) <= int_pel(x2), so its rightmost tap is in range; an end output x > x2 >= x1 has
//   int_pel(x) >= int_pel(x1), so its leftmost tap is in range; the middle has both.  With x1 > x2 the reference clamps both ends itself.
//   svt_av1_down2_symeven_c / down2_symodd: l1 and l2 are even, the initial part has i <= l2 - 2 <= length - 5 (symeven, taps up to
//   i + 4) or <= length - 4 (symodd, taps up to i + 3), the end part has i >= l1 = 4 (taps down to i - 3); l1 > l2 clamps both ends.
#include <algorithm>

#include "../../include/svt_hip_scale.h"
#include "common.hpp"
#include "resize_device.hpp"

using namespace svthip;
using namespace svthip::resize;
using svthip::conv::ldpx;
using svthip::conv::rnd;
using svthip::conv::stpx;

namespace {

constexpr uint32_t MAX_DIM = 16384;  // (length << 14) and x * delta stay inside int32, as the reference needs them to

// resize_multistep of one axis, planned on the host: no division on the device
struct Axis {
    int32_t in_len, mid_len, out_len;  // mid_len: what the interpolation reads (after the halving, if there is one)
    int32_t delta, offset;             // svt_av1_interpolate_core_c(mid_len -> out_len)
    uint8_t halve;                     // 0 none, 1 svt_av1_down2_symeven_c, 2 down2_symodd
    uint8_t interp;                    // 0: the output is the (halved) input sample
    uint8_t bank, pad_;
};

struct Pass {
    const void *src;
    void       *dst;
    uint32_t    src_step, src_line, dst_step, dst_line;  // in samples: along the axis, and from one line to the next
    uint32_t    lines;                                   // 0: the plane takes no part in this pass
    Axis        axis;
    uint8_t     is16, bd, vertical, pad_;
};
struct PassArgs {
    Pass p[SVT_HIP_SCALE_MAX_PLANES];
};

__constant__ const int16_t DOWN2_SYMEVEN[4] = {56, 12, -3, -1}, DOWN2_SYMODD[4] = {64, 35, 0, -3};  // the half filters (resize.c:29-30)

__device__ __forceinline__ int32_t clip_bd(int32_t v, int bd) {
    const int32_t hi = (1 << bd) - 1;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

// sample j of the halved line: taps around input sample 2 j, indices clamped to [0, len - 1]
template <class At>
__device__ __forceinline__ int32_t halved(int halve, int j, int len, int bd, At at) {
    const int i   = 2 * j;
    int32_t   sum = 1 << (FILTER_BITS - 1);
    if (halve == 1) {
#pragma unroll
        for (int t = 0; t < 4; t++) sum += (at(max(i - t, 0)) + at(min(i + 1 + t, len - 1))) * DOWN2_SYMEVEN[t];
    } else {
        sum += at(i) * DOWN2_SYMODD[0];
#pragma unroll
        for (int t = 1; t < 4; t++) sum += (at(max(i - t, 0)) + at(min(i + t, len - 1))) * DOWN2_SYMODD[t];
    }
    return clip_bd(sum >> FILTER_BITS, bd);
}

// blockIdx: (64 samples along the memory rows, 4 memory rows, plane)
__global__ __launch_bounds__(256) void resize_pass_kernel(const PassArgs args) {
    __shared__ alignas(16) int16_t taps[BANK_ELEMS];
    const Pass    &p  = args.p[blockIdx.z];
    const Axis    &a  = p.axis;
    const uint32_t nx = p.vertical ? p.lines : (uint32_t)a.out_len, ny = p.vertical ? (uint32_t)a.out_len : p.lines;
    if (!p.lines || blockIdx.x * 64 >= nx || blockIdx.y * 4 >= ny)  // the grid is that of the largest plane
        return;
    if (a.interp) {
        stage_bank<256>(a.bank, taps);
        __syncthreads();
    }
    const uint32_t cx = blockIdx.x * 64 + (threadIdx.x & 63), cy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cx >= nx || cy >= ny)
        return;
    const int       pos = (int)(p.vertical ? cy : cx), is16 = p.is16, bd = p.bd, halve = a.halve;
    const ptrdiff_t line = p.vertical ? cx : cy, in0 = line * (ptrdiff_t)p.src_line, step = p.src_step;
    const void     *src  = p.src;
    const auto      at   = [&](int i) { return ldpx(src, in0 + i * step, is16); };
    const auto      mid  = [&](int i) { return halve ? halved(halve, i, a.in_len, bd, at) : at(i); };
    int32_t         v;
    if (a.interp) {
        const int32_t y = a.offset + (1 << 7) + pos * a.delta;  // RS_SCALE_EXTRA_OFF; phase (y >> 8) & 63
        v = clip_bd(rnd(filter8_clamped(taps + ((y >> 8) & (PHASES - 1)) * TAPS, (y >> 14) - (TAPS / 2 - 1), a.mid_len - 1, mid), FILTER_BITS), bd);
    } else {
        v = mid(pos);
    }
    stpx(p.dst, (size_t)(line * (ptrdiff_t)p.dst_line + (ptrdiff_t)pos * p.dst_step), is16, v, 16);
}

// ---- super-res ------------------------------------------------------------------------------------------------------------
struct SrCol {  // one tile column, from the host
    int32_t x0_qn, up_x0, down_x0, pad_;
};
struct SrPlane {
    const void *src;
    void       *dst;
    uint32_t    src_stride, dst_stride, rows, up_width;
    int32_t     step, last;  // x_step_qn; the last column a tap may read
    uint16_t    col_base, n_cols;
    uint8_t     is16, bd, pad_[2];
};
struct SrArgs {
    SrPlane p[SVT_HIP_SCALE_MAX_PLANES];
};

// blockIdx: (256 output samples, row, plane)
__global__ __launch_bounds__(256) void superres_kernel(const SrArgs args, const SrCol *__restrict__ cols) {
    __shared__ alignas(16) int16_t taps[BANK_ELEMS];
    __shared__ SrCol               col[SVT_HIP_SCALE_MAX_TILE_COLS];
    const SrPlane &p = args.p[blockIdx.z];
    if (blockIdx.x * 256 >= p.up_width || blockIdx.y >= p.rows)
        return;
    stage_bank<256>(0, taps);
    if (threadIdx.x < p.n_cols)
        col[threadIdx.x] = cols[p.col_base + threadIdx.x];
    __syncthreads();
    const int x = (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= (int)p.up_width)
        return;
    int j = 0;  // the tile column of x: the last one that starts at or before it
    for (int k = 1; k < p.n_cols; k++) j = x >= col[k].up_x0 ? k : j;
    const int32_t   x_qn = col[j].x0_qn + (x - col[j].up_x0) * p.step;
    const int       is16 = p.is16;
    const ptrdiff_t row  = (ptrdiff_t)blockIdx.y * p.src_stride;
    const void     *src  = p.src;
    const auto      at   = [&](int i) { return ldpx(src, row + i, is16); };
    const int32_t   sum  = filter8_clamped(taps + ((x_qn & 16383) >> 8) * TAPS, col[j].down_x0 + (x_qn >> 14) - TAPS / 2, p.last, at);
    stpx(p.dst, (size_t)blockIdx.y * p.dst_stride + x, is16, rnd(sum, FILTER_BITS), p.bd);
}

intptr_t widen(int32_t status) { return SVT_HIP_SCALE_STATUS(status); }

const char *bad_samples(uint8_t is_16bit, uint8_t bit_depth) {
    if (is_16bit > 1)
        return "is_16bit above 1";
    if (bit_depth != 8 && (!is_16bit || (bit_depth != 10 && bit_depth != 12)))
        return "bit depth not 8 (uint8 samples) or 8 / 10 / 12 (uint16 samples)";
    return nullptr;
}

// false: the axis needs two or more halvings (get_down2_steps, resize.c:149)
bool plan_axis(uint32_t in, uint32_t out, Axis &a) {
    a = Axis{(int32_t)in, (int32_t)in, (int32_t)out, 0, 0, 0, 0, 0, 0};
    if (in == out)
        return true;
    uint32_t steps = 0, len = in, proj;
    while ((proj = (len + 1) >> 1) >= out) {
        steps++, len = proj;
        if (len == 1)
            break;
    }
    if (steps > 1)
        return false;
    if (steps)
        a.halve = in & 1 ? 2 : 1, a.mid_len = (int32_t)len;
    a.interp = (uint32_t)a.mid_len != out;
    if (a.interp) {
        const int32_t m = a.mid_len, o = (int32_t)out;
        a.delta  = (int32_t)((((uint32_t)m << 14) + out / 2) / out);
        a.offset = m > o ? (((m - o) << 13) + o / 2) / o : -(((o - m) << 13) + o / 2) / o;
        a.bank   = (uint8_t)choose_bank(m, o);
    }
    return true;
}

const char *bad_resize_plane(const SvtHipResizePlane &p, Axis &ax, Axis &ay) {
    if (!p.src || !p.dst)
        return "NULL plane";
    if (!p.src_width || !p.src_height || !p.dst_width || !p.dst_height)
        return "empty plane";
    if (std::max(std::max(p.src_width, p.src_height), std::max(p.dst_width, p.dst_height)) > MAX_DIM)
        return "plane larger than 16384";
    if (p.src_stride < p.src_width || p.dst_stride < p.dst_width)
        return "stride smaller than the width";
    if (const char *why = bad_samples(p.is_16bit, p.bit_depth))
        return why;
    if (!plan_axis(p.src_width, p.dst_width, ax) || !plan_axis(p.src_height, p.dst_height, ay))
        return "two or more halvings on an axis";
    return nullptr;
}

// the intermediate of a plane that resizes both axes
uint64_t plane_workspace(const SvtHipResizePlane &p) {
    return p.src_width != p.dst_width && p.src_height != p.dst_height ? up256((uint64_t)p.dst_width * p.src_height * (p.is_16bit ? 2 : 1)) : 0;
}

}  // namespace

extern "C" size_t svt_hip_resize_workspace_bytes(const SvtHipResizePlane *planes, uint32_t n) {
    size_t need = 0;
    for (uint32_t i = 0; planes && i < n; i++) need += plane_workspace(planes[i]);
    return need;
}

extern "C" intptr_t svt_hip_resize_planes(const SvtHipResizePlane *planes, uint32_t n, void *d_workspace, size_t workspace_bytes, void *stream) {
    static const char *const fn = "svt_hip_resize_planes";
    if (!planes)
        return widen(refuse("%s: NULL argument", fn));
    if (n > SVT_HIP_SCALE_MAX_PLANES)
        return widen(refuse("%s: %u planes, at most %d a call", fn, n, SVT_HIP_SCALE_MAX_PLANES));
    if (n == 0)
        return widen(SVT_HIP_OK);
    PassArgs rows = {}, cols = {};
    uint64_t need = 0;
    uint32_t rx = 0, ry = 0, cx = 0, cy = 0;  // the grids' extents in samples
    for (uint32_t i = 0; i < n; i++) {
        const SvtHipResizePlane &p = planes[i];
        Axis                     ax, ay;
        if (const char *why = bad_resize_plane(p, ax, ay))
            return widen(refuse("%s: plane %u: %s (%u x %u, stride %u -> %u x %u, stride %u, %u bit)", fn, i, why, p.src_width, p.src_height, p.src_stride,
                                 p.dst_width, p.dst_height, p.dst_stride, p.bit_depth));
        const bool  vert = p.src_height != p.dst_height, horz = p.src_width != p.dst_width || !vert;
        void *const mid  = horz && vert ? (uint8_t *)d_workspace + need : nullptr;
        need += plane_workspace(p);
        if (horz) {
            rows.p[i] = Pass{p.src, vert ? mid : p.dst, 1, p.src_stride, 1, vert ? p.dst_width : p.dst_stride, p.src_height, ax, p.is_16bit, p.bit_depth, 0, 0};
            rx = std::max(rx, p.dst_width), ry = std::max(ry, p.src_height);
        }
        if (vert) {
            cols.p[i] = Pass{horz ? mid : p.src, p.dst, horz ? p.dst_width : p.src_stride, 1, p.dst_stride, 1, p.dst_width, ay, p.is_16bit, p.bit_depth, 1, 0};
            cx = std::max(cx, p.dst_width), cy = std::max(cy, p.dst_height);
        }
    }
    if (need && (!d_workspace || ((uintptr_t)d_workspace & 255) || workspace_bytes < need))
        return widen(refuse("%s: workspace %p of %llu bytes, %llu needed, 256-byte aligned", fn, d_workspace, (unsigned long long)workspace_bytes,
                             (unsigned long long)need));
    TierBCall c(fn, stream);
    if (!c.ok())
        return widen(c.status());
    if (rx)
        hipLaunchKernelGGL(resize_pass_kernel, dim3((rx + 63) / 64, (ry + 3) / 4, n), dim3(256), 0, c.stream(), rows);
    if (cx)
        hipLaunchKernelGGL(resize_pass_kernel, dim3((cx + 63) / 64, (cy + 3) / 4, n), dim3(256), 0, c.stream(), cols);
    return widen(c.finish());
}

extern "C" intptr_t svt_hip_superres_upscale_planes(const SvtHipSuperresPlane *planes, uint32_t n, void *stream) {
    static const char *const fn = "svt_hip_superres_upscale_planes";
    if (!planes)
        return widen(refuse("%s: NULL argument", fn));
    if (n > SVT_HIP_SCALE_MAX_PLANES)
        return widen(refuse("%s: %u planes, at most %d a call", fn, n, SVT_HIP_SCALE_MAX_PLANES));
    if (n == 0)
        return widen(SVT_HIP_OK);
    SrArgs   args = {};
    SrCol    cols[SVT_HIP_SCALE_MAX_PLANES * SVT_HIP_SCALE_MAX_TILE_COLS];
    uint32_t n_cols = 0, max_w = 0, max_rows = 0;
    for (uint32_t i = 0; i < n; i++) {
        const SvtHipSuperresPlane &p   = planes[i];
        const char                *why = nullptr;
        if (!p.src || !p.dst)
            why = "NULL plane";
        else if (!p.rows || !p.frame_width)
            why = "empty plane";
        else if (p.superres_upscaled_width < p.frame_width)
            why = "upscaled width below the frame width";
        else if (p.superres_denominator < 8 || p.superres_denominator > 16)
            why = "denominator outside 8 .. 16";
        else if (p.sub_x > 1)
            why = "sub_x above 1";
        else if (!(why = bad_samples(p.is_16bit, p.bit_depth)) && (p.tile_cols < 1 || p.tile_cols > SVT_HIP_SCALE_MAX_TILE_COLS))
            why = "tile_cols outside 1 .. 64";
        for (uint32_t j = 0; !why && j < p.tile_cols; j++)
            if (p.tile_col_start_mi[0] != 0 || p.tile_col_start_mi[j + 1] <= p.tile_col_start_mi[j])
                why = "tile column starts do not increase from 0";
        // svt_av1_upscale_normative_rows, per tile column
        const int32_t down_w = (p.frame_width + p.sub_x) >> p.sub_x, up_w = (p.superres_upscaled_width + p.sub_x) >> p.sub_x;
        const int32_t denom = p.superres_denominator, shift = 2 - p.sub_x;  // MI_SIZE_LOG2 - sub_x
        const int32_t last  = why ? 0 : ((int32_t)p.tile_col_start_mi[p.tile_cols] << shift);
        if (!why && (p.src_stride < (uint32_t)last || p.dst_stride < (uint32_t)up_w))
            why = "stride smaller than the width";
        if (why)
            return widen(refuse("%s: plane %u: %s (frame %u -> %u, denominator %u, %u rows, strides %u and %u, %u tile columns, %u bit)", fn, i, why,
                                 p.frame_width, p.superres_upscaled_width, p.superres_denominator, p.rows, p.src_stride, p.dst_stride, p.tile_cols, p.bit_depth));
        const int32_t step = ((down_w << 14) + up_w / 2) / up_w;                      // av1_get_upscale_convolve_step
        const int32_t err  = up_w * step - (down_w << 14);                             // get_upscale_convolve_x0
        int32_t       x0_qn = (int32_t)((uint32_t)((-((up_w - down_w) << 13) + up_w / 2) / up_w + (1 << 7) - err / 2) & 16383u);
        args.p[i] = SrPlane{p.src, p.dst, p.src_stride, p.dst_stride, p.rows, (uint32_t)up_w, step, last - 1, (uint16_t)n_cols, p.tile_cols, p.is_16bit, p.bit_depth, {0, 0}};
        for (uint32_t j = 0; j < p.tile_cols; j++) {
            const int32_t down_x0 = (int32_t)p.tile_col_start_mi[j] << shift, down_x1 = (int32_t)p.tile_col_start_mi[j + 1] << shift;
            const int32_t up_x0 = down_x0 * denom / 8, up_x1 = j + 1 == p.tile_cols ? up_w : down_x1 * denom / 8;
            cols[n_cols++] = SrCol{x0_qn, up_x0, down_x0, 0};
            x0_qn += (up_x1 - up_x0) * step - ((down_x1 - down_x0) << 14);
        }
        max_w = std::max(max_w, (uint32_t)up_w), max_rows = std::max(max_rows, p.rows);
    }
    if (max_rows > 65535)
        return widen(refuse("%s: %u rows, at most 65535", fn, max_rows));
    TierBCall    c(fn, stream);
    const SrCol *d_cols = (const SrCol *)c.stage(cols, n_cols * sizeof(SrCol));
    if (!c.ok())
        return widen(c.status());
    hipLaunchKernelGGL(superres_kernel, dim3((max_w + 255) / 256, max_rows, n), dim3(256), 0, c.stream(), args, d_cols);
    return widen(c.finish());
}

SVT_HIP_MODULE_WARMUP(loopfilter_resize)
