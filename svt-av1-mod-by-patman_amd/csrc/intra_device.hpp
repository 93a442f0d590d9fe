// intra_device.hpp — 8-bit luma intra predictors of the open-loop (source-based) search as __device__ functions over above / left
// edge arrays: the neighbour gather, the DC family, V, H, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH, the directional zones z1 / z2 / z3, the
// intra edge filter with its strength rule and the corner filter.  Paths relative to the reference's Source/Lib/Codec:
//   neighbours          svt_aom_update_neighbor_samples_array_open_loop_mb   enc_intra_prediction.c:1127-1212
//   filter_edges        filter_intra_edge (the 16x16 geometry of the open-loop search) intra_prediction.c:2521-2577,
//                       filter_intra_edge_corner :2293, svt_aom_intra_edge_filter_strength :180, svt_av1_filter_intra_edge_c :156
//   predict_sample      svt_aom_intra_prediction_open_loop_mb :2579-2600: svt_aom_dr_predictor :2273 (z1 / z2 / z3 :314-468),
//                       svt_aom_dc_pred[x > 0][y > 0], svt_aom_eb_pred (:1023-1200)
// Edge arrays: above[-1 .. 2 BS - 1], left[-1 .. 2 BS - 1] ([-1] = the top-left sample).  Templated on the block size BS; the open-loop
// search instantiates 16 only.  Edge upsampling is not implemented: svt_aom_use_intra_edge_upsample (:146) is 0 for every block with
// bs0 + bs1 > 16, i.e. for BS >= 16 (static_assert below).  Used by intra_search.hip and tpl.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svthip {
namespace intra {

enum : int { DC = 0, V = 1, H = 2, D45 = 3, D135 = 4, D113 = 5, D157 = 6, D203 = 7, D67 = 8, SMOOTH = 9, SMOOTH_V = 10, SMOOTH_H = 11, PAETH = 12, MODES = 13 };

__constant__ const int16_t MODE_ANGLE[MODES] = {0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0};  // mode_to_angle_map (intra_prediction.h:65)
// sm_weight_arrays (intra_prediction.c:26): the weights of size bs start at [bs]
__constant__ const uint8_t SM_WEIGHTS[128] = {
    0,   0,   255, 128, 255, 149, 85,  64,  255, 197, 146, 105, 73,  50,  37,  32,  255, 225, 196, 170, 145, 123, 102, 84,  68,  54,
    43,  33,  26,  20,  17,  16,  255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92,  83,  74,  66,  59,  52,  45,
    39,  34,  29,  25,  21,  17,  14,  12,  10,  9,   8,   8,   255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163,
    156, 150, 144, 138, 133, 127, 121, 116, 111, 106, 101, 96,  91,  86,  82,  77,  73,  69,  65,  61,  57,  54,  50,  47,  44,  41,
    38,  35,  32,  29,  27,  25,  22,  20,  18,  16,  15,  13,  12,  10,  9,   8,   7,   6,   6,   5,   5,   4,   4,   4};
// eb_dr_intra_derivative (intra_prediction.c:245)
__constant__ const uint16_t DR_DERIV[90] = {0,   0, 0,  1023, 0, 0,  547, 0, 0,  372, 0, 0, 0, 0,  273, 0, 0,  215, 0, 0,  178, 0, 0, 151, 0, 0,
                                            132, 0, 0,  116,  0, 0,  102, 0, 0,  0,   90, 0, 0, 80, 0,   0, 71, 0,   0, 64, 0,   0, 57, 0, 0,  51, 0,
                                            0,   45, 0, 0,    0, 40, 0,   0, 35, 0,   0,  31, 0, 0,  27,  0, 0,  23,  0, 0,  19,  0, 0, 15, 0, 0,  0,
                                            0,   11, 0, 0,    7, 0,  0,   3, 0,  0};
__constant__ const uint8_t EDGE_KERNEL[3][5] = {{0, 4, 8, 4, 0}, {0, 5, 6, 5, 0}, {2, 4, 4, 4, 2}};  // svt_av1_filter_intra_edge_c

__device__ __forceinline__ uint32_t nb_ld8(const uint8_t *p) { return *(const __attribute__((address_space(1))) uint8_t *)p; }

// svt_aom_update_neighbor_samples_array_open_loop_mb[_recon] (enc_intra_prediction.c:1127-1300) for a BS x BS block with
// use_top_right_bottom_left = update_top_neighbor = 1; above_ref / left_ref point at the [-1] entries, 2 BS + 1 of each are written.
// pic0 = sample (0, 0) of a plane in global memory.  One lane.
template <uint32_t BS>
__device__ void neighbours(uint8_t *above_ref, uint8_t *left_ref, const uint8_t *pic0, uint32_t stride, uint32_t x, uint32_t y, uint32_t width,
                           uint32_t height) {
    const uint32_t bw = BS, bh = BS, n = 2 * BS;
    const uint8_t *src = pic0 + (size_t)y * stride + x;
    for (uint32_t i = 0; i <= n; i++) above_ref[i] = 127, left_ref[i] = 129;
    uint8_t *a = above_ref, *l = left_ref;
    if (x != 0 && y != 0)
        *a = *l = (uint8_t)nb_ld8(src - stride - 1);
    else
        *a = *l = 128;
    a++, l++;
    uint32_t count = n;
    if (x != 0) {
        const uint8_t *rp = src - 1;
        if (y == 0)
            l[-1] = (uint8_t)nb_ld8(rp);
        count = (y + count > height) ? count - (y + count - height) : count;
        for (uint32_t i = 0; i < count; i++, rp += stride) *l++ = (uint8_t)nb_ld8(rp);
        l += n - count;
        for (uint32_t i = 0; i < bh; i++) l[-(int)bh + (int)i] = l[-(int)bh - 1];
    } else if (y != 0) {
        count = (y + count > height) ? count - (y + count - height) : count;
        const uint8_t v = (uint8_t)nb_ld8(src - stride);
        for (uint32_t i = 0; i <= count; i++) l[(int)i - 1] = v;
        a[-1] = v;
    } else
        l += count;
    count = n;
    if (y != 0) {
        count = (x + count > width) ? count - (x + count - width) : count;
        for (uint32_t i = 0; i < count; i++) a[i] = (uint8_t)nb_ld8(src - stride + i);
        if (x != 0)
            for (uint32_t i = 0; i < bw; i++) a[bw + i] = a[bw - 1];
    } else if (x != 0) {
        count = (x + count > width) ? count - (x + count - width) : count;
        const uint8_t v = *(l - count);
        for (uint32_t i = 0; i <= count; i++) a[(int)i - 1] = v;
    }
}

__device__ __forceinline__ bool is_directional(int mode) { return mode >= V && mode <= D67; }

// svt_aom_intra_edge_filter_strength (intra_prediction.c:180) with type 0 (the open-loop search has no smooth neighbours)
__device__ __forceinline__ int edge_strength(int blk_wh, int delta) {
    const int d = delta < 0 ? -delta : delta;
    if (blk_wh <= 8)
        return d >= 56 ? 1 : 0;
    if (blk_wh <= 16)
        return d >= 40 ? 1 : 0;
    if (blk_wh <= 24)
        return d >= 32 ? 3 : (d >= 16 ? 2 : (d >= 8 ? 1 : 0));
    if (blk_wh <= 32)
        return d >= 32 ? 3 : (d >= 4 ? 2 : (d >= 1 ? 1 : 0));
    return d >= 1 ? 3 : 0;
}

// p[k] of svt_av1_filter_intra_edge_c: the edge that starts at the [-1] entry; k = 0 is the (corner-filtered) top-left sample
__device__ __forceinline__ int edge_at(const uint8_t *e, int corner, int k) { return k == 0 ? corner : (int)e[k - 1]; }
// one output sample p[k] (1 <= k < sz) of svt_av1_filter_intra_edge_c: 5 taps over the unfiltered copy, indices clamped to [0, sz - 1]
__device__ __forceinline__ int edge_tap(const uint8_t *e, int corner, int k, int sz, int strength) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        int i = k - 2 + j;
        i     = i < 0 ? 0 : (i > sz - 1 ? sz - 1 : i);
        s += edge_at(e, corner, i) * (int)EDGE_KERNEL[strength - 1][j];
    }
    return (s + 8) >> 4;
}

// filter_intra_edge (intra_prediction.c:2521-2577) of a directional mode other than V / H: above0 / left0 (the gathered edges, [0]
// entries; [-1] valid) -> above / left (same layout, written).  The whole wave calls it, lane k < 2 BS + 1 writes entry k - 1 of both;
// the caller puts a barrier behind it.  max_w / max_h = scs->max_input_luma_width / height (the number of 16-wide columns and
// 16-high rows that bounds n_top_px / n_left_px); x, y = block origin.
template <int BS>
__device__ void filter_edges(const uint8_t *above0, const uint8_t *left0, uint8_t *above, uint8_t *left, int p_angle, int x, int y, int max_w,
                             int max_h) {
    static_assert(BS >= 16, "edge upsampling (bs0 + bs1 <= 16) is not implemented");
    const int lane = threadIdx.x;
    // the reference hard-wires TX_16X16 here; the search instantiates BS = 16 only
    const int mb_stride = (max_w + 15) >> 4, mb_height = (max_h + 15) >> 4;
    const int n_top  = y > 0 ? min(BS, mb_stride * 16 - x + BS) : 0;
    const int n_left = x > 0 ? min(BS, mb_height * 16 - y + BS) : 0;
    const bool need_above = p_angle < 180, need_left = p_angle > 90;  // need_above_left = 1 for every directional mode
    const bool need_right = p_angle < 90, need_bottom = p_angle > 180;
    int        corner_a = above0[-1], corner_l = left0[-1];
    if (need_above && need_left && 2 * BS >= 24)  // filter_intra_edge_corner
        corner_a = corner_l = (left0[0] * 5 + above0[-1] * 6 + above0[0] * 5 + 8) >> 4;
    if (lane <= 2 * BS) {
        const int k = lane;
        int       va = edge_at(above0, corner_a, k), vl = edge_at(left0, corner_l, k);
        if (need_above && n_top > 0) {
            const int st = edge_strength(2 * BS, p_angle - 90), sz = n_top + 1 + (need_right ? BS : 0);
            if (st && k >= 1 && k < sz)
                va = edge_tap(above0, corner_a, k, sz, st);
        }
        if (need_left && n_left > 0) {
            const int st = edge_strength(2 * BS, p_angle - 180), sz = n_left + 1 + (need_bottom ? BS : 0);
            if (st && k >= 1 && k < sz)
                vl = edge_tap(left0, corner_l, k, sz, st);
        }
        above[k - 1] = (uint8_t)va, left[k - 1] = (uint8_t)vl;
    }
}

__device__ __forceinline__ int interp5(int a, int b, int shift) { return (a * (32 - shift) + b * shift + 16) >> 5; }

// svt_aom_dr_predictor (intra_prediction.c:2273) with upsampling 0, sample (r, c) of a BS x BS block; angle != 90, 180
template <int BS>
__device__ __forceinline__ uint32_t dr_sample(const uint8_t *above, const uint8_t *left, int angle, int r, int c) {
    constexpr int max_base = 2 * BS - 1;
    int           v;
    if (angle < 90) {  // z1: dx = derivative[angle], dy = 1
        const int x = (r + 1) * (int)DR_DERIV[angle], base = (x >> 6) + c, shift = (x & 0x3f) >> 1;
        v = base < max_base ? interp5(above[base], above[base + 1], shift) : above[max_base];
    } else if (angle < 180) {  // z2: dx = derivative[180 - angle], dy = derivative[angle - 90]
        const int x = -(r + 1) * (int)DR_DERIV[180 - angle], base1 = (x >> 6) + c;
        if (base1 >= -1) {
            v = interp5(above[base1], above[base1 + 1], (x & 0x3f) >> 1);
        } else {
            const int y = (r << 6) - (c + 1) * (int)DR_DERIV[angle - 90], base2 = y >> 6;
            v = interp5(left[base2], left[base2 + 1], (y & 0x3f) >> 1);
        }
    } else {  // z3: dx = 1, dy = derivative[270 - angle]
        const int y = (c + 1) * (int)DR_DERIV[270 - angle], base = (y >> 6) + r, shift = (y & 0x3f) >> 1;
        v = base < max_base ? interp5(left[base], left[base + 1], shift) : left[max_base];
    }
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// DC value of svt_aom_dc_pred[x > 0][y > 0]: dc / dc_left / dc_top / dc_128; sum_above / sum_left over the first BS entries
template <int BS>
__device__ __forceinline__ uint32_t dc_of(uint32_t sum_above, uint32_t sum_left, bool has_left, bool has_above) {
    constexpr int LOG = BS == 4 ? 2 : (BS == 8 ? 3 : (BS == 16 ? 4 : (BS == 32 ? 5 : 6)));
    if (has_left && has_above)
        return (sum_above + sum_left + BS) >> (LOG + 1);
    if (has_left)
        return (sum_left + BS / 2) >> LOG;
    if (has_above)
        return (sum_above + BS / 2) >> LOG;
    return 128;
}

__device__ __forceinline__ uint32_t absdiff(int a, int b) { return (uint32_t)(a > b ? a - b : b - a); }

// sample (r, c) of a non-DC mode of svt_aom_intra_prediction_open_loop_mb; `above` / `left` are the edges the mode predicts from (the
// filtered copies for z1 / z2 / z3, the gathered ones otherwise)
template <int BS>
__device__ __forceinline__ uint32_t predict_sample(int mode, const uint8_t *above, const uint8_t *left, int r, int c) {
    switch (mode) {
    case V: return above[c];
    case H: return left[r];
    case SMOOTH: {  // log2_scale 9
        const uint32_t wh = SM_WEIGHTS[BS + r], ww = SM_WEIGHTS[BS + c];
        return (wh * above[c] + (256 - wh) * left[BS - 1] + ww * left[r] + (256 - ww) * above[BS - 1] + 256) >> 9;
    }
    case SMOOTH_V: {
        const uint32_t w = SM_WEIGHTS[BS + r];
        return (w * above[c] + (256 - w) * left[BS - 1] + 128) >> 8;
    }
    case SMOOTH_H: {
        const uint32_t w = SM_WEIGHTS[BS + c];
        return (w * left[r] + (256 - w) * above[BS - 1] + 128) >> 8;
    }
    case PAETH: {  // paeth_predictor_single
        const int t = above[c], l = left[r], tl = above[-1], base = t + l - tl;
        const uint32_t pl = absdiff(base, l), pt = absdiff(base, t), ptl = absdiff(base, tl);
        return (uint32_t)((pl <= pt && pl <= ptl) ? l : (pt <= ptl ? t : tl));
    }
    default: return dr_sample<BS>(above, left, MODE_ANGLE[mode], r, c);
    }
}

}  // namespace intra
}  // namespace svthip
