// subpel_device.hpp — what the sub-pel kernels of inter_subpel.hip and inter_obmc.hip share: the filter tables of
// svt_aom_upsampled_pred_c, the two-pass prediction of one candidate vector from a reference window staged in LDS, and the sums
// of a workgroup.  The kernels differ in what they do with a predicted sample: src - pre there, wsrc - pre * mask here.
#pragma once
#include "../../include/svt_hip_inter.h"
#include "blend_device.hpp"
#include "mv_cost_device.hpp"

namespace svthip {
namespace subpel {

constexpr int MAX_FULL_PEL_VAL = (1 << 10) - 1;      // av1me.h:24-27
constexpr int SMALL_AREA = 256;                      // the single-wave kernels take blocks up to this many samples

// av1_bilinear_filters, av1_sub_pel_filters_4 and av1_sub_pel_filters_8 (variance.c:73-140): av1_get_filter(USE_2_TAPS ..
// USE_8_TAPS), row = subpel_q3 << 1.  Only the even rows are ever addressed.
__constant__ const int16_t FILTERS[3][8][8] = {
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, 0, 112, 16, 0, 0, 0}, {0, 0, 0, 96, 32, 0, 0, 0}, {0, 0, 0, 80, 48, 0, 0, 0},
     {0, 0, 0, 64, 64, 0, 0, 0}, {0, 0, 0, 48, 80, 0, 0, 0}, {0, 0, 0, 32, 96, 0, 0, 0}, {0, 0, 0, 16, 112, 0, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, -8, 122, 18, -4, 0, 0}, {0, 0, -12, 110, 38, -8, 0, 0}, {0, 0, -14, 94, 58, -10, 0, 0},
     {0, 0, -12, 76, 76, -12, 0, 0}, {0, 0, -10, 58, 94, -14, 0, 0}, {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -4, 18, 122, -8, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 2, -10, 122, 18, -4, 0, 0}, {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0},
     {0, 2, -14, 76, 76, -14, 2, 0}, {0, 2, -12, 58, 94, -16, 2, 0}, {0, 2, -10, 38, 110, -14, 2, 0}, {0, 0, -4, 18, 122, -10, 2, 0}}};
// first tap that is not zero and one past the last, per table, for a direction with a sub-pel offset
__constant__ const int8_t TAP_RANGE[3][2] = {{3, 5}, {2, 6}, {1, 7}};

__device__ __forceinline__ int clip_pixel(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__device__ __forceinline__ int log2_pow2(int v) { return 31 - __clz(v); }

// the 22 sizes of init_fn_ptr (av1me.c:31-170): both sides a power of two in 4 .. 128, aspect at most 4 : 1
__device__ __forceinline__ bool is_block_size(int w, int h) {
    const bool pow2 = w >= 4 && w <= 128 && h >= 4 && h <= 128 && !(w & (w - 1)) && !(h & (h - 1));
    return pow2 && w <= 4 * h && h <= 4 * w;
}

__device__ __forceinline__ SvtHipMv mv_of(int row, int col) {
    SvtHipMv mv;
    mv.row = (int16_t)row, mv.col = (int16_t)col;
    return mv;
}

struct Window {         // what a candidate's prediction is computed from
    const uint8_t *win; // LDS: the reference window, row 0 / column 0 = margin above / left of the sample (base_row, base_col) points at
    uint8_t       *tmp; // LDS: the intermediate of the first pass, rows 1 .. h + 5 of [h + 7][w]
    int32_t       *red; // LDS: per-wave partial sums, two per wave
    int            w, h, lw, win_stride, log2_area;
    int            base_row, base_col;  // full-pel
    int            margin;              // at least 4 more than the full-pel distance of any candidate from the base
    int            table;               // row of FILTERS
};

// svt_aom_upsampled_pred_c at mv: two separable passes over the window with a uint8 intermediate in LDS, clipped between the
// passes as svt_aom_convolve8_horiz_c / svt_aom_convolve8_vert_c leave it; a direction without a sub-pel offset filters with the
// identity kernel, which is exact.  each(i, r, c, pre) gets sample i = r * w + c of the prediction; a thread gets the samples
// tid, tid + NT, ...  Inlined at every call: as a function it costs a call frame in scratch and thirty more VGPRs.
template <int NT, class Each> __device__ __forceinline__ void predict(const Window &b, SvtHipMv mv, Each each) {
    const int tid = threadIdx.x, w = b.w, h = b.h, lw = b.lw, ws = b.win_stride;
    // window row / column of tap 0 of sample (0, 0), less 3
    const int oy = (mv.row >> 3) - b.base_row + b.margin - 3, ox = (mv.col >> 3) - b.base_col + b.margin - 3;
    const int sy = mv.row & 7, sx = mv.col & 7;
    const int16_t *fx = FILTERS[b.table][sx], *fy = FILTERS[b.table][sy];
    const int kx0 = sx ? TAP_RANGE[b.table][0] : 3, kx1 = sx ? TAP_RANGE[b.table][1] : 4;
    const int ky0 = sy ? TAP_RANGE[b.table][0] : 3, ky1 = sy ? TAP_RANGE[b.table][1] : 4;
    __syncthreads();  // the previous candidate's second pass has read tmp, its sums have been read from red
    // horizontal pass over the rows the vertical taps reach: tmp row t is reference row t - 3 of the block
    const int t0 = ky0, rows = h - 1 + ky1 - ky0;
    for (int i = tid; i < (rows << lw); i += NT) {
        const int      t = t0 + (i >> lw), c = i & (w - 1);
        const uint8_t *p = b.win + (t + oy) * ws + c + ox;
        int            s = 64;
        for (int k = kx0; k < kx1; k++) s += fx[k] * p[k];
        b.tmp[(t << lw) + c] = (uint8_t)clip_pixel(s >> 7);
    }
    __syncthreads();
    for (int i = tid; i < (h << lw); i += NT) {
        const int      r = i >> lw, c = i & (w - 1);
        const uint8_t *p = b.tmp + (r << lw) + c;
        int            s = 64;
        for (int k = ky0; k < ky1; k++) s += fy[k] * p[k << lw];
        each(i, r, c, clip_pixel(s >> 7));
    }
}

// the sums of the workgroup in every lane: across the lanes by shuffles, across the waves through red
template <int NT> __device__ __forceinline__ void block_sums(int32_t *red, int &sum, uint32_t &sse) {
    const int tid = threadIdx.x;
    sum = (int)blend::wave_sum((uint32_t)sum), sse = blend::wave_sum(sse);
    if (NT > 64) {
        if ((tid & 63) == 0)
            red[2 * (tid >> 6)] = sum, red[2 * (tid >> 6) + 1] = (int32_t)sse;
        __syncthreads();
        sum = 0, sse = 0;
#pragma unroll
        for (int v = 0; v < NT / 64; v++) sum += red[2 * v], sse += (uint32_t)red[2 * v + 1];
    }
}

}  // namespace subpel
}  // namespace svthip
