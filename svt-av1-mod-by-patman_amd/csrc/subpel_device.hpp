// subpel_device.hpp — what the motion-search kernels of mode decision (inter_subpel.hip, inter_fpel.hip, inter_obmc.hip) share.  All
// three: the walk of a batch's descriptors by the two instantiations that share a call, the staging of a rectangle of a picture in LDS,
// the variance from the sums.  The sub-pel ones: the filter tables of svt_aom_upsampled_pred_c, the two-pass prediction of one candidate
// vector from a reference window staged in LDS and its variance, and the sums of a workgroup.  They differ in what they make of a
// predicted sample: src - pre in inter_subpel.hip, wsrc - pre * mask in inter_obmc.hip.
#pragma once
#include "../../include/svt_hip_inter.h"
#include "blend_device.hpp"
#include "mv_cost_device.hpp"

namespace svthip {
namespace subpel {

constexpr int SMALL_AREA = 256;  // the single-wave kernels take blocks up to this many samples
constexpr int SMALL_SIDE = 32;   // the full-pel kernel with the small LDS footprint takes blocks whose sides are at most this
typedef const __attribute__((address_space(1))) uint8_t g_u8;  // pictures are global memory: no flat loads

// ---- the batch ----------------------------------------------------------------------------------------------------------------------
// The two classes of a batch call, and which of its two instantiations takes a descriptor: the large one those of its class that are
// good (every status code for "good" is 0), the small one all others, so every bad descriptor too.  (Before this rule a bad
// descriptor of a large size other than BAD_SIZE went to the large instantiation of the sub-pel and OBMC kernels; the records are the
// same either way, but a bad 128 x 128 target descriptor with addressable outputs now has them zeroed by one wave.)  fpel_kernel spells
// the rule out, with a side above SMALL_SIDE as the large class.
template <class Large> __device__ __forceinline__ bool takes(bool large_kernel, int status, Large is_large) { return (status == 0 && is_large()) == large_kernel; }
struct ByArea {
    template <class Desc> __device__ bool operator()(const Desc &d) const { return (int)d.w * d.h > SMALL_AREA; }
};

__device__ __forceinline__ void set_status(uint32_t &record, int status) { record = (uint32_t)status; }
template <class Record> __device__ __forceinline__ void set_status(Record &record, int status) { record.status = (uint8_t)status; }

// One workgroup's walk over the descriptors of a batch: it strides over them when there are more than the grid holds and skips the
// other instantiation's.  A descriptor's record starts as zeroes with status_of(d); body(d, record) completes it for a good one,
// bad(d) sees the others; thread 0 stores it.  Everything is inlined into the kernel.
template <bool LARGE, class Desc, class Record, class Status, class Large, class Body, class Bad>
__device__ __forceinline__ void for_each_descriptor(const Desc *__restrict__ d_desc, Record *__restrict__ d_record, uint32_t n, Status status_of, Large is_large,
                                                    Body body, Bad bad) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Desc d = d_desc[i];
        const int  status = status_of(d);
        if (!takes(LARGE, status, [&] { return is_large(d); }))
            continue;
        Record r = {};
        set_status(r, status);
        if (status == 0)
            body(d, r);
        else
            bad(d);
        if (threadIdx.x == 0)
            d_record[i] = r;
    }
}
template <bool LARGE, class Desc, class Record, class Status, class Large, class Body>
__device__ __forceinline__ void for_each_descriptor(const Desc *__restrict__ d_desc, Record *__restrict__ d_record, uint32_t n, Status status_of, Large is_large, Body body) {
    for_each_descriptor<LARGE>(d_desc, d_record, n, status_of, is_large, body, [](const Desc &) {});
}

// n bytes of a pitched rectangle of global memory into LDS, row_bytes to a row; four loads in flight per thread
template <int NT> __device__ __forceinline__ void stage_rows(uint8_t *lds, const uint8_t *global, int64_t pitch, int row_bytes, int n) {
    g_u8 *g = (g_u8 *)global;
    for (int k0 = threadIdx.x; k0 < n; k0 += 4 * NT) {
        uint8_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = k0 + j * NT, y = k / row_bytes;
            v[j] = k < n ? g[y * pitch + (k - y * row_bytes)] : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (k0 + j * NT < n)
                lds[k0 + j * NT] = v[j];
    }
}

struct Error {
    uint32_t var, sse;
};
// what a vf of variance.c makes of a block's sum and sum of squares
__device__ __forceinline__ Error variance_of(int sum, uint32_t sse, int log2_area) { return {sse - (uint32_t)(((int64_t)sum * sum) >> log2_area), sse}; }

// ---- the sub-pel prediction ---------------------------------------------------------------------------------------------------------

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
    int32_t       *red; // LDS: per-wave partial sums, as many per wave as the widest block_sums of the kernel
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

// the N sums of the workgroup in every lane: across the lanes by shuffles, across the waves through red (N words per wave), which the
// previous sums have been read from
template <int NT, int N> __device__ __forceinline__ void block_sums(int32_t *red, uint32_t (&v)[N]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = blend::wave_sum(v[j]);
    if (NT > 64) {
        if ((tid & 63) == 0) {
#pragma unroll
            for (int j = 0; j < N; j++) red[N * (tid >> 6) + j] = (int32_t)v[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < N; j++) {
            v[j] = 0;
#pragma unroll
            for (int k = 0; k < NT / 64; k++) v[j] += (uint32_t)red[N * k + j];
        }
    }
}

// vf(prediction at mv, .): the variance and the sum of squares of diff(i, r, c, pre) over the block's samples
template <int NT, class Diff> __device__ __forceinline__ Error predicted_error(const Window &b, SvtHipMv mv, Diff diff) {
    uint32_t s[2] = {0, 0};  // sum, sse
    predict<NT>(b, mv, [&](int i, int r, int c, int pre) {
        const int v = diff(i, r, c, pre);
        s[0] += (uint32_t)v, s[1] += (uint32_t)(v * v);
    });
    block_sums<NT>(b.red, s);
    return variance_of((int)s[0], s[1], b.log2_area);
}

}  // namespace subpel
}  // namespace svthip
