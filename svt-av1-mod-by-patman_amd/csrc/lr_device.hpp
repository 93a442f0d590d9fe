// lr_device.hpp — device code shared by the loop-restoration kernels (loopfilter_sgr.hip, loopfilter_wiener.hip,
// loopfilter_lr_frame.hip): the self-guided filter and the Wiener filter of ONE processing unit whose samples (with their
// 3-sample border) already sit in LDS.  Who fills the tile decides what the filter sees: straight picture samples for the
// per-unit entry points, the stripe-boundary rows of svt_aom_setup_processing_stripe_boundary for the frame-level pass.
// Both tile filters hand every result to a sink: a store, a sum, whatever the caller does with it.
// Also here: what the restoration decisions share (loopfilter_sgr.hip, loopfilter_wiener_pick.hip, loopfilter_rest_pick.hip): the
// projection of svt_apply_selfguided_restoration, the clamped tile load of the two picks, the projection sums, the solver, the batched
// error and finer search of the self-guided filter (the batch size a template parameter), the first minimum over candidates, the
// sub-exponential bit count and RDCOST_DBL.  lr_pick.hpp adds what only the two plane picks need.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svthip {
namespace lr {

constexpr int RST_BITS = 4, PRJ_BITS = 7, SGR_BITS = 8, MTABLE_BITS = 20, RECIP_BITS = 12;
constexpr int TP = 72;   // LDS pitch of the sample tile (64 + 2*3 = 70 used)
constexpr int AP = 67;   // LDS pitch of the A / B maps (66 used, odd)
constexpr int PRJ_MIN0 = -96, PRJ_MAX0 = 31, PRJ_MIN1 = -32, PRJ_MAX1 = 95;  // restoration.h:101-104

constexpr int32_t SGR_PRM[16][4] = {/* r0, r1, s0, s1: svt_aom_eb_sgr_params (restoration.c:85-103); host code reads the radii */
                                           {2, 1, 140, 3236}, {2, 1, 112, 2158}, {2, 1, 93, 1618}, {2, 1, 80, 1438},
                                      {2, 1, 70, 1295},  {2, 1, 58, 1177},  {2, 1, 47, 1079}, {2, 1, 37, 996},
                                      {2, 1, 30, 925},   {2, 1, 25, 863},   {0, 1, -1, 2589}, {0, 1, -1, 1618},
                                      {0, 1, -1, 1177},  {0, 1, -1, 925},   {2, 0, 56, -1},   {2, 0, 22, -1}};

__device__ __forceinline__ int32_t rnd(int32_t v, int n) { return (v + ((1 << n) >> 1)) >> n; }
__device__ __forceinline__ int32_t ldpx(const void *p, size_t idx, int is16) {
    return is16 ? ((const __attribute__((address_space(1))) uint16_t *)p)[idx] : ((const __attribute__((address_space(1))) uint8_t *)p)[idx];  // pictures are global memory: no flat loads
}
__device__ __forceinline__ void stpx(void *p, size_t idx, int is16, int32_t v) {
    if (is16)
        ((uint16_t *)p)[idx] = (uint16_t)v;
    else
        ((uint8_t *)p)[idx] = (uint8_t)v;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rows x cols samples from (y, x) of a plane into an LDS tile of the given pitch, by the nt threads of the workgroup.  Coordinates are
// clamped to the plane: outside the cropped plane the samples replicate its edge (svt_extend_frame), nothing outside is read.
__device__ __forceinline__ void load_tile_clamped(uint16_t *tile, int pitch, const void *plane, uint32_t stride, int is16, int plane_w, int plane_h, int y, int x,
                                                  int rows, int cols, int nt) {
    for (int idx = threadIdx.x; idx < rows * cols; idx += nt) {
        const int r = idx / cols, c = idx - r * cols;
        const int yy = min(max(y + r, 0), plane_h - 1), xx = min(max(x + c, 0), plane_w - 1);
        tile[r * pitch + c] = (uint16_t)ldpx(plane, (size_t)yy * stride + xx, is16);
    }
}

// A / B of one map position from the LDS tile (restoration.c:709-770 / 842-903); (i, j) relative to the unit, r = 1 | 2
template <int R> __device__ __forceinline__ void ab_at(const uint16_t *tile, int i, int j, uint32_t s, int bd, int32_t &A, int32_t &B) {
    // box sums over (2R + 1)^2 samples.  A lane's 2R + 1 samples of a row start at a 2-byte aligned address; read as adjacent 16-bit
    // values they become one unaligned ds_read_b64, which gfx950 executes one lane per cycle (tools/ubench/lds_unaligned.hip).  So: the
    // R + 1 aligned dwords that hold them, funnel-shifted by the lane's parity (the pitch is even: one parity for all rows), the odd
    // sample masked; sum and sum of squares by v_dot2_u32_u16.
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const int      e0 = (i + 3 - R) * TP + j + 3 - R;
    const uint32_t sh = (uint32_t)(e0 & 1) * 16;
    const u16x2    ones = {1, 1};
    uint32_t       sum = 0, ssq = 0;
#pragma unroll
    for (int dy = 0; dy <= 2 * R; dy++) {
        const uint32_t *q = (const uint32_t *)tile + ((e0 + dy * TP) >> 1);
        uint32_t        d[R + 1];
#pragma unroll
        for (int k = 0; k <= R; k++) d[k] = q[k];
#pragma unroll
        for (int k = 0; k <= R; k++) {
            uint32_t pr = __builtin_amdgcn_alignbit(d[k < R ? k + 1 : k], d[k], sh);
            if (k == R)
                pr &= 0xffffu;
            const u16x2 v = __builtin_bit_cast(u16x2, pr);
            sum = __builtin_amdgcn_udot2(v, ones, sum, false), ssq = __builtin_amdgcn_udot2(v, v, ssq, false);
        }
    }
    constexpr uint32_t n = (2 * R + 1) * (2 * R + 1), one_by_n = (4096 + n / 2) / n;  // svt_aom_eb_one_by_x[n - 1]
    const uint32_t a = (ssq + ((1u << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8)), b = (sum + ((1u << (bd - 8)) >> 1)) >> (bd - 8);
    const uint32_t p = (a * n < b * b) ? 0u : a * n - b * b;
    uint32_t       z = (p * s + (1u << (MTABLE_BITS - 1))) >> MTABLE_BITS;
    z                = z > 255 ? 255 : z;
    A = z == 0 ? 1 : (z == 255 ? 256 : (int32_t)((256 * z + (z + 1) / 2) / (z + 1)));  // svt_aom_eb_x_by_xplus1[z]
    B = (int32_t)(((uint32_t)(256 - A) * sum * one_by_n + (1u << (RECIP_BITS - 1))) >> RECIP_BITS);
}

// The projection of svt_apply_selfguided_restoration (restoration.c:957-992): sample x restored from its two filtered values
__device__ __forceinline__ int32_t sgr_project(int32_t x, int32_t f0, int32_t f1, const int xq[2], int r0, int r1, int bd) {
    const int32_t u = x << RST_BITS;
    int32_t       v = u << PRJ_BITS;
    if (r0 > 0)
        v += xq[0] * (f0 - u);
    if (r1 > 0)
        v += xq[1] * (f1 - u);
    const int16_t wv = (int16_t)rnd(v, PRJ_BITS + RST_BITS);
    return clampi(wv, 0, (1 << bd) - 1);
}

// Filter of one processing unit of w x h samples (<= 64 x 64) from the LDS tile (pitch TP, sample (0,0) at [3][3]); Am / Bm are
// 66 x AP int32 scratch maps in LDS.  Nothing is stored: sink(i, j, sample, f0, f1) gets every sample of the unit with its two filtered
// values (0 where the radius is 0).  Called by all NT threads of the workgroup after a barrier that made the tile visible; contains barriers.
template <int NT, class Sink>
__device__ __forceinline__ void sgr_tile_filter_to(const uint16_t *tile, int32_t *Am, int32_t *Bm, int tid, int w, int h, int ep, int bd, Sink sink) {
    const int r0 = SGR_PRM[ep][0], r1 = SGR_PRM[ep][1];
    constexpr int PER = 64 * 64 / NT;  // samples per thread of a 64x64 unit
    int32_t       f0[PER];
    if (r0 > 0) {  // selfguided_restoration_fast_internal: maps on rows -1, 1, 3, ...
        const int nrows = (h + 2 + 1) / 2, W2 = w + 2;
        for (int idx = tid; idx < nrows * W2; idx += NT) {
            const int ii = idx / W2, j = idx - ii * W2 - 1, i = 2 * ii - 1;
            ab_at<2>(tile, i, j, (uint32_t)SGR_PRM[ep][2], bd, Am[(i + 1) * AP + j + 1], Bm[(i + 1) * AP + j + 1]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int idx = tid + k * NT;
            f0[k]         = 0;
            if (idx < w * h) {
                const int  i = idx / w, j = idx - i * w;
                const int *A = &Am[(i + 1) * AP + j + 1], *B = &Bm[(i + 1) * AP + j + 1];
                int32_t    a, b, nb;
                if (!(i & 1)) {
                    nb = 5;
                    a  = (A[-AP] + A[AP]) * 6 + (A[-AP - 1] + A[AP - 1] + A[-AP + 1] + A[AP + 1]) * 5;
                    b  = (B[-AP] + B[AP]) * 6 + (B[-AP - 1] + B[AP - 1] + B[-AP + 1] + B[AP + 1]) * 5;
                } else {
                    nb = 4;
                    a  = A[0] * 6 + (A[-1] + A[1]) * 5;
                    b  = B[0] * 6 + (B[-1] + B[1]) * 5;
                }
                const int32_t v = a * (int32_t)tile[(i + 3) * TP + j + 3] + b;
                f0[k]           = rnd(v, SGR_BITS + nb - RST_BITS);
            }
        }
        __syncthreads();
    }
    if (r1 > 0) {  // selfguided_restoration_internal (r = 1): maps on every row
        const int W2 = w + 2;
        for (int idx = tid; idx < (h + 2) * W2; idx += NT) {
            const int ii = idx / W2, j = idx - ii * W2 - 1, i = ii - 1;
            ab_at<1>(tile, i, j, (uint32_t)SGR_PRM[ep][3], bd, Am[(i + 1) * AP + j + 1], Bm[(i + 1) * AP + j + 1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int idx = tid + k * NT;
        if (idx >= w * h)
            continue;
        const int i = idx / w, j = idx - i * w;
        int32_t   f1 = 0;
        if (r1 > 0) {
            const int    *A = &Am[(i + 1) * AP + j + 1], *B = &Bm[(i + 1) * AP + j + 1];
            const int32_t a = (A[0] + A[-1] + A[1] + A[-AP] + A[AP]) * 4 + (A[-AP - 1] + A[AP - 1] + A[-AP + 1] + A[AP + 1]) * 3;
            const int32_t b = (B[0] + B[-1] + B[1] + B[-AP] + B[AP]) * 4 + (B[-AP - 1] + B[AP - 1] + B[-AP + 1] + B[AP + 1]) * 3;
            f1              = rnd(a * (int32_t)tile[(i + 3) * TP + j + 3] + b, SGR_BITS + 5 - RST_BITS);
        }
        sink(i, j, (int32_t)tile[(i + 3) * TP + j + 3], f0[k], f1);
    }
}

// Separable 7-tap Wiener filter of one tw x th (<= 64 x 64) unit: `in` = LDS tile of (th + 7) x (tw + 7) samples (4-byte aligned, WIENER_IN_SLACK readable elements behind it), pitch IP, sample
// (0,0) at [3][3]; `tmp` = (th + 7) x 64 uint16 LDS scratch.  svt_av1_(highbd_)wiener_convolve_add_src (convolve.c:57-200).
constexpr int WIENER_IP = 64 + 8, WIENER_IN_SLACK = 2;  // the horizontal pass reads one dword past the last sample of a row
typedef short lr_i16x2 __attribute__((ext_vector_type(2)));
// The filtered sample of (r, c) goes to sink(r, c, v): a store, or whatever else the caller does with it.
template <int NT, class Sink>
__device__ __forceinline__ void wiener_tile_filter_to(const uint16_t *in, uint16_t *tmp, int tid, int tw, int th, const int16_t *fx, const int16_t *fy, int bd,
                                                      int r0, int r1, Sink sink) {
    constexpr int IP = WIENER_IP;
    const int limit = (1 << (bd + 1 + 7 - r0)) - 1;
    // the seven horizontal taps (+ 128 on the centre one: the "add_src" term) as four packed pairs, the 8th coefficient is zero by
    // construction.  The seven samples of a lane start at a 2-byte aligned address: adjacent 16-bit reads become ONE unaligned
    // ds_read_b64 / b128, which gfx950 executes one lane per cycle (tools/ubench/lds_unaligned.hip) — read the aligned dwords around
    // them and funnel-shift by the lane's parity instead; v_dot2_i32_i16 does two taps per instruction.
    uint32_t fxp[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int32_t lo = fx[2 * k] + (2 * k == 3 ? 128 : 0), hi2 = 2 * k + 1 < 7 ? fx[2 * k + 1] + (2 * k + 1 == 3 ? 128 : 0) : 0;
        fxp[k] = __builtin_amdgcn_readfirstlane((int32_t)(((uint32_t)lo & 0xffffu) | ((uint32_t)hi2 << 16)));
    }
    for (int idx = tid; idx < (th + 7) * tw; idx += NT) {
        const int r = idx / tw, c = idx - r * tw, e = r * IP + c;
        const uint32_t *q  = (const uint32_t *)in + (e >> 1);
        const uint32_t  sh = (uint32_t)(e & 1) * 16;
        uint32_t        d[5];
#pragma unroll
        for (int k = 0; k < 5; k++) d[k] = q[k];
        int32_t sum = 1 << (bd + 7 - 1);
#pragma unroll
        for (int k = 0; k < 4; k++)
            sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(lr_i16x2, __builtin_amdgcn_alignbit(d[k + 1], d[k], sh)), __builtin_bit_cast(lr_i16x2, fxp[k]), sum, false);
        const int32_t v = (sum + ((1 << r0) >> 1)) >> r0;
        tmp[r * 64 + c] = (uint16_t)(v < 0 ? 0 : (v > limit ? limit : v));
    }
    __syncthreads();
    const int hi = (1 << bd) - 1;
    for (int idx = tid; idx < th * tw; idx += NT) {
        const int r = idx / tw, c = idx - r * tw;
        int32_t   sum = ((int32_t)tmp[(r + 3) * 64 + c] << 7) - (1 << (bd + r1 - 1));
#pragma unroll
        for (int k = 0; k < 7; k++) sum += (int32_t)tmp[(r + k) * 64 + c] * fy[k];
        int32_t v = (sum + ((1 << r1) >> 1)) >> r1;
        v         = v < 0 ? 0 : (v > hi ? hi : v);
        sink(r, c, v);
    }
}
// ... stored at (y0 + r, x0 + c) of dst
template <int NT>
__device__ __forceinline__ void wiener_tile_filter(const uint16_t *in, uint16_t *tmp, int tid, int tw, int th, int x0, int y0, const int16_t *fx,
                                                   const int16_t *fy, int bd, int r0, int r1, int is16, void *__restrict__ dst, uint32_t dst_stride) {
    wiener_tile_filter_to<NT>(in, tmp, tid, tw, th, fx, fy, bd, r0, r1,
                              [&](int r, int c, int32_t v) { stpx(dst, (size_t)(y0 + r) * dst_stride + x0 + c, is16, v); });
}

// ---- block-wide int64 reductions -------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// sum over the block; result valid in every thread.  scratch: one long long per wave (+1)
__device__ inline long long block_sum64(long long v, long long *scratch) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_sum64(v);
    __syncthreads();  // scratch free
    if (lane == 0)
        scratch[wv] = v;
    __syncthreads();
    long long t = 0;
    for (int i = 0; i < nw; i++) t += scratch[i];
    return t;
}

struct UnitData {
    const void    *src, *dat;
    const int32_t *flt0, *flt1;
    uint32_t       src_stride, dat_stride, flt0_stride, flt1_stride, width, height;
    int            is16, r0, r1;
};

// svt_av1_{lowbd,highbd}_pixel_proj_error_c over the unit (block-wide) for NB decoded candidates xq in ONE pass (the pass is bound by its
// reads: two filtered values, dat and src per sample); every thread gets all NB sums.  scratch: NB long long per wave.  A plane whose
// radius is 0 is not read, so with both radii 0 the error is that of dat - src whatever xq holds: the Tier A projection leaves can pass
// such parameters.
template <int NB> __device__ inline void unit_errors(const UnitData &u, const int (*xq)[2], long long *out, long long *scratch) {
    long long      acc[NB] = {};
    const uint32_t n = u.width * u.height;
#pragma unroll(NB > 1 ? 2 : 1)  // a batch has the work to fill two iterations in flight; one candidate per pass is the plain loop
    for (uint32_t idx = threadIdx.x; idx < n; idx += blockDim.x) {
        const uint32_t i = idx / u.width, j = idx - i * u.width;
        const int32_t  d = ldpx(u.dat, (size_t)i * u.dat_stride + j, u.is16), s = ldpx(u.src, (size_t)i * u.src_stride + j, u.is16);
        const int32_t  uu = d << RST_BITS;
        const int32_t  a0 = u.r0 > 0 ? u.flt0[(size_t)i * u.flt0_stride + j] - uu : 0, a1 = u.r1 > 0 ? u.flt1[(size_t)i * u.flt1_stride + j] - uu : 0;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const int32_t v = (1 << (RST_BITS + PRJ_BITS - 1)) + xq[k][0] * a0 + xq[k][1] * a1, e = (v >> (RST_BITS + PRJ_BITS)) + d - s;
            acc[k] += (long long)e * e;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < NB; k++) acc[k] = wave_sum64(acc[k]);
    __syncthreads();  // scratch free
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NB; k++) scratch[wv * NB + k] = acc[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NB; k++) {
        long long t = 0;
        for (int w = 0; w < nw; w++) t += scratch[w * NB + k];
        out[k] = t;
    }
}

// the five sums of svt_get_proj_subspace_c (block-wide)
__device__ inline void unit_sums(const UnitData &u, long long out[5], long long *scratch) {
    long long      a[5] = {0, 0, 0, 0, 0};
    const uint32_t n    = u.width * u.height;
    for (uint32_t idx = threadIdx.x; idx < n; idx += blockDim.x) {
        const uint32_t  i = idx / u.width, j = idx - i * u.width;
        const long long uu = (long long)ldpx(u.dat, (size_t)i * u.dat_stride + j, u.is16) << RST_BITS;
        const long long s  = ((long long)ldpx(u.src, (size_t)i * u.src_stride + j, u.is16) << RST_BITS) - uu;
        const long long f1 = u.r0 > 0 ? u.flt0[(size_t)i * u.flt0_stride + j] - uu : 0;
        const long long f2 = u.r1 > 0 ? u.flt1[(size_t)i * u.flt1_stride + j] - uu : 0;
        a[0] += f1 * f1, a[1] += f2 * f2, a[2] += f1 * f2, a[3] += f1 * s, a[4] += f2 * s;
    }
    for (int k = 0; k < 5; k++) out[k] = block_sum64(a[k], scratch);
}

// closed-form part of svt_get_proj_subspace_c (restoration_pick.c:471-506), IEEE double without contraction
__device__ inline void solve_subspace(const long long sums[5], int size, int r0, int r1, int xq[2]) {
    double H00 = (double)sums[0], H11 = (double)sums[1], H01 = (double)sums[2], C0 = (double)sums[3], C1 = (double)sums[4];
    xq[0] = xq[1] = 0;
    H00 /= size, H01 /= size, H11 /= size, C0 /= size, C1 /= size;
    const double H10 = H01;
    if (r0 == 0) {
        if (H11 < 1e-8)
            return;
        xq[1] = (int)rint(C1 / H11 * (1 << PRJ_BITS));
    } else if (r1 == 0) {
        if (H00 < 1e-8)
            return;
        xq[0] = (int)rint(C0 / H00 * (1 << PRJ_BITS));
    } else {
        const double det = H00 * H11 - H01 * H10;
        if (det < 1e-8)
            return;
        const double x0 = (H11 * C0 - H01 * C1) / det, x1 = (H00 * C1 - H10 * C0) / det;
        xq[0] = (int)rint(x0 * (1 << PRJ_BITS)), xq[1] = (int)rint(x1 * (1 << PRJ_BITS));
    }
}
// svt_decode_xq (restoration.c:634-645); the host decodes with it too
__host__ __device__ inline void decode_xq(const int xqd[2], int xq[2], int r0, int r1) {
    if (r0 == 0)
        xq[0] = 0, xq[1] = (1 << PRJ_BITS) - xqd[1];
    else if (r1 == 0)
        xq[0] = xqd[0], xq[1] = 0;
    else
        xq[0] = xqd[0], xq[1] = (1 << PRJ_BITS) - xq[0] - xqd[1];
}
__device__ inline void encode_xq(const int xq[2], int xqd[2], int r0, int r1) {
    if (r0 == 0) {
        xqd[0] = 0;
        xqd[1] = clampi((1 << PRJ_BITS) - xq[1], PRJ_MIN1, PRJ_MAX1);
    } else if (r1 == 0) {
        xqd[0] = clampi(xq[0], PRJ_MIN0, PRJ_MAX0);
        xqd[1] = clampi((1 << PRJ_BITS) - xqd[0], PRJ_MIN1, PRJ_MAX1);
    } else {
        xqd[0] = clampi(xq[0], PRJ_MIN0, PRJ_MAX0);
        xqd[1] = clampi((1 << PRJ_BITS) - xqd[0] - xq[1], PRJ_MIN1, PRJ_MAX1);
    }
}

// finer_search_pixel_proj_error (restoration_pick.c:320-411) with start_step 2, block-wide: every thread runs the (uniform) control flow,
// every pass over the unit is a block reduction whose result all threads see.  xqd is moved in place; trials = get_pixel_proj_error calls.
// The accepted path and the count of trials are the reference's; what NB sets is how many errors one pass over the unit yields: a walk
// at step 2 ("at the highest step size continue moving in the same direction") has its next NB moves evaluated together, and the moves
// behind the first refused one are dropped unused (and not counted).  NB = 1 is the reference's loop trial by trial.  scratch: as unit_errors.
template <int NB> __device__ inline long long finer_search(const UnitData &u, int xqd[2], int do_refine, long long *scratch, int &trials) {
    int       cq[NB][2];
    long long e[NB];
    auto errors = [&]() {
        int xq[NB][2];
#pragma unroll
        for (int k = 0; k < NB; k++) decode_xq(cq[k], xq[k], u.r0, u.r1);
        unit_errors<NB>(u, xq, e, scratch);
    };
#pragma unroll
    for (int k = 0; k < NB; k++) cq[k][0] = xqd[0], cq[k][1] = xqd[1];
    errors();
    long long err = e[0];
    trials        = 1;
    if (!do_refine)
        return err;
    for (int s = 2; s >= 1; s >>= 1)
        for (int p = 0; p < 2; ++p) {
            if ((u.r0 == 0 && p == 0) || (u.r1 == 0 && p == 1))
                continue;
            const int lo = p == 0 ? PRJ_MIN0 : PRJ_MIN1, hi = p == 0 ? PRJ_MAX0 : PRJ_MAX1;
            int       skip = 0;
            for (int dir = -1; dir <= 1; dir += 2) {  // the two do-while loops
                for (bool walk = true; walk;) {
                    const int cur = p == 0 ? xqd[0] : xqd[1], room = (dir < 0 ? cur - lo : hi - cur) / s, nb = min(room, s == 2 ? NB : 1);
                    if (nb == 0)
                        break;  // the move would leave the range: `break` without a trial
#pragma unroll
                    for (int k = 0; k < NB; k++) {
                        const int v = cur + dir * s * (min(k, nb - 1) + 1);
                        cq[k][0] = p == 0 ? v : xqd[0], cq[k][1] = p == 0 ? xqd[1] : v;
                    }
                    errors();
                    walk = s == 2;
#pragma unroll
                    for (int k = 0; k < NB; k++) {
                        if (k >= nb)
                            break;
                        trials++;
                        if (e[k] > err) {  // refused: the move is undone, the walk ends
                            walk = false;
                            break;
                        }
                        err = e[k], skip |= dir < 0;
                        if (p == 0)
                            xqd[0] += dir * s;
                        else
                            xqd[1] += dir * s;
                    }
                }
                if (skip)
                    break;
            }
            if (skip)
                break;  // `if (skip) break;` leaves the loop over p
        }
    return err;
}

// The first strictly smallest error in candidate order (restoration_pick.c:638-643); c[i].err is candidate i's
template <class Cand> __device__ __forceinline__ int first_min(const Cand *c, int n) {
    int b = 0;
    for (int i = 1; i < n; i++)
        if (c[i].err < c[b].err)
            b = i;
    return b;
}

// svt_aom_count_primitive_refsubexpfin (entropy_coding.c:2805-2951)
__device__ inline int count_refsubexpfin(int n, int k, int ref, int v) {
    auto recenter = [](int r, int v) { return v > (r << 1) ? v : (v >= r ? (v - r) << 1 : ((r - v) << 1) - 1); };
    ref &= 0xffff, v &= 0xffff;
    v = ((ref << 1) <= n ? recenter(ref, v) : recenter((n - 1 - ref) & 0xffff, (n - 1 - v) & 0xffff)) & 0xffff;
    int count = 0, i = 0, mk = 0;
    for (;;) {
        const int b = i ? k + i - 1 : k, a = 1 << b;
        if (n <= mk + 3 * a) {
            const int nn = (n - mk) & 0xffff, vv = (v - mk) & 0xffff;  // svt_aom_count_primitive_quniform
            if (nn > 1) {
                const int l = 32 - __clz(nn - 1), m = (1 << l) - nn;
                count += vv < m ? l - 1 : l;
            }
            break;
        }
        count++;
        if (v >= mk + a)
            i++, mk += a;
        else {
            count += b;
            break;
        }
    }
    return count;
}

__device__ __forceinline__ double rdcost_dbl(int rdmult, long long rate, long long dist) {  // RDCOST_DBL (restoration.h:346)
    return (((double)rate * (double)rdmult) / 512.0) + ((double)dist * 128.0);
}

}  // namespace lr
}  // namespace svthip
