// pyramid.hip — 1/4 and 1/16 decimation with fused edge padding, and per-64x64 block mean / variance.
// Replaces svt_aom_downsample_filtering_input_picture (pic_analysis_process.c:1922-1979 of the reference,
// leaf svt_aom_downsample_2d_c :131-161 + svt_aom_generate_padding pic_operators.c:338-383) and
// compute_picture_spatial_statistics (:1533-1553, leaf compute_block_mean_compute_variance :307-1382).
// Both are pure HBM-bound streaming kernels (1.5625*P and P + 170*B bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "sad_device.hpp"

using namespace svthip;

namespace {

// One thread = one output dword (4 horizontally adjacent samples) of the PADDED destination plane.
// Output sample (X, Y) of the padded buffer = decimated sample (clamp(X-pad), clamp(Y-pad)): this is
// exactly what downsample followed by svt_aom_generate_padding produces.
// STEP = 2: mean of in(2i..2i+1, 2j..2j+1).  STEP = 4: mean of in(4i+1..4i+2, 4j+1..4j+2).
template <int STEP>
__device__ __forceinline__ void downsample_pad_body(const uint8_t *__restrict__ in, uint32_t in_stride, uint8_t *__restrict__ out,
                                                    uint32_t out_stride, uint32_t out_w, uint32_t out_h, uint32_t pad, uint32_t Y) {
    const uint32_t X4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;  // first padded column of this dword
    if (X4 >= out_stride || Y >= out_h + 2 * pad)
        return;
    int yi = (int)Y - (int)pad;
    yi     = yi < 0 ? 0 : (yi > (int)out_h - 1 ? (int)out_h - 1 : yi);
    constexpr int  OFF = STEP == 2 ? 0 : 1;
    const uint8_t *r0  = in + (size_t)(STEP * yi + OFF) * in_stride;
    const uint8_t *r1  = r0 + in_stride;
    uint32_t       res = 0;
    const int      x0  = (int)X4 - (int)pad;
    if (STEP == 2 && x0 >= 0 && x0 + 3 < (int)out_w && ((((uintptr_t)r0 | in_stride) & 3u) == 0) && ((x0 & 1) == 0)) {
        // interior fast path: 8 input bytes per row as two aligned dwords
        const uint32_t *pa = (const uint32_t *)(r0 + 2 * x0), *pb = (const uint32_t *)(r1 + 2 * x0);
        const uint2     a = make_uint2(pa[0], pa[1]), b = make_uint2(pb[0], pb[1]);
        // per 16-bit pair: bytes (lo, hi) of both rows
        auto avg2 = [](uint32_t ta, uint32_t tb, int sh) -> uint32_t {
            const uint32_t s = ((ta >> sh) & 0xff) + ((ta >> (sh + 8)) & 0xff) + ((tb >> sh) & 0xff) + ((tb >> (sh + 8)) & 0xff);
            return (s + 2) >> 2;
        };
        res = avg2(a.x, b.x, 0) | (avg2(a.x, b.x, 16) << 8) | (avg2(a.y, b.y, 0) << 16) | (avg2(a.y, b.y, 16) << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (X4 + k >= out_stride)
                break;
            int xi = x0 + k;
            xi     = xi < 0 ? 0 : (xi > (int)out_w - 1 ? (int)out_w - 1 : xi);
            const int      xs = STEP * xi + OFF;
            const uint32_t s  = (uint32_t)r0[xs] + r0[xs + 1] + r1[xs] + r1[xs + 1];
            res |= ((s + 2) >> 2) << (8 * k);
        }
    }
    uint8_t *o = out + (size_t)Y * out_stride + X4;
    if (X4 + 3 < out_stride && (((uintptr_t)o) & 3u) == 0) {
        *(uint32_t *)o = res;
    } else {
        for (int k = 0; k < 4 && X4 + k < out_stride; k++) o[k] = (uint8_t)(res >> (8 * k));
    }
}

template <int STEP>
__global__ __launch_bounds__(256) void downsample_pad_kernel(const uint8_t *__restrict__ in, uint32_t in_stride,
                                                             uint8_t *__restrict__ out, uint32_t out_stride,
                                                             uint32_t out_w, uint32_t out_h, uint32_t pad) {
    downsample_pad_body<STEP>(in, in_stride, out, out_stride, out_w, out_h, pad, blockIdx.y);
}

constexpr uint32_t BATCH_ROWS = 4;
// Batched form: blockIdx.z = picture.  level 0: full -> quarter (STEP 2), 1: quarter -> sixteenth (STEP 2),
// 2: full -> sixteenth (STEP 4, HME level 1 off).
__global__ __launch_bounds__(256) void downsample_pad_batch_kernel(const SvtHipAnalysisJob *__restrict__ jobs, int level) {
    const SvtHipPyramid8 &y = jobs[blockIdx.z].pyr;
    const SvtHipPlane8   &i = level == 1 ? y.quarter : y.full, &o = level == 0 ? y.quarter : y.sixteenth;
    const uint8_t        *in = i.buf + i.org_x + (size_t)i.org_y * i.stride;
    // BATCH_ROWS output rows per workgroup: a row of one dword per thread is too little work per launch slot
    for (uint32_t r = 0; r < BATCH_ROWS; r++) {
        if (level == 2)
            downsample_pad_body<4>(in, i.stride, o.buf, o.stride, o.width, o.height, o.org_x, blockIdx.y * BATCH_ROWS + r);
        else
            downsample_pad_body<2>(in, i.stride, o.buf, o.stride, o.width, o.height, o.org_x, blockIdx.y * BATCH_ROWS + r);
    }
}

// Edge replication of a plane in place (svt_aom_generate_padding); interior untouched.
__global__ __launch_bounds__(256) void pad_plane_kernel(uint8_t *__restrict__ buf, uint32_t stride, uint32_t w,
                                                        uint32_t h, uint32_t pad_x, uint32_t pad_y) {
    const uint32_t X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    if (X >= stride)
        return;
    const bool inside = X >= pad_x && X < pad_x + w && Y >= pad_y && Y < pad_y + h;
    if (inside)
        return;
    int xi = (int)X - (int)pad_x, yi = (int)Y - (int)pad_y;
    xi     = xi < 0 ? 0 : (xi > (int)w - 1 ? (int)w - 1 : xi);
    yi     = yi < 0 ? 0 : (yi > (int)h - 1 ? (int)h - 1 : yi);
    buf[(size_t)Y * stride + X] = buf[(size_t)(pad_y + yi) * stride + pad_x + xi];
}

// One wave64 per 64x64 block, one lane per 8x8 sub-block; 4 blocks per workgroup.
__device__ __forceinline__ void variance_body(const uint8_t *__restrict__ pic /* at (org_x, org_y) */, uint32_t stride, uint32_t b64_w,
                                              uint32_t n_b64, uint16_t *__restrict__ variance, uint64_t *__restrict__ mean,
                                              int full_precision) {
    __shared__ uint64_t m8[4][64], q8[4][64], m16[4][16], q16[4][16], m32[4][4], q32[4][4];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t b  = blockIdx.x * 4 + wv;
    const bool     on = b < n_b64;
    if (on) {
        const uint32_t bx = b % b64_w, by = b / b64_w;
        const uint32_t sx = lane & 7, sy = lane >> 3;
        const uint8_t *p  = pic + (size_t)(64 * by + 8 * sy) * stride + 64 * bx + 8 * sx;
        uint32_t       s = 0, ss = 0;
        const int      step = full_precision ? 1 : 2;
        for (int r = 0; r < 8; r += step) {
            const uint8_t *row = p + (size_t)r * stride;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const uint32_t v = row[c];
                s += v, ss += v * v;
            }
        }
        // sub-sampled: sum<<3, sumsq<<11 (pic_analysis_process.c:234-272); full: (sum<<8)/64, (sumsq<<16)/64
        m8[wv][lane] = full_precision ? ((uint64_t)s << 2) : ((uint64_t)s << 3);
        q8[wv][lane] = full_precision ? ((uint64_t)ss << 10) : ((uint64_t)ss << 11);
    }
    __syncthreads();
    if (on && lane < 16) {
        const uint32_t a = 16 * (lane >> 2) + 2 * (lane & 3);
        m16[wv][lane]    = (m8[wv][a] + m8[wv][a + 1] + m8[wv][a + 8] + m8[wv][a + 9]) >> 2;
        q16[wv][lane]    = (q8[wv][a] + q8[wv][a + 1] + q8[wv][a + 8] + q8[wv][a + 9]) >> 2;
    }
    __syncthreads();
    if (on && lane < 4) {
        const uint32_t a = 8 * (lane >> 1) + 2 * (lane & 1);
        m32[wv][lane]    = (m16[wv][a] + m16[wv][a + 1] + m16[wv][a + 4] + m16[wv][a + 5]) >> 2;
        q32[wv][lane]    = (q16[wv][a] + q16[wv][a + 1] + q16[wv][a + 4] + q16[wv][a + 5]) >> 2;
    }
    __syncthreads();
    if (!on)
        return;
    uint16_t *vo = variance + (size_t)85 * b;
    uint64_t *mo = mean ? mean + (size_t)85 * b : nullptr;
    for (uint32_t i = lane; i < 85; i += 64) {
        uint64_t m, q;
        if (i == 0) {
            m = (m32[wv][0] + m32[wv][1] + m32[wv][2] + m32[wv][3]) >> 2;
            q = (q32[wv][0] + q32[wv][1] + q32[wv][2] + q32[wv][3]) >> 2;
        } else if (i < 5) {
            m = m32[wv][i - 1], q = q32[wv][i - 1];
        } else if (i < 21) {
            m = m16[wv][i - 5], q = q16[wv][i - 5];
        } else {
            m = m8[wv][i - 21], q = q8[wv][i - 21];
        }
        vo[i] = (uint16_t)((q - m * m) >> 16);
        if (mo)
            mo[i] = m;
    }
}

__global__ __launch_bounds__(256) void variance_kernel(const uint8_t *__restrict__ pic, uint32_t stride, uint32_t b64_w, uint32_t n_b64,
                                                       uint16_t *__restrict__ variance, uint64_t *__restrict__ mean, int full_precision) {
    variance_body(pic, stride, b64_w, n_b64, variance, mean, full_precision);
}
__global__ __launch_bounds__(256) void variance_batch_kernel(const SvtHipAnalysisJob *__restrict__ jobs, int full_precision) {
    const SvtHipAnalysisJob &j = jobs[blockIdx.y];
    const SvtHipPlane8      &f = j.pyr.full;
    const uint32_t           bw = (f.width + 63u) / 64u, bh = (f.height + 63u) / 64u;
    variance_body(f.buf + f.org_x + (size_t)f.org_y * f.stride, f.stride, bw, bw * bh, j.variance, j.mean, full_precision);
}

// ------------------------------------------------------------------------------------------------
// Fused picture analysis: one read of the full plane gives both decimated planes, their padding and the block statistics.
// One wave64 per 128x64 tile of the full plane (two 64x64 blocks side by side), no barrier and no LDS.  Lane (px, py) =
// (lane & 7, lane >> 3) owns the 16x8 patch at (16 px, 8 py) of the tile and loads it as eight 16-byte rows, so one load
// instruction of the wave reads 8 rows of 128 contiguous bytes.  A patch is two whole 8x8 blocks, 8x4 quarter samples and
// 4x2 sixteenth samples: only the reduction tree of the statistics crosses lanes (shuffles), nothing crosses waves.
// The bytes loaded are exactly those variance_body reads (every row of every 64x64 block that exists; with sub-sampled
// statistics the odd rows below the picture are left out), so no load needs a clamped form.
// ------------------------------------------------------------------------------------------------
typedef uint64_t __attribute__((aligned(1))) u64_unaligned;
__device__ __forceinline__ void store_any(uint8_t *g, uint8_t v) { *(__attribute__((address_space(1))) uint8_t *)g = v; }
__device__ __forceinline__ void store_any(uint8_t *g, uint32_t v) { *(__attribute__((address_space(1))) dev::u32_unaligned *)g = v; }
__device__ __forceinline__ void store_any(uint8_t *g, uint64_t v) { *(__attribute__((address_space(1))) u64_unaligned *)g = v; }
__device__ __forceinline__ void store_any(uint8_t *g, dev::u128v v) { *(__attribute__((address_space(1))) dev::u128_unaligned *)g = v; }

// n copies of the byte v from p on, any alignment
__device__ __forceinline__ void fill_bytes(uint8_t *p, uint32_t n, uint32_t v) {
    const uint32_t   w  = v * 0x01010101u;
    const dev::u128v w4 = {w, w, w, w};
    uint32_t         i  = 0;
    for (; i + 16 <= n; i += 16) store_any(p + i, w4);
    for (; i < n; i++) store_any(p + i, (uint8_t)v);
}

// bytes (a0 a1 a2 a3), (b0 b1 b2 b3) -> (a0 + a1 + b0 + b1 + 2) >> 2 in bits 0-7 and (a2 + a3 + b2 + b3 + 2) >> 2 in bits 16-23
__device__ __forceinline__ uint32_t avg2x2_pairs(uint32_t a, uint32_t b) {
    const uint32_t s = (a & 0x00ff00ffu) + ((a >> 8) & 0x00ff00ffu) + (b & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu) + 0x00020002u;
    return (s >> 2) & 0x00ff00ffu;
}
// the two means of `lo` and the two of `hi` as four adjacent bytes
__device__ __forceinline__ uint32_t pack_pairs(uint32_t lo, uint32_t hi) {
    return ((lo | (lo >> 8)) & 0xffffu) | ((hi | (hi >> 8)) << 16);
}

// The CL x RL samples one lane holds of a decimated plane, at column cx0 / row cy0 of its picture area (r0 .. r3: CL bytes
// each, first column lowest), go to the plane together with the replicated padding they define: the lanes holding column 0 /
// the last column write the left / right padding of their rows (right: up to the stride), the lanes holding row 0 / the
// last row repeat that over the top / bottom padding rows, corners included.  Every byte of stride * (height + 2 * pad)
// is written by exactly one lane, as downsample_pad_body leaves it.
template <int CL, int RL>
__device__ __forceinline__ void store_decimated(const SvtHipPlane8 &o, uint32_t cx0, uint32_t cy0, uint64_t r0, uint64_t r1, uint64_t r2 = 0,
                                                uint64_t r3 = 0) {
    const uint32_t dw = o.width, dh = o.height, pad = o.org_x, stride = o.stride;
    if (cx0 >= dw || cy0 >= dh)
        return;
    const uint32_t nc = dw - cx0 < (uint32_t)CL ? dw - cx0 : (uint32_t)CL, nr = dh - cy0 < (uint32_t)RL ? dh - cy0 : (uint32_t)RL;
    const bool     left = cx0 == 0, right = cx0 + nc == dw;
    // rows of the padded plane this lane writes: its own, preceded by the top padding / followed by the bottom padding
    const uint32_t y_own = pad + cy0, y_beg = cy0 == 0 ? 0 : y_own, y_end = cy0 + nr == dh ? dh + 2 * pad : y_own + nr;
    for (uint32_t Y = y_beg; Y < y_end; Y++) {
        const uint32_t r = Y < y_own ? 0 : (Y - y_own < nr ? Y - y_own : nr - 1);
        uint64_t       v = r == 1 ? r1 : r0;  // scalars, not an array: a row picked by a run-time index stays in registers
        if (RL == 4)
            v = r == 2 ? r2 : (r == 3 ? r3 : v);
        uint8_t *row = o.buf + (size_t)Y * stride, *p = row + pad + cx0;
        if (nc == (uint32_t)CL) {
            if (CL == 8)
                store_any(p, v);
            else
                store_any(p, (uint32_t)v);
        } else {
            for (uint32_t k = 0; k < nc; k++) store_any(p + k, (uint8_t)(v >> (8 * k)));
        }
        if (left)
            fill_bytes(row, pad, (uint32_t)v & 0xffu);
        if (right)
            fill_bytes(row + pad + dw, stride - pad - dw, (uint32_t)(v >> (8 * (nc - 1))) & 0xffu);
    }
}

__device__ __forceinline__ uint64_t xor_add(uint64_t v, int mask) { return v + __shfl_xor((unsigned long long)v, mask, 64); }

template <bool L1, bool FP>
__device__ __forceinline__ void analysis_fused_body(const SvtHipAnalysisJob &j) {
    const SvtHipPlane8 &f  = j.pyr.full;
    const uint32_t      W = f.width, H = f.height;
    const uint32_t      bw = (W + 63u) / 64u, bh = (H + 63u) / 64u, tw = (bw + 1u) / 2u;  // 64x64 blocks, tiles per row
    const uint32_t      t = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= tw * bh)  // the grid is sized by the largest job; uniform over the wave
        return;
    const uint32_t ty = t / tw, tx = t - ty * tw;
    const uint32_t lane = threadIdx.x & 63u, px = lane & 7u, py = lane >> 3;
    const uint32_t bx = 2u * tx + (px >> 2);
    const bool     on = bx < bw;  // the right half of the last tile of a row may have no block
    const uint32_t X0 = 128u * tx + 16u * px, Y0 = 64u * ty + 8u * py;
    // Eight loads with no branch between them, so all are in flight at once.  A lane without a block loads what the lane
    // 64 columns to its left loads, and an odd row below the picture that sub-sampled statistics do not read is replaced by
    // the even row above it: neither value is ever used (see below), and no byte is read that variance_body does not read.
    const uint8_t *p = f.buf + f.org_x + (on ? X0 : X0 - 64u) + (size_t)(f.org_y + Y0) * f.stride;
    dev::u128v     d[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint32_t rl = FP || !(r & 1) || Y0 + r < H ? r : r - 1;
        d[r]              = dev::load_u128_any(p + (size_t)rl * f.stride);
    }

    // decimated planes.  A lane of a block that does not exist lies right of every decimated sample and writes nothing;
    // a row pair with a replaced row lies below them.
    uint64_t s16[2];
    if (L1) {
        uint64_t q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const dev::u128v a = d[2 * k], b = d[2 * k + 1];
            q[k] = dev::pair64(pack_pairs(avg2x2_pairs(a.x, b.x), avg2x2_pairs(a.y, b.y)),
                               pack_pairs(avg2x2_pairs(a.z, b.z), avg2x2_pairs(a.w, b.w)));
        }
        store_decimated<8, 4>(j.pyr.quarter, X0 >> 1, Y0 >> 1, q[0], q[1], q[2], q[3]);
#pragma unroll
        for (int k = 0; k < 2; k++)  // from the rounded quarter samples, as the second downsample does
            s16[k] = pack_pairs(avg2x2_pairs((uint32_t)q[2 * k], (uint32_t)q[2 * k + 1]),
                                avg2x2_pairs((uint32_t)(q[2 * k] >> 32), (uint32_t)(q[2 * k + 1] >> 32)));
    } else {
#pragma unroll
        for (int k = 0; k < 2; k++) {  // STEP 4: columns 4i + 1, 4i + 2 of rows 4j + 1, 4j + 2
            const dev::u128v a = d[4 * k + 1], b = d[4 * k + 2];
            auto mid = [](uint32_t ta, uint32_t tb) -> uint32_t {
                return (((ta >> 8) & 0xffu) + ((ta >> 16) & 0xffu) + ((tb >> 8) & 0xffu) + ((tb >> 16) & 0xffu) + 2u) >> 2;
            };
            s16[k] = mid(a.x, b.x) | (mid(a.y, b.y) << 8) | (mid(a.z, b.z) << 16) | (mid(a.w, b.w) << 24);
        }
    }
    store_decimated<4, 2>(j.pyr.sixteenth, X0 >> 2, Y0 >> 2, s16[0], s16[1]);

    // statistics of the two 8x8 blocks of the patch, then the tree of variance_body: the 16x16 block is both 8x8 of this
    // lane and of lane ^ 8, the 32x32 block joins lanes ^ 1 and ^ 16, the 64x64 block lanes ^ 2 and ^ 32.  The two blocks
    // of a tile differ in bit 2 of the lane and never mix, so what a lane without a block carries does not matter.
    uint32_t sa = 0, sb = 0, qa = 0, qb = 0;
#pragma unroll
    for (int r = 0; r < 8; r += FP ? 1 : 2) {
        sa = __builtin_amdgcn_sad_u8(d[r].y, 0u, __builtin_amdgcn_sad_u8(d[r].x, 0u, sa));
        sb = __builtin_amdgcn_sad_u8(d[r].w, 0u, __builtin_amdgcn_sad_u8(d[r].z, 0u, sb));
        qa = __builtin_amdgcn_udot4(d[r].y, d[r].y, __builtin_amdgcn_udot4(d[r].x, d[r].x, qa, false), false);
        qb = __builtin_amdgcn_udot4(d[r].w, d[r].w, __builtin_amdgcn_udot4(d[r].z, d[r].z, qb, false), false);
    }
    // sub-sampled: sum << 3, sumsq << 11; full: (sum << 8) / 64, (sumsq << 16) / 64
    const uint64_t m8a = (uint64_t)sa << (FP ? 2 : 3), m8b = (uint64_t)sb << (FP ? 2 : 3);
    const uint64_t q8a = (uint64_t)qa << (FP ? 10 : 11), q8b = (uint64_t)qb << (FP ? 10 : 11);
    const uint64_t m16 = xor_add(m8a + m8b, 8) >> 2, q16 = xor_add(q8a + q8b, 8) >> 2;
    const uint64_t m32 = xor_add(xor_add(m16, 1), 16) >> 2, q32 = xor_add(xor_add(q16, 1), 16) >> 2;
    const uint64_t m64 = xor_add(xor_add(m32, 2), 32) >> 2, q64 = xor_add(xor_add(q32, 2), 32) >> 2;
    if (!on)
        return;
    const uint32_t b  = ty * bw + bx, cx = px & 3u;
    uint16_t      *vo = j.variance + (size_t)85 * b;
    uint64_t      *mo = j.mean ? j.mean + (size_t)85 * b : nullptr;
    auto put = [&](uint32_t i, uint64_t m, uint64_t q) {  // global stores, not the flat ones a generic pointer gets
        *(__attribute__((address_space(1))) uint16_t *)(vo + i) = (uint16_t)((q - m * m) >> 16);
        if (mo)
            *(__attribute__((address_space(1))) uint64_t *)(mo + i) = m;
    };
    put(21u + 8u * py + 2u * cx, m8a, q8a);
    put(22u + 8u * py + 2u * cx, m8b, q8b);
    if (!(py & 1u))
        put(5u + 4u * (py >> 1) + cx, m16, q16);
    if (!(py & 3u) && !(cx & 1u))
        put(1u + 2u * (py >> 2) + (cx >> 1), m32, q32);
    if (py == 0 && cx == 0)
        put(0, m64, q64);
}

// blockIdx.y = picture, four tiles (waves) per workgroup
template <bool L1, bool FP>
__global__ __launch_bounds__(256) void analysis_fused_kernel(const SvtHipAnalysisJob *__restrict__ jobs) {
    // A copy made in 8-byte words: the whole descriptor comes through scalar loads up front (its 16-bit fields would each
    // take a vector load and a wait where they are first used) and stays in scalar registers across the stores.
    SvtHipAnalysisJob j;
    static_assert(sizeof(j) % 8 == 0 && alignof(SvtHipAnalysisJob) == 8, "copied as 64-bit words");
    uint64_t w[sizeof(j) / 8];
#pragma unroll
    for (uint32_t i = 0; i < sizeof(j) / 8; i++) w[i] = ((const uint64_t *)(jobs + blockIdx.y))[i];
    memcpy(&j, w, sizeof(j));
    analysis_fused_body<L1, FP>(j);
}

// The fused kernel takes decimated planes of the sizes the reference allocates (max_width >> 1 and >> 2, and the same of
// the height: reference_object.c:227-241); with those every decimated sample depends on samples of its own tile only.
bool fused_sizes(const SvtHipPyramid8 &y, int32_t hme_level1_enabled) {
    const uint32_t w = y.full.width, h = y.full.height;
    return y.sixteenth.width == (w >> 2) && y.sixteenth.height == (h >> 2) &&
           (!hme_level1_enabled || (y.quarter.width == (w >> 1) && y.quarter.height == (h >> 1)));
}

bool plane_ok(const SvtHipPlane8 *p) {
    return p && p->buf && p->width && p->height && p->stride >= (uint32_t)p->width + 2u * p->org_x;
}

}  // namespace

extern "C" int32_t svt_hip_pyramid_frame(const SvtHipPlane8 *full, const SvtHipPlane8 *quarter,
                                         const SvtHipPlane8 *sixteenth, int32_t hme_level1_enabled, void *stream) {
    if (!plane_ok(full) || !plane_ok(sixteenth) || (hme_level1_enabled && !plane_ok(quarter)))
        return refuse("svt_hip_pyramid_frame: bad plane descriptor");
    // The reference writes the decimated picture at org_x + org_x*stride (pic_analysis_process.c:1934,1953):
    // it only works for org_x == org_y, and so do we.
    if (sixteenth->org_x != sixteenth->org_y || (hme_level1_enabled && quarter->org_x != quarter->org_y))
        return refuse("svt_hip_pyramid_frame: decimated planes need org_x == org_y (reference quirk)");
    TierBCall c("svt_hip_pyramid_frame", stream);
    if (!c.ok())
        return c.status();
    hipStream_t    st   = c.stream();
    const uint8_t *fsrc = full->buf + full->org_x + (size_t)full->org_y * full->stride;
    auto launch = [&](const uint8_t *in, uint32_t in_stride, const SvtHipPlane8 *o, int step) {
        const uint32_t rows = o->height + 2u * o->org_y;
        dim3           grid((o->stride / 4 + 1 + 255) / 256, rows);
        if (step == 2)
            hipLaunchKernelGGL(downsample_pad_kernel<2>, grid, dim3(256), 0, st, in, in_stride, o->buf, o->stride,
                               (uint32_t)o->width, (uint32_t)o->height, (uint32_t)o->org_x);
        else
            hipLaunchKernelGGL(downsample_pad_kernel<4>, grid, dim3(256), 0, st, in, in_stride, o->buf, o->stride,
                               (uint32_t)o->width, (uint32_t)o->height, (uint32_t)o->org_x);
    };
    if (hme_level1_enabled) {
        launch(fsrc, full->stride, quarter, 2);
        launch(quarter->buf + quarter->org_x + (size_t)quarter->org_y * quarter->stride, quarter->stride, sixteenth, 2);
    } else {
        launch(fsrc, full->stride, sixteenth, 4);
    }
    return c.finish();
}

extern "C" int32_t svt_hip_pad_plane(const SvtHipPlane8 *plane, void *stream) {
    if (!plane_ok(plane))
        return refuse("svt_hip_pad_plane: bad plane descriptor");
    TierBCall c("svt_hip_pad_plane", stream);
    if (!c.ok())
        return c.status();
    dim3 grid((plane->stride + 255) / 256, plane->height + 2u * plane->org_y);
    hipLaunchKernelGGL(pad_plane_kernel, grid, dim3(256), 0, c.stream(), plane->buf, plane->stride,
                       (uint32_t)plane->width, (uint32_t)plane->height, (uint32_t)plane->org_x, (uint32_t)plane->org_y);
    return c.finish();
}

extern "C" int32_t svt_hip_variance_frame(const SvtHipPlane8 *full, uint16_t *d_variance, uint64_t *d_mean,
                                          int32_t full_precision, void *stream) {
    if (!plane_ok(full) || !d_variance)
        return refuse("svt_hip_variance_frame: bad argument");
    TierBCall c("svt_hip_variance_frame", stream);
    if (!c.ok())
        return c.status();
    const uint32_t bw = (full->width + 63u) / 64u, bh = (full->height + 63u) / 64u, nb = bw * bh;
    hipLaunchKernelGGL(variance_kernel, dim3((nb + 3) / 4), dim3(256), 0, c.stream(),
                       (const uint8_t *)(full->buf + full->org_x + (size_t)full->org_y * full->stride), full->stride, bw,
                       nb, d_variance, d_mean, (int)full_precision);
    return c.finish();
}

// Batched picture analysis: pyramids + variances of n pictures in one fused launch (blockIdx.y = picture), or in the three
// launches of the single-picture kernels' batch forms (blockIdx.z / .y = picture) when a descriptor has other sizes.
extern "C" int32_t svt_hip_analysis_frames(const SvtHipAnalysisJob *jobs, uint32_t n_jobs, int32_t hme_level1_enabled,
                                           int32_t full_precision, void *stream) {
    if (!jobs || n_jobs == 0 || n_jobs > 65535)
        return refuse("svt_hip_analysis_frames: bad job count");
    // SVTAV1_HIP_ANALYSIS_FUSED=0: every batch through the three launches, for A/B runs
    static const bool fused_on = !(getenv("SVTAV1_HIP_ANALYSIS_FUSED") && atoi(getenv("SVTAV1_HIP_ANALYSIS_FUSED")) == 0);
    bool              fused    = fused_on;
    uint32_t max_q_stride = 0, max_q_rows = 0, max_s_stride = 0, max_s_rows = 0, max_nb = 0, max_tiles = 0;
    for (uint32_t i = 0; i < n_jobs; i++) {
        const SvtHipPyramid8 &y = jobs[i].pyr;
        if (!plane_ok(&y.full) || !plane_ok(&y.sixteenth) || (hme_level1_enabled && !plane_ok(&y.quarter)) || !jobs[i].variance ||
            y.sixteenth.org_x != y.sixteenth.org_y || (hme_level1_enabled && y.quarter.org_x != y.quarter.org_y))
            return refuse("svt_hip_analysis_frames: job %u: bad plane descriptor / missing output", i);
        max_q_stride = y.quarter.stride > max_q_stride ? y.quarter.stride : max_q_stride;
        max_q_rows   = y.quarter.height + 2u * y.quarter.org_y > max_q_rows ? y.quarter.height + 2u * y.quarter.org_y : max_q_rows;
        max_s_stride = y.sixteenth.stride > max_s_stride ? y.sixteenth.stride : max_s_stride;
        max_s_rows   = y.sixteenth.height + 2u * y.sixteenth.org_y > max_s_rows ? y.sixteenth.height + 2u * y.sixteenth.org_y : max_s_rows;
        const uint32_t nb = ((y.full.width + 63u) / 64u) * ((y.full.height + 63u) / 64u);
        max_nb            = nb > max_nb ? nb : max_nb;
        const uint32_t nt = (((y.full.width + 63u) / 64u + 1u) / 2u) * ((y.full.height + 63u) / 64u);
        max_tiles         = nt > max_tiles ? nt : max_tiles;
        fused             = fused && fused_sizes(y, hme_level1_enabled);
    }
    TierBCall                c("svt_hip_analysis_frames", stream);
    const SvtHipAnalysisJob *d_jobs = (const SvtHipAnalysisJob *)c.stage(jobs, (size_t)n_jobs * sizeof(SvtHipAnalysisJob));
    if (!d_jobs)
        return c.status();
    hipStream_t st = c.stream();
    if (fused) {
        const dim3 grid((max_tiles + 3) / 4, n_jobs);
        if (hme_level1_enabled && full_precision)
            hipLaunchKernelGGL((analysis_fused_kernel<true, true>), grid, dim3(256), 0, st, d_jobs);
        else if (hme_level1_enabled)
            hipLaunchKernelGGL((analysis_fused_kernel<true, false>), grid, dim3(256), 0, st, d_jobs);
        else if (full_precision)
            hipLaunchKernelGGL((analysis_fused_kernel<false, true>), grid, dim3(256), 0, st, d_jobs);
        else
            hipLaunchKernelGGL((analysis_fused_kernel<false, false>), grid, dim3(256), 0, st, d_jobs);
        return c.finish();
    }
    if (hme_level1_enabled) {
        hipLaunchKernelGGL(downsample_pad_batch_kernel, dim3((max_q_stride / 4 + 1 + 255) / 256, (max_q_rows + BATCH_ROWS - 1) / BATCH_ROWS, n_jobs), dim3(256), 0, st, d_jobs, 0);
        hipLaunchKernelGGL(downsample_pad_batch_kernel, dim3((max_s_stride / 4 + 1 + 255) / 256, (max_s_rows + BATCH_ROWS - 1) / BATCH_ROWS, n_jobs), dim3(256), 0, st, d_jobs, 1);
    } else {
        hipLaunchKernelGGL(downsample_pad_batch_kernel, dim3((max_s_stride / 4 + 1 + 255) / 256, (max_s_rows + BATCH_ROWS - 1) / BATCH_ROWS, n_jobs), dim3(256), 0, st, d_jobs, 2);
    }
    hipLaunchKernelGGL(variance_batch_kernel, dim3((max_nb + 3) / 4, n_jobs), dim3(256), 0, st, d_jobs, (int)full_precision);
    return c.finish();
}

// ------------------------------------------------------------------------------------------------
// Tier A (host pointers): stage the touched bytes, run the same kernels, copy back.
// ------------------------------------------------------------------------------------------------
// Generic strided decimation used by the per-call entry point (no padding involved).
__global__ __launch_bounds__(256) static void downsample_plain_kernel(const uint8_t *__restrict__ in, uint32_t in_stride,
                                                                       uint32_t in_w, uint32_t in_h,
                                                                       uint8_t *__restrict__ out, uint32_t out_stride,
                                                                       uint32_t step) {
    const uint32_t ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    const uint32_t half = step >> 1, x = half + ox * step, y = half + oy * step;
    if (x >= in_w || y >= in_h)
        return;
    const uint8_t *p = in + (size_t)y * in_stride + x;
    const uint32_t s = (uint32_t)p[-(ptrdiff_t)in_stride - 1] + p[-(ptrdiff_t)in_stride] + p[-1] + p[0];
    out[(size_t)oy * out_stride + ox] = (uint8_t)((s + 2) >> 2);
}

TIER_A_LEAF(void, svt_aom_downsample_2d,
            (uint8_t *input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height, uint8_t
             *decim_samples, uint32_t decim_stride, uint32_t decim_step),
            (input_samples, input_stride, input_area_width, input_area_height, decim_samples, decim_stride, decim_step)) {
    const uint32_t half = decim_step >> 1;
    if (decim_step == 0 || input_area_width <= half || input_area_height <= half)
        return;
    TierAStage     s("svt_aom_downsample_2d");
    const uint32_t ow = (input_area_width - half + decim_step - 1) / decim_step;
    const uint32_t oh = (input_area_height - half + decim_step - 1) / decim_step;
    // reads start one row / one column before (half,half): rows half-1 .., columns half-1 ..
    const size_t   in_first = (size_t)(half - 1) * input_stride + (half - 1);
    const size_t   in_span  = (size_t)(input_area_height - half) * input_stride + (input_area_width - half + 1);
    const size_t   out_span = (size_t)(oh - 1) * decim_stride + ow;
    const size_t   off_in = s.in(input_samples + in_first, in_span, 256), off_out = s.out(out_span);
    s.upload();
    // device pointer equivalent of `input_samples`: never dereferenced below in_first
    hipLaunchKernelGGL(downsample_plain_kernel, dim3((ow + 255) / 256, oh), dim3(256), 0, s.stream(), s.dev<const uint8_t>(off_in) - in_first,
                       input_stride, input_area_width, input_area_height, s.dev(off_out), decim_stride, decim_step);
    s.finish(off_out, out_span);
    copy_rows(decim_samples, decim_stride, s.host(off_out), decim_stride, oh, ow);
}

// 8x8 block statistics: n8 side-by-side 8x8 blocks, (sum, sum of squares) over rows 0..7 step `rstep`.
__global__ __launch_bounds__(64) static void block8_stats_kernel(const uint8_t *__restrict__ in, uint32_t stride,
                                                                 uint32_t n8, uint32_t w, uint32_t hrows, uint32_t rstep,
                                                                 uint32_t *__restrict__ out) {
    const uint32_t k = threadIdx.x;
    if (k >= n8)
        return;
    uint32_t s = 0, ss = 0;
    for (uint32_t r = 0; r < hrows; r += rstep)
        for (uint32_t c = 0; c < w; c++) {
            const uint32_t v = in[(size_t)r * stride + w * k + c];
            s += v, ss += v * v;
        }
    out[2 * k] = s, out[2 * k + 1] = ss;
}

static void block_stats_host(const uint8_t *in, uint32_t stride, uint32_t n8, uint32_t w, uint32_t hrows, uint32_t rstep,
                             uint32_t *res /* 2*n8 */) {
    TierAStage   s("block statistics");
    const size_t off_in = s.in(in, (size_t)(hrows - 1) * stride + (size_t)w * n8, 256), off_out = s.out(8 * n8);
    s.upload();
    hipLaunchKernelGGL(block8_stats_kernel, dim3(1), dim3(64), 0, s.stream(), s.dev<const uint8_t>(off_in), stride, n8, w, hrows, rstep,
                       s.dev<uint32_t>(off_out));
    s.finish(off_out, 8 * n8);
    memcpy(res, s.host(off_out), 8 * n8);
}

TIER_A_LEAF(void, svt_compute_interm_var_four8x8,
            (uint8_t *input_samples, uint16_t input_stride, uint64_t *mean_of8x8_blocks, uint64_t *mean_of_squared8x8_blocks),
            (input_samples, input_stride, mean_of8x8_blocks, mean_of_squared8x8_blocks)) {
    uint32_t r[8];
    block_stats_host(input_samples, input_stride, 4, 8, 8, 2, r);
    for (int k = 0; k < 4; k++) {
        mean_of8x8_blocks[k]         = (uint64_t)r[2 * k] << 3;
        mean_of_squared8x8_blocks[k] = (uint64_t)r[2 * k + 1] << 11;
    }
}
TIER_A_LEAF(uint64_t, svt_compute_sub_mean_8x8,
            (uint8_t *input_samples, uint16_t input_stride),
            (input_samples, input_stride)) {
    uint32_t r[2];
    block_stats_host(input_samples, input_stride, 1, 8, 8, 2, r);
    return (uint64_t)r[0] << 3;
}
TIER_A_LEAF(uint64_t, svt_compute_mean_8x8,
            (uint8_t *input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height),
            (input_samples, input_stride, input_area_width, input_area_height)) {
    uint32_t r[2];
    block_stats_host(input_samples, input_stride, 1, input_area_width, input_area_height, 1, r);
    return ((uint64_t)r[0] << 8) / (input_area_width * input_area_height);
}
TIER_A_LEAF(uint64_t, svt_compute_mean_square_values_8x8,
            (uint8_t *input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height),
            (input_samples, input_stride, input_area_width, input_area_height)) {
    uint32_t r[2];
    block_stats_host(input_samples, input_stride, 1, input_area_width, input_area_height, 1, r);
    return ((uint64_t)r[1] << 16) / (input_area_width * input_area_height);
}

SVT_HIP_MODULE_WARMUP(pyramid)
