// warp_device.hpp — the 8 x 8 block of AV1's warp filter (svt_av1_warp_affine_c, warped_motion.c:570-680, and its 16-bit twin)
// for one wave, shared by the prediction and the global-motion error kernels of inter_warp.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace svthip {
namespace warp {

constexpr int FILTER_ROWS = 193;  // WARPEDPIXEL_PREC_SHIFTS * 3 + 1 rows of 8 taps
constexpr int PREC_BITS   = 16;   // WARPEDMODEL_PREC_BITS
constexpr int DIFF_BITS   = 10;   // WARPEDDIFF_PREC_BITS
constexpr int REDUCE_BITS = 6;    // WARP_PARAM_REDUCE_BITS

struct Model {  // wmmat[0 .. 5] and the shear of EbWarpedMotionParams
    int32_t mat[6];
    int     alpha, beta, gamma, delta;
};

// is_affine_shear_allowed (warped_motion.c:357-363).  With it, every filter index of a block lies in [0, FILTER_ROWS): the index
// depends on the 16-bit fraction of the block centre and on at most 4 |alpha| + 7 |beta| (4 |gamma| + 4 |delta|) beyond it.
__host__ __device__ inline bool shear_allowed(int alpha, int beta, int gamma, int delta) {
    return 4 * abs(alpha) + 7 * abs(beta) < (1 << PREC_BITS) && 4 * abs(gamma) + 4 * abs(delta) < (1 << PREC_BITS);
}

__device__ inline int round_shift(int v, int n) { return (v + ((1 << n) >> 1)) >> n; }

// reduce_bits_horiz of both reference functions (the 8-bit one is the 16-bit one with bd = 8 for round_0 >= 1)
__device__ inline int reduce_bits_horiz(int bd, int round_0) { return round_0 + max(bd + 7 - round_0 - 14, 0); }

struct WaveLds {             // one wave's staging
    uint16_t win[15][16];    // the clamped 15 x 15 source window
    // the 15 x 8 horizontal sums: bd + 8 - reduce_bits_horiz <= 15 bits.  reduce_bits_horiz is max(round_0, bd - 7), so that
    // holds for every round_0 >= 1 a descriptor may carry, not only for the rounds of get_conv_params
    uint16_t hs[15][8];
};

// The filter table into LDS, by the whole workgroup; the first barrier inside block8() publishes it.
__device__ inline void load_filter(int16_t *lds, const int16_t *__restrict__ table) {
    for (int t = (int)threadIdx.x; t < FILTER_ROWS * 8; t += (int)blockDim.x) lds[t] = table[t];
}

// The 8 x 8 block whose top-left output sample is (i, j) of the plane.  Every wave of the workgroup calls this the same number
// of times (two barriers inside); a wave without a block passes active == false.  Returns the vertical filter's sum, offset
// included and not yet rounded, of output sample (lane >> 3, lane & 7) of the block.
template <bool IS16>
__device__ inline int block8(const void *__restrict__ ref, uint32_t stride, int width, int height, const Model &m, int i, int j, int ssx,
                             int ssy, int bd, int reduce_h, const int16_t *filt, WaveLds &l, int lane, bool active) {
    int sx4 = 0, sy4 = 0;
    if (active) {
        // the reference's int32 arithmetic, with the wrap-around spelled out
        const uint32_t src_x = (uint32_t)(j + 4) << ssx, src_y = (uint32_t)(i + 4) << ssy;
        const int32_t  dst_x = (int32_t)((uint32_t)m.mat[2] * src_x + (uint32_t)m.mat[3] * src_y + (uint32_t)m.mat[0]);
        const int32_t  dst_y = (int32_t)((uint32_t)m.mat[4] * src_x + (uint32_t)m.mat[5] * src_y + (uint32_t)m.mat[1]);
        const int32_t  x4 = dst_x >> ssx, y4 = dst_y >> ssy;
        const int      ix4 = x4 >> PREC_BITS, iy4 = y4 >> PREC_BITS;
        sx4 = ((x4 & ((1 << PREC_BITS) - 1)) - 4 * m.alpha - 4 * m.beta) & ~((1 << REDUCE_BITS) - 1);
        sy4 = ((y4 & ((1 << PREC_BITS) - 1)) - 4 * m.gamma - 4 * m.delta) & ~((1 << REDUCE_BITS) - 1);
        for (int t = lane; t < 15 * 15; t += 64) {
            const int    r = t / 15, c = t - r * 15;
            const int    y = min(max(iy4 - 7 + r, 0), height - 1), x = min(max(ix4 - 7 + c, 0), width - 1);
            const size_t at = (size_t)y * stride + x;
            l.win[r][c] = IS16 ? ((const uint16_t *)ref)[at] : ((const uint8_t *)ref)[at];
        }
    }
    __syncthreads();
    if (active) {
        for (int t = lane; t < 15 * 8; t += 64) {  // two horizontal sums per lane
            const int      r = t >> 3, c = t & 7;
            const int      sx = sx4 + m.beta * (r - 3) + m.alpha * c;
            const int16_t *coeffs = filt + (round_shift(sx, DIFF_BITS) + 64) * 8;
            int            sum = 1 << (bd + 6);
#pragma unroll
            for (int k = 0; k < 8; k++) sum += (int)l.win[r][c + k] * coeffs[k];
            l.hs[r][c] = (uint16_t)round_shift(sum, reduce_h);
        }
    }
    __syncthreads();
    int sum = 0;
    if (active) {  // one output sample per lane
        const int      r = lane >> 3, c = lane & 7;
        const int      sy = sy4 + m.delta * r + m.gamma * c;
        const int16_t *coeffs = filt + (round_shift(sy, DIFF_BITS) + 64) * 8;
        sum = 1 << (bd + 14 - reduce_h);
#pragma unroll
        for (int k = 0; k < 8; k++) sum += (int)l.hs[r + k][c] * coeffs[k];
    }
    return sum;
}

}  // namespace warp
}  // namespace svthip
