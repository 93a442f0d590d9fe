// ifs_device.hpp — the pieces of the interpolation filter search (inter_ifs.hip): one sample of an sr or a jnt prediction from a
// reference window staged in LDS, with the tap arithmetic of convolve_device.hpp (convolve_tile_t, whose results these must equal sample
// for sample), and the Laplacian rate / distortion model of enc_inter_prediction.c:2178-2275.
#pragma once
#include "convolve_device.hpp"

namespace svthip {
namespace ifs {

using namespace conv;

constexpr int ROUND_0 = 3, ROUND_1_SINGLE = 11, ROUND_1_COMPOUND = 7;  // get_conv_params_no_round at 8 and 10 bit (convolve.h:40-68)

// One reference of a block under one filter pair: its window in LDS (`in`, rows of IP, staged with the margins of the directions that have
// a phase), the horizontal pass's intermediate (`im`, rows of TILE, filled only when both directions have one), and the taps of its two
// phases, uniform, the horizontal ones as packed pairs.
struct Ref {
    const uint16_t *in;
    const int16_t  *im;
    bool            hx, hy;
    uint32_t        xp[4];
    int32_t         y[8];
};

__device__ __forceinline__ void load_taps_x(Ref &f, const int16_t *filters, int bank, int phase) {
    const int16_t *t = filters + (bank * 16 + phase) * 8;
#pragma unroll
    for (int k = 0; k < 4; k++) f.xp[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(uint16_t)t[2 * k] | ((uint32_t)(uint16_t)t[2 * k + 1] << 16)));
}
__device__ __forceinline__ void load_taps_y(Ref &f, const int16_t *filters, int bank, int phase) {
    const int16_t *t = filters + (bank * 16 + phase) * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) f.y[k] = __builtin_amdgcn_readfirstlane((int)t[k]);
}

// the tw x th tile at (x0, y0) of the block and its margins into `in`
template <int NT>
__device__ __forceinline__ void stage_window(uint16_t *__restrict__ in, const void *ref, uint32_t stride, int x0, int y0, int tw, int th, bool hx, bool hy, int is16) {
    const int fo_h = hx ? 3 : 0, fo_v = hy ? 3 : 0, ew = tw + (hx ? 7 : 0), eh = th + (hy ? 7 : 0);
    for (int idx = threadIdx.x; idx < eh * ew; idx += NT) {
        const int r = idx / ew, c = idx - r * ew;
        in[r * IP + c] = (uint16_t)ldpx(ref, (ptrdiff_t)(y0 + r - fo_v) * (ptrdiff_t)stride + (x0 + c - fo_h), is16);
    }
}

// the horizontal pass of 2d_sr and of jnt_2d (the same arithmetic): th + 7 rows
template <int NT> __device__ __forceinline__ void horizontal_pass(const Ref &f, int16_t *__restrict__ im, int tw, int th, int bd) {
    for (int idx = threadIdx.x; idx < (th + 7) * tw; idx += NT) {
        const int r = idx / tw, c = idx - r * tw;
        im[r * TILE + c] = (int16_t)(uint16_t)rnd(hsum8(f.in, r * IP + c, f.xp, 1 << (bd + FILTER_BITS - 1)), ROUND_0);
    }
}

__device__ __forceinline__ int32_t clip_bd(int32_t v, int bd) {
    const int32_t hi = (1 << bd) - 1;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

// svt_av1_convolve_{2d, x, y, 2d_copy}_sr and the highbd set: the predicted sample
__device__ __forceinline__ int32_t sr_sample(const Ref &f, int r, int c, int bd, bool is16) {
    constexpr int r0 = ROUND_0, r1 = ROUND_1_SINGLE;
    if (f.hx && f.hy) {
        const int bits = 2 * FILTER_BITS - r0 - r1, offset_bits = bd + 2 * FILTER_BITS - r0;
        int32_t   sum = 1 << offset_bits;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += f.y[k] * (int32_t)f.im[(r + k) * TILE + c];
        int32_t res = rnd(sum, r1) - ((1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1)));
        if (!is16)
            res = (int16_t)res;  // the 8-bit function narrows to int16 first (inter_prediction.c:343-345)
        return clip_bd(rnd(res, bits), bd);
    }
    if (f.hx)
        return clip_bd(rnd(rnd(hsum8(f.in, r * IP + c, f.xp, 0), r0), FILTER_BITS - r0), bd);
    if (f.hy) {
        int32_t res = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) res += f.y[k] * (int32_t)f.in[(r + k) * IP + c];
        return clip_bd(rnd(res, FILTER_BITS), bd);
    }
    return f.in[r * IP + c];
}

// svt_av1_jnt_convolve_{2d, x, y, 2d_copy} and the highbd set: the offset intermediate that goes to the ConvBufType plane
__device__ __forceinline__ int32_t jnt_intermediate(const Ref &f, int r, int c, int bd) {
    constexpr int r0 = ROUND_0, r1 = ROUND_1_COMPOUND;
    const int     offset_bits = bd + 2 * FILTER_BITS - r0, round_bits = 2 * FILTER_BITS - r0 - r1;
    const int32_t round_offset = (1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1));
    if (f.hx && f.hy) {
        int32_t sum = 1 << offset_bits;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += f.y[k] * (int32_t)f.im[(r + k) * TILE + c];
        return (uint16_t)rnd(sum, r1);
    }
    if (f.hy) {
        int32_t res = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) res += f.y[k] * (int32_t)f.in[(r + k) * IP + c];
        res *= 1 << (FILTER_BITS - r0);
        return rnd(res, r1) + round_offset;
    }
    if (f.hx)
        return (1 << (FILTER_BITS - r1)) * rnd(hsum8(f.in, r * IP + c, f.xp, 0), r0) + round_offset;
    return (uint16_t)((uint16_t)((int32_t)f.in[r * IP + c] << round_bits) + (uint16_t)round_offset);
}

// what the second jnt call leaves in the picture: the stored intermediate of the first (a uint16) averaged with the second's
__device__ __forceinline__ int32_t jnt_sample(int32_t res0, int32_t res1, int compound, int fwd, int bck, int bd) {
    constexpr int r0 = ROUND_0, r1 = ROUND_1_COMPOUND;
    const int     offset_bits = bd + 2 * FILTER_BITS - r0, round_bits = 2 * FILTER_BITS - r0 - r1;
    int32_t       tmp = (uint16_t)res0;
    tmp               = compound == 3 ? (tmp * fwd + res1 * bck) >> 4 : (tmp + res1) >> 1;
    tmp -= (1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1));
    return clip_bd(rnd(tmp, round_bits), bd);
}

// ---- model_rd_norm, svt_av1_model_rd_from_var_lapndz, model_rd_from_sse (enc_inter_prediction.c:2178-2275) ------------------------------
__constant__ const int32_t RATE_TAB_Q10[] = {
    65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376, 3307,
    3244,  3186, 3133, 3037, 2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001, 1928, 1862,
    1802,  1748, 1698, 1651, 1608, 1530, 1460, 1398, 1342, 1290, 1243, 1199, 1159, 1086, 1021, 963,  911,  864,  821,  781,  745,  680,
    623,   574,  530,  490,  455,  424,  395,  345,  304,  269,  239,  213,  190,  171,  154,  126,  104,  87,   73,   61,   52,   44,
    38,    28,   21,   16,   12,   10,   8,    6,    5,    3,    2,    1,    1,    1,    0,    0,
};
__constant__ const int32_t DIST_TAB_Q10[] = {
    0,   0,   1,   1,   1,   2,   2,   2,   3,   3,   4,   5,   5,   6,   7,   7,   8,   9,   11,  12,   13,   15,   16,   17,   18,   21,   24,
    26,  29,  31,  34,  36,  39,  44,  49,  54,  59,  64,  69,  73,  78,  88,  97,  106, 115,  124,  133,  142,  151,  167,  184,  200,  215,  231,
    245, 260, 274, 301, 327, 351, 375, 397, 418, 439, 458, 495, 528, 559, 587, 613, 637,  659,  680,  717,  749,  777,  801,  823,  842,  859,  874,
    899, 919, 936, 949, 960, 969, 977, 983, 994, 1001, 1006, 1010, 1013, 1015, 1017, 1018, 1020, 1022, 1022, 1023, 1023, 1023, 1024,
};
__constant__ const int32_t XSQ_IQ_Q10[] = {
    0,     4,     8,     12,    16,    20,    24,    28,    32,    40,    48,    56,    64,    72,    80,    88,     96,     112,    128,    144,    160,
    176,   192,   208,   224,   256,   288,   320,   352,   384,   416,   448,   480,   544,   608,   672,   736,    800,    864,    928,    992,    1120,
    1248,  1376,  1504,  1632,  1760,  1888,  2016,  2272,  2528,  2784,  3040,  3296,  3552,  3808,  4064,  4576,   5088,   5600,   6112,   6624,   7136,
    7648,  8160,  9184,  10208, 11232, 12256, 13280, 14304, 15328, 16352, 18400, 20448, 22496, 24544, 26592,  28640,  30688,  32736,  36832,  40928,  45024,
    49120, 53216, 57312, 61408, 65504, 73696, 81888, 90080, 98272, 106464, 114656, 122848, 131040, 147424, 163808, 180192, 196576, 212960, 229344, 245728,
};

// model_rd_from_sse(.., simple_model_rd_from_var = 0): *rate as the int32 the function writes, *dist after its << 4
__device__ __forceinline__ void model_rd_from_sse(int n_log2, int quantizer, int bd, uint64_t sse, int32_t *rate, uint64_t *dist) {
    const int64_t  var   = (int64_t)sse;
    const uint32_t qstep = (uint32_t)(quantizer >> (bd - 5));
    if (var == 0) {
        *rate = 0, *dist = 0;
        return;
    }
    const uint64_t xsq_q10_64 = ((((uint64_t)qstep * qstep) << (n_log2 + 10)) + (uint64_t)(var >> 1)) / (uint64_t)var;
    const int32_t  xsq_q10    = (int32_t)(xsq_q10_64 < 245727 ? xsq_q10_64 : 245727);  // MAX_XSQ_Q10
    const int32_t  tmp = (xsq_q10 >> 2) + 8, k = (31 - __clz(tmp)) - 3, xq = (k << 3) + ((tmp >> k) & 0x7);
    const int32_t  a_q10 = ((xsq_q10 - XSQ_IQ_Q10[xq]) << 10) >> (2 + k), b_q10 = (1 << 10) - a_q10;
    const int32_t  r_q10 = (RATE_TAB_Q10[xq] * b_q10 + RATE_TAB_Q10[xq + 1] * a_q10) >> 10;
    const int32_t  d_q10 = (DIST_TAB_Q10[xq] * b_q10 + DIST_TAB_Q10[xq + 1] * a_q10) >> 10;
    *rate = (int32_t)(((uint32_t)r_q10 << n_log2) + 1u) >> 1;  // ROUND_POWER_OF_TWO(r_q10 << n_log2, 10 - AV1_PROB_COST_SHIFT)
    *dist = (uint64_t)((var * (int64_t)d_q10 + 512) >> 10) << 4;
}

}  // namespace ifs
}  // namespace svthip
