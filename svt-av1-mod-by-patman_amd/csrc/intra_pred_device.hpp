// intra_pred_device.hpp — the AV1 intra predictor of any transform-block size as __device__ functions, one wave per block:
// build_intra_predictors / build_intra_predictors_high (enc_intra_prediction.c:60-435, paths relative to the reference's
// Source/Lib/Codec) and everything behind them, the smooth inter-intra combination (inter_prediction.c:2128-2214, 2341-2372) and
// CfL (intra_prediction.c:420-465, C_DEFAULT/cfl_c.c).  Used by intra_predict.hip only.
//
// The edges of a block live in LDS as uint16 for every bit depth, laid out as the reference's above_data / left_data are: entry
// [0] at index EDGE_ORG, the fill (0x80 bytes) in every entry the preparation does not write, so that whatever a predictor reads
// is what the reference reads.  There are two copies: the edge filter reads copy 0 and writes copy 1, the upsampler reads copy 1
// and writes copy 0, so every output entry is one lane's work.  A wave synchronises with itself only (wave_sync): waves of a
// workgroup never wait for each other.
// The constant tables of intra_device.hpp are shared; none of its templates is used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svt_hip_intra.h"
#include "blend_device.hpp"
#include "intra_device.hpp"

namespace svthip {
namespace intrapred {

using blend::load4;
using blend::store4;
using blend::wave_sum;
using namespace intra;  // mode numbers, MODE_ANGLE, SM_WEIGHTS, DR_DERIV, EDGE_KERNEL, interp5, edge_strength (filt_type 0)

constexpr int EDGE_ORG = 16;                   // index of entry [0]: 32 bytes, so that four entries from a multiple of 4 are one 8-byte read
constexpr int EDGE_LEN = EDGE_ORG + 128 + 16;  // MAX_TX_SIZE * 2 + 32, the reference's high-bit-depth arrays
constexpr int FI_STRIDE = 36;                  // pitch of the filter-intra block [33][33] ...
constexpr int FI_COL0 = 3;                     // ... whose column c sits at index FI_COL0 + c: four samples from column 1 + 4 i are one aligned 8-byte read
constexpr int FILTER_INTRA_NONE = 5;           // FILTER_INTRA_MODES

// eb_av1_filter_intra_taps (AV1 specification 7.11.2.3, Intra_Filter_Taps): [mode][output sample of the 4 x 2 block][p0 .. p6]
__constant__ const int8_t FILTER_INTRA_TAPS[5][8][8] = {
    {{-6, 10, 0, 0, 0, 12, 0, 0}, {-5, 2, 10, 0, 0, 9, 0, 0}, {-3, 1, 1, 10, 0, 7, 0, 0}, {-3, 1, 1, 2, 10, 5, 0, 0},
     {-4, 6, 0, 0, 0, 2, 12, 0},  {-3, 2, 6, 0, 0, 2, 9, 0},  {-3, 2, 2, 6, 0, 2, 7, 0},  {-3, 1, 2, 2, 6, 3, 5, 0}},
    {{-10, 16, 0, 0, 0, 10, 0, 0}, {-6, 0, 16, 0, 0, 6, 0, 0}, {-4, 0, 0, 16, 0, 4, 0, 0}, {-2, 0, 0, 0, 16, 2, 0, 0},
     {-10, 16, 0, 0, 0, 0, 10, 0}, {-6, 0, 16, 0, 0, 0, 6, 0}, {-4, 0, 0, 16, 0, 0, 4, 0}, {-2, 0, 0, 0, 16, 0, 2, 0}},
    {{-8, 8, 0, 0, 0, 16, 0, 0}, {-8, 0, 8, 0, 0, 16, 0, 0}, {-8, 0, 0, 8, 0, 16, 0, 0}, {-8, 0, 0, 0, 8, 16, 0, 0},
     {-4, 4, 0, 0, 0, 0, 16, 0}, {-4, 0, 4, 0, 0, 0, 16, 0}, {-4, 0, 0, 4, 0, 0, 16, 0}, {-4, 0, 0, 0, 4, 0, 16, 0}},
    {{-2, 8, 0, 0, 0, 10, 0, 0}, {-1, 3, 8, 0, 0, 6, 0, 0}, {-1, 2, 3, 8, 0, 4, 0, 0}, {0, 1, 2, 3, 8, 2, 0, 0},
     {-1, 4, 0, 0, 0, 3, 10, 0}, {-1, 3, 4, 0, 0, 4, 6, 0}, {-1, 2, 3, 4, 0, 4, 4, 0}, {-1, 2, 2, 3, 4, 3, 3, 0}},
    {{-12, 14, 0, 0, 0, 14, 0, 0}, {-10, 0, 14, 0, 0, 12, 0, 0}, {-9, 0, 0, 14, 0, 11, 0, 0}, {-8, 0, 0, 0, 14, 10, 0, 0},
     {-10, 12, 0, 0, 0, 0, 14, 0}, {-9, 1, 12, 0, 0, 0, 12, 0},  {-8, 0, 0, 12, 0, 1, 11, 0}, {-7, 0, 0, 1, 12, 1, 9, 0}}};
// ii_weights1d (inter_prediction.c:2128; AV1 specification 7.11.3.13, Ii_Weights_1d)
__constant__ const uint8_t II_WEIGHTS[128] = {
    60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22, 21, 20,
    19, 19, 18, 18, 17, 16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9,  9,  9,  8,  8,  8,  8,  7,  7,  7,  7,
    6,  6,  6,  6,  6,  5,  5,  5,  5,  5,  4,  4,  4,  4,  4,  4,  4,  4,  3,  3,  3,  3,  3,  3,  3,  3,  3,  2,  2,  2,  2,  2,
    2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1};

struct WaveLds {
    alignas(16) uint16_t edge[2][2][EDGE_LEN];  // [copy][0 above, 1 left][entry + EDGE_ORG]
    alignas(16) uint16_t blk[33 * FI_STRIDE + 4];  // filter-intra: row 0 = above[-1 ..], column 0 = left
};

// All 64 lanes of the wave call it in uniform control flow: LDS writes before it are seen by LDS reads after it.  LDS serves one
// wave's accesses in order; the fences keep the compiler from moving them across.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int load_px(const void *p, ptrdiff_t i, bool is16) {
    return is16 ? (int)((const uint16_t *)p)[i] : (int)((const uint8_t *)p)[i];
}
__device__ __forceinline__ int clip_px(int v, int maxv) { return min(max(v, 0), maxv); }
// ROUND_POWER_OF_TWO_SIGNED
__device__ __forceinline__ int round_signed(int v, int n) { return v < 0 ? -((-v + ((1 << n) >> 1)) >> n) : (v + ((1 << n) >> 1)) >> n; }

__device__ __forceinline__ bool tx_side(int v) { return v == 4 || v == 8 || v == 16 || v == 32 || v == 64; }
__device__ __forceinline__ bool depth_ok(int is_16bit, int bit_depth) {
    return is_16bit <= 1 && (bit_depth == 8 || bit_depth == 10 || bit_depth == 12) && (is_16bit || bit_depth == 8);
}
__device__ __forceinline__ bool aligned_px(const void *p, int is_16bit) { return !is_16bit || ((uintptr_t)p & 1) == 0; }

// The conditions the reference asserts (or its callers guarantee), see SvtHipIntraPredDesc.
__device__ inline bool pred_desc_ok(const SvtHipIntraPredDesc &d) {
    const int w = d.w, h = d.h;
    if (!d.dst || !tx_side(w) || !tx_side(h) || w > 4 * h || h > 4 * w || !depth_ok(d.is_16bit, d.bit_depth))
        return false;
    if (d.mode >= MODES || (is_directional(d.mode) ? (d.angle_delta < -3 || d.angle_delta > 3) : d.angle_delta != 0))
        return false;
    if (d.filter_intra_mode > FILTER_INTRA_NONE || (d.filter_intra_mode != FILTER_INTRA_NONE && (d.mode != DC || w > 32 || h > 32)))
        return false;
    if (d.filt_type > 1 || d.disable_edge_filter > 1)
        return false;
    if (d.n_top_px > w || d.n_left_px > h || d.n_topright_px > w || d.n_bottomleft_px > h || (d.n_topright_px && d.n_top_px != w) ||
        (d.n_bottomleft_px && d.n_left_px != h))
        return false;
    if ((d.n_top_px && !d.above) || (d.n_left_px && !d.left) || (d.inter && d.ii_mode > 3))
        return false;
    return aligned_px(d.dst, d.is_16bit) && aligned_px(d.above, d.is_16bit) && aligned_px(d.left, d.is_16bit) && aligned_px(d.inter, d.is_16bit);
}

// svt_aom_intra_edge_filter_strength (intra_prediction.c:180)
__device__ __forceinline__ int edge_strength_of(int blk_wh, int delta, int type) {
    if (!type)
        return edge_strength(blk_wh, delta);
    const int d = delta < 0 ? -delta : delta;
    if (blk_wh <= 8)
        return d >= 64 ? 2 : (d >= 40 ? 1 : 0);
    if (blk_wh <= 16)
        return d >= 48 ? 2 : (d >= 20 ? 1 : 0);
    if (blk_wh <= 24)
        return d >= 4 ? 3 : 0;
    return d >= 1 ? 3 : 0;
}
// svt_aom_use_intra_edge_upsample (intra_prediction.c:146)
__device__ __forceinline__ bool use_upsample(int blk_wh, int delta, int type) {
    const int d = delta < 0 ? -delta : delta;
    return d > 0 && d < 40 && (type ? blk_wh <= 8 : blk_wh <= 16);
}

// p[i] (1 <= i < sz) of svt_av1_filter_intra_edge[_high]_c; e = the unfiltered edge ([0] entry), corner = p[0]
__device__ __forceinline__ int filter_tap(const uint16_t *e, int corner, int i, int sz, int strength) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int k = min(max(i - 2 + j, 0), sz - 1);
        s += (k == 0 ? corner : (int)e[k - 1]) * (int)EDGE_KERNEL[strength - 1][j];
    }
    return (s + 8) >> 4;
}

// entry q (>= -2) of an edge after svt_av1_upsample_intra_edge[_high]_c over sz entries; e = the edge before ([0] entry)
__device__ __forceinline__ int upsampled_entry(const uint16_t *e, int q, int sz, int maxv) {
    if (q == -2)
        return e[-1];
    if (q > 2 * sz - 2)
        return e[q];
    if (!(q & 1))
        return e[q >> 1];
    const int i = (q + 1) >> 1;  // in[m] = p[clamp(m - 2, -1, sz - 1)]
    const int s = -(int)e[max(i - 2, -1)] + 9 * (int)e[i - 1] + 9 * (int)e[min(i, sz - 1)] - (int)e[min(i + 1, sz - 1)];
    return clip_px((s + 8) >> 4, maxv);
}

enum : int { K_FILL, K_DC, K_V, K_H, K_SMOOTH, K_SMOOTH_V, K_SMOOTH_H, K_PAETH, K_Z1, K_Z2, K_Z3, K_BLOCK };

// four entries from a multiple of four: one 8-byte LDS read
__device__ __forceinline__ void edge4(const uint16_t *e, int c0, int v[4]) {
    const uint2 q = *(const uint2 *)(e + c0);
    v[0] = q.x & 0xFFFF, v[1] = q.x >> 16, v[2] = q.y & 0xFFFF, v[3] = q.y >> 16;
}
// e[b], e[b + 1] for any b >= -2: the compiler would merge the two 16-bit reads into one 4-byte read that is unaligned for odd b (65
// cycles per wave); read the two aligned dwords around them and shift by the parity instead
__device__ __forceinline__ int interp_at(const uint16_t *e, int b, int shift) {
    const uint32_t *p = (const uint32_t *)(e + (b & ~1));
    const uint32_t  q = __builtin_amdgcn_alignbit(p[1], p[0], (b & 1) << 4);
    return interp5((int)(q & 0xFFFF), (int)(q >> 16), shift);
}
__device__ __forceinline__ void weights4(int at, int v[4]) {  // sm_weight_arrays[at .. at + 3], at a multiple of four
    uint32_t q;
    __builtin_memcpy(&q, &SM_WEIGHTS[at], 4);
    v[0] = q & 0xFF, v[1] = (q >> 8) & 0xFF, v[2] = (q >> 16) & 0xFF, v[3] = q >> 24;
}

// One transform block.  The whole wave calls it with the same (validated) descriptor; lane = 0 .. 63.
__device__ inline void predict_block(const SvtHipIntraPredDesc &d, WaveLds &lds, int lane) {
    const int  w = d.w, h = d.h, mode = d.mode, bd = d.bit_depth;
    const bool is16 = d.is_16bit != 0;
    const int  base = 128 << (bd - 8), maxv = (1 << bd) - 1;
    const int  n_top = d.n_top_px, n_left = d.n_left_px;
    const bool is_dr = is_directional(mode), use_fi = d.filter_intra_mode != FILTER_INTRA_NONE;
    // extend_modes (intra_prediction.c:469) and its overrides
    bool need_above = mode != H && mode != D203, need_left = mode != V && mode != D45 && mode != D67;
    bool need_al = mode == D135 || mode == D113 || mode == D157 || mode == PAETH, need_right = false, need_bottom = false;
    int  p_angle = 0;
    if (is_dr) {
        p_angle    = (int)MODE_ANGLE[mode] + 3 * d.angle_delta;
        need_above = p_angle < 180, need_left = p_angle > 90, need_al = true;
        need_right = p_angle < 90, need_bottom = p_angle > 180;
    }
    if (use_fi)
        need_above = need_left = need_al = true;

    const int above0 = n_top > 0 ? load_px(d.above, 0, is16) : 0, left0 = n_left > 0 ? load_px(d.left, 0, is16) : 0;
    int       kind = K_FILL, value = 0, up_above = 0, up_left = 0, dx = 1, dy = 1;
    const uint16_t *ea = nullptr, *el = nullptr;
    if ((!need_above && n_left == 0) || (!need_left && n_top == 0)) {
        value = need_left ? (n_top > 0 ? above0 : base + 1) : (n_left > 0 ? left0 : base - 1);
    } else {
        // ---- the edges: copy, replicate, fall back ------------------------------------------------------------------------
        const int fill = is16 ? 0x8080 : 0x80;
        const int top_need = w + (need_right ? h : 0), left_need = h + (need_bottom ? w : 0);
        const int top_cnt = n_top + (need_right ? d.n_topright_px : 0), left_cnt = n_left + (need_bottom ? d.n_bottomleft_px : 0);
        int       corner = base;
        if (n_top > 0 && n_left > 0)
            corner = load_px(d.above, -1, is16);
        else if (n_top > 0)
            corner = above0;
        else if (n_left > 0)
            corner = left0;
        const int k_end = EDGE_ORG + w + h + 16;  // past everything a predictor, the filter or the upsampler touches
        uint16_t *a0 = lds.edge[0][0], *l0 = lds.edge[0][1], *a1 = lds.edge[1][0], *l1 = lds.edge[1][1];
        for (int k = EDGE_ORG - 2 + lane; k < k_end; k += 64) {
            const int e = k - EDGE_ORG;
            int       va = fill, vl = fill;
            if (need_above && e >= 0 && e < top_need)
                va = n_top > 0 ? load_px(d.above, min(e, top_cnt - 1), is16) : (n_left > 0 ? left0 : base - 1);
            if (need_left && e >= 0 && e < left_need)
                vl = n_left > 0 ? load_px(d.left, (ptrdiff_t)min(e, left_cnt - 1) * d.left_stride, is16) : (n_top > 0 ? above0 : base + 1);
            if (need_al && e == -1)
                va = vl = corner;
            a0[k] = (uint16_t)va, l0[k] = (uint16_t)vl;
        }
        wave_sync();
        int cur = 0;
        // ---- directional modes: corner filter, edge filter, upsampling ------------------------------------------------------
        if (is_dr && !d.disable_edge_filter && p_angle != 90 && p_angle != 180) {
            const int ft = d.filt_type;
            int       cv = a0[EDGE_ORG - 1];
            if (need_above && need_left && w + h >= 24)  // filter_intra_edge_corner
                cv = ((int)l0[EDGE_ORG] * 5 + cv * 6 + (int)a0[EDGE_ORG] * 5 + 8) >> 4;
            const int sa = need_above && n_top > 0 ? edge_strength_of(w + h, p_angle - 90, ft) : 0;
            const int sl = need_left && n_left > 0 ? edge_strength_of(w + h, p_angle - 180, ft) : 0;
            const int na = n_top + 1 + (need_right ? h : 0), nl = n_left + 1 + (need_bottom ? w : 0);
            for (int k = EDGE_ORG - 2 + lane; k < k_end; k += 64) {
                const int i = k - EDGE_ORG + 1;  // index into p = edge - 1
                int       va = i == 0 ? cv : (int)a0[k], vl = i == 0 ? cv : (int)l0[k];
                if (sa && i >= 1 && i < na)
                    va = filter_tap(a0 + EDGE_ORG, cv, i, na, sa);
                if (sl && i >= 1 && i < nl)
                    vl = filter_tap(l0 + EDGE_ORG, cv, i, nl, sl);
                a1[k] = (uint16_t)va, l1[k] = (uint16_t)vl;
            }
            wave_sync();
            cur      = 1;
            up_above = need_above && use_upsample(w + h, p_angle - 90, ft);
            up_left  = need_left && use_upsample(w + h, p_angle - 180, ft);
            if (up_above || up_left) {
                const int sza = w + (need_right ? h : 0), szl = h + (need_bottom ? w : 0);
                for (int k = EDGE_ORG - 2 + lane; k < k_end; k += 64) {
                    const int q = k - EDGE_ORG;
                    a0[k] = (uint16_t)(up_above ? upsampled_entry(a1 + EDGE_ORG, q, sza, maxv) : (int)a1[k]);
                    l0[k] = (uint16_t)(up_left ? upsampled_entry(l1 + EDGE_ORG, q, szl, maxv) : (int)l1[k]);
                }
                wave_sync();
                cur = 0;
            }
        }
        ea = lds.edge[cur][0] + EDGE_ORG, el = lds.edge[cur][1] + EDGE_ORG;

        if (use_fi) {
            // ---- filter-intra: 4 x 2 sub-blocks in anti-diagonal steps, lane = 8 * (sub-block column) + output sample -----------
            uint16_t *blk = lds.blk;
            for (int k = lane; k <= w; k += 64) blk[FI_COL0 + k] = ea[k - 1];
            if (lane < h)
                blk[(lane + 1) * FI_STRIDE + FI_COL0] = el[lane];
            const int i = lane >> 3, o = lane & 7, nsx = w >> 2, nsy = h >> 1, fim = d.filter_intra_mode;
            int       t[7];
#pragma unroll
            for (int j = 0; j < 7; j++) t[j] = FILTER_INTRA_TAPS[fim][o][j];
            wave_sync();
            for (int s = 0; s < nsx + nsy - 1; s++) {
                const int j = s - i;
                if (i < nsx && j >= 0 && j < nsy) {
                    const uint16_t *p = blk + (2 * j) * FI_STRIDE + FI_COL0 + 4 * i;  // row r - 1, column c - 1
                    int             a[4];
                    edge4(p + 1, 0, a);
                    const int v = t[0] * p[0] + t[1] * a[0] + t[2] * a[1] + t[3] * a[2] + t[4] * a[3] + t[5] * p[FI_STRIDE] + t[6] * p[2 * FI_STRIDE];
                    blk[(2 * j + 1 + (o >> 2)) * FI_STRIDE + FI_COL0 + 4 * i + 1 + (o & 3)] = (uint16_t)clip_px(round_signed(v, 4), maxv);
                }
                wave_sync();
            }
            kind = K_BLOCK;
        } else if (is_dr) {
            if (p_angle == 90)
                kind = K_V;
            else if (p_angle == 180)
                kind = K_H;
            else if (p_angle < 90)
                kind = K_Z1, dx = DR_DERIV[p_angle];
            else if (p_angle < 180)
                kind = K_Z2, dx = DR_DERIV[180 - p_angle], dy = DR_DERIV[p_angle - 90];
            else
                kind = K_Z3, dy = DR_DERIV[270 - p_angle];
        } else if (mode == DC) {  // svt_aom_dc_pred[n_left_px > 0][n_top_px > 0]
            uint32_t s = 0;
            if (n_top > 0 && lane < w)
                s += ea[lane];
            if (n_left > 0 && lane < h)
                s += el[lane];
            s               = wave_sum(s);
            const int count = (n_top > 0 ? w : 0) + (n_left > 0 ? h : 0);
            kind = K_DC, value = count ? (int)((s + (count >> 1)) / count) : base;
        } else {
            kind = mode == SMOOTH ? K_SMOOTH : (mode == SMOOTH_V ? K_SMOOTH_V : (mode == SMOOTH_H ? K_SMOOTH_H : K_PAETH));
        }
    }

    // ---- the samples: a lane takes four adjacent samples of a row -------------------------------------------------------------
    const int      nq = w >> 2, lq = __ffs(nq) - 1, items = nq * h, px = is16 ? 2 : 1;
    const int      ii_mode = d.ii_mode, ii_scale = 128 / max(w, h);  // ii_size_scales[plane_bsize]
    const uint8_t *inter = (const uint8_t *)d.inter;
    uint8_t       *dst = (uint8_t *)d.dst;
    for (int it = lane; it < items; it += 64) {
        const int r = it >> lq, c0 = (it & (nq - 1)) << 2;
        int       v[4];
        switch (kind) {
        case K_FILL:
        case K_DC: v[0] = v[1] = v[2] = v[3] = value; break;
        case K_V: edge4(ea, c0, v); break;
        case K_H: v[0] = v[1] = v[2] = v[3] = el[r]; break;
        case K_SMOOTH: {
            int a[4], ww[4];
            edge4(ea, c0, a), weights4(w + c0, ww);
            const int wh = SM_WEIGHTS[h + r], below = el[h - 1], right = ea[w - 1], l = el[r];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (wh * a[k] + (256 - wh) * below + ww[k] * l + (256 - ww[k]) * right + 256) >> 9;
            break;
        }
        case K_SMOOTH_V: {
            int a[4];
            edge4(ea, c0, a);
            const int wh = SM_WEIGHTS[h + r], below = el[h - 1];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (wh * a[k] + (256 - wh) * below + 128) >> 8;
            break;
        }
        case K_SMOOTH_H: {
            int ww[4];
            weights4(w + c0, ww);
            const int right = ea[w - 1], l = el[r];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (ww[k] * l + (256 - ww[k]) * right + 128) >> 8;
            break;
        }
        case K_PAETH: {
            int a[4];
            edge4(ea, c0, a);
            const int l = el[r], tl = ea[-1];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int      t = a[k], b = t + l - tl;
                const uint32_t pl = absdiff(b, l), pt = absdiff(b, t), ptl = absdiff(b, tl);
                v[k]              = (pl <= pt && pl <= ptl) ? l : (pt <= ptl ? t : tl);
            }
            break;
        }
        case K_Z1: {  // svt_av1_[highbd_]dr_prediction_z1_c
            const int max_base = (w + h - 1) << up_above, x = (r + 1) * dx, shift = ((x << up_above) & 0x3F) >> 1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int b = (x >> (6 - up_above)) + ((c0 + k) << up_above);
                v[k]        = b < max_base ? clip_px(interp_at(ea, b, shift), maxv) : (int)ea[max_base];
            }
            break;
        }
        case K_Z2: {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c = c0 + k, x = (c << 6) - (r + 1) * dx, b1 = x >> (6 - up_above);
                if (b1 >= -(1 << up_above)) {
                    v[k] = interp_at(ea, b1, ((x << up_above) & 0x3F) >> 1);
                } else {
                    const int y = (r << 6) - (c + 1) * dy, b2 = y >> (6 - up_left);
                    v[k]        = interp_at(el, b2, ((y << up_left) & 0x3F) >> 1);
                }
                v[k] = clip_px(v[k], maxv);
            }
            break;
        }
        case K_Z3: {
            const int max_base = (w + h - 1) << up_left;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int y = (c0 + k + 1) * dy, b = (y >> (6 - up_left)) + (r << up_left), shift = ((y << up_left) & 0x3F) >> 1;
                v[k]        = b < max_base ? clip_px(interp_at(el, b, shift), maxv) : (int)el[max_base];
            }
            break;
        }
        default: {  // K_BLOCK
            edge4(lds.blk + (r + 1) * FI_STRIDE + FI_COL0 + 1, c0, v);
        }
        }
        if (inter) {  // svt_aom_combine_interintra[_highbd], use_wedge_interintra == 0: AOM_BLEND_A64(mask, intra, inter)
            int q[4];
            is16 ? load4<true>(inter + ((size_t)r * d.inter_stride + c0) * 2, 4, q) : load4<false>(inter + (size_t)r * d.inter_stride + c0, 4, q);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int at = ii_mode == 1 ? r : (ii_mode == 2 ? c0 + k : min(r, c0 + k));
                const int m  = ii_mode == 0 ? 32 : (int)II_WEIGHTS[at * ii_scale];
                v[k]         = (m * v[k] + (64 - m) * q[k] + 32) >> 6;
            }
        }
        uint8_t *o = dst + ((size_t)r * d.dst_stride + c0) * px;
        is16 ? store4<true>(o, 4, v) : store4<false>(o, 4, v);
    }
}

// ---- CfL ---------------------------------------------------------------------------------------------------------------------
__device__ inline bool cfl_desc_ok(const SvtHipCflDesc &d) {
    const auto side = [](int v) { return v == 4 || v == 8 || v == 16 || v == 32; };
    if (!d.luma || !d.pred || !d.dst || !side(d.w) || !side(d.h) || d.alpha_q3 < -16 || d.alpha_q3 > 16 || !depth_ok(d.is_16bit, d.bit_depth))
        return false;
    return aligned_px(d.luma, d.is_16bit) && aligned_px(d.pred, d.is_16bit) && aligned_px(d.dst, d.is_16bit) && ((uintptr_t)d.ac_out & 1) == 0;
}

constexpr int CFL_QUADS = 4;  // 32 x 32 chroma samples are 256 quads: four per lane

// One chroma block: svt_cfl_luma_subsampling_420_{lbd,hbd}_c, svt_subtract_average_c, svt_cfl_predict_{lbd,hbd}_c.  The AC block
// stays in registers.
template <bool IS16> __device__ inline void cfl_block(const SvtHipCflDesc &d, int lane) {
    constexpr int  PX = IS16 ? 2 : 1;
    const int      w = d.w, h = d.h, nq = w >> 2, lq = __ffs(nq) - 1, items = nq * h;
    const int      alpha = d.alpha_q3, maxv = (1 << d.bit_depth) - 1;
    const uint8_t *luma = (const uint8_t *)d.luma, *pred = (const uint8_t *)d.pred;
    int            ac[CFL_QUADS][4];
    uint32_t       sum = 0;
#pragma unroll
    for (int j = 0; j < CFL_QUADS; j++) {
        const int it = lane + 64 * j;
#pragma unroll
        for (int k = 0; k < 4; k++) ac[j][k] = 0;
        if (it < items) {
            const int      r = it >> lq, c0 = (it & (nq - 1)) << 2;
            const uint8_t *p = luma + ((size_t)(2 * r) * d.luma_stride + 2 * c0) * PX;
            int            a[8], b[8];
            load4<IS16>(p, 4, a), load4<IS16>(p + 4 * PX, 4, a + 4);
            load4<IS16>(p + (size_t)d.luma_stride * PX, 4, b), load4<IS16>(p + ((size_t)d.luma_stride + 4) * PX, 4, b + 4);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                ac[j][k] = (a[2 * k] + a[2 * k + 1] + b[2 * k] + b[2 * k + 1]) << 1;
                sum += (uint32_t)ac[j][k];
            }
        }
    }
    sum           = wave_sum(sum);
    const int avg = (int)((sum + (uint32_t)((w * h) >> 1)) >> (__ffs(w) + __ffs(h) - 2));
#pragma unroll
    for (int j = 0; j < CFL_QUADS; j++) {
        const int it = lane + 64 * j;
        if (it < items) {
            const int r = it >> lq, c0 = (it & (nq - 1)) << 2;
            int       q[4], o[4];
            load4<IS16>(pred + ((size_t)r * d.pred_stride + c0) * PX, 4, q);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                ac[j][k] -= avg;
                o[k] = clip_px(round_signed(alpha * ac[j][k], 6) + q[k], maxv);
            }
            if (d.ac_out) {
                int16_t *a = d.ac_out + r * SVT_HIP_CFL_BUF_LINE + c0;
                if (((uintptr_t)a & 7) == 0) {
                    *(uint2 *)a = make_uint2((uint32_t)(uint16_t)ac[j][0] | ((uint32_t)(uint16_t)ac[j][1] << 16),
                                             (uint32_t)(uint16_t)ac[j][2] | ((uint32_t)(uint16_t)ac[j][3] << 16));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) a[k] = (int16_t)ac[j][k];
                }
            }
            store4<IS16>((uint8_t *)d.dst + ((size_t)r * d.dst_stride + c0) * PX, 4, o);
        }
    }
}

}  // namespace intrapred
}  // namespace svthip
