// inter_blend.hip — the second half of inter prediction on gfx950: masked-compound and OBMC blends, and the
// compound mask search.  Replaces svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c, svt_aom_(highbd_)blend_a64_mask_c, the vmask / hmask
// blends (blend_a64_mask.c:34-367, inter_prediction.c:2374-2404), svt_av1_build_compound_diffwtd_mask_d16_c
// (C_DEFAULT/inter_prediction_c.c:15-40), and pick_interinter_wedge / pick_interinter_seg with use_rate == 0 behind the residuals
// of svt_aom_calc_pred_masked_compound (enc_inter_prediction.c:386-449, 501-547, 4676-4719).
//
// Blend: streaming, one wave per workgroup, up to four workgroups per descriptor; a lane takes four adjacent samples of a row.
// Search: one wave per block; residuals stay in registers, every sum is an exact integer and crosses the lanes by shuffles.
#include "../../include/svt_hip_inter.h"
#include "blend_device.hpp"
#include "common.hpp"

using namespace svthip;
using namespace svthip::blend;

namespace {

constexpr int BLEND_CHUNKS = 4;  // workgroups per descriptor: 128 x 128 samples = 4096 quads = 4 x 16 passes of a wave

__device__ bool blend_desc_ok(const SvtHipBlendDesc &d) {
    if (d.w == 0 || d.h == 0 || d.w > 128 || d.h > 128 || d.kind >= SVT_HIP_BLEND_KINDS || !d.src0 || !d.src1 || !d.dst || !d.mask)
        return false;
    if (d.is_16bit > 1 || (d.bit_depth != 8 && d.bit_depth != 10 && d.bit_depth != 12) || (!d.is_16bit && d.bit_depth != 8))
        return false;
    if (d.kind <= SVT_HIP_BLEND_D16_DIFFWTD && (d.w < 4 || d.h < 4 || d.round_0 + d.round_1 > 14))
        return false;
    if (d.kind == SVT_HIP_BLEND_D16 || d.kind == SVT_HIP_BLEND_MASK ? (d.subw > 1 || d.subh > 1) : (d.subw || d.subh))
        return false;
    return d.kind == SVT_HIP_BLEND_D16_DIFFWTD ? d.mask_type <= 1 : d.mask_type == 0;
}

// D16: the sources are ConvBufType.  IS16: dst (and the pixel sources) are uint16.
template <bool D16, bool IS16> __device__ void blend_block(const SvtHipBlendDesc &d, int chunk) {
    constexpr bool SRC16 = D16 || IS16;
    constexpr int  SPX = SRC16 ? 2 : 1, DPX = IS16 ? 2 : 1;
    const int      w = d.w, h = d.h, nq = (w + 3) >> 2, items = nq * h;
    const int      per = (((items + BLEND_CHUNKS - 1) / BLEND_CHUNKS) + 63) & ~63;  // whole passes of the wave
    const int      begin = chunk * per, end = min(items, begin + per);
    const int      kind = d.kind, sub = d.subw | (d.subh << 1);
    const int      round_bits = 14 - d.round_0 - d.round_1, offset_bits = d.bit_depth + 14 - d.round_0;
    const int      round_offset = (1 << (offset_bits - d.round_1)) + (1 << (offset_bits - d.round_1 - 1));
    const int      diff_round = round_bits + d.bit_depth - 8, max_px = (1 << d.bit_depth) - 1;
    const bool     inverse = d.mask_type != 0;
    const uint8_t *s0 = (const uint8_t *)d.src0, *s1 = (const uint8_t *)d.src1;
    uint8_t       *dst = (uint8_t *)d.dst, *mask = d.mask;
    const size_t   ms = d.mask_stride;

    for (int it = begin + (int)threadIdx.x; it < end; it += 64) {
        const int row = it / nq, x = (it - row * nq) << 2, n = min(4, w - x);
        int       a[4], b[4], m[4], o[4];
        load4<SRC16>(s0 + ((size_t)row * d.src0_stride + x) * SPX, n, a);
        load4<SRC16>(s1 + ((size_t)row * d.src1_stride + x) * SPX, n, b);
        if (kind == SVT_HIP_BLEND_D16_DIFFWTD) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int diff = (abs(a[k] - b[k]) + ((1 << diff_round) >> 1)) >> diff_round;
                const int mm = min(38 + (diff >> 4), 64);
                m[k] = inverse ? 64 - mm : mm;
            }
            store4<false>(mask + (size_t)row * w + x, n, m);
        } else if (kind == SVT_HIP_BLEND_VMASK) {
            m[0] = m[1] = m[2] = m[3] = mask[row];
        } else if (kind == SVT_HIP_BLEND_HMASK) {
            load4<false>(mask + x, n, m);
        } else if (sub == 0) {
            load4<false>(mask + row * ms + x, n, m);
        } else if (sub == 1) {  // subw: AOM_BLEND_AVG of two columns
            int v[8];
            load8_u8(mask + row * ms + 2 * x, n, v);
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = (v[2 * k] + v[2 * k + 1] + 1) >> 1;
        } else if (sub == 2) {  // subh: AOM_BLEND_AVG of two rows
            int u[4], v[4];
            load4<false>(mask + (2 * row) * ms + x, n, u);
            load4<false>(mask + (2 * row + 1) * ms + x, n, v);
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = (u[k] + v[k] + 1) >> 1;
        } else {  // both: rounded mean of 2 x 2
            int u[8], v[8];
            load8_u8(mask + (2 * row) * ms + 2 * x, n, u);
            load8_u8(mask + (2 * row + 1) * ms + 2 * x, n, v);
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = (u[2 * k] + v[2 * k] + u[2 * k + 1] + v[2 * k + 1] + 2) >> 2;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int acc = m[k] * a[k] + (64 - m[k]) * b[k];
            if (D16) {
                const int res = (acc >> 6) - round_offset;
                o[k] = min(max((res + ((1 << round_bits) >> 1)) >> round_bits, 0), max_px);
            } else {
                o[k] = (acc + 32) >> 6;
            }
        }
        store4<IS16>(dst + ((size_t)row * d.dst_stride + x) * DPX, n, o);
    }
}

// Workgroup (g, c) visits the four descriptors of group g and takes chunk (c + j) % 4 of the j-th: a small block (one chunk) costs
// one wave instead of one busy and three empty ones, a large block is still spread over four waves.
__global__ __launch_bounds__(64) void blend_kernel(const SvtHipBlendDesc *__restrict__ descs, uint32_t n) {
    for (uint32_t j = 0; j < BLEND_CHUNKS; j++) {
        const uint32_t i = blockIdx.x * BLEND_CHUNKS + j;
        if (i >= n)
            break;
        const SvtHipBlendDesc d = descs[i];  // uniform: scalar loads
        if (!blend_desc_ok(d))
            continue;
        const int chunk = (int)((blockIdx.y + j) % BLEND_CHUNKS);
        if (d.kind <= SVT_HIP_BLEND_D16_DIFFWTD)
            d.is_16bit ? blend_block<true, true>(d, chunk) : blend_block<true, false>(d, chunk);
        else
            d.is_16bit ? blend_block<false, true>(d, chunk) : blend_block<false, false>(d, chunk);
    }
}

// ---- mask search -------------------------------------------------------------------------------------------------------
constexpr int WEDGE_QUADS = 4;  // the largest wedge size, 32 x 32, is 256 quads: four per lane

__device__ int search_desc_status(const SvtHipMaskSearchDesc &d) {
    const auto size_ok = [](int v) { return v == 8 || v == 16 || v == 32 || v == 64 || v == 128; };
    if (!d.src || !d.pred0 || !d.pred1 || !size_ok(d.w) || !size_ok(d.h) || d.is_16bit > 1 ||
        (d.bit_depth != 8 && d.bit_depth != 10 && d.bit_depth != 12) || (!d.is_16bit && d.bit_depth != 8))
        return SVT_HIP_MASK_SEARCH_BAD_DESC;
    if (d.wedge_masks && (d.w > 32 || d.h > 32))
        return SVT_HIP_MASK_SEARCH_BAD_WEDGE_SIZE;
    return SVT_HIP_MASK_SEARCH_OK;
}

struct SearchSums {  // per-lane partial sums over the block
    uint32_t sad;
    SplitSum ss0, ss1, dw0, dw1;
};

// One quad of the block: SAD, residual energies and the two difference-weighted masks go into the sums; src - pred1,
// pred1 - pred0 and the clamped difference of the squared residuals come back for the wedges.
template <bool IS16>
__device__ inline void search_quad(const SvtHipMaskSearchDesc &d, int q, int lq, SearchSums &a, int r1v[4], int d10v[4], int dsv[4]) {
    constexpr int PX = IS16 ? 2 : 1;
    const int     row = q >> lq, x = (q - (row << lq)) << 2, bd_shift = d.bit_depth - 8;
    int           s[4], p0[4], p1[4];
    load4<IS16>((const uint8_t *)d.src + ((size_t)row * d.src_stride + x) * PX, 4, s);
    load4<IS16>((const uint8_t *)d.pred0 + ((size_t)row * d.pred0_stride + x) * PX, 4, p0);
    load4<IS16>((const uint8_t *)d.pred1 + ((size_t)row * d.pred1_stride + x) * PX, 4, p1);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r0 = s[k] - p0[k], r1 = s[k] - p1[k], d10 = p1[k] - p0[k], ad = abs(d10);
        a.sad += (uint32_t)ad;
        a.ss0.add((uint32_t)(r0 * r0)), a.ss1.add((uint32_t)(r1 * r1));
        const int m = min(38 + ((ad >> bd_shift) >> 4), 64);  // DIFFWTD_38; its inverse is 64 - m
        const int t0 = clamp_i16(64 * r1 + m * d10), t1 = clamp_i16(64 * r1 + (64 - m) * d10);
        a.dw0.add((uint32_t)(t0 * t0)), a.dw1.add((uint32_t)(t1 * t1));
        r1v[k] = r1, d10v[k] = d10, dsv[k] = clamp_i16(r0 * r0 - r1 * r1);
    }
}

// One wave per block, no LDS: a lane keeps the residuals of its quads in registers (wedge sizes: at most four quads), every
// sum is an exact integer and crosses the lanes by shuffles.
template <bool IS16> __device__ void search_block(const SvtHipMaskSearchDesc &d, SvtHipMaskSearchResult *res) {
    const int      lane = (int)threadIdx.x;
    const int      w = d.w, N = w * d.h, Q = N >> 2, lq = __ffs(w) - 3;  // a row holds 1 << lq quads
    const uint8_t *masks = d.wedge_masks;
    SearchSums     a{};
    // lane i < 16 ends up with wedge index i: its sum of ds * mask and the squared sums under both signs
    uint32_t w_dsm = 0, w_lo0 = 0, w_hi0 = 0, w_lo1 = 0, w_hi1 = 0;
    if (masks) {
        int r1v[WEDGE_QUADS][4], d10v[WEDGE_QUADS][4], dsv[WEDGE_QUADS][4];
#pragma unroll
        for (int j = 0; j < WEDGE_QUADS; j++) {
#pragma unroll
            for (int k = 0; k < 4; k++) r1v[j][k] = d10v[j][k] = dsv[j][k] = 0;
            if (lane + 64 * j < Q)
                search_quad<IS16>(d, lane + 64 * j, lq, a, r1v[j], d10v[j], dsv[j]);
        }
#pragma unroll 4
        for (int i = 0; i < SVT_HIP_WEDGE_TYPES; i++) {
            // both masks of the index: the sign is only known after the block-wide sum, so the squared sums are taken under
            // both and selected afterwards
            uint32_t dsm = 0;
            SplitSum e0{0, 0}, e1{0, 0};
#pragma unroll
            for (int j = 0; j < WEDGE_QUADS; j++) {
                const int q = lane + 64 * j;
                if (q < Q) {
                    int m0[4], m1[4];
                    load4<false>(masks + (size_t)(2 * i) * N + 4 * q, 4, m0);
                    load4<false>(masks + (size_t)(2 * i + 1) * N + 4 * q, 4, m1);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        dsm += (uint32_t)(dsv[j][k] * m0[k]);
                        const int t0 = clamp_i16(64 * r1v[j][k] + m0[k] * d10v[j][k]), t1 = clamp_i16(64 * r1v[j][k] + m1[k] * d10v[j][k]);
                        e0.add((uint32_t)(t0 * t0)), e1.add((uint32_t)(t1 * t1));
                    }
                }
            }
            const uint32_t t[5] = {wave_sum(dsm), wave_sum(e0.lo), wave_sum(e0.hi), wave_sum(e1.lo), wave_sum(e1.hi)};
            if (lane == i)
                w_dsm = t[0], w_lo0 = t[1], w_hi0 = t[2], w_lo1 = t[3], w_hi1 = t[4];
        }
    } else {
        int r1v[4], d10v[4], dsv[4];
        for (int q = lane; q < Q; q += 64) search_quad<IS16>(d, q, lq, a, r1v, d10v, dsv);
    }
    const uint32_t sad = wave_sum(a.sad);
    const uint64_t ss0 = SplitSum::total(wave_sum(a.ss0.lo), wave_sum(a.ss0.hi)), ss1 = SplitSum::total(wave_sum(a.ss1.lo), wave_sum(a.ss1.hi));
    const uint64_t dw0 = SplitSum::total(wave_sum(a.dw0.lo), wave_sum(a.dw0.hi)), dw1 = SplitSum::total(wave_sum(a.dw1.lo), wave_sum(a.dw1.hi));
    uint64_t       sse = 0;
    int            sign = 0;
    if (masks) {
        const int64_t limit = ((int64_t)ss0 - (int64_t)ss1) * 32;  // (.. * (1 << WEDGE_WEIGHT_BITS)) / 2
        sign = (int64_t)(int32_t)w_dsm > limit;
        sse = ((sign ? SplitSum::total(w_lo1, w_hi1) : SplitSum::total(w_lo0, w_hi0)) + 2048) >> 12;
    }
    // lane 0 walks the indices in order (strict <: the first minimum wins) and writes the record
    SvtHipMaskSearchResult r{};
    uint64_t               best = ~0ull;
    r.best_wedge_index = -1;
#pragma unroll
    for (int i = 0; i < SVT_HIP_WEDGE_TYPES; i++) {
        const uint64_t s = ((uint64_t)(uint32_t)__shfl((int)(sse >> 32), i, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)sse, i, 64);
        const int      sg = __shfl(sign, i, 64);
        r.wedge_sse[i] = s, r.wedge_sign[i] = (uint8_t)sg;
        if (masks && s < best) {
            best = s, r.best_wedge_index = (int8_t)i, r.best_wedge_sign = (int8_t)sg;
        }
    }
    if (lane != 0)
        return;
    r.diffwtd_sse[0] = (dw0 + 2048) >> 12, r.diffwtd_sse[1] = (dw1 + 2048) >> 12;
    r.best_diffwtd_type = r.diffwtd_sse[1] < r.diffwtd_sse[0];
    r.pred0_to_pred1_dist = sad;
    *res = r;
}

__global__ __launch_bounds__(64) void mask_search_kernel(const SvtHipMaskSearchDesc *__restrict__ descs,
                                                         SvtHipMaskSearchResult *__restrict__ results) {
    const SvtHipMaskSearchDesc d = descs[blockIdx.x];  // uniform: scalar loads
    SvtHipMaskSearchResult    *res = results + blockIdx.x;
    const int                  status = search_desc_status(d);
    if (status != SVT_HIP_MASK_SEARCH_OK) {
        if (threadIdx.x == 0) {
            SvtHipMaskSearchResult r{};
            r.status = (uint8_t)status;
            *res = r;
        }
        return;
    }
    d.is_16bit ? search_block<true>(d, res) : search_block<false>(d, res);
}

}  // namespace

extern "C" int32_t svt_hip_blend_batch(const SvtHipBlendDesc *d_desc, uint32_t n, void *stream) {
    if (!d_desc || n == 0)
        return refuse("svt_hip_blend_batch: bad argument");
    TierBCall c("svt_hip_blend_batch", stream);
    if (!c.ok())
        return c.status();
    hipLaunchKernelGGL(blend_kernel, dim3((n + BLEND_CHUNKS - 1) / BLEND_CHUNKS, BLEND_CHUNKS), dim3(64), 0, c.stream(), d_desc, n);
    return c.finish();
}

extern "C" int32_t svt_hip_compound_mask_search_batch(const SvtHipMaskSearchDesc *d_desc, SvtHipMaskSearchResult *d_result, uint32_t n,
                                                      void *stream) {
    if (!d_desc || !d_result || n == 0)
        return refuse("svt_hip_compound_mask_search_batch: bad argument");
    TierBCall c("svt_hip_compound_mask_search_batch", stream);
    if (!c.ok())
        return c.status();
    hipLaunchKernelGGL(mask_search_kernel, dim3(n), dim3(64), 0, c.stream(), d_desc, d_result);
    return c.finish();
}

SVT_HIP_MODULE_WARMUP(inter_blend)
