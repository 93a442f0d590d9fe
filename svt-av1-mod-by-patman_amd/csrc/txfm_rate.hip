// txfm_rate.hip — the coefficient rate of transform blocks on device-resident quantiser output (Tier B only):
//   svt_av1_cost_coeffs_txb with allow_update_cdf = 0   (reference: rd_cost.c:434-559, reached through
//   svt_aom_txb_estimate_coeff_bits :1405-1450) and the cost tx_type_search forms from it (product_coding_loop.c:4737-4786).
// The reference walks the scan backwards; every term of its sum depends only on one position, its scan index and the levels
// of up to five neighbours, so the sum is taken BY POSITION here: the lane that owns raster position pos reads c = iscan[pos]
// and adds the eob-1 form, the DC form, the loop form or nothing.  Integer table look-ups only; sums are int32 as there.
//
// Work split: a block of n = min(w,32) * min(h,32) retained coefficients belongs to a group of min(n, 64) lanes, so 16-, 32-
// and 64-coefficient blocks sit 4, 2 and 1 to a wavefront and larger blocks take n / 64 (up to 16) positions per lane.  A
// workgroup of 256 lanes walks the batch in steps of its 256 / group blocks.  The levels (|qcoeff| clamped to 127, as
// svt_av1_txb_init_levels_c) of each block lie in LDS with the reference's row pitch of w + 4 and four zero rows below, so
// get_nz_mag and get_br_ctx read neighbours without bounds tests; the two rows the reference keeps above are never read by
// either and are left out.  Blocks with eob <= 1 or a closed-form rate read no level, as in the reference.
// Rate tables: one launch has one size context, so each workgroup stages the two planes' SvtHipCoeffCost (7552 B) of its first block's
// table set into LDS once and keeps them for all its steps (the grid is capped, a workgroup takes many steps); a block of another
// table set reads its own through the cache.  Reading all of them through the cache is the LDS_TABLES = false instance, kept for
// svt_hip_txb_cost_batch_placed: 13 - 15 % slower at every size (profiles/txb_cost_4k.json).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svt_hip_txfm.h"
#include "common.hpp"
#include "txb_geometry.hpp"
#include "txfm_rate_device.hpp"

using namespace svthip;
using namespace svthip::rate;

namespace {

// what the kernel reads of the launch; the first four are TxbGeometry's
struct TxbCostLaunch {
    int32_t  orient, txs_ctx, sqr, sqr_up;
    int32_t  dist_shift;  // (MAX_TX_SCALE - tx_scale) * 2: 2, 0 or -2
    uint32_t area_th;     // (w * h) >> 6
    uint32_t n_tables, n_blocks;
};

// the eob == 1 form (av1_cost_coeffs_txb_loop_cost_one_eob, rd_cost.c:310-337): no level is read
__device__ __forceinline__ int one_eob_cost(const SvtHipCoeffCost &cc, int32_t v, int dc_sign_ctx) {
    const int level = v < 0 ? -v : v;
    int       cost = cc.base_eob[0][level ? min3(level) - 1 : 0];
    if (v != 0) {
        cost += cc.dc_sign[dc_sign_ctx][v < 0];
        if (level > 2)
            cost += range_cost(cc, 0, level);
    }
    return cost;
}

// One position's term of av1_cost_coeffs_txb_loop_cost_eob (rd_cost.c:339-431) for eob > 1 and c == eob - 1, c == 0 or
// 1 <= c <= c_start.  levels: the block's padded level array.
template <int IW, int IH>
__device__ __forceinline__ int position_cost(const SvtHipCoeffCost &cc, const uint8_t *levels, const int32_t *qc, int pos, int c, int eob,
                                             int cls, int orient, int dc_sign_ctx) {
    constexpr int  BWL = ilog2(IW), STRIDE = IW + 4, N = IW * IH;
    const int      row = pos >> BWL, col = pos & (IW - 1);
    const uint8_t *L = levels + row * STRIDE + col;
    int            level = L[0];
    int32_t        v = level;  // its sign matters to the DC term only
    if (level >= 15 || c == 0) {  // beyond the base range the Golomb tail needs the value itself
        v     = qc[pos];
        level = v < 0 ? -v : v;
    }
    const int br_ctx = level > 2 ? br_ctx_of<IW>(L, pos, row, col, cls) : 0;
    int cost;
    if (c == eob - 1) {  // c >= 1 here
        cost = cc.base_eob[eob_ctx_of<N>(c)][level ? min3(level) - 1 : 0] + (level ? 512 : 0);
    } else {
        const int ctx = nz_ctx_of<IW>(L, pos, row, col, cls, orient);
        cost = cc.base[ctx][min3(level)];
        if (level)
            cost += c == 0 ? cc.dc_sign[dc_sign_ctx][v < 0] : 512;
    }
    if (level > 2)
        cost += range_cost(cc, br_ctx, level);
    return cost;
}

// everything of one block that is summed over positions; G lanes call it together
template <int IW, int IH, int G>
__device__ __forceinline__ int coefficient_cost(const SvtHipCoeffCost &cc, const uint8_t *levels, const int32_t *qc, const int16_t *iscan,
                                                int li, int eob, int c_start, int cls, int orient, int dc_sign_ctx) {
    constexpr int N = IW * IH;
    int           cost = 0;
    if (eob == 1) {
        if (li == 0)
            cost = one_eob_cost(cc, qc[0], dc_sign_ctx);
        return cost;
    }
#pragma unroll
    for (int k = 0; k < N / G; k++) {
        const int pos = li + k * G, c = iscan[pos];
        if (c == eob - 1 || (c >= 0 && c <= c_start))
            cost += position_cost<IW, IH>(cc, levels, qc, pos, c, eob, cls, orient, dc_sign_ctx);
    }
    return cost;
}

template <int IW, int IH, bool LDS_TABLES>
__global__ __launch_bounds__(256) void txb_cost_kernel(const uint8_t *__restrict__ base, const SvtHipTxbCostDesc *__restrict__ descs,
                                                       const SvtHipRateTables *__restrict__ tables, const SvtHipTxfmResult *__restrict__ results,
                                                       const uint64_t (*__restrict__ dist)[2], SvtHipTxbCost *__restrict__ out, TxbCostLaunch prm) {
    constexpr int N = IW * IH, G = group_lanes(N), BLOCKS = 256 / G;
    constexpr int ROW_WORDS = Levels<IW, IH>::ROW_WORDS, LEVEL_WORDS = Levels<IW, IH>::WORDS;
    __shared__ uint32_t        lv[BLOCKS][LEVEL_WORDS];
    __shared__ int32_t staged_words[LDS_TABLES ? TABLE_WORDS : 1];  // both planes of the table set of the workgroup's first block
    const SvtHipCoeffCost *staged = (const SvtHipCoeffCost *)staged_words;
    const int      gi = threadIdx.x / G, li = threadIdx.x % G;
    uint32_t       first_table = 0;
    if (LDS_TABLES) {
        first_table = descs[blockIdx.x * BLOCKS].table;  // the grid never exceeds the batch
        first_table = first_table < prm.n_tables ? first_table : prm.n_tables - 1;
        const int32_t *src = (const int32_t *)&tables[first_table].coeff[prm.txs_ctx][0];
        for (int i = threadIdx.x; i < TABLE_WORDS; i += 256) staged_words[i] = src[i];
    }
    for (uint32_t b0 = blockIdx.x * BLOCKS; b0 < prm.n_blocks; b0 += gridDim.x * BLOCKS) {
        const uint32_t tb = b0 + gi;
        const bool     active = tb < prm.n_blocks;
        SvtHipTxbCostDesc d = descs[active ? tb : prm.n_blocks - 1];
        int            eob = results ? results[active ? tb : 0].eob : d.eob;
        eob = eob < N ? eob : N;
        const bool short_form = (d.est_mode >= SVT_HIP_TXB_COST_SHORT_SMALL && (uint32_t)eob < prm.area_th) || d.est_mode >= SVT_HIP_TXB_COST_SHORT_ALL;
        const bool exact = active && eob > 0 && !short_form;
        const int32_t *qc = (const int32_t *)(base + d.qcoeff_off);
        __syncthreads();  // the levels of the previous step have been read (and, first time round, the staged tables written)
        if (exact && eob > 1) {  // svt_av1_txb_init_levels_c, four levels to a word; the pad columns and rows are zero
            const bool vec = (((uintptr_t)qc) & 15) == 0;
            for (int wd = li; wd < LEVEL_WORDS; wd += G) {
                const int r = wd / ROW_WORDS, c4 = wd - r * ROW_WORDS;
                uint32_t  word = 0;
                if (r < IH && c4 < IW / 4) {
                    const int32_t *q = qc + r * IW + c4 * 4;
                    int32_t        v[4];
                    if (vec) {
                        const int4 q4 = *(const int4 *)q;
                        v[0] = q4.x, v[1] = q4.y, v[2] = q4.z, v[3] = q4.w;
                    } else {
                        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
                    }
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t a = v[j] < 0 ? 0u - (uint32_t)v[j] : (uint32_t)v[j];
                        word |= (a < 127 ? a : 127) << (8 * j);
                    }
                }
                lv[gi][wd] = word;
            }
        }
        __syncthreads();
        int cost = 0;
        const uint32_t ti = d.table < prm.n_tables ? d.table : prm.n_tables - 1;
        const SvtHipRateTables &t = tables[ti];
        const int plane = d.plane_type != 0, cls = tx_class_of(d.tx_type & 15);
        const int skip_ctx = d.txb_skip_ctx < 12 ? d.txb_skip_ctx : 12, sign_ctx = d.dc_sign_ctx < 2 ? d.dc_sign_ctx : 2;
        const SvtHipCoeffCost &cc_global = t.coeff[prm.txs_ctx][plane];
        if (exact) {
            const int div = (int)d.fast_coeff_est_level - (int)d.subres_step;
            const int by = eob / (div > 1 ? div : 1), c_start = eob - 2 < by ? eob - 2 : by;
            const int16_t *iscan = (const int16_t *)(base + d.iscan_off);
            const uint8_t *levels = (const uint8_t *)lv[gi];
            if (LDS_TABLES && ti == first_table)
                cost = coefficient_cost<IW, IH, G>(staged[plane], levels, qc, iscan, li, eob, c_start, cls, prm.orient, sign_ctx);
            else
                cost = coefficient_cost<IW, IH, G>(cc_global, levels, qc, iscan, li, eob, c_start, cls, prm.orient, sign_ctx);
            if (li == 0) {
                cost += cc_global.txb_skip[skip_ctx][0] + eob_cost(eob, t.eob[ilog2(N) - 4][plane], cc_global.eob_extra, cls);
                if (!plane)
                    cost += tx_type_rate(t, d, prm.sqr, prm.sqr_up);
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) cost += __shfl_xor(cost, off, 64);
        if (active && li == 0) {
            uint64_t bits;
            if (short_form)
                bits = d.est_mode >= SVT_HIP_TXB_COST_SHORT_SMALL && (uint32_t)eob < prm.area_th ? 6000 + 1000 * (uint64_t)eob : 3000 + 100 * (uint64_t)eob;
            else if (eob == 0)
                bits = (uint64_t)(int64_t)cc_global.txb_skip[skip_ctx][1];
            else
                bits = (uint64_t)(int64_t)cost << ((d.flags & SVT_HIP_TXB_COST_NO_SHIFT) ? 0 : d.subres_step);
            uint64_t rd = 0;
            if (dist) {  // product_coding_loop.c:4737-4749 and RDCOST (rd_cost.h:37)
                uint64_t dd = dist[tb][0] + (results ? results[tb].three_quad_energy : 0);
                dd = (prm.dist_shift < 0 ? dd << -prm.dist_shift : dd >> prm.dist_shift) << d.subres_step;
                rd = (uint64_t)((((int64_t)bits * (int64_t)d.lambda + 256) >> 9) + (int64_t)dd * 128);
            }
            SvtHipTxbCost r;
            r.bits = bits, r.rd_cost = rd;
            out[tb] = r;
        }
    }
}

constexpr bool kTablesInLds = true;  // svt_hip_txb_cost_batch: the faster placement at every size of profiles/txb_cost_4k.json

}  // namespace

extern "C" int32_t svt_hip_txb_cost_batch_placed(const uint8_t *d_base, const SvtHipTxbCostDesc *d_desc, const SvtHipRateTables *d_tables,
                                                 uint32_t n_tables, const SvtHipTxfmResult *d_txfm_result, const uint64_t (*d_distortion)[2],
                                                 SvtHipTxbCost *d_out, uint32_t n_blocks, uint32_t w, uint32_t h, uint32_t tables_in_lds,
                                                 void *stream) {
    const TxbGeometry g(w, h);
    if (!g.valid || n_tables == 0 || (n_blocks > 0 && (!d_base || !d_desc || !d_tables || !d_out)))
        return refuse("svt_hip_txb_cost_batch: bad argument (%u x %u, %u table sets, %u blocks)", w, h, n_tables, n_blocks);
    if (n_blocks == 0)
        return SVT_HIP_OK;
    TierBCall c("svt_hip_txb_cost_batch_placed", stream);
    if (!c.ok())
        return c.status();
    const TxbCostLaunch prm{g.orient, g.txs_ctx, g.sqr, g.sqr_up, (1 - g.tx_scale) * 2, g.pixels >> 6, n_tables, n_blocks};
    const dim3  grid(grid_blocks(n_blocks, 256 / group_lanes(g.retained), (uint32_t)cu_count() * 8));  // 8 workgroups fill a CU's wave slots
    const bool  launched = for_retained_shape(g.iw, g.ih, [&](auto W, auto H) {
        constexpr int IW = decltype(W)::value, IH = decltype(H)::value;
        const auto    kernel = tables_in_lds ? txb_cost_kernel<IW, IH, true> : txb_cost_kernel<IW, IH, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c.stream(), d_base, d_desc, d_tables, d_txfm_result, d_distortion, d_out, prm);
    });
    if (!launched) {
        set_error("svt_hip_txb_cost_batch: no kernel for the retained shape %u x %u", g.iw, g.ih);
        return SVT_HIP_ERR_RUNTIME;
    }
    return c.finish();
}

extern "C" int32_t svt_hip_txb_cost_batch(const uint8_t *d_base, const SvtHipTxbCostDesc *d_desc, const SvtHipRateTables *d_tables,
                                          uint32_t n_tables, const SvtHipTxfmResult *d_txfm_result, const uint64_t (*d_distortion)[2],
                                          SvtHipTxbCost *d_out, uint32_t n_blocks, uint32_t w, uint32_t h, void *stream) {
    return svt_hip_txb_cost_batch_placed(d_base, d_desc, d_tables, n_tables, d_txfm_result, d_distortion, d_out, n_blocks, w, h, kTablesInLds,
                                         stream);
}

SVT_HIP_MODULE_WARMUP(txfm_rate)
