// txfm_rate_device.hpp — what the rate (txfm_rate.hip) and the RDOQ trellis (txfm_rdoq.hip) share on the device: the layout of a
// block's level array and of the staged tables, and the closed forms of the coefficient entropy model: the transform class,
// get_golomb_cost, get_br_cost, get_eob_cost, the is_eob context and the two contexts a position takes from the levels of its
// neighbours.  Only what leaves both kernels' instruction streams as they were lives here: the level fill, the table staging, the
// per-block clamps and the group reductions compile differently as functions (a callee is simplified before it is inlined), so
// each kernel keeps its own.  Their host side is txb_geometry.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svt_hip_txfm.h"

namespace svthip {
namespace rate {

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

// A block's level array, four levels to a word: row pitch IW + 4 and four zero rows below (the layout of svt_av1_txb_init_levels_c
// without the two rows it keeps above, which neither context reads).  `L` below points at a position inside it.
template <int IW, int IH>
struct Levels { static constexpr int STRIDE = IW + 4, ROW_WORDS = STRIDE / 4, WORDS = ROW_WORDS * (IH + 4); };

constexpr int TABLE_WORDS = 2 * sizeof(SvtHipCoeffCost) / 4;  // both planes of one table set at one size context, as staged in LDS

// tx_type_to_class (cabac_context_model.h:459-476): 0 two-dimensional, 1 horizontal, 2 vertical
__device__ __forceinline__ int tx_class_of(int tx_type) { return tx_type < 10 ? 0 : (tx_type & 1) ? 1 : 2; }

// get_golomb_cost (rd_cost.c:90-97)
__device__ __forceinline__ int golomb_cost(int level) {
    if (level < 15)
        return 0;
    const int length = 32 - __clz(level - 14);
    return (2 * length - 1) * 512;
}

// get_eob_cost (rd_cost.c:281-298) with get_eob_pos_token, eb_k_eob_group_start and eb_k_eob_offset_bits in closed form
__device__ __forceinline__ int eob_cost(int eob, const int32_t (*eob_bits)[11], const int32_t (*eob_extra)[2], int cls) {
    const int pt = eob < 2 ? eob : 33 - __clz(eob - 1);
    int       cost = eob_bits[cls != 0][pt - 1];
    const int offset_bits = pt - 2;
    if (offset_bits > 0) {
        const int extra = eob - ((1 << offset_bits) + 1);
        cost += eob_extra[pt - 3][(extra >> (offset_bits - 1)) & 1] + (offset_bits - 1) * 512;
    }
    return cost;
}

// get_br_cost: lps_cost[ctx][..] + Golomb tail of a level above NUM_BASE_LEVELS
__device__ __forceinline__ int range_cost(const SvtHipCoeffCost &cc, int br_ctx, int level) {
    const int base_range = level - 3;
    return cc.lps[br_ctx][base_range < 12 ? base_range : 12] + golomb_cost(level);
}

__device__ __forceinline__ int min3(int v) { return v < 3 ? v : 3; }

// av1_transform_type_rate_estimation (rd_cost.c:113-158) with get_ext_tx_set_type / ext_tx_set_index (definitions.h:1795-1836), which
// is also av1_txt_rate_est (product_coding_loop.c:4432-4454); sqr, sqr_up: TxbGeometry's
__device__ inline int tx_type_rate(const SvtHipRateTables &t, const SvtHipTxbCostDesc &d, int sqr, int sqr_up) {
    const int is_inter = d.pred_mode >= 13 && d.pred_mode < 25;
    int       set_type;  // TxSetType
    if (sqr_up > 3)
        set_type = 0;
    else if (sqr_up == 3)
        set_type = is_inter ? 1 : 0;
    else if (d.reduced_tx_set)
        set_type = is_inter ? 1 : 2;
    else if (is_inter)
        set_type = sqr == 2 ? 4 : 5;
    else
        set_type = sqr == 2 ? 2 : 3;
    if (set_type == 0)  // one type in the set
        return 0;
    const int tx_type = d.tx_type & 15, sq = sqr < 3 ? sqr : 3;
    if (is_inter) {
        const int set = set_type == 1 ? 3 : set_type == 4 ? 2 : 1;
        return t.inter_tx_type[set][sq][tx_type];
    }
    const int set = set_type == 3 ? 1 : 2;
    int       dir = d.pred_mode;
    if (d.filter_intra_mode < 5)  // fimode_to_intradir
        dir = d.filter_intra_mode == 1 ? 1 : d.filter_intra_mode == 2 ? 2 : d.filter_intra_mode == 3 ? 6 : 0;
    return t.intra_tx_type[set][sq][dir < 12 ? dir : 12][tx_type];
}

// get_nz_map_ctx with is_eob (encode_txb_ref_c.c:17-27), get_lower_levels_ctx_eob: of scan index c >= 1 (scan index 0 has context 0)
template <int N>
__device__ __forceinline__ int eob_ctx_of(int c) { return c <= N / 8 ? 1 : c <= N / 4 ? 2 : 3; }

// get_br_ctx (common_utils.h:104-141) of raster position pos = row * IW + col
template <int IW>
__device__ __forceinline__ int br_ctx_of(const uint8_t *L, int pos, int row, int col, int cls) {
    constexpr int STRIDE = IW + 4;
    int mag = L[1] + L[STRIDE];
    mag += cls == 0 ? L[STRIDE + 1] : cls == 1 ? L[2] : L[2 * STRIDE];
    mag    = (mag + 1) >> 1;
    int br_ctx = mag < 6 ? mag : 6;
    if (pos != 0)
        br_ctx += (cls == 0 ? (row < 2 && col < 2) : cls == 1 ? col == 0 : row == 0) ? 7 : 14;
    return br_ctx;
}

// get_nz_mag + get_nz_map_ctx_from_stats (coefficients.h:2884-2943); orient: sign of w - h
template <int IW>
__device__ __forceinline__ int nz_ctx_of(const uint8_t *L, int pos, int row, int col, int cls, int orient) {
    constexpr int STRIDE = IW + 4;
    int ctx = 0;
    if (cls != 0 || pos != 0) {
        int mag = min3(L[1]) + min3(L[STRIDE]);
        if (cls == 0)
            mag += min3(L[STRIDE + 1]) + min3(L[2]) + min3(L[2 * STRIDE]);
        else if (cls == 2)
            mag += min3(L[2 * STRIDE]) + min3(L[3 * STRIDE]) + min3(L[4 * STRIDE]);
        else
            mag += min3(L[2]) + min3(L[3]) + min3(L[4]);
        ctx = (mag + 1) >> 1;
        ctx = ctx < 4 ? ctx : 4;
        if (cls == 0) {  // the rule eb_av1_nz_map_ctx_offset was generated by
            if (orient < 0 && row < 2)
                ctx += 11;
            else if (orient > 0 && col < 2)
                ctx += 16;
            else
                ctx += row + col < 2 ? 1 : row + col < 4 ? 6 : 21;
        } else {  // nz_map_ctx_offset_1d
            const int k = cls == 1 ? col : row;
            ctx += k == 0 ? 26 : k == 1 ? 31 : 36;
        }
    }
    return ctx;
}

}  // namespace rate
}  // namespace svthip
