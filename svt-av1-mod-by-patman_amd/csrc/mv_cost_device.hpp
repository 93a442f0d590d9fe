// mv_cost_device.hpp — the motion-vector rules the motion searches of mode decision share: the two range rules, which the host's
// svt_hip_*_mv_limits and the OBMC search apply, svt_mv_cost, and svt_mv_err_cost (mcomp.c:44-68), which both svt_mv_err_cost_ of the
// sub-pel trees (inter_subpel.hip) and svt_aom_fp_mv_err_cost of the full-pel search (inter_fpel.hip) end in.
#pragma once
#include "../../include/svt_hip_inter.h"

namespace svthip {
namespace subpel {

constexpr int MV_LOW = -(1 << 14), MV_UPP = 1 << 14;  // cabac_context_model.h:523-525
constexpr int MAX_FULL_PEL_VAL = (1 << 10) - 1;       // av1me.h:24-27

__host__ __device__ constexpr int lesser(int a, int b) { return a < b ? a : b; }
__host__ __device__ constexpr int greater(int a, int b) { return a > b ? a : b; }

// Limits are {col_min, col_max, row_min, row_max}.
// svt_av1_set_mv_search_range (av1me.c:205-226): full-pel limits narrowed to what can be coded against ref_mv
__host__ __device__ inline void set_mv_search_range(int32_t lim[4], SvtHipMv ref_mv) {
    const int col = ref_mv.col, row = ref_mv.row;
    lim[0] = greater(lim[0], greater((col >> 3) - MAX_FULL_PEL_VAL + !!(col & 7), (MV_LOW >> 3) + 1));
    lim[1] = lesser(lim[1], lesser((col >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1));
    lim[2] = greater(lim[2], greater((row >> 3) - MAX_FULL_PEL_VAL + !!(row & 7), (MV_LOW >> 3) + 1));
    lim[3] = lesser(lim[3], lesser((row >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1));
}
// svt_av1_set_subpel_mv_search_range (mcomp.h:113-125), set_subpel_mv_search_range (av1me.c:778-790): the limits in 1/8 units of a
// sub-pel search from the full-pel limits fp
__host__ __device__ inline void set_subpel_mv_search_range(int32_t lim[4], const int32_t fp[4], SvtHipMv ref_mv) {
    const int max_mv = MAX_FULL_PEL_VAL * 8;
    lim[0] = greater(MV_LOW + 1, greater(fp[0] * 8, ref_mv.col - max_mv)), lim[1] = lesser(MV_UPP - 1, lesser(fp[1] * 8, ref_mv.col + max_mv));
    lim[2] = greater(MV_LOW + 1, greater(fp[2] * 8, ref_mv.row - max_mv)), lim[3] = lesser(MV_UPP - 1, lesser(fp[3] * 8, ref_mv.row + max_mv));
}

// svt_mv_joint of a vector difference, and what MV_COST_ENTROPY makes of svt_mv_cost's rate (mcomp.h:136-139, mcomp.c:50-55); a search
// that has the table entries of a tile's rows and columns at hand (inter_fpel.hip) builds the cost from these
__device__ __forceinline__ int mv_joint(int16_t dr, int16_t dc) { return dr == 0 ? (dc == 0 ? 0 : 1) : (dc == 0 ? 2 : 3); }
// mvjcost[joint] by selection: indexing the by-value job with a run-time index would put it in scratch
__device__ __forceinline__ int mv_joint_cost(const SvtHipSubpelJob &job, int joint) {
    return joint == 0 ? job.mvjcost[0] : joint == 1 ? job.mvjcost[1] : joint == 2 ? job.mvjcost[2] : job.mvjcost[3];
}
__device__ __forceinline__ int mv_table_index(int16_t d) { return min(max((int)d, MV_LOW), MV_UPP); }
__device__ __forceinline__ int mv_entropy_cost(int rate, int error_per_bit) {
    return (int)(((int64_t)rate * error_per_bit + (1 << 13)) >> 14);  // RDDIV_BITS + AV1_PROB_COST_SHIFT - RD_EPB_SHIFT + 4
}
// svt_mv_cost (mcomp.h:136-139) of a difference that has been stored in the int16 fields of an MV
__device__ __forceinline__ int mv_rate(int16_t dr, int16_t dc, const SvtHipSubpelJob &job) {
    return job.mvjcost[mv_joint(dr, dc)] + job.mvcost[0][mv_table_index(dr)] + job.mvcost[1][mv_table_index(dc)];
}

// svt_mv_err_cost: the cost of mv against ref_mv under one of the six MV_COST_TYPEs; job's tables are read by MV_COST_ENTROPY only.
// WITH_ENTROPY = false: for a caller that has dealt with MV_COST_ENTROPY itself.
template <bool WITH_ENTROPY = true> __device__ __forceinline__ int mv_err_cost(SvtHipMv mv, SvtHipMv ref_mv, int mv_cost_type, int error_per_bit, const SvtHipSubpelJob &job) {
    const int16_t dr = (int16_t)(mv.row - ref_mv.row), dc = (int16_t)(mv.col - ref_mv.col);  // MV fields: int16
    const int     l1 = (int16_t)abs((int)dr) + (int16_t)abs((int)dc);
    switch (mv_cost_type) {
    case 0: return WITH_ENTROPY ? mv_entropy_cost(mv_rate(dr, dc, job), error_per_bit) : 0;  // MV_COST_ENTROPY
    case 1: return (2 * l1) >> 3;  // SSE_LAMBDA_LOWRES
    case 2: return 0;              // SSE_LAMBDA_MIDRES is 0
    case 3: return l1 >> 3;        // SSE_LAMBDA_HDRES
    case 4: return (int)(((int64_t)(l1 << 8) * error_per_bit + (1 << 13)) >> 14);  // MV_COST_OPT
    default: return 0;             // MV_COST_NONE
    }
}

}  // namespace subpel
}  // namespace svthip
