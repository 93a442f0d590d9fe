// intra_search.hip — the open-loop intra search of TPL level 1 on gfx950 (include/svt_hip_intra.h): every 16x16 block of one or more
// source pictures over DC_PRED .. intra_mode_end with SAD or SATD cost, as the source-based path of tpl_mc_flow_dispenser_sb_generic
// (src_ops_process.c:519-760) does it at dispenser_search_level 0.
//
// One wavefront per block, grid (blocks, pictures): lane (lr, lc) owns the four source samples of row lr = lane / 4 from column
// lc = 4 (lane % 4) on, in one register.  Lane 0 gathers the block's neighbours into LDS (intra::neighbours); then per mode, in the
// reference's order: the directional modes other than V / H filter a copy of the edges (one lane per edge entry), every lane predicts
// its four samples (intra::predict_sample), and
//   SAD:  `v_sad_u8` against the source register and a wave sum;
//   SATD: the prediction is parked in LDS; after four modes the fused transform block of txfm_block.hpp (residual source - prediction ->
//         DCT_DCT 16x16 with the pf_shape zero-out -> svt_aom_satd, no quantiser) runs the four of them side by side, 16 lanes each.
// The first strict minimum wins.  No run-time-indexed private arrays, no 64-bit division.
#include <cstdint>
#include <cstring>

#include "../../include/svt_hip_intra.h"
#include "common.hpp"
#include "intra_device.hpp"
#include "txfm_block.hpp"

using namespace svthip;

namespace {

constexpr int BS = 16, SLOTS = 4;           // modes per transform round: four groups of 16 lanes
__device__ const uint16_t INTRA_ISCAN[256] = {0};  // not read (no quantiser); the descriptor still gets a valid address

__device__ __forceinline__ uint32_t ld4u(const uint8_t *p) {  // four samples of a row that need not be aligned
    typedef uint32_t __attribute__((aligned(1))) u32u;
    return *(const __attribute__((address_space(1))) u32u *)p;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void intra_search_kernel(const SvtHipIntraSearchJob *jobs) {
    __shared__ int32_t  tile[SLOTS * 16 * 17];
    __shared__ uint32_t pred_lds[SLOTS][BS * BS / 4];
    __shared__ uint8_t  edges[4][48];  // gathered above / left, filtered above / left: entry [-1] at index 7
    const SvtHipIntraSearchJob &j = jobs[blockIdx.y];
    const uint32_t W = j.src.width, H = j.src.height, cols = (W + 15) >> 4, rows = (H + 15) >> 4;
    if (blockIdx.x >= cols * rows)
        return;
    const uint32_t cy = blockIdx.x / cols, cx = blockIdx.x - cy * cols, x = cx * BS, y = cy * BS;
    const int      lane = threadIdx.x;
    const size_t   cell = (size_t)cy * cols + cx;
    int64_t       *mc   = j.mode_cost ? j.mode_cost + cell * intra::MODES : nullptr;
    if (x + BS / 2 > W || y + BS / 2 > H) {  // less than half of the block inside: not searched
        if (lane == 0)
            j.best_mode[cell] = 0xFF, j.best_cost[cell] = INT64_MAX;
        if (mc && lane < intra::MODES)
            mc[lane] = INT64_MAX;
        return;
    }
    const uint32_t ss   = j.src.stride;
    const uint8_t *src0 = j.src.buf + (size_t)j.src.org_y * ss + j.src.org_x;
    const uint8_t *src  = src0 + (size_t)y * ss + x;
    const int      lr = lane >> 2, lc = (lane & 3) * 4;
    const uint32_t spx = ld4u(src + (size_t)lr * ss + lc);
    uint8_t *above0 = &edges[0][8], *left0 = &edges[1][8], *above = &edges[2][8], *left = &edges[3][8];
    if (lane == 0)
        intra::neighbours<BS>(above0 - 1, left0 - 1, src0, ss, x, y, W, H);
    __syncthreads();
    const uint32_t dc = intra::dc_of<BS>(wave_sum(lane < BS ? above0[lane] : 0u), wave_sum(lane < BS ? left0[lane] : 0u), x > 0, y > 0);

    const int  mode_end = j.ctrls.intra_mode_end, max_w = j.ctrls.max_input_luma_width, max_h = j.ctrls.max_input_luma_height;
    const bool use_sad  = j.ctrls.use_sad;
    uint8_t   *pout     = j.pred ? j.pred + cell * (intra::MODES * BS * BS) + lr * BS + lc : nullptr;
    int64_t    best = INT64_MAX;
    int        best_mode = intra::DC;
    // SATD: the transform block of 16 lanes g reads slot g of the predictions (a flat address of LDS) and the block's source rows
    SvtHipTxfmDesc d;
    memset(&d, 0, sizeof(d));
    const int g = lane >> 4;
    d.residual_off = (uint64_t)(uintptr_t)src, d.residual_stride = ss;
    d.pred_off = (uint64_t)(uintptr_t)&pred_lds[g][0], d.pred_stride = BS;
    d.coeff_off = d.qcoeff_off = d.dqcoeff_off = d.recon_off = SVT_HIP_NO_OFFSET;
    d.qm_off = d.iqm_off = SVT_HIP_NO_OFFSET, d.iscan_off = (uint64_t)(uintptr_t)INTRA_ISCAN;
    d.tx_type = 0, d.shape = j.ctrls.pf_shape, d.bit_depth = 8, d.quant_mode = SVT_HIP_QUANT_NONE, d.log_scale = 0;
    d.flags = (uint8_t)(SVT_HIP_TX_FWD | SVT_HIP_TX_SRC_PRED | SVT_HIP_TX_SATD);

    for (int m0 = 0; m0 <= mode_end; m0 += SLOTS) {
        for (int k = 0; k < SLOTS && m0 + k <= mode_end; k++) {
            const int      mode     = m0 + k;
            const int      angle    = intra::MODE_ANGLE[mode];
            const bool     filtered = intra::is_directional(mode) && angle != 90 && angle != 180;
            const uint8_t *pa = above0, *pl = left0;
            if (filtered) {
                intra::filter_edges<BS>(above0, left0, above, left, angle, (int)x, (int)y, max_w, max_h);
                __syncthreads();
                pa = above, pl = left;
            }
            uint32_t pv = dc * 0x01010101u;
            if (mode != intra::DC) {
                pv = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) pv |= intra::predict_sample<BS>(mode, pa, pl, lr, lc + i) << (8 * i);
            }
            if (pout) {
                uint8_t *o = pout + mode * (BS * BS);
                o[0] = (uint8_t)pv, o[1] = (uint8_t)(pv >> 8), o[2] = (uint8_t)(pv >> 16), o[3] = (uint8_t)(pv >> 24);
            }
            if (use_sad) {
                const int64_t cost = wave_sum(__builtin_amdgcn_sad_u8(spx, pv, 0u));
                if (mc && lane == 0)
                    mc[mode] = cost;
                if (cost < best)
                    best = cost, best_mode = mode;
            } else {
                pred_lds[k][lane] = pv;  // lane = lr * 4 + lc / 4: the slot is the 16x16 block in raster order
            }
            if (filtered)
                __syncthreads();  // the filtered edges are rewritten by the next directional mode
        }
        if (!use_sad) {
            __syncthreads();
            SvtHipTxfmResult res;
            memset(&res, 0, sizeof(res));
            txb::txfm_block<BS, BS>((uint8_t *)nullptr, d, &res, m0 + g <= mode_end, lane & 15, tile + g * (16 * 17));
            for (int k = 0; k < SLOTS && m0 + k <= mode_end; k++) {
                const int64_t cost = (int64_t)(uint32_t)__shfl((int)res.satd, 16 * k, 64);  // lane 16 k holds group k's result
                if (mc && lane == 0)
                    mc[m0 + k] = cost;
                if (cost < best)
                    best = cost, best_mode = m0 + k;
            }
            __syncthreads();  // slots and tile are rewritten by the next round
        }
    }
    if (lane == 0)
        j.best_mode[cell] = (uint8_t)best_mode, j.best_cost[cell] = best;
    if (mc && lane > mode_end && lane < intra::MODES)
        mc[lane] = INT64_MAX;
}

}  // namespace

extern "C" int32_t svt_hip_intra_search_frames(const SvtHipIntraSearchJob *jobs, uint32_t n, void *stream) {
    auto bad = [](uint32_t i, const char *m) { return refuse("svt_hip_intra_search_frames: job %u: %s", i, m); };
    if (!jobs || n == 0 || n > 65535)
        return refuse("svt_hip_intra_search_frames: NULL jobs or job count not in 1 .. 65535");
    uint32_t max_cells = 0;
    for (uint32_t i = 0; i < n; i++) {
        const SvtHipIntraSearchJob &jb = jobs[i];
        const SvtHipIntraCtrls     &c  = jb.ctrls;
        if (c.intra_mode_end >= SVT_HIP_INTRA_MODES || c.use_sad > 1 || c.pf_shape > 2)
            return bad(i, "ctrls out of range (intra_mode_end 0 .. 12, use_sad 0 / 1, pf_shape 0 .. 2)");
        if (c.subsample_tx != 0)
            return bad(i, "subsample_tx must be 0 (16x16 blocks)");
        if (!jb.src.buf || !jb.best_mode || !jb.best_cost)
            return bad(i, "NULL source plane or output array");
        if (jb.src.width == 0 || jb.src.height == 0)
            return bad(i, "empty picture");
        if (jb.src.stride < (uint32_t)jb.src.org_x + ((jb.src.width + 15u) & ~15u))
            return bad(i, "stride cannot hold org_x + width rounded up to 16 (the blocks at the right edge read that far)");
        const uint32_t cells = ((jb.src.width + 15u) >> 4) * ((jb.src.height + 15u) >> 4);
        max_cells            = cells > max_cells ? cells : max_cells;
    }
    TierBCall                   c("svt_hip_intra_search_frames", stream);
    const SvtHipIntraSearchJob *d_jobs = (const SvtHipIntraSearchJob *)c.stage(jobs, sizeof(SvtHipIntraSearchJob) * n);
    if (!d_jobs)
        return c.status();
    hipLaunchKernelGGL(intra_search_kernel, dim3(max_cells, n), dim3(64), 0, c.stream(), d_jobs);
    return c.finish();
}

SVT_HIP_MODULE_WARMUP(intra_search)
