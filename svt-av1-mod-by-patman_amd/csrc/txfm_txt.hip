// txfm_txt.hip — the transform-type search of a transform block on device-resident records (Tier B only): what tx_type_search
// (reference: product_coding_loop.c:4458-4940) does around the per-candidate stages the other txfm_*.hip files hold:
//   the spatial distortion of :4697-4718 per candidate,
//   the loop's decision (:4581-4812) per block with its four data-dependent exits, in the reference's integer types,
//   the copy of the winner's arrays (copy_txt_data, :4923-4926),
// and svt_hip_txt_search_batch, which enqueues the whole chain on one stream.
//
// Work split of the decision: the replay of one block is a serial walk over at most 16 candidates that reads four small records per
// candidate, so a block takes ONE lane; the copies are bandwidth work over n = min(w,32) * min(h,32) coefficients twice and w x h
// pixels, so a block takes a wavefront.  Two ways to join them, both kept behind svt_hip_txt_select_batch_mapped:
//   0  one kernel, a workgroup is one wavefront: its lanes replay 64 blocks, then it copies the winners of those 64 one after the other,
//   1  two kernels: the replay (a lane per block), then the copies with a wavefront per block, which reads the winner from d_out.
// The spatial distortion takes a wavefront per candidate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svt_hip_txfm.h"
#include "common.hpp"
#include "txb_geometry.hpp"
#include "txfm_block.hpp"
#include "txfm_rate_device.hpp"

using namespace svthip;
using namespace svthip::rate;

namespace {

constexpr uint32_t kNoCand = 0xFFFFFFFFu;

// what the kernels read of the launch; sqr, sqr_up and the shift are TxbGeometry's
struct TxtLaunch {
    int32_t  sqr, sqr_up;
    int32_t  dist_shift;  // (MAX_TX_SCALE - tx_scale) * 2: 2, 0 or -2
    uint32_t retained, w, h;
    uint32_t n_tables, n_cand_total, n_blocks;
    uint32_t recon;  // 0: a search without its inverse-only pass: d_distortion holds no spatial sums and recon_off no reconstruction
};

// the candidates of a block that exist: n_cand clamped to 16 and cut at the end of the per-candidate arrays
__device__ __forceinline__ uint32_t cand_count(const SvtHipTxtDesc &d, uint32_t n_cand_total) {
    if (d.first_cand >= n_cand_total)
        return 0;
    const uint32_t left = n_cand_total - d.first_cand, n = d.n_cand < SVT_HIP_TXT_MAX_CAND ? d.n_cand : SVT_HIP_TXT_MAX_CAND;
    return n < left ? n : left;
}

__device__ __forceinline__ int crop_of(uint32_t crop, uint32_t side) { return crop == 0 || crop > side ? (int)side : (int)crop; }

// {sum (src - recon)^2, sum (src - pred)^2} << 4 over cw x ch pixels, by the 64 lanes of a wavefront; lane 0 stores
template <class PIX>
__device__ __forceinline__ void spatial_pair(const uint8_t *base, const SvtHipTxfmDesc &d, uint64_t src_off, uint32_t src_stride, int cw, int ch, int lane,
                                             uint64_t *out) {
    uint64_t a = 0, b = 0;
    if (d.pred_off != SVT_HIP_NO_OFFSET && d.recon_off != SVT_HIP_NO_OFFSET) {
        const PIX *src = (const PIX *)(base + src_off), *pred = (const PIX *)(base + d.pred_off), *rec = (const PIX *)(base + d.recon_off);
        for (int i = lane; i < cw * ch; i += 64) {
            const int     r = i / cw, c = i - r * cw;
            const int32_t s = src[(size_t)r * src_stride + c];
            const int32_t er = s - (int32_t)rec[(size_t)r * d.recon_stride + c], ep = s - (int32_t)pred[(size_t)r * d.pred_stride + c];
            a += (uint64_t)((int64_t)er * er), b += (uint64_t)((int64_t)ep * ep);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64), b += __shfl_xor(b, off, 64);
    if (lane == 0)
        out[0] = a << 4, out[1] = b << 4;
}

// BY_BLOCK = false: a wavefront per candidate, its source from srcs[candidate].
// BY_BLOCK = true:  a wavefront per (block, k < 16); the candidates of blocks with SVT_HIP_TXT_SPATIAL_SSE, their source from the block.
template <bool BY_BLOCK>
__global__ __launch_bounds__(256) void spatial_distortion_kernel(const uint8_t *__restrict__ base, const SvtHipTxfmDesc *__restrict__ descs,
                                                                 const SvtHipSpatialSrc *__restrict__ srcs, const SvtHipTxtDesc *__restrict__ blocks,
                                                                 uint64_t (*__restrict__ out)[2], uint32_t n_items, uint32_t n_cand_total, uint32_t w,
                                                                 uint32_t h) {
    const uint32_t item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (item >= n_items)
        return;
    uint32_t cand = item, src_stride, crop_w, crop_h;
    uint64_t src_off;
    if (BY_BLOCK) {
        const SvtHipTxtDesc &b = blocks[item / SVT_HIP_TXT_MAX_CAND];
        const uint32_t       k = item % SVT_HIP_TXT_MAX_CAND;
        if (!(b.flags & SVT_HIP_TXT_SPATIAL_SSE) || k >= cand_count(b, n_cand_total))
            return;
        cand = b.first_cand + k, src_off = b.src_off, src_stride = b.src_stride, crop_w = b.crop_w, crop_h = b.crop_h;
    } else {
        const SvtHipSpatialSrc &s = srcs[item];
        src_off = s.src_off, src_stride = s.src_stride, crop_w = s.crop_w, crop_h = s.crop_h;
    }
    const SvtHipTxfmDesc &d = descs[cand];
    const int             cw = crop_of(crop_w, w), ch = crop_of(crop_h, h);
    if (d.flags & SVT_HIP_TX_PIXEL16)
        spatial_pair<uint16_t>(base, d, src_off, src_stride, cw, ch, (int)lane, out[cand]);
    else
        spatial_pair<uint8_t>(base, d, src_off, src_stride, cw, ch, (int)lane, out[cand]);
}

// The inverse-only pass of the search over the descriptors of its FIRST pass: every block is taken as quant_mode NONE / flags TX_INV
// (+ TX_PIXEL16 as given), so dqcoeff_off is read and recon_off written; a block that lacks one of dqcoeff_off, pred_off and recon_off is
// left out.  txfm_block (txfm_block.hpp) with the mapping of txfm_kernel (txfm.hip), which stays as it is.
template <int W, int H>
__global__ __launch_bounds__((txb::Geo<W, H>::NT * txb::Geo<W, H>::L), (txb::Geo<W, H>::MINW)) void inverse_only_kernel(uint8_t *__restrict__ base,
                                                                                              const SvtHipTxfmDesc *__restrict__ descs,
                                                                                              SvtHipTxfmResult *__restrict__ results, uint32_t n) {
    using G = txb::Geo<W, H>;
    constexpr int L = G::L, PW = G::PW, NT = G::NT;
    __shared__ int32_t buf[NT][H * PW];
    const int          t = threadIdx.x % L, slot = threadIdx.x / L;
    const uint32_t     i = blockIdx.x * NT + slot;
    const uint32_t     tb = i < n ? i : 0;
    SvtHipTxfmDesc     d = descs[tb];
    const bool         live = i < n && d.dqcoeff_off != SVT_HIP_NO_OFFSET && d.pred_off != SVT_HIP_NO_OFFSET && d.recon_off != SVT_HIP_NO_OFFSET;
    d.quant_mode = SVT_HIP_QUANT_NONE, d.flags = (uint8_t)((d.flags & SVT_HIP_TX_PIXEL16) | SVT_HIP_TX_INV);
    txb::txfm_block<W, H>(base, d, results + tb, live, t, buf[slot]);
}

bool launch_inverse_only(uint32_t w, uint32_t h, uint8_t *base, const SvtHipTxfmDesc *descs, SvtHipTxfmResult *res, uint32_t n, hipStream_t st) {
#define CASE(W, H)                                                                                                                                   \
    if (w == W && h == H) {                                                                                                                          \
        using G = txb::Geo<W, H>;                                                                                                                    \
        hipLaunchKernelGGL((inverse_only_kernel<W, H>), dim3((n + G::NT - 1) / G::NT), dim3(G::NT * G::L), 0, st, base, descs, res, n);              \
        return true;                                                                                                                                 \
    }
    CASE(4, 4) CASE(8, 8) CASE(16, 16) CASE(32, 32) CASE(64, 64) CASE(4, 8) CASE(8, 4) CASE(8, 16) CASE(16, 8) CASE(16, 32)
    CASE(32, 16) CASE(32, 64) CASE(64, 32) CASE(4, 16) CASE(16, 4) CASE(8, 32) CASE(32, 8) CASE(16, 64) CASE(64, 16)
#undef CASE
    return false;
}

// RDCOST (rd_cost.h:37) as the uint64_t the loop compares
__device__ __forceinline__ uint64_t rdcost(uint32_t lambda, uint64_t rate, uint64_t dist) {
    return (uint64_t)((((int64_t)rate * (int64_t)lambda + 256) >> 9) + (int64_t)dist * 128);
}

// The loop of tx_type_search (:4581-4812) over the candidates of block b, by one lane.  Writes out[b]; returns the winner's index into the
// per-candidate arrays, or kNoCand.
__device__ uint32_t replay(const SvtHipTxtDesc &b, const SvtHipTxbCostDesc *__restrict__ cdescs, const SvtHipRateTables *__restrict__ tables,
                           const SvtHipTxfmResult *__restrict__ results, const SvtHipRdoqResult *__restrict__ rdoq,
                           const uint64_t (*__restrict__ dist)[2], const SvtHipTxbCost *__restrict__ cost, SvtHipTxtResult *__restrict__ out,
                           const TxtLaunch &prm) {
    const uint32_t n = cand_count(b, prm.n_cand_total), lambda = b.full_lambda;
    uint64_t       best_cost = ~(uint64_t)0, dct_cost = ~(uint64_t)0;
    int32_t        best_satd = INT32_MAX;
    uint32_t       best_non_coeff = 64 * 64, winner = kNoCand;
    SvtHipTxtResult r;
    r.bits = 0, r.distortion[0] = r.distortion[1] = 0, r.eob = 0, r.quant_mask = r.cost_mask = 0, r.tx_type = 0 /* DCT_DCT */, r.cand = 0xFF, r.cul_level = 0;
    for (int k = 0; k < 7; k++) r.pad_[k] = 0;
    const bool     early = (b.flags & SVT_HIP_TXT_EARLY_EXIT) != 0, spatial = prm.recon && (b.flags & SVT_HIP_TXT_SPATIAL_SSE) != 0;
    const uint64_t cost_th = b.early_exit_dist_th ? rdcost(lambda, 1, (uint64_t)(uint32_t)(b.tx_pixels * b.early_exit_dist_th)) : 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t           i = b.first_cand + k;
        const SvtHipTxbCostDesc &cd = cdescs[i];
        const int                tx_type = cd.tx_type & 15;
        if ((b.group_start >> k) & 1)
            best_non_coeff = 64 * 64;
        if (tx_type != 0 && b.txt_rate_cost_th) {
            const uint32_t ti = cd.table < prm.n_tables ? cd.table : prm.n_tables - 1;
            const int      rate = tx_type_rate(tables[ti], cd, prm.sqr, prm.sqr_up);
            if (rdcost(lambda, (uint64_t)(int64_t)rate, 0) * 1000 > dct_cost * b.txt_rate_cost_th)
                continue;
        }
        const SvtHipTxfmResult res = results[i];
        if (b.satd_early_exit_th) {
            const int32_t satd = (int32_t)res.satd;
            if (satd < best_satd)
                best_satd = satd;
            else if ((int32_t)((uint32_t)(satd - best_satd) * 100u) > (int32_t)((uint32_t)best_satd * (uint32_t)b.satd_early_exit_th))
                continue;
        }
        r.quant_mask |= (uint16_t)(1u << k);
        const uint32_t eob = res.eob;
        if (eob == 0 && tx_type != 0)
            continue;
        uint64_t dr = dist[i][0], dp = dist[i][1];
        if (!spatial) {
            const int step = cd.subres_step < 2 ? cd.subres_step : 2;  // mds_subres_step is 0 .. 2
            dr += res.three_quad_energy, dp += res.three_quad_energy;
            dr = (prm.dist_shift < 0 ? dr << -prm.dist_shift : dr >> prm.dist_shift) << step;
            dp = (prm.dist_shift < 0 ? dp << -prm.dist_shift : dp >> prm.dist_shift) << step;
        }
        if (rdcost(lambda, 0, dr) > best_cost)
            continue;
        r.cost_mask |= (uint16_t)(1u << k);
        const uint64_t bits = cost[i].bits, c = rdcost(lambda, bits, dr);
        if (c < best_cost) {
            best_cost = c, best_non_coeff = eob, winner = i;
            r.bits = bits, r.distortion[0] = dr, r.distortion[1] = dp, r.eob = (uint16_t)eob, r.tx_type = (uint8_t)tx_type, r.cand = (uint8_t)k;
            r.cul_level = rdoq ? rdoq[i].cul_level : 0;
            if (tx_type == 0)
                dct_cost = c;
        }
        if (early && (best_non_coeff < b.early_exit_coeff_th || best_cost < cost_th))
            break;
    }
    r.cost = best_cost;
    *out = r;
    return winner;
}

// copy_txt_data for one block, by the 64 lanes of a wavefront: the winner's qcoeff, dqcoeff and reconstruction to the block's destinations
__device__ __forceinline__ void gather(uint8_t *base, const SvtHipTxtDesc &b, const SvtHipTxfmDesc &wd, const TxtLaunch &prm, int lane) {
    if (b.dst_qcoeff_off != SVT_HIP_NO_OFFSET && wd.qcoeff_off != SVT_HIP_NO_OFFSET && b.dst_qcoeff_off != wd.qcoeff_off) {
        const int32_t *s = (const int32_t *)(base + wd.qcoeff_off);
        int32_t       *d = (int32_t *)(base + b.dst_qcoeff_off);
        for (uint32_t i = lane; i < prm.retained; i += 64) d[i] = s[i];
    }
    if (b.dst_dqcoeff_off != SVT_HIP_NO_OFFSET && wd.dqcoeff_off != SVT_HIP_NO_OFFSET && b.dst_dqcoeff_off != wd.dqcoeff_off) {
        const int32_t *s = (const int32_t *)(base + wd.dqcoeff_off);
        int32_t       *d = (int32_t *)(base + b.dst_dqcoeff_off);
        for (uint32_t i = lane; i < prm.retained; i += 64) d[i] = s[i];
    }
    if (prm.recon && b.dst_recon_off != SVT_HIP_NO_OFFSET && wd.recon_off != SVT_HIP_NO_OFFSET && b.dst_recon_off != wd.recon_off) {
        const uint32_t pixels = prm.w * prm.h;
        if (wd.flags & SVT_HIP_TX_PIXEL16) {
            const uint16_t *s = (const uint16_t *)(base + wd.recon_off);
            uint16_t       *d = (uint16_t *)(base + b.dst_recon_off);
            for (uint32_t i = lane; i < pixels; i += 64) d[(size_t)(i / prm.w) * b.dst_recon_stride + i % prm.w] = s[(size_t)(i / prm.w) * wd.recon_stride + i % prm.w];
        } else {
            const uint8_t *s = base + wd.recon_off;
            uint8_t       *d = base + b.dst_recon_off;
            for (uint32_t i = lane; i < pixels; i += 64) d[(size_t)(i / prm.w) * b.dst_recon_stride + i % prm.w] = s[(size_t)(i / prm.w) * wd.recon_stride + i % prm.w];
        }
    }
}

// mapping 0: replay and copies in one kernel; a workgroup is one wavefront and walks the batch in steps of 64 blocks
__global__ __launch_bounds__(64) void select_gather_kernel(uint8_t *base, const SvtHipTxtDesc *__restrict__ blocks, const SvtHipTxfmDesc *__restrict__ tdescs,
                                                           const SvtHipTxbCostDesc *__restrict__ cdescs, const SvtHipRateTables *__restrict__ tables,
                                                           const SvtHipTxfmResult *__restrict__ results, const SvtHipRdoqResult *__restrict__ rdoq,
                                                           const uint64_t (*__restrict__ dist)[2], const SvtHipTxbCost *__restrict__ cost,
                                                           SvtHipTxtResult *__restrict__ out, TxtLaunch prm) {
    __shared__ uint32_t winner[64];
    for (uint32_t b0 = blockIdx.x * 64; b0 < prm.n_blocks; b0 += gridDim.x * 64) {
        const uint32_t b = b0 + threadIdx.x;
        __syncthreads();  // the winners of the previous step have been read
        winner[threadIdx.x] = b < prm.n_blocks ? replay(blocks[b], cdescs, tables, results, rdoq, dist, cost, out + b, prm) : kNoCand;
        __syncthreads();
        const uint32_t here = prm.n_blocks - b0 < 64 ? prm.n_blocks - b0 : 64;
        for (uint32_t j = 0; j < here; j++) {
            const uint32_t wi = winner[j];
            if (wi != kNoCand)
                gather(base, blocks[b0 + j], tdescs[wi], prm, (int)threadIdx.x);
        }
    }
}

// mapping 1: the replay alone, a lane per block
__global__ __launch_bounds__(256) void select_kernel(const SvtHipTxtDesc *__restrict__ blocks, const SvtHipTxbCostDesc *__restrict__ cdescs,
                                                     const SvtHipRateTables *__restrict__ tables, const SvtHipTxfmResult *__restrict__ results,
                                                     const SvtHipRdoqResult *__restrict__ rdoq, const uint64_t (*__restrict__ dist)[2],
                                                     const SvtHipTxbCost *__restrict__ cost, SvtHipTxtResult *__restrict__ out, TxtLaunch prm) {
    for (uint32_t b = blockIdx.x * 256 + threadIdx.x; b < prm.n_blocks; b += gridDim.x * 256)
        replay(blocks[b], cdescs, tables, results, rdoq, dist, cost, out + b, prm);
}

// mapping 1: the copies, a wavefront per block; the winner is the one the replay left in out[b]
__global__ __launch_bounds__(256) void gather_kernel(uint8_t *base, const SvtHipTxtDesc *__restrict__ blocks, const SvtHipTxfmDesc *__restrict__ tdescs,
                                                     const SvtHipTxtResult *__restrict__ out, TxtLaunch prm) {
    for (uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6); b < prm.n_blocks; b += gridDim.x * 4) {
        const uint32_t k = out[b].cand;
        if (k < cand_count(blocks[b], prm.n_cand_total))
            gather(base, blocks[b], tdescs[blocks[b].first_cand + k], prm, (int)(threadIdx.x & 63));
    }
}

constexpr size_t   align_up(size_t v) { return (v + 255) & ~(size_t)255; }
// svt_hip_txt_select_batch: the faster split of profiles/txt_search_4k.json by retained coefficients.  With 16 of them a block's copies are
// two wave-wide stores, and one kernel is ahead by 14 %; from 32 on the wavefront per block wins, by 9 % at 4 x 8 up to 13 x at 32 x 32,
// where one wavefront copying 64 blocks in turn leaves most of the device idle.
constexpr uint32_t mapping_for(uint32_t retained) { return retained <= 16 ? 0 : 1; }

// the per-candidate records of svt_hip_txt_search_batch in its scratch, each 256-byte aligned
struct SearchScratch {
    size_t result_a, result_b, rdoq, dist, cost, bytes;
    constexpr explicit SearchScratch(uint32_t n_cand)
        : result_a(0), result_b(result_a + align_up((size_t)n_cand * sizeof(SvtHipTxfmResult))),
          rdoq(result_b + align_up((size_t)n_cand * sizeof(SvtHipTxfmResult))), dist(rdoq + align_up((size_t)n_cand * sizeof(SvtHipRdoqResult))),
          cost(dist + align_up((size_t)n_cand * 16)), bytes(cost + align_up((size_t)n_cand * sizeof(SvtHipTxbCost))) {}
};

}  // namespace

extern "C" int32_t svt_hip_txfm_spatial_distortion_batch(const uint8_t *d_base, const SvtHipTxfmDesc *d_desc, const SvtHipSpatialSrc *d_src,
                                                         uint64_t (*d_distortion)[2], uint32_t n_blocks, uint32_t w, uint32_t h, void *stream) {
    const TxbGeometry g(w, h);
    if (!g.valid || (n_blocks > 0 && (!d_base || !d_desc || !d_src || !d_distortion)))
        return refuse("svt_hip_txfm_spatial_distortion_batch: bad argument (%u x %u, %u blocks)", w, h, n_blocks);
    if (n_blocks == 0)
        return SVT_HIP_OK;
    TierBCall c("svt_hip_txfm_spatial_distortion_batch", stream);
    if (!c.ok())
        return c.status();
    hipLaunchKernelGGL(spatial_distortion_kernel<false>, dim3((n_blocks + 3) / 4), dim3(256), 0, c.stream(), d_base, d_desc, d_src,
                       (const SvtHipTxtDesc *)nullptr, d_distortion, n_blocks, n_blocks, w, h);
    return c.finish();
}

namespace {
// svt_hip_txt_select_batch[_mapped]; recon = false is the call of a search that ran no inverse-only pass (TxtLaunch::recon)
int32_t select_batch(uint8_t *d_base, const SvtHipTxtDesc *d_desc, const SvtHipTxfmDesc *d_txfm_desc, const SvtHipTxbCostDesc *d_cost_desc,
                     const SvtHipRateTables *d_tables, uint32_t n_tables, const SvtHipTxfmResult *d_txfm_result, const SvtHipRdoqResult *d_rdoq_result,
                     const uint64_t (*d_distortion)[2], const SvtHipTxbCost *d_cost, SvtHipTxtResult *d_out, uint32_t n_cand_total, uint32_t n_blocks,
                     uint32_t w, uint32_t h, uint32_t mapping, bool recon, void *stream) {
    const TxbGeometry g(w, h);
    if (!g.valid || mapping > 1 || n_tables == 0 ||
        (n_blocks > 0 && (!d_base || !d_desc || !d_txfm_desc || !d_cost_desc || !d_tables || !d_txfm_result || !d_distortion || !d_cost || !d_out)))
        return refuse("svt_hip_txt_select_batch: bad argument (%u x %u, %u table sets, %u blocks, mapping %u)", w, h, n_tables, n_blocks, mapping);
    if (n_blocks == 0)
        return SVT_HIP_OK;
    TierBCall c("svt_hip_txt_select_batch", stream);
    if (!c.ok())
        return c.status();
    const TxtLaunch   prm{g.sqr, g.sqr_up, (1 - g.tx_scale) * 2, g.retained, w, h, n_tables, n_cand_total, n_blocks, recon ? 1u : 0u};
    const hipStream_t st = c.stream();
    const uint32_t    cap = (uint32_t)cu_count() * 16;
    if (mapping == 0) {
        hipLaunchKernelGGL(select_gather_kernel, dim3(grid_blocks(n_blocks, 64, cap)), dim3(64), 0, st, d_base, d_desc, d_txfm_desc, d_cost_desc, d_tables,
                           d_txfm_result, d_rdoq_result, d_distortion, d_cost, d_out, prm);
    } else {
        hipLaunchKernelGGL(select_kernel, dim3(grid_blocks(n_blocks, 256, cap)), dim3(256), 0, st, d_desc, d_cost_desc, d_tables, d_txfm_result,
                           d_rdoq_result, d_distortion, d_cost, d_out, prm);
        hipLaunchKernelGGL(gather_kernel, dim3(grid_blocks(n_blocks, 4, cap)), dim3(256), 0, st, d_base, d_desc, d_txfm_desc,
                           (const SvtHipTxtResult *)d_out, prm);
    }
    return c.finish();
}
}  // namespace

extern "C" int32_t svt_hip_txt_select_batch_mapped(uint8_t *d_base, const SvtHipTxtDesc *d_desc, const SvtHipTxfmDesc *d_txfm_desc,
                                                   const SvtHipTxbCostDesc *d_cost_desc, const SvtHipRateTables *d_tables, uint32_t n_tables,
                                                   const SvtHipTxfmResult *d_txfm_result, const SvtHipRdoqResult *d_rdoq_result,
                                                   const uint64_t (*d_distortion)[2], const SvtHipTxbCost *d_cost, SvtHipTxtResult *d_out,
                                                   uint32_t n_cand_total, uint32_t n_blocks, uint32_t w, uint32_t h, uint32_t mapping, void *stream) {
    return select_batch(d_base, d_desc, d_txfm_desc, d_cost_desc, d_tables, n_tables, d_txfm_result, d_rdoq_result, d_distortion, d_cost, d_out,
                        n_cand_total, n_blocks, w, h, mapping, true, stream);
}

extern "C" int32_t svt_hip_txt_select_batch(uint8_t *d_base, const SvtHipTxtDesc *d_desc, const SvtHipTxfmDesc *d_txfm_desc,
                                            const SvtHipTxbCostDesc *d_cost_desc, const SvtHipRateTables *d_tables, uint32_t n_tables,
                                            const SvtHipTxfmResult *d_txfm_result, const SvtHipRdoqResult *d_rdoq_result,
                                            const uint64_t (*d_distortion)[2], const SvtHipTxbCost *d_cost, SvtHipTxtResult *d_out,
                                            uint32_t n_cand_total, uint32_t n_blocks, uint32_t w, uint32_t h, void *stream) {
    return select_batch(d_base, d_desc, d_txfm_desc, d_cost_desc, d_tables, n_tables, d_txfm_result, d_rdoq_result, d_distortion, d_cost, d_out,
                        n_cand_total, n_blocks, w, h, mapping_for(TxbGeometry(w, h).retained), true, stream);
}

extern "C" size_t svt_hip_txt_search_scratch_bytes(uint32_t n_cand, uint32_t n_blocks) {
    (void)n_blocks;  // every record in the scratch is per candidate; the per-block records are the caller's d_out
    return SearchScratch(n_cand).bytes;
}

extern "C" int32_t svt_hip_txt_search_batch(uint8_t *d_base, const SvtHipTxfmDesc *d_txfm_desc, const SvtHipRdoqDesc *d_rdoq_desc,
                                            const SvtHipTxbCostDesc *d_cost_desc, const SvtHipRateTables *d_tables, uint32_t n_tables,
                                            const SvtHipTxtDesc *d_desc, void *d_scratch, size_t scratch_bytes, SvtHipTxtResult *d_out,
                                            uint32_t n_cand, uint32_t n_blocks, uint32_t w, uint32_t h, uint32_t flags, void *stream) {
    const TxbGeometry g(w, h);
    const SearchScratch s(n_cand);
    if (!g.valid || n_tables == 0 ||
        (n_blocks > 0 && (!d_base || !d_txfm_desc || !d_cost_desc || !d_tables || !d_desc || !d_scratch || !d_out || scratch_bytes < s.bytes)))
        return refuse("svt_hip_txt_search_batch: bad argument (%u x %u, %u table sets, %u candidates of %u blocks, %zu bytes of scratch where %zu are needed)",
                      w, h, n_tables, n_cand, n_blocks, scratch_bytes, s.bytes);
    if (n_blocks == 0)
        return SVT_HIP_OK;
    TierBCall c("svt_hip_txt_search_batch", stream);
    if (!c.ok())
        return c.status();
    uint8_t *const          scratch = (uint8_t *)d_scratch;
    SvtHipTxfmResult *const result_a = (SvtHipTxfmResult *)(scratch + s.result_a), *const result_b = (SvtHipTxfmResult *)(scratch + s.result_b);
    SvtHipRdoqResult *const rdoq = d_rdoq_desc ? (SvtHipRdoqResult *)(scratch + s.rdoq) : nullptr;
    uint64_t(*const dist)[2] = (uint64_t(*)[2])(scratch + s.dist);
    SvtHipTxbCost *const cost = (SvtHipTxbCost *)(scratch + s.cost);
    const hipStream_t    st = c.stream();
    int32_t              rc = SVT_HIP_OK;
    if (n_cand > 0) {
        if ((rc = svt_hip_txfm_quant_batch(d_base, d_txfm_desc, result_a, n_cand, w, h, st)) != SVT_HIP_OK)
            return rc;
        if (rdoq && (rc = svt_hip_rdoq_batch(d_base, d_txfm_desc, d_rdoq_desc, d_tables, n_tables, result_a, rdoq, n_cand, w, h, st)) != SVT_HIP_OK)
            return rc;
        if (flags & SVT_HIP_TXT_SEARCH_INVERSE) {
            if ((rc = txfm_ready()) != SVT_HIP_OK)
                return rc;
            if (!launch_inverse_only(w, h, d_base, d_txfm_desc, result_b, n_cand, st)) {
                set_error("svt_hip_txt_search_batch: no inverse kernel for %u x %u", w, h);
                return SVT_HIP_ERR_RUNTIME;
            }
        }
        if ((rc = svt_hip_txfm_distortion_batch(d_base, d_txfm_desc, dist, n_cand, w, h, st)) != SVT_HIP_OK)
            return rc;
        if (flags & SVT_HIP_TXT_SEARCH_INVERSE) {
            const uint32_t items = n_blocks * SVT_HIP_TXT_MAX_CAND;
            hipLaunchKernelGGL(spatial_distortion_kernel<true>, dim3((items + 3) / 4), dim3(256), 0, st, (const uint8_t *)d_base, d_txfm_desc,
                               (const SvtHipSpatialSrc *)nullptr, d_desc, dist, items, n_cand, w, h);
        }
        if ((rc = svt_hip_txb_cost_batch(d_base, d_cost_desc, d_tables, n_tables, result_a, dist, cost, n_cand, w, h, st)) != SVT_HIP_OK)
            return rc;
    }
    rc = select_batch(d_base, d_desc, d_txfm_desc, d_cost_desc, d_tables, n_tables, result_a, rdoq, dist, cost, d_out, n_cand, n_blocks, w, h,
                      mapping_for(g.retained), (flags & SVT_HIP_TXT_SEARCH_INVERSE) != 0, st);
    return rc == SVT_HIP_OK ? c.finish() : rc;
}

SVT_HIP_MODULE_WARMUP(txfm_txt)
