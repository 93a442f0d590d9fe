// txfm_rdoq.hip — the RDOQ stage of the quantiser on device-resident quantiser output (Tier B only): svt_aom_quantize_inv_quantize
// (reference: full_loop.c:1562-1685) from the point after its first quantiser, with svt_fast_optimize_b, svt_av1_optimize_b
// (:1124-1331) and svt_av1_compute_cul_level_c (:1444-1460).  Integer arithmetic only, widths as in the reference.
//
// Work split: as txfm_rate.hip a block of n = min(w,32) * min(h,32) retained coefficients belongs to a group of min(n, 64) lanes,
// so 16-, 32- and 64-coefficient blocks sit 4, 2 and 1 to a wavefront; a workgroup is ONE wavefront (its barriers cost nothing)
// and walks the batch in steps of its 64 / group blocks.  The group does what is a pure function of a position together: the
// re-quantisation (quant_one of txfm_block.hpp), update_coeff_eob_fast (the new eob is a maximum over positions), the levels and
// the scan (from iscan) into LDS, and the cul_level sum.  The head of the trellis (last coefficient, update_coeff_eob while at most
// four non-zeros survive, update_skip) carries accu_rate / accu_dist and is walked by the group's first lane in scan order; it
// reads zero / non-zero and every context from the LDS levels and touches global memory only at non-zero positions.  Behind it
// accu_rate is dead: update_coeff_simple decides a position from its own values and the FINAL levels of neighbours that all lie
// on later anti-diagonals and later in scan order (tests/test_rdoq_abi.py::test_neighbours_follow_in_scan_order), so
//   ROUNDS = false  the first lane goes on in scan order,
//   ROUNDS = true   the group takes one anti-diagonal per round, last first, a lane per position, a barrier between rounds,
// and both leave the same arrays.  The baseline these two are measured against is LANE = true: the group is ONE lane, 64 blocks to
// a wavefront, every phase of a block by its lane; no lane idles during the heads, but the per-position phases run n times per
// lane and its loads no longer coalesce.  Its levels and scans, 64 of each, fit the 64 KB of a workgroup's LDS up to 128 retained
// coefficients (8 x 16: 41 KB with the tables; 16 x 16 would need 68 KB), so it exists for those sizes only.
// svt_hip_rdoq_batch launches the fastest of each size (profiles/rdoq_4k.json), svt_hip_rdoq_batch_mapped any.  nz_ci lives in LDS: indexed dynamically in registers it would go to scratch.  The two SvtHipCoeffCost planes of the workgroup's first table set are staged
// in LDS as in txb_cost_kernel; a block of another set reads its own through the cache.
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

// what the kernel reads of the launch; all but the counts are TxbGeometry's
struct RdoqLaunch {
    int32_t  orient, txs_ctx, tx_scale;
    int32_t  sqrt_px;  // sqrt_retained
    uint32_t pixels, n_tables, n_blocks;
};

// the walk of svt_av1_optimize_b over one block, by one lane
template <int IW, int IH>
struct Trellis {
    static constexpr int BWL = ilog2(IW), STRIDE = Levels<IW, IH>::STRIDE, N = IW * IH;
    const SvtHipCoeffCost *cc;
    const int32_t (*eob_bits)[11];
    uint8_t       *levels;  // LDS, padded
    const int16_t *scan;    // LDS
    int16_t       *nz_ci;   // LDS, 5 entries
    const int32_t *tc;
    int32_t       *qc, *dqc;
    const uint8_t *iqm;
    int32_t        dq[2];
    int            shift, cls, orient, sign_ctx, sharpness;
    int64_t        rdmult;

    __device__ __forceinline__ int64_t rdcost(int rate, int64_t dist) const { return (((int64_t)rate * rdmult + 256) >> 9) + dist * 128; }
    __device__ __forceinline__ int64_t dist(int32_t t, int32_t d) const {
        const int64_t diff = ((int64_t)t - d) * ((int64_t)1 << shift);
        return diff * diff;
    }
    __device__ __forceinline__ int dqv(int ci) const {
        const int v = dq[ci != 0];
        return iqm ? (iqm[ci] * v + 16) >> 5 : v;
    }
    __device__ __forceinline__ uint8_t *lv(int ci) const { return levels + (ci >> BWL) * STRIDE + (ci & (IW - 1)); }
    __device__ __forceinline__ int      lower_ctx(int ci) const { return nz_ctx_of<IW>(lv(ci), ci, ci >> BWL, ci & (IW - 1), cls, orient); }
    __device__ __forceinline__ int      br_ctx(int ci) const { return br_ctx_of<IW>(lv(ci), ci, ci >> BWL, ci & (IW - 1), cls); }
    __device__ __forceinline__ int      eob_ctx(int si) const { return si == 0 ? 0 : eob_ctx_of<N>(si); }
    // get_br_ctx_eob
    __device__ __forceinline__ int br_ctx_eob(int ci) const {
        if (ci == 0)
            return 0;
        const int row = ci >> BWL, col = ci & (IW - 1);
        return (cls == 0 ? (row < 2 && col < 2) : cls == 1 ? col == 0 : row == 0) ? 7 : 14;
    }
    // get_coeff_cost_general; abs_qc >= 1 where is_last
    __device__ __forceinline__ int cost_general(bool is_last, int ci, int abs_qc, int sign, int ctx) const {
        int cost = is_last ? cc->base_eob[ctx][min3(abs_qc) - 1] : cc->base[ctx][min3(abs_qc)];
        if (abs_qc != 0) {
            cost += ci == 0 ? cc->dc_sign[sign_ctx][sign] : 512;
            if (abs_qc > 2)
                cost += range_cost(*cc, is_last ? br_ctx_eob(ci) : br_ctx(ci), abs_qc);
        }
        return cost;
    }
    // get_coeff_cost_eob; abs_qc >= 1
    __device__ __forceinline__ int cost_eob(int ci, int abs_qc, int sign, int ctx) const {
        int cost = cc->base_eob[ctx][min3(abs_qc) - 1] + (ci == 0 ? cc->dc_sign[sign_ctx][sign] : 512);
        if (abs_qc > 2)
            cost += range_cost(*cc, br_ctx_eob(ci), abs_qc);
        return cost;
    }
    // get_two_coeff_cost_simple with get_br_cost_with_diff; abs_qc >= 1
    __device__ __forceinline__ int two_cost_simple(int ci, int abs_qc, int ctx, int &cost_low) const {
        int cost = cc->base[ctx][min3(abs_qc)] + 512;
        int diff = abs_qc <= 3 ? cc->base[ctx][abs_qc + 4] : 0;
        if (abs_qc > 2) {
            const int32_t *lps = cc->lps[br_ctx(ci)];
            const int      base_range = abs_qc - 3 < 12 ? abs_qc - 3 : 12;
            int            golomb_bits = 0;
            if (abs_qc <= 15)
                diff += lps[base_range + 13];
            if (abs_qc >= 15) {
                const int r = abs_qc - 14;
                // golomb_bits_cost[r] is get_golomb_cost and golomb_cost_diff[r] is 1024 at the powers of two from 2, 512 at r = 1
                golomb_bits = golomb_cost(abs_qc);
                diff += r == 1 ? 512 : (r & (r - 1)) == 0 ? 1024 : 0;
            }
            cost += lps[base_range] + golomb_bits;
        }
        cost_low = cost - diff;
        return cost;
    }
    __device__ __forceinline__ void set_low(int ci, int abs_low, int32_t q_low, int32_t dq_low) const {
        qc[ci] = q_low, dqc[ci] = dq_low;
        *lv(ci) = (uint8_t)(abs_low < 127 ? abs_low : 127);
    }

    // update_coeff_general
    __device__ void update_general(int &accu_rate, int64_t &accu_dist, int si, int eob) const {
        const int     ci = scan[si];
        const int32_t q = qc[ci];
        const bool    is_last = si == eob - 1;
        const int     ctx = is_last ? eob_ctx(si) : lower_ctx(ci);
        if (q == 0) {
            accu_rate += cc->base[ctx][0];
            return;
        }
        const int     sign = q < 0, abs_qc = q < 0 ? -q : q;
        const int32_t t = tc[ci], d = dqc[ci];
        const int64_t dist_ = dist(t, d), dist0 = dist(t, 0);
        const int     rate = cost_general(is_last, ci, abs_qc, sign, ctx);
        const int64_t rd = rdcost(rate, dist_);
        int32_t       q_low = 0, dq_low = 0;
        int           abs_low = 0, rate_low;
        int64_t       dist_low;
        if (abs_qc == 1) {
            dist_low = dist0;
            rate_low = cc->base[ctx][0];
        } else {
            abs_low = abs_qc - 1;
            const int32_t adq = txd::mul32(abs_low, dqv(ci)) >> shift;
            q_low = sign ? -abs_low : abs_low, dq_low = sign ? -adq : adq;
            dist_low = dist(t, dq_low);
            rate_low = cost_general(is_last, ci, abs_low, sign, ctx);
        }
        if (rdcost(rate_low, dist_low) < rd) {
            set_low(ci, abs_low, q_low, dq_low);
            accu_rate += rate_low, accu_dist += dist_low - dist0;
        } else {
            accu_rate += rate, accu_dist += dist_ - dist0;
        }
    }

    // update_coeff_eob
    __device__ void update_eob(int &accu_rate, int64_t &accu_dist, int &eob, int &nz_num, int si) const {
        const int     ci = scan[si];
        const int     ctx = lower_ctx(ci);
        if (*lv(ci) == 0) {
            accu_rate += cc->base[ctx][0];
            return;
        }
        const int32_t q = qc[ci], t = tc[ci], d = dqc[ci];
        const int     sign = q < 0, abs_qc = q < 0 ? -q : q;
        const int64_t dist0 = dist(t, 0);
        int64_t       dist_ = dist(t, d) - dist0;
        int           rate = cost_general(false, ci, abs_qc, sign, ctx);
        int64_t       rd = rdcost(accu_rate + rate, accu_dist + dist_);
        int32_t       q_low = 0, dq_low = 0;
        int           abs_low = 0, rate_low;
        int64_t       dist_low, rd_low;
        if (abs_qc == 1) {
            dist_low = 0;
            rate_low = cc->base[ctx][0];
            rd_low   = rdcost(accu_rate + rate_low, accu_dist);
        } else {
            abs_low = abs_qc - 1;
            const int32_t adq = txd::mul32(abs_low, dqv(ci)) >> shift;
            q_low = sign ? -abs_low : abs_low, dq_low = sign ? -adq : adq;
            dist_low = dist(t, dq_low) - dist0;
            rate_low = cost_general(false, ci, abs_low, sign, ctx);
            rd_low   = rdcost(accu_rate + rate_low, accu_dist + dist_low);
        }
        bool          lower_new_eob = false;
        const int     new_eob = si + 1, ctx_new = eob_ctx(si);
        const int     new_eob_cost = eob_cost(new_eob, eob_bits, cc->eob_extra, cls);
        int           rate_new = new_eob_cost + cost_eob(ci, abs_qc, sign, ctx_new);
        int64_t       dist_new = dist_, rd_new = rdcost(rate_new, dist_new);
        if (abs_low > 0) {
            const int     rate_new_low = new_eob_cost + cost_eob(ci, abs_low, sign, ctx_new);
            const int64_t rd_new_low = rdcost(rate_new_low, dist_low);
            if (rd_new_low < rd_new)
                lower_new_eob = true, rd_new = rd_new_low, rate_new = rate_new_low, dist_new = dist_low;
        }
        bool lower = false;
        if (rd_low < rd)
            lower = true, rd = rd_low, rate = rate_low, dist_ = dist_low;
        if (sharpness == 0 && rd_new < rd) {
            for (int ni = 0; ni < nz_num; ni++) {
                const int last = nz_ci[ni];
                *lv(last) = 0, qc[last] = 0, dqc[last] = 0;
            }
            eob = new_eob, nz_num = 0, accu_rate = rate_new, accu_dist = dist_new, lower = lower_new_eob;
        } else {
            accu_rate += rate, accu_dist += dist_;
        }
        if (lower)
            set_low(ci, abs_low, q_low, dq_low);
        if (!lower || abs_low != 0)
            nz_ci[nz_num++] = (int16_t)ci;
    }

    // update_coeff_simple; accu_rate is dead here
    __device__ void update_simple(int ci) const {
        if (*lv(ci) == 0)
            return;
        const int32_t q = qc[ci], t = tc[ci], d = dqc[ci];
        const int32_t abs_qc = q < 0 ? -q : q, abs_t = t < 0 ? -t : t, abs_d = d < 0 ? -d : d;
        if (abs_d < abs_t)
            return;
        int           rate_low;
        const int     rate = two_cost_simple(ci, abs_qc, lower_ctx(ci), rate_low);
        const int64_t rd = rdcost(rate, dist(abs_t, abs_d));
        const int32_t abs_low = abs_qc - 1, abs_d_low = txd::mul32(abs_low, dqv(ci)) >> shift;
        if (rdcost(rate_low, dist(abs_t, abs_d_low)) < rd)
            set_low(ci, abs_low, q < 0 ? -abs_low : abs_low, q < 0 ? -abs_d_low : abs_d_low);
    }

    // svt_av1_optimize_b from `int accu_rate = eob_cost` up to update_skip: the part that carries accu_rate / accu_dist; eob >= 1 and
    // qc[scan[eob - 1]] != 0.  Returns the new eob; si: the scan index update_coeff_simple starts at (-1: nothing is left, 0: DC only).
    __device__ int head(int eob, int eob_cost_, bool fast_mode, int skip_cost, int non_skip_cost, bool &skipped, int &si) const {
        int       accu_rate = eob_cost_;
        int64_t   accu_dist = 0;
        int       nz_num = 1;
        si = eob - 1;
        const int ci = scan[si];
        nz_ci[0] = (int16_t)ci;
        const int32_t q = qc[ci];
        if (q >= 2 || q <= -2) {
            update_general(accu_rate, accu_dist, si, eob);
        } else {
            accu_rate += cost_eob(ci, 1, q < 0, eob_ctx(si));
            const int32_t t = tc[ci];
            accu_dist += dist(t, dqc[ci]) - dist(t, 0);
        }
        --si;
        for (; si >= 0 && nz_num <= 4 && !fast_mode; --si) update_eob(accu_rate, accu_dist, eob, nz_num, si);
        if (si == -1 && nz_num <= 4) {  // update_skip
            if (sharpness == 0 && rdcost(skip_cost, 0) < rdcost(accu_rate + non_skip_cost, accu_dist)) {
                for (int i = 0; i < nz_num; i++) {
                    const int z = nz_ci[i];
                    qc[z] = 0, dqc[z] = 0;
                }
                eob = 0, skipped = true;
            }
        }
        return eob;
    }
    // the DC position behind update_coeff_simple; its accu_rate and accu_dist are dead
    __device__ void dc(int eob) const {
        int     rate = 0;
        int64_t dummy = 0;
        update_general(rate, dummy, 0, eob);
    }
};

template <int G>
__device__ __forceinline__ int group_max_i(int v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

template <int IW, int IH, bool ROUNDS, bool LANE>
__global__ __launch_bounds__(64) void rdoq_kernel(uint8_t *base, const SvtHipTxfmDesc *__restrict__ tdescs, const SvtHipRdoqDesc *__restrict__ descs,
                                                  const SvtHipRateTables *__restrict__ tables, SvtHipTxfmResult *results, SvtHipRdoqResult *out,
                                                  RdoqLaunch prm) {
    constexpr int N = IW * IH, G = LANE ? 1 : group_lanes(N), BLOCKS = 64 / G, PER = N / G;
    constexpr int ROW_WORDS = Levels<IW, IH>::ROW_WORDS, LEVEL_WORDS = Levels<IW, IH>::WORDS;
    __shared__ uint32_t lv[BLOCKS][LEVEL_WORDS];
    __shared__ int16_t  scan_lds[BLOCKS][N];
    __shared__ int16_t  nz_lds[BLOCKS][8];
    __shared__ int32_t  walked[BLOCKS][3];  // eob, path bits and where update_coeff_simple starts, left by the walking lane for its group
    __shared__ int32_t  staged_words[TABLE_WORDS];
    const SvtHipCoeffCost *staged = (const SvtHipCoeffCost *)staged_words;
    const int gi = threadIdx.x / G, li = threadIdx.x % G;
    uint32_t  first_table = descs[blockIdx.x * BLOCKS].table;  // the grid never exceeds the batch
    first_table = first_table < prm.n_tables ? first_table : prm.n_tables - 1;
    {
        const int32_t *src = (const int32_t *)&tables[first_table].coeff[prm.txs_ctx][0];
        for (int i = threadIdx.x; i < TABLE_WORDS; i += 64) staged_words[i] = src[i];
        for (int i = li; i < N; i += G) scan_lds[gi][i] = 0;  // every entry is a position of the block from here on
    }
    for (uint32_t b0 = blockIdx.x * BLOCKS; b0 < prm.n_blocks; b0 += gridDim.x * BLOCKS) {
        const uint32_t tb = b0 + gi;
        const bool     active = tb < prm.n_blocks;
        const uint32_t bi = active ? tb : prm.n_blocks - 1;
        const SvtHipTxfmDesc tq = tdescs[bi];
        const SvtHipRdoqDesc rd = descs[bi];
        const SvtHipTxfmResult res = results[bi];
        const int32_t *tc = (const int32_t *)(base + tq.coeff_off);
        int32_t       *qc = (int32_t *)(base + tq.qcoeff_off), *dqc = (int32_t *)(base + tq.dqcoeff_off);
        const int16_t *iscan = (const int16_t *)(base + tq.iscan_off);
        int            eob = res.eob < N ? res.eob : N;
        int            path = SVT_HIP_RDOQ_PATH_NOT_FLAGGED;
        const int      shift = prm.tx_scale;
        const int32_t  dq0 = tq.dequant[0], dq1 = tq.dequant[1];
        const bool     b_family = tq.quant_mode == SVT_HIP_QUANT_B || tq.quant_mode == SVT_HIP_QUANT_B_HBD;

        // ---- what svt_aom_quantize_inv_quantize decides before the trellis (full_loop.c:1566-1659)
        bool perform = active && (rd.flags & SVT_HIP_RDOQ_PERFORM);
        bool requant = false, trim = false;
        if (perform && rd.satd_factor != 255) {
            int32_t satd = (int32_t)res.satd;
            satd = shift < 1 ? satd >> (1 - shift) : satd << (shift - 1);  // RIGHT_SIGNED_SHIFT(satd, MAX_TX_SCALE - tx_scale)
            const int pic_bd = rd.pic_bit_depth ? rd.pic_bit_depth : tq.bit_depth;  // enhanced_pic->bit_depth
            satd >>= pic_bd > 8 ? pic_bd - 8 : 0;
            const int32_t qstep = dq1 >> (rd.dequant_shift < 31 ? rd.dequant_shift : 31);
            if ((uint64_t)(int64_t)satd > (uint64_t)rd.satd_factor * (uint64_t)(int64_t)qstep * (uint64_t)prm.sqrt_px)
                perform = false, requant = true, path = SVT_HIP_RDOQ_PATH_REQUANT_SATD;
        }
        if (perform) {
            if (eob == 0) {
                perform = false, path = SVT_HIP_RDOQ_PATH_EOB_ZERO;
            } else {
                const int eob_perc = eob * 100 / (int)prm.pixels;
                if (eob_perc >= rd.eob_th)
                    perform = false, requant = true, path = SVT_HIP_RDOQ_PATH_REQUANT_EOB;
                else
                    trim = eob_perc >= rd.eob_fast_th;
            }
        }
        // ---- the quantize_b family over the block (a pure function of coeff: what the reference's second call leaves)
        {
            int last = 0;
            if (requant && !b_family) {
                SvtHipTxfmDesc bq = tq;
                for (int k = 0; k < 2; k++) bq.zbin[k] = rd.zbin[k], bq.round[k] = rd.round[k], bq.quant[k] = rd.quant[k], bq.quant_shift[k] = rd.quant_shift[k];
                bq.quant_mode = tq.quant_mode == SVT_HIP_QUANT_FP_HBD || (tq.quant_mode == SVT_HIP_QUANT_NONE && tq.bit_depth > 8) ? SVT_HIP_QUANT_B_HBD
                                                                                                                                : SVT_HIP_QUANT_B;
                txb::QP qp;
                txb::load_qp(qp, bq, base);
                for (int k = 0; k < PER; k++) {
                    const int pos = li + k * G;
                    int32_t   a, b;
                    txb::quant_one(qp, tc[pos], (uint32_t)pos, a, b);
                    qc[pos] = a, dqc[pos] = b;
                    const int c = iscan[pos] & (N - 1);
                    last = a != 0 && c + 1 > last ? c + 1 : last;
                }
            }
            last = group_max_i<G>(last);
            if (requant && !b_family)
                eob = last;
        }
        // ---- update_coeff_eob_fast, once for eob_fast_th and once more for fast_mode behind the early exit
        const uint32_t ti = rd.table < prm.n_tables ? rd.table : prm.n_tables - 1;
        const SvtHipRateTables &t = tables[ti];
        const int plane = rd.plane_type != 0, cls = tx_class_of(tq.tx_type & 15);
        const int skip_ctx = rd.txb_skip_ctx < 12 ? rd.txb_skip_ctx : 12, sign_ctx = rd.dc_sign_ctx < 2 ? rd.dc_sign_ctx : 2;
        const SvtHipCoeffCost &cc_global = t.coeff[prm.txs_ctx][plane];
        const SvtHipCoeffCost *cc = ti == first_table ? &staged[plane] : &cc_global;
        const int32_t (*eob_bits)[11] = t.eob[ilog2(N) - 4][plane];
        const int zbin0 = dq0 + ((dq0 * 70 + 64) >> 7), zbin1 = dq1 + ((dq1 * 70 + 64) >> 7);
        int       eob_cost_ = 0;
        bool      entered = false;  // inside svt_av1_optimize_b, past its early exit
        __syncthreads();  // the staged tables (first step); LDS of the previous step has been read
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {
            int keep = 0;
            if (trim) {
                for (int k = 0; k < PER; k++) {
                    const int pos = li + k * G, c = iscan[pos] & (N - 1);
                    if (c < eob) {
                        const int32_t co = tc[pos];
                        const int64_t a = co < 0 ? -(int64_t)co : (int64_t)co;
                        if (!((a << (1 + shift)) < (pos ? zbin1 : zbin0) || qc[pos] == 0))
                            keep = c + 1 > keep ? c + 1 : keep;
                    }
                }
            }
            keep = group_max_i<G>(keep);
            if (trim) {
                for (int k = 0; k < PER; k++) {
                    const int pos = li + k * G, c = iscan[pos] & (N - 1);
                    if (c >= keep && c < eob)
                        qc[pos] = 0, dqc[pos] = 0;
                }
                eob = keep, path |= SVT_HIP_RDOQ_PATH_FAST_TRIM;
                if (eob == 0)
                    perform = false, path = (entered ? SVT_HIP_RDOQ_PATH_TRELLIS : SVT_HIP_RDOQ_PATH_EOB_ZERO) | SVT_HIP_RDOQ_PATH_FAST_TRIM;
            }
            trim = false;
            if (pass == 0 && perform) {  // the head of svt_av1_optimize_b (:1152-1167)
                eob_cost_ = eob_cost(eob, eob_bits, cc->eob_extra, cls);
                const int skip_cost = cc->txb_skip[skip_ctx][1], non_skip_cost = cc->txb_skip[skip_ctx][0];
                if (eob_cost_ < (int)((uint32_t)N * rd.early_exit_limit) && skip_cost < non_skip_cost) {
                    perform = false, path = SVT_HIP_RDOQ_PATH_EARLY_EXIT | (path & SVT_HIP_RDOQ_PATH_FAST_TRIM);
                } else {
                    path = SVT_HIP_RDOQ_PATH_TRELLIS | (path & SVT_HIP_RDOQ_PATH_FAST_TRIM);
                    entered = true;
                    trim = (rd.flags & SVT_HIP_RDOQ_FAST_MODE) != 0;
                }
            }
        }
        const bool do_walk = perform;
        __syncthreads();  // the group's stores to qcoeff / dqcoeff are visible to all its lanes
        // ---- scan and levels (svt_av1_txb_init_levels_c: the WHOLE retained array, also beyond eob) into LDS
        if (do_walk) {
            for (int k = 0; k < PER; k++) {
                const int pos = li + k * G;
                scan_lds[gi][iscan[pos] & (N - 1)] = (int16_t)pos;
            }
            for (int wd = li; wd < LEVEL_WORDS; wd += G) {
                const int r = wd / ROW_WORDS, c4 = wd - r * ROW_WORDS;
                uint32_t  word = 0;
                if (r < IH && c4 < IW / 4) {
                    const int32_t *q = qc + r * IW + c4 * 4;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int32_t  v = q[j];
                        const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
                        word |= (a < 127 ? a : 127) << (8 * j);
                    }
                }
                lv[gi][wd] = word;
            }
        }
        __syncthreads();
        // ---- the head of the walk, by the group's first lane
        Trellis<IW, IH> tw;
        tw.cc = cc, tw.eob_bits = eob_bits, tw.levels = (uint8_t *)lv[gi], tw.scan = scan_lds[gi], tw.nz_ci = nz_lds[gi];
        tw.tc = tc, tw.qc = qc, tw.dqc = dqc, tw.iqm = tq.iqm_off == SVT_HIP_NO_OFFSET ? nullptr : base + tq.iqm_off;
        tw.dq[0] = dq0, tw.dq[1] = dq1, tw.shift = shift, tw.cls = cls, tw.orient = prm.orient, tw.sign_ctx = sign_ctx;
        tw.sharpness = (rd.flags & SVT_HIP_RDOQ_SHARPNESS) != 0;
        {
            const int rweight = tw.sharpness ? 0 : 100, mult = rd.is_inter ? (plane ? 20 : 16) : (plane ? 20 : 17);  // plane_rd_mult
            tw.rdmult = ((((int64_t)rd.lambda * mult) * rweight) / 100 + 2) >> 2;
        }
        if (do_walk && li == 0) {
            const uint8_t *levels = (const uint8_t *)lv[gi];
            const int      last = scan_lds[gi][eob - 1];
            int            new_eob = eob, bits = 0, si = -1;
            if (levels[(last / IW) * Levels<IW, IH>::STRIDE + last % IW] == 0) {
                bits = SVT_HIP_RDOQ_PATH_BAD_EOB;
            } else {
                bool skipped = false;
                new_eob = tw.head(eob, eob_cost_, (rd.flags & SVT_HIP_RDOQ_FAST_MODE) != 0, cc->txb_skip[skip_ctx][1], cc->txb_skip[skip_ctx][0], skipped, si);
                bits = skipped ? SVT_HIP_RDOQ_PATH_SKIP : 0;
                if (!ROUNDS) {
                    for (int k = si; k >= 1; --k) tw.update_simple(scan_lds[gi][k]);
                    if (si >= 0)
                        tw.dc(new_eob);
                }
            }
            walked[gi][0] = new_eob, walked[gi][1] = bits, walked[gi][2] = si;
        }
        __syncthreads();
        if (ROUNDS) {  // update_coeff_simple over scan positions start .. 1, one anti-diagonal per round, then DC
            const int start = do_walk ? walked[gi][2] : -1;
            int       first = -1;  // the last anti-diagonal that holds such a position
            if (start >= 1) {
                for (int k = 0; k < PER; k++) {
                    const int pos = li + k * G, c = iscan[pos] & (N - 1), diag = pos / IW + pos % IW;
                    first = c >= 1 && c <= start && diag > first ? diag : first;
                }
            }
            first = group_max_i<64>(first);  // of the wavefront: the barriers below are the workgroup's
            for (int diag = first; diag >= 0; --diag) {
                const int row = (diag < IW ? 0 : diag - (IW - 1)) + li, col = diag - row;
                if (start >= 1 && row < IH && col >= 0) {
                    const int pos = row * IW + col, c = iscan[pos] & (N - 1);
                    if (c >= 1 && c <= start)
                        tw.update_simple(pos);
                }
                __syncthreads();
            }
            if (start >= 0 && li == 0)
                tw.dc(walked[gi][0]);
            __syncthreads();
        }
        if (do_walk)
            eob = walked[gi][0], path |= walked[gi][1];
        // ---- svt_av1_compute_cul_level_c: min(63, sum of |q| below eob), the same whether or not the sum stops early
        int cul = 0;
        if (active) {
            for (int k = 0; k < PER; k++) {
                const int pos = li + k * G;
                if ((iscan[pos] & (N - 1)) < eob) {
                    const int32_t  v = qc[pos];
                    const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
                    cul += a < 63 ? (int)a : 63;
                }
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) cul += __shfl_xor(cul, off, 64);
        if (active && li == 0) {
            cul = cul < 63 ? cul : 63;
            const int32_t dc = qc[0];
            cul = dc < 0 ? cul | 64 : dc > 0 ? cul + 128 : cul;
            SvtHipRdoqResult r;
            r.eob = (uint16_t)eob, r.cul_level = (uint8_t)cul, r.path = (uint8_t)path;
            out[tb] = r;
            if (path != SVT_HIP_RDOQ_PATH_NOT_FLAGGED)
                results[tb].eob = (uint16_t)eob;
        }
    }
}

}  // namespace

constexpr uint32_t kLaneMax = 128;  // retained coefficients up to which the lane-per-block kernels exist (LDS, see the head of the file)

// svt_hip_rdoq_batch: the fastest mapping of profiles/rdoq_4k.json by retained coefficients, all 14 retained shapes timed.  One lane
// per block wins wherever it exists: 2.2 - 2.6 x up to 32 coefficients and at 8 x 8, 1.5 x at 4 x 16 / 16 x 4, 7 % at 8 x 16; at 16 x 8 it
// ties with the rounds (0.3 %, inside the spread).  Above, the rounds are ahead of scan order by 1 - 6 % in every median, though
// only at 16 x 16 were the ranges apart in both of two runs.
constexpr uint32_t mapping_for(uint32_t retained) { return retained <= kLaneMax ? 2 : 1; }
extern "C" int32_t svt_hip_rdoq_batch_mapped(uint8_t *d_base, const SvtHipTxfmDesc *d_txfm_desc, const SvtHipRdoqDesc *d_desc,
                                      const SvtHipRateTables *d_tables, uint32_t n_tables, SvtHipTxfmResult *d_txfm_result,
                                             SvtHipRdoqResult *d_out, uint32_t n_blocks, uint32_t w, uint32_t h, uint32_t mapping, void *stream) {
    const TxbGeometry g(w, h);
    const bool        is_mapping = mapping <= 1 || (mapping == 2 && g.retained <= kLaneMax);
    if (!g.valid || !is_mapping || n_tables == 0 || (n_blocks > 0 && (!d_base || !d_txfm_desc || !d_desc || !d_tables || !d_txfm_result || !d_out)))
        return refuse("svt_hip_rdoq_batch: bad argument (%u x %u, %u table sets, %u blocks)", w, h, n_tables, n_blocks);
    if (n_blocks == 0)
        return SVT_HIP_OK;
    TierBCall c("svt_hip_rdoq_batch_mapped", stream);
    if (!c.ok())
        return c.status();
    const RdoqLaunch prm{g.orient, g.txs_ctx, g.tx_scale, (int32_t)g.sqrt_retained, g.pixels, n_tables, n_blocks};
    const dim3  grid(grid_blocks(n_blocks, mapping == 2 ? 64 : 64 / group_lanes(g.retained), (uint32_t)cu_count() * 16));
    const bool  launched = for_retained_shape(g.iw, g.ih, [&](auto W, auto H) {
        constexpr int IW = decltype(W)::value, IH = decltype(H)::value;
        auto          kernel = mapping == 1 ? rdoq_kernel<IW, IH, true, false> : rdoq_kernel<IW, IH, false, false>;
        if constexpr ((uint32_t)(IW * IH) <= kLaneMax)  // where the lane-per-block instance exists; is_mapping refused it elsewhere
            kernel = mapping == 2 ? rdoq_kernel<IW, IH, false, true> : kernel;
        hipLaunchKernelGGL(kernel, grid, dim3(64), 0, c.stream(), d_base, d_txfm_desc, d_desc, d_tables, d_txfm_result, d_out, prm);
    });
    if (!launched) {
        set_error("svt_hip_rdoq_batch: no kernel for the retained shape %u x %u", g.iw, g.ih);
        return SVT_HIP_ERR_RUNTIME;
    }
    return c.finish();
}

extern "C" int32_t svt_hip_rdoq_batch(uint8_t *d_base, const SvtHipTxfmDesc *d_txfm_desc, const SvtHipRdoqDesc *d_desc,
                                      const SvtHipRateTables *d_tables, uint32_t n_tables, SvtHipTxfmResult *d_txfm_result,
                                      SvtHipRdoqResult *d_out, uint32_t n_blocks, uint32_t w, uint32_t h, void *stream) {
    return svt_hip_rdoq_batch_mapped(d_base, d_txfm_desc, d_desc, d_tables, n_tables, d_txfm_result, d_out, n_blocks, w, h,
                                     mapping_for(TxbGeometry(w, h).retained), stream);
}

SVT_HIP_MODULE_WARMUP(txfm_rdoq)
