// inter_ifs.hip — the interpolation filter search of mode decision on gfx950: interpolation_filter_search
// (enc_inter_prediction.c:2413-2543) with model_rd_for_sb / model_rd_from_sse (:2255-2365), bit-exact, one descriptor per luma block of
// one candidate.
//
// One workgroup per descriptor, two instantiations sharing a call as in inter_subpel.hip: a single wave takes the blocks of up to 256
// samples (and every bad descriptor), four waves the larger ones, 64 x 64 tile by tile.  Per tile the window of each reference is staged
// in LDS ONCE, with the margins of the directions that have a phase, and all pairs are predicted from it: for each horizontal filter one
// horizontal pass per reference into an int16 intermediate in LDS, which the three vertical filters share.  A direction in which no
// reference has a phase cannot change the prediction, so its three filters are predicted once and the sum is reused.  The compound's
// first prediction never leaves its lane: the same lane computes both references' samples, so the ConvBufType value is a register.
// No prediction is written during the search; the squared differences go from registers to one 64-bit sum per pair (wave shuffle,
// then an LDS atomic).  With `dst`, the winner is predicted once more and written.  LDS: two windows of 71 x 72 uint16 and two
// intermediates of 71 x 64 int16, 38.7 KB (four workgroups per compute unit); 39 rows and 21.2 KB in the single-wave kernel.
#include "common.hpp"
#include "ifs_device.hpp"
#include "subpel_device.hpp"

using namespace svthip;
using namespace svthip::ifs;

namespace {

__device__ int ifs_status(const SvtHipIfsDesc &d) {
    if (!subpel::is_block_size(d.w, d.h))
        return SVT_HIP_IFS_BAD_SIZE;
    if (d.compound == 1 || d.compound > 3)
        return SVT_HIP_IFS_BAD_COMPOUND;
    if (!d.src || !d.ref0 || (d.compound && !d.ref1))
        return SVT_HIP_IFS_BAD_POINTER;
    if (d.subpel_x0 > 15 || d.subpel_y0 > 15 || d.subpel_x1 > 15 || d.subpel_y1 > 15)
        return SVT_HIP_IFS_BAD_PHASE;
    if (d.ctx[0] >= SVT_HIP_IFS_CONTEXTS || d.ctx[1] >= SVT_HIP_IFS_CONTEXTS)
        return SVT_HIP_IFS_BAD_CTX;
    if (d.compound == 3 && d.fwd_offset + d.bck_offset != 16)
        return SVT_HIP_IFS_BAD_WEIGHT;
    return SVT_HIP_IFS_OK;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// av1_get_interp_filter_params_with_block_size: the bank of d_filters for filter f over a side
__device__ __forceinline__ int bank_of(int f, int side) { return side <= 4 ? (f == 1 ? 4 : 3) : f; }

template <int NT, int ROWS, bool LARGE>
__global__ __launch_bounds__(NT) void ifs_kernel(const SvtHipIfsJob job, const SvtHipIfsDesc *__restrict__ d_desc, SvtHipIfsResult *__restrict__ d_result,
                                                 SvtHipIfsTrace *__restrict__ d_trace, uint32_t n) {
    __shared__ alignas(4) uint16_t in[2][ROWS * IP + CONV_IN_SLACK];
    __shared__ int16_t             im[2][ROWS * TILE];
    __shared__ unsigned long long  acc[SVT_HIP_IFS_COMBOS];
    __shared__ int                 winner;
    const int  bd = job.bit_depth, is16 = bd > 8;
    const bool dual = job.enable_dual_filter != 0;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const SvtHipIfsDesc d = d_desc[i];
        const int           status = ifs_status(d);
        if (!subpel::takes(LARGE, status, [&] { return (int)d.w * d.h > subpel::SMALL_AREA; }))
            continue;
        if (status) {
            if (threadIdx.x == 0) {
                SvtHipIfsResult r = {};
                r.status          = (uint8_t)status;
                d_result[i]       = r;
                if (d_trace)
                    d_trace[i] = SvtHipIfsTrace{};
            }
            continue;
        }
        const int  w = d.w, h = d.h, comp = d.compound;
        const bool anyx = d.subpel_x0 || (comp && d.subpel_x1), anyy = d.subpel_y0 || (comp && d.subpel_y1);
        const int  rstep = job.subsampled_distortion && h > 16 ? 2 : 1;  // model_rd_for_sb: every other row, the sum doubled
        Ref        f0, f1;  // named, not an array: indexing one by a loop counter puts the taps in scratch memory
        f0.in = in[0], f0.im = im[0], f0.hx = d.subpel_x0 != 0, f0.hy = d.subpel_y0 != 0;
        f1.in = in[1], f1.im = im[1], f1.hx = comp && d.subpel_x1 != 0, f1.hy = comp && d.subpel_y1 != 0;
        // a pair (fy, fx) is predicted when a tested pair maps to it once the filters of a direction without a phase count as filter 0
        uint32_t needed = 0;
        for (int k = 0; k < SVT_HIP_IFS_COMBOS; k++)
            if (dual || k / 3 == k % 3)
                needed |= 1u << ((anyy ? k / 3 : 0) * 3 + (anyx ? k % 3 : 0));
        const auto load_x = [&](int fx) {
            if (f0.hx)
                load_taps_x(f0, job.d_filters, bank_of(fx, w), d.subpel_x0);
            if (f1.hx)
                load_taps_x(f1, job.d_filters, bank_of(fx, w), d.subpel_x1);
        };
        const auto load_y = [&](int fy) {
            if (f0.hy)
                load_taps_y(f0, job.d_filters, bank_of(fy, h), d.subpel_y0);
            if (f1.hy)
                load_taps_y(f1, job.d_filters, bank_of(fy, h), d.subpel_y1);
        };
        const auto stage = [&](int x0, int y0, int tw, int th) {
            stage_window<NT>(in[0], d.ref0, d.ref0_stride, x0, y0, tw, th, f0.hx, f0.hy, is16);
            if (comp)
                stage_window<NT>(in[1], d.ref1, d.ref1_stride, x0, y0, tw, th, f1.hx, f1.hy, is16);
        };
        const auto horizontal = [&](int tw, int th) {
            if (f0.hx && f0.hy)
                horizontal_pass<NT>(f0, im[0], tw, th, bd);
            if (f1.hx && f1.hy)
                horizontal_pass<NT>(f1, im[1], tw, th, bd);
        };
        const auto sample = [&](int r, int c) {
            if (!comp)
                return sr_sample(f0, r, c, bd, is16);
            return jnt_sample(jnt_intermediate(f0, r, c, bd), jnt_intermediate(f1, r, c, bd), comp, d.fwd_offset, d.bck_offset, bd);
        };
        if (threadIdx.x < SVT_HIP_IFS_COMBOS)
            acc[threadIdx.x] = 0;
        const int tiles_x = (w + TILE - 1) / TILE, tiles = tiles_x * ((h + TILE - 1) / TILE);
        for (int tile = 0; tile < tiles; tile++) {
            const int x0 = (tile % tiles_x) * TILE, y0 = (tile / tiles_x) * TILE, tw = min(TILE, w - x0), th = min(TILE, h - y0);
            __syncthreads();  // the previous tile's (or block's) last readers of in / im, and acc is zero
            stage(x0, y0, tw, th);
            for (int fx = 0; fx < 3; fx++) {
                if (!((needed >> fx) & 0x49u))  // no fy needs this fx
                    continue;
                load_x(fx);
                __syncthreads();  // the windows are staged; the previous fx's vertical passes have read im
                horizontal(tw, th);
                __syncthreads();
                for (int fy = 0; fy < 3; fy++) {
                    if (!((needed >> (fy * 3 + fx)) & 1u))
                        continue;
                    load_y(fy);
                    uint32_t sum = 0;  // at most 16 samples of 10 bit per lane
                    for (int idx = threadIdx.x; idx < (th / rstep) * tw; idx += NT) {
                        const int     r = (idx / tw) * rstep, c = idx % tw;
                        const int32_t diff = ldpx(d.src, (ptrdiff_t)(y0 + r) * (ptrdiff_t)d.src_stride + (x0 + c), is16) - sample(r, c);
                        sum += (uint32_t)(diff * diff);
                    }
                    sum = wave_sum(sum);  // 64 lanes: below 2^32
                    if ((threadIdx.x & 63) == 0)
                        atomicAdd(&acc[fy * 3 + fx], (unsigned long long)sum);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            SvtHipIfsResult res = {};
            uint64_t        rd = ~(uint64_t)0;
            const int       n_log2 = subpel::log2_pow2(w) + subpel::log2_pow2(h);
            for (int k = 0; k < SVT_HIP_IFS_COMBOS; k++) {
                const int fy = k / 3, fx = k % 3;  // filter_sets[k] = {fy, fx}
                if (!dual && fy != fx) {
                    if (d_trace)
                        d_trace[i].sse[k] = d_trace[i].rd[k] = ~(uint64_t)0;
                    continue;
                }
                // svt_av1_get_switchable_rate: dir 0 extracts the y filter, dir 1 the x filter
                int32_t tmp_rs = job.d_switchable_rate[d.ctx[0] * 3 + fy];
                if (dual)
                    tmp_rs += job.d_switchable_rate[d.ctx[1] * 3 + fx];
                const uint64_t sse = (uint64_t)acc[(anyy ? fy : 0) * 3 + (anyx ? fx : 0)] << (rstep - 1);
                int32_t        tmp_rate = 0;
                uint64_t       tmp_dist = sse * 10;
                if (!job.skip_sse_rd_model) {
                    const int shift = 2 * (bd - 8);
                    model_rd_from_sse(n_log2, job.quantizer, bd, (sse + ((1 << shift) >> 1)) >> shift, &tmp_rate, &tmp_dist);
                }
                // RDCOST (rd_cost.h:37-39)
                const int32_t r_sum = (int32_t)((uint32_t)tmp_rs + (uint32_t)tmp_rate);
                uint64_t      tmp_rd = (uint64_t)((((int64_t)r_sum * (int64_t)job.full_lambda + 256) >> 9) + (int64_t)tmp_dist * 128);
                if (job.smooth_bias_pct && (fy == 1 || fx == 1))
                    tmp_rd = (tmp_rd * job.smooth_bias_pct) / 100;
                if (d_trace)
                    d_trace[i].sse[k] = sse, d_trace[i].rd[k] = tmp_rd;
                if (tmp_rd < rd) {
                    rd = tmp_rd;
                    res.rd = tmp_rd, res.sse = sse, res.interp_filters = (uint32_t)fy | ((uint32_t)fx << 16), res.switchable_rate = tmp_rs;
                    res.best = (uint8_t)k;
                }
            }
            d_result[i] = res;
            winner = res.best;
        }
        __syncthreads();
        if (!d.dst)
            continue;
        const int best = winner;
        load_x(best % 3), load_y(best / 3);
        for (int tile = 0; tile < tiles; tile++) {
            const int x0 = (tile % tiles_x) * TILE, y0 = (tile / tiles_x) * TILE, tw = min(TILE, w - x0), th = min(TILE, h - y0);
            __syncthreads();
            stage(x0, y0, tw, th);
            __syncthreads();
            horizontal(tw, th);
            __syncthreads();
            for (int idx = threadIdx.x; idx < th * tw; idx += NT) {
                const int r = idx / tw, c = idx % tw;
                stpx(d.dst, (size_t)(y0 + r) * d.dst_stride + x0 + c, is16, sample(r, c), 16);
            }
        }
    }
}

}  // namespace

extern "C" size_t svt_hip_ifs_search_batch(const SvtHipIfsJob *job, const SvtHipIfsDesc *d_desc, SvtHipIfsResult *d_result, SvtHipIfsTrace *d_trace,
                                           uint32_t n, void *stream) {
    if (!job || !d_desc || !d_result)
        return SVT_HIP_IFS_STATUS(refuse("svt_hip_ifs_search_batch: NULL argument"));
    if (!job->d_switchable_rate || !job->d_filters)
        return SVT_HIP_IFS_STATUS(refuse("svt_hip_ifs_search_batch: NULL table in the job"));
    if (job->bit_depth != 8 && job->bit_depth != 10)
        return SVT_HIP_IFS_STATUS(refuse("svt_hip_ifs_search_batch: bit depth %d is neither 8 nor 10", (int)job->bit_depth));
    return SVT_HIP_IFS_STATUS(launch_two_classes("svt_hip_ifs_search_batch", true, n, stream, ifs_kernel<64, 32 + 7, false>, 64, 32,
                                                 ifs_kernel<256, TILE + 7, true>, 256, 8, *job, d_desc, d_result, d_trace, n));
}

SVT_HIP_MODULE_WARMUP(inter_ifs)
