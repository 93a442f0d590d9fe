// inter_warp.hip — warped motion on gfx950: warped prediction (svt_av1_warp_affine_c / svt_aom_dec_svt_av1_highbd_warp_affine_c,
// warped_motion.c:570-680, 718-820), the global-motion error of a whole picture (svt_av1_warp_error, enc_warped_motion.c:22-98)
// and the host driver of its hill climb (svt_av1_refine_integerized_param, global_motion.c:132-251) with svt_get_shear_params
// (warped_motion.c:1045-1068).
//
// Both kernels: 256 threads, one 8 x 8 output block per wave and pass (warp_device.hpp), the filter table and the clamped
// source windows in LDS.  Error: one workgroup per 32 x 32 error block and candidate writes that block's SAD; a second kernel, one
// wave per candidate, walks the SADs in raster order and returns the first prefix above the candidate's threshold.
#include "../../include/svt_hip_inter.h"
#include "blend_device.hpp"
#include "common.hpp"
#include "warp_device.hpp"

using namespace svthip;
using namespace svthip::warp;

namespace {

constexpr int WARP_WAVES  = 4;  // waves of a workgroup
constexpr int WARP_CHUNKS = 4;  // workgroups per descriptor: 128 x 128 = 256 blocks = 4 x 16 passes of 4 waves

__device__ bool warp_desc_ok(const SvtHipWarpDesc &d) {
    if (d.p_width < 4 || d.p_height < 4 || d.p_width > 128 || d.p_height > 128 || !d.ref || d.compound > 3)
        return false;
    if ((d.compound != 1 && !d.dst) || (d.compound != 0 && !d.cbuf))
        return false;
    if (d.width == 0 || d.height == 0 || d.width > 65536 || d.height > 65536 || d.p_col < 0 || d.p_row < 0 || d.p_col > 65535 || d.p_row > 65535)
        return false;
    if (d.is_16bit > 1 || (d.bit_depth != 8 && d.bit_depth != 10 && d.bit_depth != 12) || (!d.is_16bit && d.bit_depth != 8))
        return false;
    if (d.subsampling_x > 1 || d.subsampling_y > 1 || d.round_0 < 1 || d.round_0 > 7 || (d.compound != 0 && d.round_0 + d.round_1 > 14))
        return false;
    return shear_allowed(d.alpha, d.beta, d.gamma, d.delta);
}

template <bool IS16> __device__ void warp_desc(const SvtHipWarpDesc &d, const int16_t *filt, WaveLds &l, int first) {
    const int   lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int   bw = (d.p_width + 7) >> 3, nb = bw * ((d.p_height + 7) >> 3);
    const int   bd = d.bit_depth, reduce_h = reduce_bits_horiz(bd, d.round_0), max_px = (1 << bd) - 1;
    const int   round_bits = 14 - d.round_0 - d.round_1, offset_bits = bd + 14 - d.round_0;
    const int   round_offset = (1 << (offset_bits - d.round_1)) + (1 << (offset_bits - d.round_1 - 1));
    const Model m = {{d.mat[0], d.mat[1], d.mat[2], d.mat[3], d.mat[4], d.mat[5]}, d.alpha, d.beta, d.gamma, d.delta};
    for (int base = first; base < nb; base += WARP_WAVES * WARP_CHUNKS) {
        const int  b = base + wave, by = b / bw, bx = b - by * bw;
        const bool active = b < nb;
        const int  sum = block8<IS16>(d.ref, d.ref_stride, (int)d.width, (int)d.height, m, d.p_row + 8 * by, d.p_col + 8 * bx, d.subsampling_x,
                                      d.subsampling_y, bd, reduce_h, filt, l, lane, active);
        const int  y = 8 * by + (lane >> 3), x = 8 * bx + (lane & 7);
        if (!active || y >= d.p_height || x >= d.p_width)  // a 4-wide / 4-high block is cropped here
            continue;
        int px;
        if (d.compound == 0) {
            px = round_shift(sum, 14 - reduce_h) - (1 << (bd - 1)) - (1 << bd);
        } else {
            const int v = round_shift(sum, d.round_1);
            uint16_t *p = d.cbuf + (size_t)y * d.cbuf_stride + x;
            if (d.compound == 1) {
                *p = (uint16_t)v;
                continue;
            }
            const int t = d.compound == 3 ? ((int)*p * d.fwd_offset + v * d.bck_offset) >> 4 : ((int)*p + v) >> 1;
            px = round_shift(t - round_offset, round_bits);
        }
        px = min(max(px, 0), max_px);
        const size_t at = (size_t)y * d.dst_stride + x;
        if (IS16)
            ((uint16_t *)d.dst)[at] = (uint16_t)px;
        else
            ((uint8_t *)d.dst)[at] = (uint8_t)px;
    }
}

__global__ __launch_bounds__(64 * WARP_WAVES) void warp_kernel(const SvtHipWarpDesc *__restrict__ descs, const int16_t *__restrict__ filter) {
    __shared__ __attribute__((aligned(16))) int16_t filt[FILTER_ROWS * 8];
    __shared__ WaveLds                              lds[WARP_WAVES];
    const SvtHipWarpDesc                            d = descs[blockIdx.x];  // uniform: scalar loads
    const int first = (int)blockIdx.y * WARP_WAVES;  // this workgroup's first block of the descriptor
    if (!warp_desc_ok(d) || first >= ((d.p_width + 7) >> 3) * ((d.p_height + 7) >> 3))
        return;
    load_filter(filt, filter);
    WaveLds &l = lds[threadIdx.x >> 6];
    d.is_16bit ? warp_desc<true>(d, filt, l, first) : warp_desc<false>(d, filt, l, first);
}

// ---- global-motion error ----------------------------------------------------------------------------------------------
struct ErrorGeom {
    const uint8_t *ref, *cur;
    uint32_t       ref_stride, cur_stride;
    int            ref_width, ref_height, width, height, cols, rows, chess;
};

// with chess_refn, block row r starts at column 1 (r even) or 0 (r odd) and takes every other block
__device__ inline bool block_visited(int chess, int row, int col) { return !chess || ((row + col) & 1); }

__global__ __launch_bounds__(64 * WARP_WAVES) void warp_error_sad_kernel(ErrorGeom g, const SvtHipWarpCandidate *__restrict__ cands,
                                                                         const int16_t *__restrict__ filter, uint32_t *__restrict__ sads) {
    __shared__ __attribute__((aligned(16))) int16_t filt[FILTER_ROWS * 8];
    __shared__ WaveLds                              lds[WARP_WAVES];
    __shared__ uint32_t                             part[WARP_WAVES];
    const int row = (int)blockIdx.x / g.cols, col = (int)blockIdx.x - row * g.cols;
    if (!block_visited(g.chess, row, col))
        return;
    const SvtHipWarpCandidate c = cands[blockIdx.y];  // uniform
    if (!shear_allowed(c.alpha, c.beta, c.gamma, c.delta))
        return;
    const Model m = {{c.mat[0], c.mat[1], c.mat[2], c.mat[3], c.mat[4], c.mat[5]}, c.alpha, c.beta, c.gamma, c.delta};
    const int   lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int   i0 = row * SVT_HIP_WARP_ERROR_BLOCK, j0 = col * SVT_HIP_WARP_ERROR_BLOCK;
    const int   warp_w = min(SVT_HIP_WARP_ERROR_BLOCK, g.width - j0), warp_h = min(SVT_HIP_WARP_ERROR_BLOCK, g.height - i0);
    const int   bw = (warp_w + 7) >> 3, nb = bw * ((warp_h + 7) >> 3);
    load_filter(filt, filter);
    uint32_t acc = 0;
    for (int base = 0; base < nb; base += WARP_WAVES) {
        const int  b = base + wave, by = b / bw, bx = b - by * bw;
        const bool active = b < nb;
        // get_conv_params(0, 0, 0, 8): round_0 = 3, not compound
        const int sum = block8<false>(g.ref, g.ref_stride, g.ref_width, g.ref_height, m, i0 + 8 * by, j0 + 8 * bx, 0, 0, 8, 3, filt, lds[wave], lane, active);
        const int y = 8 * by + (lane >> 3), x = 8 * bx + (lane & 7);
        if (active && y < warp_h && x < warp_w) {
            const int px = min(max(round_shift(sum, 11) - 128 - 256, 0), 255);
            acc += (uint32_t)abs(px - (int)g.cur[(size_t)(i0 + y) * g.cur_stride + j0 + x]);
        }
    }
    acc = blend::wave_sum(acc);
    if (lane == 0)
        part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        sads[(size_t)blockIdx.y * (g.cols * g.rows) + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// inclusive sum over the lanes up to and including this one
__device__ inline uint32_t wave_scan(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o)
            v += u;
    }
    return v;
}

// One wave per candidate.  64 blocks per pass: a block SAD is at most 32 * 32 * 255, so a pass sums in 32 bits; the running sum
// across passes is 64-bit.
__global__ __launch_bounds__(64) void warp_error_prefix_kernel(const SvtHipWarpCandidate *__restrict__ cands, const uint32_t *__restrict__ sads,
                                                               SvtHipWarpErrorResult *__restrict__ results, int cols, int nblocks, int chess) {
    const int                 lane = (int)threadIdx.x;
    const SvtHipWarpCandidate c = cands[blockIdx.x];
    SvtHipWarpErrorResult     r{};
    if (!shear_allowed(c.alpha, c.beta, c.gamma, c.delta)) {
        r.status = SVT_HIP_WARP_ERROR_BAD_SHEAR;
        if (lane == 0)
            results[blockIdx.x] = r;
        return;
    }
    const uint32_t *sad = sads + (size_t)blockIdx.x * nblocks;
    int64_t         total = 0;
    uint32_t        count = 0;
    for (int start = 0; start < nblocks; start += 64) {
        const int      idx = start + lane, row = idx / cols, col = idx - row * cols;
        const bool     visited = idx < nblocks && block_visited(chess, row, col);
        const uint32_t v = wave_scan(visited ? sad[idx] : 0u, lane), n = wave_scan(visited ? 1u : 0u, lane);
        const uint64_t over = __ballot(visited && total + (int64_t)v > c.best_error);
        if (over) {  // the reference returns here, with the partial sum
            const int first = __ffsll((unsigned long long)over) - 1;
            r.error = total + (int64_t)(uint32_t)__shfl((int)v, first, 64);
            r.blocks_summed = count + (uint32_t)__shfl((int)n, first, 64);
            if (lane == 0)
                results[blockIdx.x] = r;
            return;
        }
        total += (int64_t)(uint32_t)__shfl((int)v, 63, 64);
        count += (uint32_t)__shfl((int)n, 63, 64);
    }
    r.error = chess ? total * 2 : total;
    r.blocks_summed = count;
    if (lane == 0)
        results[blockIdx.x] = r;
}

inline uint32_t error_blocks(uint32_t v) { return (v + SVT_HIP_WARP_ERROR_BLOCK - 1) / SVT_HIP_WARP_ERROR_BLOCK; }
inline uint64_t sad_bytes(uint32_t width, uint32_t height, uint32_t n) {
    return (uint64_t)up256((size_t)n * error_blocks(width) * error_blocks(height) * sizeof(uint32_t));
}

bool error_job_ok(const SvtHipWarpErrorJob *job, uint32_t n) {
    return job && n && n <= 65535 && job->ref && job->cur && job->filter && job->workspace && job->ref_width && job->ref_height && job->cur_width &&
        job->cur_height && job->ref_width <= 65536 && job->ref_height <= 65536 && job->cur_width <= 65536 && job->cur_height <= 65536 &&
        job->ref_stride >= job->ref_width && job->cur_stride >= job->cur_width && job->chess_refn <= 1 &&
        job->workspace_bytes >= svt_hip_warp_error_workspace_bytes(job->cur_width, job->cur_height, n);
}

void launch_error(const SvtHipWarpErrorJob &job, const SvtHipWarpCandidate *d_cand, SvtHipWarpErrorResult *d_result, uint32_t n, hipStream_t st) {
    const ErrorGeom g = {job.ref, job.cur, job.ref_stride, job.cur_stride, (int)job.ref_width, (int)job.ref_height, (int)job.cur_width,
                         (int)job.cur_height, (int)error_blocks(job.cur_width), (int)error_blocks(job.cur_height), job.chess_refn};
    uint32_t       *sads = (uint32_t *)job.workspace;
    hipLaunchKernelGGL(warp_error_sad_kernel, dim3(g.cols * g.rows, n), dim3(64 * WARP_WAVES), 0, st, g, d_cand, job.filter, sads);
    hipLaunchKernelGGL(warp_error_prefix_kernel, dim3(n), dim3(64), 0, st, d_cand, sads, d_result, g.cols, g.cols * g.rows, g.chess);
}

// ---- svt_get_shear_params ---------------------------------------------------------------------------------------------
int clamp16(int64_t v) { return (int)(v < INT16_MIN ? INT16_MIN : v > INT16_MAX ? INT16_MAX : v); }
int64_t round_signed(int64_t v, int n) { return v < 0 ? -((-v + ((int64_t)1 << n >> 1)) >> n) : (v + ((int64_t)1 << n >> 1)) >> n; }

// resolve_divisor_32 (warped_motion.c:336-350): 1 / d = y / 2^shift; its table div_lut[f] is round(2^22 / (256 + f))
int resolve_divisor(uint32_t d, int *shift) {
    const int     msb = 31 - __builtin_clz(d);
    const int32_t e = (int32_t)(d - ((uint32_t)1 << msb));
    const int     f = msb > 8 ? (e + ((1 << (msb - 8)) >> 1)) >> (msb - 8) : e << (8 - msb);
    *shift = msb + 14;
    return ((1 << 22) + (256 + f) / 2) / (256 + f);
}

// ---- svt_av1_refine_integerized_param ---------------------------------------------------------------------------------
enum { IDENTITY = 0, TRANSLATION = 1, ROTZOOM = 2, AFFINE = 3 };

// add_param_offset (global_motion.c:89-110); parameters 6 and 7 are never searched
int32_t add_param_offset(int index, int32_t value, int32_t offset) {
    const int scale = index < 2 ? 10 : 1;   // GM_TRANS_PREC_DIFF, GM_ALPHA_PREC_DIFF
    const int limit = 1 << 12;              // GM_TRANS_MAX == GM_ALPHA_MAX
    const int centre = (index == 2 || index == 5) ? 1 << PREC_BITS : 0;
    value = ((value - centre) >> scale) + offset;
    value = value < -limit ? -limit : value > limit ? limit : value;
    return value * (1 << scale) + centre;
}

void force_wmtype(int32_t *mat, int wmtype) {
    if (wmtype <= IDENTITY)
        mat[0] = mat[1] = 0;
    if (wmtype <= TRANSLATION)
        mat[2] = 1 << PREC_BITS, mat[3] = 0;
    if (wmtype <= ROTZOOM)
        mat[4] = -mat[3], mat[5] = mat[2];
    mat[6] = mat[7] = 0;
}

int get_wmtype(const int32_t *mat) {
    if (mat[5] == (1 << PREC_BITS) && !mat[4] && mat[2] == (1 << PREC_BITS) && !mat[3])
        return !mat[1] && !mat[0] ? IDENTITY : TRANSLATION;
    return mat[2] == mat[5] && mat[3] == -mat[4] ? ROTZOOM : AFFINE;
}

// One svt_av1_warp_error: the shear of the model as it stands, THEN svt_warp_plane's ROTZOOM rule on mat[4], mat[5] -- in that
// order, as the reference has it: while parameter 2 or 3 of a ROTZOOM model is searched, gamma and delta come from the mat[4],
// mat[5] of the model evaluated before.
int32_t warp_error_once(const SvtHipWarpErrorJob &job, int32_t *mat, int wmtype, int64_t best_error, void *stream, int64_t *error) {
    int16_t shear[4];
    if (!svt_hip_warp_shear_params(mat, shear)) {
        *error = 1;
        return SVT_HIP_OK;
    }
    if (wmtype == ROTZOOM)
        mat[5] = mat[2], mat[4] = -mat[3];
    const SvtHipWarpCandidate cand = {{mat[0], mat[1], mat[2], mat[3], mat[4], mat[5]}, shear[0], shear[1], shear[2], shear[3], best_error};
    // the result slot behind the block SADs of one candidate
    SvtHipWarpErrorResult *d_result = (SvtHipWarpErrorResult *)((uint8_t *)job.workspace + sad_bytes(job.cur_width, job.cur_height, 1));
    TierBCall              c("svt_hip_gm_refine", stream);
    const auto            *d_cand = (const SvtHipWarpCandidate *)c.stage(&cand, sizeof(cand));
    if (!c.ok())
        return c.status();
    launch_error(job, d_cand, d_result, 1, c.stream());
    if (c.finish() != SVT_HIP_OK)  // the staged candidate is given back before the host waits
        return c.status();
    if (c.check(hipMemcpyAsync(error, d_result, sizeof(int64_t), hipMemcpyDeviceToHost, c.stream()), "hipMemcpyAsync"))  // the 8-byte read-back
        c.check(hipStreamSynchronize(c.stream()), "hipStreamSynchronize");
    return c.status();
}

}  // namespace

extern "C" int32_t svt_hip_warp_batch(const SvtHipWarpDesc *d_desc, uint32_t n, const int16_t *d_filter, void *stream) {
    if (!d_desc || !d_filter || n == 0)
        return refuse("svt_hip_warp_batch: bad argument");
    TierBCall c("svt_hip_warp_batch", stream);
    if (!c.ok())
        return c.status();
    hipLaunchKernelGGL(warp_kernel, dim3(n, WARP_CHUNKS), dim3(64 * WARP_WAVES), 0, c.stream(), d_desc, d_filter);
    return c.finish();
}

extern "C" int32_t svt_hip_warp_shear_params(const int32_t mat[6], int16_t out[4]) {
    if (mat[2] <= 0)  // is_affine_valid
        return 0;
    int16_t alpha = (int16_t)clamp16((int64_t)mat[2] - (1 << PREC_BITS)), beta = (int16_t)clamp16(mat[3]);
    int     shift;
    const int64_t y = resolve_divisor((uint32_t)mat[2], &shift);
    int64_t       v = ((int64_t)mat[4] * (1 << PREC_BITS)) * y;
    int16_t       gamma = (int16_t)clamp16((int)round_signed(v, shift));
    v = ((int64_t)mat[3] * mat[4]) * y;
    // the reference subtracts in int: the wrap-around of an out-of-range difference is kept
    int16_t delta = (int16_t)clamp16((int32_t)((uint32_t)mat[5] - (uint32_t)(int)round_signed(v, shift) - (uint32_t)(1 << PREC_BITS)));
    // rounded to WARP_PARAM_REDUCE_BITS and stored back into int16 fields: 32767 becomes 32768 and wraps to -32768, as there
    out[0] = (int16_t)(round_signed(alpha, REDUCE_BITS) * (1 << REDUCE_BITS));
    out[1] = (int16_t)(round_signed(beta, REDUCE_BITS) * (1 << REDUCE_BITS));
    out[2] = (int16_t)(round_signed(gamma, REDUCE_BITS) * (1 << REDUCE_BITS));
    out[3] = (int16_t)(round_signed(delta, REDUCE_BITS) * (1 << REDUCE_BITS));
    return shear_allowed(out[0], out[1], out[2], out[3]) ? 1 : 0;
}

extern "C" uint64_t svt_hip_warp_error_workspace_bytes(uint32_t width, uint32_t height, uint32_t n) {
    return width && height && n ? sad_bytes(width, height, n) + 256 : 0;
}

extern "C" int32_t svt_hip_warp_error_batch(const SvtHipWarpErrorJob *job, const SvtHipWarpCandidate *d_cand, SvtHipWarpErrorResult *d_result,
                                            uint32_t n, void *stream) {
    if (!d_cand || !d_result || !error_job_ok(job, n))
        return refuse("svt_hip_warp_error_batch: bad argument");
    TierBCall c("svt_hip_warp_error_batch", stream);
    if (!c.ok())
        return c.status();
    launch_error(*job, d_cand, d_result, n, c.stream());
    return c.finish();
}

extern "C" int32_t svt_hip_gm_refine(const SvtHipWarpErrorJob *job, int32_t wmmat[8], int32_t *wmtype, int32_t n_refinements,
                                     int64_t best_frame_error, int64_t *error, void *stream) {
    if (!wmmat || !wmtype || !error || *wmtype < IDENTITY || *wmtype > AFFINE || n_refinements < 0 || !error_job_ok(job, 1))
        return refuse("svt_hip_gm_refine: bad argument");
    TierBCall c("svt_hip_gm_refine", stream);  // every evaluation opens its own scope inside this one (warp_error_once)
    if (!c.ok())
        return c.status();
    const int type = *wmtype, n_params = 2 * type;  // max_trans_model_params
    int64_t   best_error, step_error;
#define SVT_HIP_GM_EVAL(out, threshold)                                                                 \
    do {                                                                                                \
        const int32_t rc_ = warp_error_once(*job, wmmat, type, threshold, stream, &(out));              \
        if (rc_ != SVT_HIP_OK)                                                                          \
            return rc_;                                                                                 \
    } while (0)
    force_wmtype(wmmat, type);
    SVT_HIP_GM_EVAL(best_error, best_frame_error);
    best_error = best_error < best_frame_error ? best_error : best_frame_error;
    int32_t step = 1 << (5 - 1);
    for (int i = 0; i < n_refinements; i++, step >>= 1) {
        for (int p = 0; p < n_params; p++) {
            int32_t      *param = wmmat + p;
            const int32_t curr_param = *param;
            int32_t       best_param = curr_param;
            int           step_dir = 0;
            *param = add_param_offset(p, curr_param, -step);  // look to the left
            SVT_HIP_GM_EVAL(step_error, best_error);
            if (step_error < best_error)
                best_error = step_error, best_param = *param, step_dir = -1;
            *param = add_param_offset(p, curr_param, step);  // look to the right
            SVT_HIP_GM_EVAL(step_error, best_error);
            if (step_error < best_error)
                best_error = step_error, best_param = *param, step_dir = 1;
            *param = best_param;
            while (step_dir) {  // keep going in the chosen direction until the error increases
                *param = add_param_offset(p, best_param, step * step_dir);
                SVT_HIP_GM_EVAL(step_error, best_error);
                if (step_error < best_error)
                    best_error = step_error, best_param = *param;
                else
                    *param = best_param, step_dir = 0;
            }
        }
    }
#undef SVT_HIP_GM_EVAL
    force_wmtype(wmmat, type);
    *wmtype = get_wmtype(wmmat);
    *error = best_error;
    return c.finish();
}

SVT_HIP_MODULE_WARMUP(inter_warp)
