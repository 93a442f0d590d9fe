// loopfilter_cdef_pick.hip — finish_cdef_search (enc_cdef.c:728-926) on the device: the picture's CDEF strength decision
// between svt_hip_cdef_search_plane (which leaves mse[plane][fb][gi] in device memory) and svt_hip_cdef_apply_frame (which
// takes one strength per filter block from device memory).  DESIGN.md section 9 has the chain and its measured time.
//
// The decision is joint_strength_search_dual (:697-727) for the four signalling widths i = 0..3: 1 << i greedy calls of
// svt_search_one_dual (:627-683) and 4 << i refinement calls, 5 << i steps per width.  The widths do not depend on each other,
// so they run side by side as grid rows: step s of every width that still has a step s runs in launch s, 40 steps deep.
//
//   pick_prepare     wave per filter block: participation (any 8x8 of the block filtered), luma cost = plane 0, chroma cost =
//                    U + V or the default, zero-strength bias; clears the totals and the level lists
//   per step s:
//   pick_accumulate  thread per (luma j, chroma k) pair, workgroup per (slice of filter blocks, 256 pairs): sums
//                    min(best of the levels already chosen, cost0[fb][j] + cost1[fb][k]) over its slice on chip, then ONE
//                    64-bit atomic add per pair into tot[width][j][k]
//   pick_select      workgroup per width: smallest (total, pair number) below 1 << 63 -> the level list's next slot; shifts
//                    the list when the next step is a refinement step; clears the totals it has read
//   pick_finish      RD choice over the four widths, per-block index, the map through strengths[], the result record
//
// Every sum is a uint64 sum modulo 2^64 of the same terms as the reference's, so the order in which workgroups add does not
// matter and every run gives the same bits.  Steps are ordered by the stream alone: no workgroup waits for another.
#include "common.hpp"
#include "../../include/svt_hip_lf.h"

using namespace svthip;

namespace {

constexpr int      MAXN      = SVT_HIP_CDEF_MAX_STRENGTHS;
constexpr int      WIDTHS    = 4;   // signalling widths: cdef_bits 0..3
constexpr int      MAX_LEV   = 8;   // CDEF_MAX_STRENGTHS
constexpr int      TILE      = 16;  // filter blocks staged in LDS at a time
constexpr uint64_t HUGE_MSE  = 1ull << 63;
constexpr uint64_t DEFAULT_UV = (uint64_t)1040400 * 64;  // default_mse_uv * 64 (cdef_process.c:78, :251)

// Workspace: [lev: int32 [4][2][8]] [joint: uint64 [4]] ... 512 bytes, then tot [4][n*n], cost [2][n_fb][n], part [n_fb].
constexpr size_t WS_LEV = 0, WS_JOINT = 256, WS_TOT = 512;
struct Workspace {
    int32_t  *lev;    // [width][luma / chroma][slot]
    uint64_t *joint;  // [width]: return value of the width's latest svt_search_one_dual
    uint64_t *tot;    // [width][j * n + k]
    uint64_t *cost;   // [luma / chroma][fb][gi]
    uint8_t  *part;   // [fb]: 1 = the filter block takes part
};
size_t ws_bytes(size_t n_fb, size_t n) { return up256(WS_TOT + (size_t)WIDTHS * n * n * 8 + 2 * n_fb * n * 8 + n_fb); }
Workspace ws_carve(void *base, size_t n_fb, size_t n) {
    uint8_t *b = (uint8_t *)base;
    Workspace w;
    w.lev = (int32_t *)(b + WS_LEV), w.joint = (uint64_t *)(b + WS_JOINT), w.tot = (uint64_t *)(b + WS_TOT);
    w.cost = w.tot + (size_t)WIDTHS * n * n, w.part = (uint8_t *)(w.cost + 2 * n_fb * n);
    return w;
}

struct Lists {  // what the kernels read of SvtHipCdefPickParams
    int8_t y[MAXN], uv[MAXN];
};

__device__ __forceinline__ int steps_of(int width) { return 5 << width; }
// number of levels already chosen when step s of `width` searches: s while greedy, all but the last slot while refining
__device__ __forceinline__ int chosen_at(int width, int s) { return s < (1 << width) ? s : (1 << width) - 1; }

__global__ __launch_bounds__(256) void pick_prepare(const uint64_t *__restrict__ mse, const uint8_t *__restrict__ filt, Lists lists, int n,
                                                    int n_fb, int fb_cols, uint32_t w8, uint32_t h8, uint32_t bias, Workspace ws) {
    const int tid = blockIdx.x * 256 + threadIdx.x, nthreads = gridDim.x * 256;
    for (int i = tid; i < WIDTHS * n * n; i += nthreads) ws.tot[i] = 0;
    for (int i = tid; i < WIDTHS * 2 * MAX_LEV; i += nthreads) ws.lev[i] = 0;
    for (int i = tid; i < WIDTHS; i += nthreads) ws.joint[i] = HUGE_MSE;
    const int fb = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // one wave per filter block
    if (fb >= n_fb)
        return;
    const uint32_t r = (uint32_t)(fb / fb_cols) * 8 + (lane >> 3), c = (uint32_t)(fb % fb_cols) * 8 + (lane & 7);
    const bool     filtered = r < h8 && c < w8 && filt[(size_t)r * w8 + c] != 0;
    const bool     part = __ballot(filtered) != 0;
    if (lane == 0)
        ws.part[fb] = part;
    if (lane < n) {
        const size_t at = (size_t)fb * n + lane, plane = (size_t)n_fb * n;
        uint64_t     y = mse[at], uv = lists.uv[lane] == -1 ? DEFAULT_UV : mse[plane + at] + mse[2 * plane + at];
        if (bias && lane == 0)
            y = ((uint64_t)bias * y) >> 6, uv = ((uint64_t)bias * uv) >> 6;
        ws.cost[at] = y, ws.cost[plane + at] = uv;
    }
}

// grid (pair chunks * slices, widths that still have step s); slice_len is a multiple of TILE
__global__ __launch_bounds__(256) void pick_accumulate(Workspace ws, int n, int n_fb, int s, int first_width, int n_chunks, int slice_len) {
    __shared__ uint64_t s_c0[TILE * MAXN], s_c1[TILE * MAXN], s_best[TILE];
    __shared__ int32_t  s_lev[2 * MAX_LEV];
    const int width = first_width + blockIdx.y, nb = chosen_at(width, s);
    const int chunk = blockIdx.x % n_chunks, slice = blockIdx.x / n_chunks;
    const int pair = chunk * 256 + threadIdx.x, j = pair / n, k = pair % n;
    const bool live = pair < n * n;
    if (threadIdx.x < 2 * MAX_LEV)
        s_lev[threadIdx.x] = ws.lev[width * 2 * MAX_LEV + threadIdx.x];
    const uint64_t *c0 = ws.cost, *c1 = ws.cost + (size_t)n_fb * n;
    const int       fb_end = min(n_fb, (slice + 1) * slice_len);
    uint64_t        acc = 0;
    for (int fb0 = slice * slice_len; fb0 < fb_end; fb0 += TILE) {
        __syncthreads();  // the previous tile has been read (first pass: s_lev is written)
        const int have = min(TILE, n_fb - fb0) * n;
        for (int i = threadIdx.x; i < TILE * n; i += 256) {
            const bool in = i < have;
            s_c0[i] = in ? c0[(size_t)fb0 * n + i] : 0, s_c1[i] = in ? c1[(size_t)fb0 * n + i] : 0;
        }
        __syncthreads();
        if (threadIdx.x < TILE) {
            // a block that takes no part (or lies past the grid) adds min(0, anything) = 0 to every total
            const int fb = fb0 + threadIdx.x;
            uint64_t  best = fb < n_fb && ws.part[fb] ? HUGE_MSE : 0;
            for (int gi = 0; gi < nb; gi++) {
                const uint64_t cur = s_c0[threadIdx.x * n + s_lev[gi]] + s_c1[threadIdx.x * n + s_lev[MAX_LEV + gi]];
                best = cur < best ? cur : best;
            }
            s_best[threadIdx.x] = best;
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int b = 0; b < TILE; b++) {
                const uint64_t cur = s_c0[b * n + j] + s_c1[b * n + k], best = s_best[b];
                acc += cur < best ? cur : best;
            }
        }
    }
    if (live)
        atomicAdd((unsigned long long *)&ws.tot[(size_t)width * n * n + pair], (unsigned long long)acc);
}

// grid (widths that still have step s)
__global__ __launch_bounds__(256) void pick_select(Workspace ws, int n, int s, int first_width) {
    __shared__ uint64_t s_tot[256];
    __shared__ uint32_t s_id[256];
    const int width = first_width + blockIdx.x, pairs = n * n;
    uint64_t *tot = ws.tot + (size_t)width * pairs;
    uint64_t  best = HUGE_MSE;
    uint32_t  best_id = 0;  // nothing below 1 << 63: the reference keeps (0, 0)
    for (int p = threadIdx.x; p < pairs; p += 256) {  // a thread sees its pairs in increasing order
        const uint64_t t = tot[p];
        tot[p] = 0;
        if (t < best)
            best = t, best_id = (uint32_t)p;
    }
    s_tot[threadIdx.x] = best, s_id[threadIdx.x] = best_id;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const uint64_t t = s_tot[threadIdx.x + off];
            const uint32_t d = s_id[threadIdx.x + off];
            if (t < s_tot[threadIdx.x] || (t == s_tot[threadIdx.x] && d < s_id[threadIdx.x]))
                s_tot[threadIdx.x] = t, s_id[threadIdx.x] = d;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int32_t  *l0 = ws.lev + width * 2 * MAX_LEV, *l1 = l0 + MAX_LEV;
        const int nbs = 1 << width, slot = chosen_at(width, s);
        l0[slot] = (int32_t)(s_id[0] / (uint32_t)n), l1[slot] = (int32_t)(s_id[0] % (uint32_t)n);
        ws.joint[width] = s_tot[0];
        if (s + 1 >= nbs && s + 1 < steps_of(width))  // the next step refines: drop the oldest level (:719-723)
            for (int g = 0; g < nbs - 1; g++) l0[g] = l0[g + 1], l1[g] = l1[g + 1];
    }
}

__global__ __launch_bounds__(256) void pick_finish(Workspace ws, Lists lists, int n, int n_fb, uint64_t lambda, SvtHipCdefPickResult *__restrict__ res,
                                                   uint8_t *__restrict__ fb_gi, uint8_t *__restrict__ fb_strength) {
    __shared__ int      s_count, s_bits;
    __shared__ int32_t  s_lev[2 * MAX_LEV];
    __shared__ uint64_t s_rd[WIDTHS];
    if (threadIdx.x == 0)
        s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n_fb; i += 256) mine += ws.part[i];
    if (mine)
        atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t best = HUGE_MSE;
        int      bits = 0;
        for (int i = 0; i < WIDTHS; i++) {
            const int32_t  total_bits = s_count * i + (1 << i) * 6 * 2;   // CDEF_STRENGTH_BITS * 2 per pair
            const uint64_t rate = (uint64_t)(int64_t)(total_bits * 512);  // av1_cost_literal
            const uint64_t dist = ws.joint[i] * 16;
            const uint64_t rd   = (uint64_t)((int64_t)(rate * lambda + 256) >> 9) + (dist << 7);  // RDCOST (rd_cost.h:37-39)
            s_rd[i] = rd;
            if (rd < best)
                best = rd, bits = i;
        }
        s_bits = bits;
    }
    __syncthreads();
    const int bits = s_bits, nbs = 1 << bits;
    if (threadIdx.x < 2 * MAX_LEV)
        s_lev[threadIdx.x] = (threadIdx.x & (MAX_LEV - 1)) < nbs ? ws.lev[bits * 2 * MAX_LEV + threadIdx.x] : 0;
    __syncthreads();
    const int fb = blockIdx.x * 256 + threadIdx.x;
    if (fb < n_fb) {
        uint8_t gi_out = 0xFF, y = 0, uv = 0;
        if (ws.part[fb]) {
            const uint64_t *c0 = ws.cost + (size_t)fb * n, *c1 = ws.cost + ((size_t)n_fb + fb) * n;
            uint64_t        best = HUGE_MSE;
            int             best_gi = 0;
            for (int gi = 0; gi < nbs; gi++) {
                const uint64_t cur = c0[s_lev[gi]] + c1[s_lev[MAX_LEV + gi]];
                if (cur < best)
                    best = cur, best_gi = gi;
            }
            gi_out = (uint8_t)best_gi;
            y = (uint8_t)lists.y[s_lev[best_gi]], uv = (uint8_t)lists.y[s_lev[MAX_LEV + best_gi]];  // filter_map: the luma list for both
        }
        fb_gi[fb] = gi_out, fb_strength[fb] = y, fb_strength[n_fb + fb] = uv;
    }
    if (blockIdx.x == 0 && threadIdx.x < MAX_LEV) {
        const int g = threadIdx.x;
        res->y_index[g] = s_lev[g], res->uv_index[g] = s_lev[MAX_LEV + g];
        res->y_strength[g]  = g < nbs ? (uint8_t)lists.y[s_lev[g]] : 0;
        res->uv_strength[g] = g < nbs ? (uint8_t)lists.y[s_lev[MAX_LEV + g]] : 0;
        for (int i = 0; i < WIDTHS; i++) {
            const bool used = g < (1 << i);
            res->lev0[i][g] = used ? ws.lev[i * 2 * MAX_LEV + g] : 0, res->lev1[i][g] = used ? ws.lev[i * 2 * MAX_LEV + MAX_LEV + g] : 0;
        }
        if (g < WIDTHS)
            res->joint_mse[g] = ws.joint[g], res->rd_cost[g] = s_rd[g];
        if (g == 0)
            res->cdef_bits = bits, res->nb_strengths = nbs, res->sb_count = s_count, res->pad_ = 0, res->best_cost = s_rd[bits];
    }
}

}  // namespace

extern "C" uint64_t svt_hip_cdef_pick_workspace_bytes(uint32_t n_fb, int32_t n_strengths) {
    if (n_fb == 0 || n_strengths < 1)
        return 0;
    return ws_bytes(n_fb, (size_t)(n_strengths > MAXN ? MAXN : n_strengths));
}

extern "C" int32_t svt_hip_cdef_pick_strengths(const SvtHipCdefPickParams *prm, const uint64_t *d_mse, const uint8_t *d_filt8x8,
                                               SvtHipCdefPickResult *d_result, uint8_t *d_fb_gi, uint8_t *d_fb_strength, void *d_workspace,
                                               uint64_t workspace_bytes, void *stream) {
    if (!prm || !d_mse || !d_filt8x8 || !d_result || !d_fb_gi || !d_fb_strength || !d_workspace)
        return refuse("svt_hip_cdef_pick_strengths: NULL argument");
    const int n = prm->n_strengths;
    if (n < 1 || n > MAXN)
        return refuse("svt_hip_cdef_pick_strengths: n_strengths %d outside 1..%d", n, MAXN);
    Lists lists{};
    for (int gi = 0; gi < n; gi++) {
        if (prm->strengths[gi] < 0 || prm->strengths[gi] > 63 || prm->strengths_uv[gi] < -1 || prm->strengths_uv[gi] > 63)
            return refuse("svt_hip_cdef_pick_strengths: strengths[%d] = %d (0..63) / strengths_uv[%d] = %d (-1..63) out of range", gi,
                                prm->strengths[gi], gi, prm->strengths_uv[gi]);
        lists.y[gi] = prm->strengths[gi], lists.uv[gi] = prm->strengths_uv[gi];
    }
    const uint64_t n_fb64 = (uint64_t)prm->fb_cols * prm->fb_rows;
    if (n_fb64 == 0 || n_fb64 > (1u << 24))
        return refuse("svt_hip_cdef_pick_strengths: filter-block grid %u x %u is empty or too large", prm->fb_cols, prm->fb_rows);
    if (((uint64_t)prm->w8 + 7) / 8 < prm->fb_cols || ((uint64_t)prm->h8 + 7) / 8 < prm->fb_rows)
        return refuse("svt_hip_cdef_pick_strengths: filt8x8 of %u x %u does not reach every one of the %u x %u filter blocks", prm->w8, prm->h8,
                            prm->fb_cols, prm->fb_rows);
    const int n_fb = (int)n_fb64;
    if (workspace_bytes < ws_bytes(n_fb, n) || ((uintptr_t)d_workspace & 7) || ((uintptr_t)d_result & 7))
        return refuse("svt_hip_cdef_pick_strengths: workspace of %llu bytes, %llu needed (workspace and result 8-byte aligned)",
                            (unsigned long long)workspace_bytes, (unsigned long long)ws_bytes(n_fb, n));
    TierBCall c("svt_hip_cdef_pick_strengths", stream);
    if (!c.ok())
        return c.status();
    hipStream_t     st = c.stream();
    const Workspace ws = ws_carve(d_workspace, n_fb, n);
    // slices of filter blocks: enough workgroups to fill the device a few times over, no more atomics than that needs
    const int n_chunks = (n * n + 255) / 256, tiles = (n_fb + TILE - 1) / TILE;
    const int want     = (8 * cu_count() + WIDTHS * n_chunks - 1) / (WIDTHS * n_chunks);
    const int slices0  = want < 1 ? 1 : (want > tiles ? tiles : want);
    const int slice_len = (tiles + slices0 - 1) / slices0 * TILE, slices = (n_fb + slice_len - 1) / slice_len;
    hipLaunchKernelGGL(pick_prepare, dim3((n_fb + 3) / 4), dim3(256), 0, st, d_mse, d_filt8x8, lists, n, n_fb, (int)prm->fb_cols, prm->w8, prm->h8,
                       (uint32_t)prm->zero_fs_cost_bias, ws);
    for (int s = 0; s < (5 << (WIDTHS - 1)); s++) {
        int first = 0;  // narrower widths have finished their 5 << width steps
        while ((5 << first) <= s) first++;
        hipLaunchKernelGGL(pick_accumulate, dim3(n_chunks * slices, WIDTHS - first), dim3(256), 0, st, ws, n, n_fb, s, first, n_chunks, slice_len);
        hipLaunchKernelGGL(pick_select, dim3(WIDTHS - first), dim3(256), 0, st, ws, n, s, first);
    }
    hipLaunchKernelGGL(pick_finish, dim3((n_fb + 255) / 256), dim3(256), 0, st, ws, lists, n, n_fb, (uint64_t)prm->lambda, d_result, d_fb_gi,
                       d_fb_strength);
    return c.finish();
}

SVT_HIP_MODULE_WARMUP(loopfilter_cdef_pick)
