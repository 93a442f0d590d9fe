// intra_palette.hip — the luma palette of mode decision on device-resident planes (include/svt_hip_intra.h): search_palette_luma
// (palette.c:309-434) with the rate terms of av1_intra_fast_cost (rd_cost.c:691-704), the palette branch of
// svt_av1_predict_intra_block[_16bit], and svt_aom_is_screen_content.  Integer arithmetic throughout.
//
//   palette_search_kernel   one workgroup of four waves per block.  The in-bounds pixels are read once into LDS (the `data` raster of the
//                           reference) and counted into an LDS histogram; wave 0 compacts the histogram into at most 64 (value, count)
//                           pairs in ascending value order, one per lane.  Everything k-means does per pixel depends on the pixel's
//                           value alone, so a run works on one pair per lane: assignment per lane, the count-weighted sums, counts and
//                           the int64 distance by wave reductions, the previous indices in a register.  Only the refill of an empty
//                           cluster looks a pixel up in the raster.  The 7 + 7 candidates are independent: the waves take them in turn,
//                           the centroids of a wave live in LDS and every lane executes the short serial steps (snap, sort, duplicates)
//                           on them with the same values.  Thread 0 then applies the slot rule; for every kept candidate the workgroup
//                           fills a value -> index table, writes the extended map from it (LDS, then dwords to memory) and sums
//                           the colour-index costs over the in-bounds positions, each of which is independent once the map exists.
//                           The record is composed in LDS and stored whole.
//   palette_predict_kernel  one workgroup per transform block: dst = palette[map]
//   sc_classify_kernel      one wave per eight whole 16 x 16 blocks: the colours of a block as a 256-bit set, sum and sum of squares against
//                           128; integer atomics on the record, and the wave that takes the last ticket derives the four classes
#include "../../include/svt_hip_intra.h"
#include "common.hpp"

using namespace svthip;

namespace {

constexpr int MAX_SIZE = SVT_HIP_PALETTE_MAX_SIZE, MAX_CANDS = SVT_HIP_PALETTE_MAX_CANDS, MAX_COLORS = 64, MAX_PX = 64 * 64;
constexpr int JOBS = 14, COST_SHIFT = 9;  // 7 dominant-colour + 7 k-means candidates; AV1_PROB_COST_SHIFT

struct SearchArgs {
    const SvtHipPaletteDesc  *desc;  // device copy of the caller's array
    const SvtHipPaletteRates *rates;
    uint32_t                  step, bit_depth, max_itr, pad_;
};

__device__ inline int wave_sum(int v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline long long wave_sum64(long long v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline unsigned wave_max(unsigned v) {
    for (int o = 32; o; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}

// svt_av1_calc_indices_dim1 for one value: the first of the nearest centroids
__device__ inline int nearest(int v, const int *cen, int k) {
    int best = 0, best_d = (v - cen[0]) * (v - cen[0]);
    for (int j = 1; j < k; j++) {
        const int d = (v - cen[j]) * (v - cen[j]);
        if (d < best_d)
            best_d = d, best = j;
    }
    return best;
}

__device__ inline long long total_dist(int v, int cnt, const int *cen, int idx) {
    const int d = v - cen[idx];
    return wave_sum64((long long)cnt * (d * d));
}

// svt_av1_k_means_dim1_c on the (value, count) pair of each lane; cen and pre are the wave's own, written by every lane alike.
// data: the raster of the n_px in-bounds pixels.
__device__ inline void k_means(int v, int cnt, int *cen, int *pre, int k, int max_itr, const uint16_t *data, int n_px) {
    int       idx  = nearest(v, cen, k);
    long long dist = total_dist(v, cnt, cen, idx);
    for (int it = 0; it < max_itr; it++) {
        const long long pre_dist = dist;
        const int       pre_idx  = idx;
        for (int j = 0; j < k; j++) pre[j] = cen[j];
        unsigned state = data[0];  // calc_centroids seeds it anew at every update
        for (int j = 0; j < k; j++) {
            const int in = idx == j, count = wave_sum(in ? cnt : 0), sum = wave_sum(in ? cnt * v : 0);
            if (count == 0) {
                state  = state * 1103515245u + 12345u;
                cen[j] = data[(state / 65536 % 32768) % (unsigned)n_px];
            } else
                cen[j] = (sum + (count >> 1)) / count;
        }
        idx  = nearest(v, cen, k);
        dist = total_dist(v, cnt, cen, idx);
        if (dist > pre_dist) {  // never taken in one dimension; restated all the same
            for (int j = 0; j < k; j++) cen[j] = pre[j];
            idx = pre_idx;
            break;
        }
        bool same = true;
        for (int j = 0; j < k; j++) same &= cen[j] == pre[j];
        if (same)
            break;
    }
}

// The front of palette_rd_y: optimize_palette_colors, then av1_remove_duplicates.  Returns the number of colours left in cen.
__device__ inline int snap_sort_unique(int *cen, int n, const uint16_t *cache, int n_cache) {
    if (n_cache > 0)
        for (int i = 0; i < n; i++) {
            int min_diff = abs(cen[i] - (int)cache[0]), at = 0;
            for (int j = 1; j < n_cache; j++) {
                const int diff = abs(cen[i] - (int)cache[j]);
                if (diff < min_diff)
                    min_diff = diff, at = j;
            }
            if (min_diff <= 1)
                cen[i] = cache[at];
        }
    for (int i = 1; i < n; i++) {  // ascending; the order of equal values cannot be seen
        const int c = cen[i];
        int       j = i;
        for (; j > 0 && cen[j - 1] > c; j--) cen[j] = cen[j - 1];
        cen[j] = c;
    }
    int k = 1;
    for (int i = 1; i < n; i++)
        if (cen[i] != cen[i - 1])
            cen[k++] = cen[i];
    return k;
}

__device__ inline int ceil_log2(int n) { return n < 2 ? 0 : 32 - __clz(n - 1); }

// svt_av1_palette_color_cost_y: the colours the cache does not hold are delta coded (delta_encode_cost with min_val 1)
__device__ inline int color_cost_y(const uint16_t *colors, int k, const uint16_t *cache, int n_cache, int bit_depth) {
    unsigned in_cache = 0;  // bit j: colors[j] is in the cache
    int      n_in     = 0;
    for (int i = 0; i < n_cache && n_in < k; i++)
        for (int j = 0; j < k; j++)
            if (colors[j] == cache[i]) {
                in_cache |= 1u << j, n_in++;
                break;
            }
    const int num  = k - __popc(in_cache);
    int       bits = 0;
    if (num > 0) {
        bits = bit_depth;
        if (num > 1) {
            bits += 2;
            int first = -1, prev = -1, max_delta = 0;
            for (int j = 0; j < k; j++)
                if (!((in_cache >> j) & 1)) {
                    if (prev < 0)
                        first = colors[j];
                    else
                        max_delta = max(max_delta, (int)colors[j] - prev);
                    prev = colors[j];
                }
            int per_delta = max(ceil_log2(max_delta), bit_depth - 3), range = (1 << bit_depth) - first - 1;
            prev          = -1;
            for (int j = 0; j < k; j++)
                if (!((in_cache >> j) & 1)) {
                    if (prev >= 0) {
                        bits += per_delta;
                        range -= (int)colors[j] - prev;
                        per_delta = min(per_delta, ceil_log2(range));
                    }
                    prev = colors[j];
                }
        }
    }
    return (n_cache + bits) << COST_SHIFT;
}

// svt_aom_get_palette_color_index_context_optimized at (r, c) != (0, 0) of a map of stride `stride`: ctx * 8 + the re-ordered index
__device__ inline int color_context(const uint8_t *map, int stride, int r, int c) {
    int nb[3] = {c > 0 ? map[r * stride + c - 1] : -1, r > 0 ? map[(r - 1) * stride + c] : -1, c > 0 && r > 0 ? map[(r - 1) * stride + c - 1] : -1};
    int sc[3] = {2, 2, 1};  // left, top, top-left
    if (nb[0] == nb[1]) {
        sc[0] += sc[1], nb[1] = -1;
        if (nb[0] == nb[2])
            sc[0] += sc[2], nb[2] = -1;
    } else if (nb[0] == nb[2])
        sc[0] += sc[2], nb[2] = -1;
    else if (nb[1] == nb[2])
        sc[1] += sc[2], nb[2] = -1;
    int col[3] = {-1, -1, -1}, scr[3] = {0, 0, 0}, valid = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (nb[i] != -1) {  // valid is at most i: a chain of selects, no indexing by a variable
            if (valid == 0)
                col[0] = nb[i], scr[0] = sc[i];
            else if (valid == 1)
                col[1] = nb[i], scr[1] = sc[i];
            else
                col[2] = nb[i], scr[2] = sc[i];
            valid++;
        }
    int t;
#define SWAP_RANK(a, b) (t = scr[a], scr[a] = scr[b], scr[b] = t, t = col[a], col[a] = col[b], col[b] = t)
    if (scr[0] < scr[1] || (scr[0] == scr[1] && col[0] > col[1]))
        SWAP_RANK(0, 1);
    if (scr[0] < scr[2])
        SWAP_RANK(0, 2);
    if (scr[1] < scr[2])
        SWAP_RANK(1, 2);
#undef SWAP_RANK
    const int cur = map[r * stride + c];
    int       idx = cur, same = -1;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (col[i] > cur)
            idx++;
        else if (col[i] == cur)
            same = i;
    }
    if (same != -1)
        idx = same;
    // hash 1 * first + 2 * second + 2 * third: 2 -> 0, 5 -> 4, 6 -> 3, 7 -> 2, 8 -> 1
    const int hash = scr[0] + 2 * scr[1] + 2 * scr[2];
    const int ctx  = hash == 2 ? 0 : 9 - hash;
    return ctx * 8 + idx;
}

__global__ __launch_bounds__(256) void palette_search_kernel(const SearchArgs args) {
    __shared__ SvtHipPaletteRecord s_rec;
    __shared__ uint16_t            s_data[MAX_PX];
    __shared__ uint32_t            s_hist[1024];
    __shared__ __attribute__((aligned(4))) uint8_t s_map[MAX_PX];
    __shared__ uint8_t             s_lut[1024];
    __shared__ int                 s_val[MAX_COLORS], s_cnt[MAX_COLORS], s_top[MAX_SIZE], s_cen[4][MAX_SIZE], s_pre[4][MAX_SIZE];
    __shared__ int                 s_jk[JOBS], s_jn[JOBS], s_jcol[JOBS][MAX_SIZE], s_keep[MAX_CANDS], s_cost[5 * 8];
    __shared__ int                 s_colors, s_bad, s_nkeep, s_sum;

    const SvtHipPaletteDesc &d = args.desc[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = d.width, h = d.height, rows = d.rows, cols = d.cols, n_px = rows * cols, bd = (int)args.bit_depth, bins = 1 << bd;

    for (int i = tid; i < (int)(sizeof(s_rec) / 4); i += 256) ((uint32_t *)&s_rec)[i] = 0;
    for (int i = tid; i < bins; i += 256) s_hist[i] = 0;
    if (tid == 0)
        s_bad = 0, s_sum = 0;
    __syncthreads();

    // the pixels, once: the raster and the histogram
    for (int p = tid; p < n_px; p += 256) {
        const int    r = p / cols, c = p % cols;
        const size_t at = (size_t)(d.org_y + r) * d.stride + d.org_x + c;
        int          v  = bd == 8 ? ((const uint8_t *)d.src)[at] : ((const uint16_t *)d.src)[at];
        if (v >= bins)  // svt_av1_count_colors_highbd gives up: no colours
            s_bad = 1, v = 0;
        s_data[p] = (uint16_t)v;
        atomicAdd(&s_hist[v], 1u);
    }
    __syncthreads();

    if (wave == 0) {  // the distinct values in ascending order, the first 64 of them kept
        int base = 0;
        for (int b0 = 0; b0 < bins; b0 += 64) {
            const uint32_t           n    = s_hist[b0 + lane];
            const unsigned long long mask = __ballot(n > 0);
            const int                at   = base + __popcll(mask & ((1ull << lane) - 1));
            if (n > 0 && at < MAX_COLORS)
                s_val[at] = b0 + lane, s_cnt[at] = (int)n;
            base += __popcll(mask);
        }
        if (lane == 0)
            s_colors = base;
    } else if (tid == 64) {  // svt_get_palette_cache_y: the two ascending lists merged, a value that equals the last one added dropped
        int a = 0, l = 0, n = 0, an = d.above_n, ln = d.left_n;
        while (a < an || l < ln) {
            uint16_t v;
            if (a < an && l < ln) {
                const uint16_t va = d.above[a], vl = d.left[l];
                if (vl < va)
                    v = vl, l++;
                else {
                    v = va, a++;
                    if (vl == va)
                        l++;
                }
            } else if (a < an)
                v = d.above[a++];
            else
                v = d.left[l++];
            if (!(n > 0 && v == s_rec.cache[n - 1]))
                s_rec.cache[n++] = v;
        }
        s_rec.n_cache = (uint8_t)n;
    }
    __syncthreads();

    const int colors  = s_bad ? 0 : s_colors;
    const int n_cache = s_rec.n_cache;
    if (colors > 1 && colors <= MAX_COLORS) {  // block-uniform
        const int v = lane < colors ? s_val[lane] : 0, cnt = lane < colors ? s_cnt[lane] : 0;
        if (wave == 0) {  // the most frequent values; the lowest value among equal counts
            int left = cnt;
            for (int i = 0; i < min(colors, MAX_SIZE); i++) {
                const unsigned key = wave_max(((unsigned)left << 6) | (unsigned)(63 - lane));
                const int      win = 63 - (int)(key & 63);
                if (lane == win)
                    s_top[i] = v, left = 0;
            }
        }
        __syncthreads();

        const int n_max = min(colors, MAX_SIZE);
        int      *cen = s_cen[wave], *pre = s_pre[wave];
        for (int job = wave; job < JOBS; job += 4) {  // wave-uniform from here to the barrier
            const int k_means_job = job >= 7;
            const int n           = k_means_job ? n_max - (job - 7) : n_max - job * (int)args.step;
            int       k           = 0;
            if (n >= 2) {
                if (!k_means_job)
                    for (int i = 0; i < n; i++) cen[i] = s_top[i];
                else if (colors == 2)
                    cen[0] = s_val[0], cen[1] = s_val[colors - 1];
                else {
                    const int lb = s_val[0], ub = s_val[colors - 1];
                    for (int i = 0; i < n; i++) cen[i] = lb + (2 * i + 1) * (ub - lb) / n / 2;
                    k_means(v, cnt, cen, pre, n, (int)args.max_itr, s_data, n_px);
                }
                k = snap_sort_unique(cen, n, s_rec.cache, n_cache);
                for (int i = 0; i < k; i++) s_jcol[job][i] = cen[i];
            }
            s_jk[job] = k, s_jn[job] = n;
        }
        __syncthreads();

        if (tid == 0) {  // a candidate keeps its slot only with more than 2 colours; the order is dominant first, n descending
            int kept = 0;
            for (int job = 0; job < JOBS; job++)
                if (s_jk[job] > 2)
                    s_keep[kept++] = job;
            s_nkeep = kept;
        }
        __syncthreads();

        const int n_keep = s_nkeep, bsize_ctx = (31 - __clz(w)) + (31 - __clz(h)) - 6;
        for (int s = 0; s < n_keep; s++) {
            const int  job = s_keep[s], k = s_jk[job];
            const int *col = s_jcol[job];
            if (tid < colors)
                s_lut[s_val[tid]] = (uint8_t)nearest(s_val[tid], col, k);
            if (tid < 40)
                s_cost[tid] = args.rates->palette_ycolor_fac_bitss[k - 2][tid >> 3][tid & 7];
            __syncthreads();
            for (int p = tid; p < w * h; p += 256) {  // extend_palette_color_map: the last valid column and row repeat
                const int r = min(p / w, rows - 1), c = min(p % w, cols - 1);
                s_map[p]    = s_lut[s_data[r * cols + c]];
            }
            __syncthreads();
            uint32_t *out = (uint32_t *)(d.maps + (size_t)s * w * h);
            for (int q = tid; q < w * h / 4; q += 256) out[q] = ((const uint32_t *)s_map)[q];
            int bits = 0;
            for (int p = tid + 1; p < n_px; p += 256) bits += s_cost[color_context(s_map, w, p / cols, p % cols)];
            bits = wave_sum(bits);
            if (lane == 0)
                atomicAdd(&s_sum, bits);
            __syncthreads();
            if (tid == 0) {
                SvtHipPaletteCand &cand = s_rec.cand[s];
                cand.origin = job >= 7 ? SVT_HIP_PALETTE_KMEANS : SVT_HIP_PALETTE_DOMINANT, cand.n = (uint8_t)s_jn[job], cand.palette_size = (uint8_t)k;
                for (int i = 0; i < k; i++) cand.palette_colors[i] = (uint16_t)min(max(col[i], 0), bins - 1);
                const int l = 32 - __clz(k), m = (1 << l) - k;  // svt_aom_write_uniform_cost(k, map[0])
                cand.size_bits  = args.rates->palette_ysize_fac_bits[bsize_ctx][k - 2] + ((s_map[0] < m ? l - 1 : l) << COST_SHIFT);
                cand.color_bits = color_cost_y(cand.palette_colors, k, s_rec.cache, n_cache, bd);
                cand.map_bits   = s_sum;
                s_sum           = 0;
            }
            __syncthreads();  // s_cost, s_lut and s_map are rewritten in the next round
        }
        if (tid == 0)
            s_rec.n_cands = (uint8_t)n_keep;
    }
    if (tid == 0)
        s_rec.colors = (uint16_t)colors;
    __syncthreads();
    for (int i = tid; i < (int)(sizeof(s_rec) / 4); i += 256) ((uint32_t *)d.record)[i] = ((const uint32_t *)&s_rec)[i];
}

__global__ __launch_bounds__(256) void palette_predict_kernel(const SvtHipPalettePredDesc *__restrict__ desc, uint32_t n) {
    if (blockIdx.x >= n)
        return;
    const SvtHipPalettePredDesc d = desc[blockIdx.x];
    const int                   bd = d.bit_depth;
    if (!d.map || !d.colors || !d.dst || !d.w || !d.h || (int)d.x + d.w > (int)d.map_width || (bd != 8 && bd != 10) || (!d.is_16bit && bd != 8) ||
        d.is_16bit > 1 || (d.is_16bit && ((uintptr_t)d.dst & 1)) || ((uintptr_t)d.colors & 1))
        return;
    __shared__ uint16_t pal[MAX_SIZE];
    if (threadIdx.x < MAX_SIZE)
        pal[threadIdx.x] = (uint16_t)min((int)d.colors[threadIdx.x], (1 << bd) - 1);
    __syncthreads();
    for (int p = threadIdx.x; p < d.w * d.h; p += 256) {
        const int      r = p / d.w, c = p % d.w;
        const uint16_t v = pal[d.map[(size_t)(r + d.y) * d.map_width + c + d.x] & 7];
        if (d.is_16bit)
            ((uint16_t *)d.dst)[(size_t)r * d.dst_stride + c] = v;
        else
            ((uint8_t *)d.dst)[(size_t)r * d.dst_stride + c] = (uint8_t)v;
    }
}

constexpr uint32_t SC_PER_WAVE = 8;  // 16 x 16 blocks a wave counts before it touches the record: three atomics per eight blocks

__global__ __launch_bounds__(64) void sc_classify_kernel(const uint8_t *__restrict__ plane, uint32_t width, uint32_t height, uint32_t stride, uint32_t bx,
                                                         uint32_t blocks, SvtHipScClass *__restrict__ out) {
    const int      lane = threadIdx.x;
    const uint32_t end = min(blocks, (blockIdx.x + 1) * SC_PER_WAVE);
    uint32_t       counts_1 = 0, counts_2 = 0;
    for (uint32_t b = blockIdx.x * SC_PER_WAVE; b < end; b++) {
        const uint32_t     x0 = (b % bx) * 16 + (lane & 3) * 4, y0 = (b / bx) * 16 + (lane >> 2);
        const uint8_t     *p  = plane + (size_t)y0 * stride + x0;
        unsigned long long set[4] = {0, 0, 0, 0};  // the block's colours: bit v % 64 of set[v / 64]
        int                sum = 0, sse = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int v = p[i], dv = v - 128;
            sum += dv, sse += dv * dv;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if ((v >> 6) == q)
                    set[q] |= 1ull << (v & 63);
        }
        int nb_colors = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            for (int o = 32; o; o >>= 1) set[q] |= __shfl_xor(set[q], o);
            nb_colors += __popcll(set[q]);
        }
        sum = wave_sum(sum), sse = wave_sum(sse);
        if (nb_colors > 1 && nb_colors <= 4) {  // is_valid_palette_nb_colors
            // svt_aom_variance16x16 against 128, then ROUND_POWER_OF_TWO(var, 8) > 0
            const uint32_t var = (uint32_t)sse - (uint32_t)(((long long)sum * sum) >> 8);
            counts_1++, counts_2 += ((var + 128) >> 8) > 0;
        }
    }
    if (lane == 0) {
        if (counts_1)
            atomicAdd(&out->counts_1, counts_1);
        if (counts_2)
            atomicAdd(&out->counts_2, counts_2);
        __threadfence();
        const uint32_t ticket = atomicAdd(&out->pad_[0], 1u);
        if (ticket == gridDim.x - 1) {  // every other wave has added its blocks
            __threadfence();
            const int c1 = (int)atomicAdd(&out->counts_1, 0u), c2 = (int)atomicAdd(&out->counts_2, 0u), area = (int)(width * height);
            const int cls0 = c1 * 256 * 10 > area, cls1 = cls0 && c2 * 256 * 12 > area;
            out->sc_class[0] = (uint8_t)cls0, out->sc_class[1] = (uint8_t)cls1;
            out->sc_class[2] = (uint8_t)(cls1 || (c1 * 256 * 10 > area * 4 && c2 * 256 * 30 > area));
            out->sc_class[3] = (uint8_t)(cls1 || (c1 * 256 * 8 > area && c2 * 256 * 50 > area));
            out->blocks = blocks, out->pad_[0] = 0;
        }
    }
}

uint64_t widen(int32_t status) { return SVT_HIP_PALETTE_STATUS(status); }

bool pow2_8_64(uint32_t v) { return v == 8 || v == 16 || v == 32 || v == 64; }

}  // namespace

extern "C" uint64_t svt_hip_palette_search_batch(const SvtHipPaletteCtrls *ctrls, const SvtHipPaletteDesc *desc, uint32_t n, void *stream) {
    static const char *const fn = "svt_hip_palette_search_batch";
    if (!ctrls || !desc || !n)
        return widen(refuse("%s: NULL argument or no descriptor", fn));
    if (!ctrls->d_rates || ((uintptr_t)ctrls->d_rates & 3))
        return widen(refuse("%s: NULL or misaligned rate table", fn));
    if (ctrls->bit_depth != 8 && ctrls->bit_depth != 10)
        return widen(refuse("%s: bit_depth %u, 8 or 10 allowed", fn, ctrls->bit_depth));
    if (ctrls->dominant_color_step != 1 && ctrls->dominant_color_step != 2)
        return widen(refuse("%s: dominant_color_step %u, 1 or 2 allowed", fn, ctrls->dominant_color_step));
    if (ctrls->max_itr < 1 || ctrls->max_itr > 50)
        return widen(refuse("%s: max_itr %u, 1 .. 50 allowed", fn, ctrls->max_itr));
    for (uint32_t i = 0; i < n; i++) {
        const SvtHipPaletteDesc &d = desc[i];
        if (!d.src || !d.record || !d.maps)
            return widen(refuse("%s: descriptor %u: NULL pointer", fn, i));
        if (!pow2_8_64(d.width) || !pow2_8_64(d.height) || d.width > 4 * d.height || d.height > 4 * d.width)
            return widen(refuse("%s: descriptor %u: %u x %u is no block size of 8 .. 64", fn, i, d.width, d.height));
        if (!d.rows || !d.cols || d.rows > d.height || d.cols > d.width)
            return widen(refuse("%s: descriptor %u: %u rows, %u cols of a %u x %u block", fn, i, d.rows, d.cols, d.width, d.height));
        if (d.above_n > SVT_HIP_PALETTE_MAX_SIZE || d.left_n > SVT_HIP_PALETTE_MAX_SIZE)
            return widen(refuse("%s: descriptor %u: neighbour palettes of %u and %u colours, at most %d", fn, i, d.above_n, d.left_n, SVT_HIP_PALETTE_MAX_SIZE));
        for (uint32_t j = 0; j < SVT_HIP_PALETTE_MAX_SIZE; j++)
            if ((j < d.above_n && d.above[j] >> ctrls->bit_depth) || (j < d.left_n && d.left[j] >> ctrls->bit_depth))
                return widen(refuse("%s: descriptor %u: neighbour colour beyond %u bits", fn, i, ctrls->bit_depth));
        if (((uintptr_t)d.record & 7) || ((uintptr_t)d.maps & 3))
            return widen(refuse("%s: descriptor %u: misaligned record or map storage", fn, i));
        if (ctrls->bit_depth == 10 && ((uintptr_t)d.src & 1))
            return widen(refuse("%s: descriptor %u: odd uint16 plane", fn, i));
        if ((uint64_t)d.org_x + d.cols > d.stride)
            return widen(refuse("%s: descriptor %u: stride %u cannot hold column %u", fn, i, d.stride, d.org_x + d.cols));
    }
    TierBCall   c(fn, stream);
    const auto *d_desc = (const SvtHipPaletteDesc *)c.stage(desc, (size_t)n * sizeof(*desc));
    if (!c.ok())
        return widen(c.status());
    const SearchArgs args = {d_desc, ctrls->d_rates, ctrls->dominant_color_step, ctrls->bit_depth, ctrls->max_itr, 0};
    hipLaunchKernelGGL(palette_search_kernel, dim3(n), dim3(256), 0, c.stream(), args);
    return widen(c.finish());
}

extern "C" uint64_t svt_hip_palette_predict_batch(const SvtHipPalettePredDesc *d_desc, uint32_t n, void *stream) {
    static const char *const fn = "svt_hip_palette_predict_batch";
    if (!d_desc || !n)
        return widen(refuse("%s: NULL descriptors or none", fn));
    TierBCall c(fn, stream);
    if (!c.ok())
        return widen(c.status());
    hipLaunchKernelGGL(palette_predict_kernel, dim3(n), dim3(256), 0, c.stream(), d_desc, n);
    return widen(c.finish());
}

extern "C" uint64_t svt_hip_sc_classify(const uint8_t *d_plane, uint32_t width, uint32_t height, uint32_t stride, SvtHipScClass *d_out, void *stream) {
    static const char *const fn = "svt_hip_sc_classify";
    if (!d_plane || !d_out)
        return widen(refuse("%s: NULL argument", fn));
    if (!width || !height || width > 16384 || height > 16384 || (uint64_t)width * height * 50 > 0x7fffffffull)  // the reference's int products
        return widen(refuse("%s: plane of %u x %u, 1 .. 16384 each and at most 2^31 / 50 pixels", fn, width, height));
    if (stride < width)
        return widen(refuse("%s: stride %u smaller than the width %u", fn, stride, width));
    if ((uintptr_t)d_out & 3)
        return widen(refuse("%s: misaligned record", fn));
    TierBCall c(fn, stream);
    if (!c.ok())
        return widen(c.status());
    if (!c.check(hipMemsetAsync(d_out, 0, sizeof(*d_out), c.stream()), "hipMemsetAsync"))
        return widen(c.status());
    const uint32_t bx = width / 16, blocks = bx * (height / 16);
    hipLaunchKernelGGL(sc_classify_kernel, dim3(blocks ? (blocks + SC_PER_WAVE - 1) / SC_PER_WAVE : 1), dim3(64), 0, c.stream(), d_plane, width, height, stride, bx, blocks, d_out);
    return widen(c.finish());
}

SVT_HIP_MODULE_WARMUP(intra_palette)
