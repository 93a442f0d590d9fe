// inter_gm.hip — the pixel work of global motion's front end on device-resident luma planes (include/svt_hip_inter.h):
// svt_av1_fast_corner_detect (corner_detect.c:19-30 over third_party/fastfeat) and svt_av1_determine_correspondence with
// improve_correspondence (corner_match.c:87-218).  Integer arithmetic throughout; the correlation's one f64 multiply and one f64
// divide are IEEE operations on the device as on the host (the library is built with -ffp-contract=off).
//
// Detection, four launches over all planes of a call:
//   gm_score_kernel   a 64 x 16 tile plus a 3-pixel halo in LDS; per pixel the bright / dark ring masks, the nine-in-a-row test by
//                     rotate-and, and for the few pixels that pass it the score min(254, m - 1), m the largest over the 16 arcs and both
//                     signs of the smallest +-(ring - centre) on the arc (what fast9_score's bisection converges to); a byte score
//                     map, 0 = no corner
//   gm_rows_kernel    one wave per row: the 8-neighbour suppression of nonmax.c on the score map; the survivors of a row as a bit
//                     map (one ballot per 64 pixels) and their number
//   gm_offsets_kernel one workgroup per plane: the exclusive prefix sum of the row counts, in place, and the record's count / found
//   gm_emit_kernel    one wave per row: a survivor's place is the row's offset plus its rank in the bit map, so the order is the
//                     raster order whatever order the waves run in
// Matching, two launches over all jobs of a call:
//   gm_match_kernel   one wave per frame corner: the frame window once in LDS (four pixels to a dword), the lanes walk the reference
//                     corners whose y lies within the threshold (the records are in raster order: a binary search finds the range), the wave reduces on
//                     (largest correlation, smallest index); the threshold test; then both 9 x 9 refinements with the 81 positions
//                     spread over the lanes, reduced on (largest correlation, smallest scan index).  The record goes to the slot of
//                     the frame corner's own index, x = -1 for a corner that yields none
//   gm_compact_kernel one workgroup per job closes the gaps in frame-corner order, in place, and writes the count
#include <algorithm>

#include "../../include/svt_hip_inter.h"
#include "common.hpp"

using namespace svthip;

namespace {

constexpr int TILE_W = 64, TILE_H = 16, HALO = 3, TILE_PITCH = 72;  // LDS tile of the score kernel: (64 + 6) x (16 + 6) bytes
constexpr int FAST_BARRIER = 18;
constexpr int SEARCH_BY2   = 4;  // SEARCH_SZ_BY2
constexpr int MAX_SZ       = SVT_HIP_GM_MAX_MATCH_SZ;

struct DetectPlane {
    const uint8_t *luma;
    uint8_t       *score;  // [height][width]
    uint64_t      *keep;   // [height][words_per_row(width)] survivors, bit x % 64 of word x / 64
    uint32_t      *rows;   // [height + 1] survivors of a row, then of the rows above it; [height]: of the plane
    uint32_t       width, height, stride, pad_;
};
struct DetectArgs {
    DetectPlane p[SVT_HIP_GM_MAX_PLANES];
};

struct MatchJob {
    const uint8_t         *frm, *ref;
    const SvtHipGmCorners *fc, *rc;
    uint32_t               width, height, frm_stride, ref_stride;
    uint32_t               fq, rq, match_sz, pad_;
};
struct MatchArgs {
    MatchJob j[SVT_HIP_GM_MAX_PLANES];
};

// the largest over the 16 arcs of nine of the smallest d on the arc
__device__ inline int best_arc(const int (&d)[16]) {
    int m2[16], m4[16], m8[16], best = -256;
#pragma unroll
    for (int k = 0; k < 16; k++) m2[k] = min(d[k], d[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) m4[k] = min(m2[k], m2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) m8[k] = min(m4[k], m4[(k + 4) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) best = max(best, min(m8[k], d[(k + 8) & 15]));
    return best;
}

__device__ inline bool nine_in_a_row(uint32_t m) {  // m: 16 ring bits
    const uint32_t mm = m | (m << 16);              // (mm >> k) & 0xffff is m rotated by k
    uint32_t       r  = mm & (mm >> 1);
    r &= r >> 2;   // runs of 4
    r &= r >> 4;   // runs of 8
    r &= mm >> 8;  // runs of 9; bits 0 .. 15 see only bits below 32 of mm: 15 + 8 + 7 = 30
    return (r & 0xffffu) != 0;
}

__global__ __launch_bounds__(256) void gm_score_kernel(const DetectArgs args) {
    // fast_9.c:2941-2956: the ring as (dx, dy), in its own order
    constexpr int RING_X[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int RING_Y[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    __shared__ uint8_t tile[(TILE_H + 2 * HALO) * TILE_PITCH];
    const DetectPlane &p  = args.p[blockIdx.z];
    const int          x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H, w = (int)p.width, h = (int)p.height;
    if (x0 >= w || y0 >= h)
        return;
    for (int i = threadIdx.x; i < (TILE_H + 2 * HALO) * (TILE_W + 2 * HALO); i += 256) {
        const int ty = i / (TILE_W + 2 * HALO), tx = i % (TILE_W + 2 * HALO);
        const int x = x0 + tx - HALO, y = y0 + ty - HALO;
        tile[ty * TILE_PITCH + tx] = (x >= 0 && x < w && y >= 0 && y < h) ? p.luma[(size_t)y * p.stride + x] : 0;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63;
    for (int ly = threadIdx.x >> 6; ly < TILE_H; ly += 4) {
        const int x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h)
            continue;
        int score = 0;
        if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
            const uint8_t *c = &tile[(ly + HALO) * TILE_PITCH + lx + HALO];
            const int      v = c[0];
            int            d[16];
            uint32_t       bright = 0, dark = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                d[k] = (int)c[RING_Y[k] * TILE_PITCH + RING_X[k]] - v;
                bright |= (uint32_t)(d[k] > FAST_BARRIER) << k;
                dark |= (uint32_t)(d[k] < -FAST_BARRIER) << k;
            }
            if (nine_in_a_row(bright) || nine_in_a_row(dark)) {
                int m = best_arc(d);
#pragma unroll
                for (int k = 0; k < 16; k++) d[k] = -d[k];
                m     = max(m, best_arc(d));
                score = min(254, m - 1);  // m > 18 here
            }
        }
        p.score[(size_t)y * w + x] = (uint8_t)score;
    }
}

// nonmax.c on the score map: a corner survives unless one of its eight neighbours is a corner whose score is >= its own
__device__ inline bool survives(const uint8_t *score, int w, int h, int x, int y) {
    const int s = score[(size_t)y * w + x];
    if (!s)
        return false;
    int top = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int nx = x + dx, ny = y + dy;
            if ((dx || dy) && nx >= 0 && nx < w && ny >= 0 && ny < h)
                top = max(top, (int)score[(size_t)ny * w + nx]);
        }
    return top < s;
}

__host__ __device__ inline uint32_t words_per_row(uint32_t width) { return (width + 63) / 64; }

__global__ __launch_bounds__(64) void gm_rows_kernel(const DetectArgs args) {
    const DetectPlane &p = args.p[blockIdx.y];
    const int          y = blockIdx.x, w = (int)p.width, h = (int)p.height;
    if (y >= h)
        return;
    uint64_t *keep = p.keep + (size_t)y * words_per_row(p.width);
    uint32_t  n    = 0;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int                x    = x0 + (int)threadIdx.x;
        const unsigned long long mask = __ballot(x < w && survives(p.score, w, h, x, y));
        if (threadIdx.x == 0)
            keep[x0 / 64] = mask;
        n += (uint32_t)__popcll(mask);
    }
    if (threadIdx.x == 0)
        p.rows[y] = n;
}

// rows[y] becomes the number of survivors above row y, rows[height] their total
__global__ __launch_bounds__(256) void gm_offsets_kernel(const DetectArgs args, SvtHipGmCorners *__restrict__ d_out) {
    __shared__ uint32_t wave_n[4];
    const DetectPlane  &p = args.p[blockIdx.x];
    const uint32_t      h = p.height, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t            base = 0;
    for (uint32_t y0 = 0; y0 < h; y0 += 256) {
        const uint32_t y = y0 + tid, n = y < h ? p.rows[y] : 0;
        uint32_t       upto = n;  // of this row and the wave's rows before it
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(upto, o);
            if ((int)lane >= o)
                upto += t;
        }
        if (lane == 63)
            wave_n[wave] = upto;
        __syncthreads();
        uint32_t before = base;
        for (uint32_t v = 0; v < wave; v++) before += wave_n[v];
        if (y < h)
            p.rows[y] = before + upto - n;
        base += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        __syncthreads();  // wave_n is rewritten in the next round
    }
    if (tid == 0) {
        p.rows[h] = base;
        d_out[blockIdx.x].found = base, d_out[blockIdx.x].count = min(base, (uint32_t)SVT_HIP_GM_MAX_CORNERS);
    }
}

__global__ __launch_bounds__(64) void gm_emit_kernel(const DetectArgs args, SvtHipGmCorners *__restrict__ d_out) {
    const DetectPlane &p = args.p[blockIdx.y];
    const int          y = blockIdx.x, w = (int)p.width, h = (int)p.height, lane = threadIdx.x;
    if (y >= h)
        return;
    SvtHipGmCorners &out  = d_out[blockIdx.y];
    uint32_t         base = p.rows[y];
    if (base >= SVT_HIP_GM_MAX_CORNERS || p.rows[y + 1] == base)
        return;
    const uint64_t *keep = p.keep + (size_t)y * words_per_row(p.width);
    for (int x0 = 0; x0 < w; x0 += 64) {
        const uint64_t mask = keep[x0 / 64];
        const uint32_t at   = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
        if (((mask >> lane) & 1) && at < SVT_HIP_GM_MAX_CORNERS)
            out.xy[2 * at] = x0 + lane, out.xy[2 * at + 1] = y;
        base += (uint32_t)__popcll(mask);
    }
}

// ---- matching ------------------------------------------------------------------------------------------------------------

struct Best {
    double   ncc;
    uint32_t idx;  // ~0u: none
};

// (largest ncc, smallest idx) over the wave; every lane gets the result.  A lane that found nothing holds (0.0, ~0u).
__device__ inline Best wave_best(Best b) {
    for (int o = 32; o; o >>= 1) {
        const double   n = __shfl_xor(b.ncc, o);
        const uint32_t i = __shfl_xor(b.idx, o);
        if (n > b.ncc || (n == b.ncc && i < b.idx))
            b.ncc = n, b.idx = i;
    }
    return b;
}

__device__ inline int wave_sum(int v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline bool eligible_point(int x, int y, int w, int h, int by2) { return x >= by2 && y >= by2 && x + by2 < w && y + by2 < h; }

// The template lives in LDS as rows of TPL_ROW dwords, four pixels to a dword, zero behind the window's last column.
constexpr int TPL_ROW = (MAX_SZ + 3) / 4;

// The sz x sz window of im centred at (x, y) into tpl; returns the wave's sum and sum of squares of it.
__device__ inline void load_template(uint32_t *tpl, const uint8_t *im, uint32_t stride, int x, int y, int sz, int &sum, int &sumsq) {
    const int by2 = (sz - 1) / 2;
    int       s = 0, q = 0;
    __syncthreads();  // the previous template's readers are done (a workgroup is one wave)
    if (threadIdx.x < MAX_SZ * TPL_ROW)
        tpl[threadIdx.x] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < sz * sz; t += 64) {
        const int r = t / sz, c = t % sz;
        const int v = im[(size_t)(y - by2 + r) * stride + (x - by2 + c)];
        ((uint8_t *)tpl)[r * (TPL_ROW * 4) + c] = (uint8_t)v;
        s += v, q += v * v;
    }
    __syncthreads();
    sum = wave_sum(s), sumsq = wave_sum(q);
}

// svt_av1_compute_cross_correlation_c with im1's window in tpl (its sum in sum1) and im2's centred at (x2, y2).  A window row is read
// four pixels at a time, as dwords at whatever alignment the row has, and its last one or three pixels byte by byte, so that nothing
// beyond the window is touched; the three sums are 4-way dot products.  No sum leaves 31 bits up to match_sz 13.
__device__ inline double cross_correlation(const uint32_t *tpl, int sum1, const uint8_t *im2, uint32_t stride2, int x2, int y2, int sz) {
    const int      by2 = (sz - 1) / 2, sz_sq = sz * sz, full = sz >> 2, tail = sz & 3;  // sz is odd: tail is 1 or 3
    uint32_t       sum2 = 0, sumsq2 = 0, cross = 0;
    const uint8_t *row = im2 + (size_t)(y2 - by2) * stride2 + (x2 - by2);
    for (int i = 0; i < sz; i++, row += stride2, tpl += TPL_ROW) {
        for (int k = 0; k < full; k++) {
            uint32_t v;
            __builtin_memcpy(&v, row + 4 * k, 4);
            cross = __builtin_amdgcn_udot4(tpl[k], v, cross, false), sumsq2 = __builtin_amdgcn_udot4(v, v, sumsq2, false);
            sum2 = __builtin_amdgcn_udot4(v, 0x01010101u, sum2, false);
        }
        uint32_t v = row[4 * full];
        if (tail == 3)
            v |= (uint32_t)row[4 * full + 1] << 8 | (uint32_t)row[4 * full + 2] << 16;
        cross = __builtin_amdgcn_udot4(tpl[full], v, cross, false), sumsq2 = __builtin_amdgcn_udot4(v, v, sumsq2, false);
        sum2 = __builtin_amdgcn_udot4(v, 0x01010101u, sum2, false);
    }
    const int var2 = (int)sumsq2 * sz_sq - (int)sum2 * (int)sum2, cov = (int)cross * sz_sq - sum1 * (int)sum2;
    if (cov < 0)
        return 0.0;
    return ((double)cov * (double)cov) / (double)var2;
}

// One pass of improve_correspondence: the 81 offsets around (mx, my) in im2, scanned y outer and x inner, against the template; the
// distance is taken to (fx, fy).  Returns the winning offset, (0, 0) when no correlation exceeds 0.
__device__ inline void refine(const uint32_t *tpl, int sum1, const uint8_t *im2, uint32_t stride2, int mx, int my, int fx, int fy, int w, int h, int sz,
                              int thresh_sqr, int &best_x, int &best_y) {
    const int by2 = (sz - 1) / 2;
    Best      b   = {0.0, ~0u};
    for (int k = threadIdx.x; k < (2 * SEARCH_BY2 + 1) * (2 * SEARCH_BY2 + 1); k += 64) {
        const int px = mx + k % (2 * SEARCH_BY2 + 1) - SEARCH_BY2, py = my + k / (2 * SEARCH_BY2 + 1) - SEARCH_BY2;
        const int dx = fx - px, dy = fy - py;
        if (!eligible_point(px, py, w, h, by2) || dx * dx + dy * dy > thresh_sqr)
            continue;
        const double ncc = cross_correlation(tpl, sum1, im2, stride2, px, py, sz);
        if (ncc > b.ncc)
            b.ncc = ncc, b.idx = (uint32_t)k;
    }
    b      = wave_best(b);
    best_x = b.idx == ~0u ? 0 : (int)(b.idx % (2 * SEARCH_BY2 + 1)) - SEARCH_BY2;
    best_y = b.idx == ~0u ? 0 : (int)(b.idx / (2 * SEARCH_BY2 + 1)) - SEARCH_BY2;
}

// The first of n corners in raster order whose y is at least `row` (n when there is none)
__device__ inline uint32_t first_row_at_least(const int32_t *xy, uint32_t n, int row) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = (a + b) / 2;
        if (xy[2 * m + 1] < row)
            a = m + 1;
        else
            b = m;
    }
    return a;
}

__device__ inline void store_pts(SvtHipGmMatches &out, uint32_t i, int x, int y, int rx, int ry) {
    int2 *p = (int2 *)&out.pts[4 * i];  // pts starts 8 bytes into the record
    p[0] = make_int2(x, y), p[1] = make_int2(rx, ry);
}

__global__ __launch_bounds__(64) void gm_match_kernel(const MatchArgs args, SvtHipGmMatches *__restrict__ d_out) {
    __shared__ uint32_t tpl[MAX_SZ * TPL_ROW];
    const MatchJob  &job = args.j[blockIdx.y];
    const uint32_t   i = blockIdx.x, lane = threadIdx.x;
    const uint32_t   nf = min(job.fc->count, (uint32_t)SVT_HIP_GM_MAX_CORNERS) * job.fq / 4, nr = min(job.rc->count, (uint32_t)SVT_HIP_GM_MAX_CORNERS) * job.rq / 4;
    if (i >= nf)
        return;
    SvtHipGmMatches &out = d_out[blockIdx.y];
    const int        w = (int)job.width, h = (int)job.height, sz = (int)job.match_sz, by2 = (sz - 1) / 2;
    const int        thresh = max(w, h) >> 4, thresh_sqr = thresh * thresh;
    int              x = job.fc->xy[2 * i], y = job.fc->xy[2 * i + 1];
    if (!eligible_point(x, y, w, h, by2)) {
        if (lane == 0)
            store_pts(out, i, -1, 0, 0, 0);
        return;
    }
    int sum1, sumsq1;
    load_template(tpl, job.frm, job.frm_stride, x, y, sz, sum1, sumsq1);
    // the reference corners with y - thresh <= ry <= y + thresh: [lo, hi) of a record in raster order
    const int32_t *rxy = job.rc->xy;
    const uint32_t lo = first_row_at_least(rxy, nr, y - thresh), hi = first_row_at_least(rxy, nr, y + thresh + 1);
    Best best = {0.0, ~0u};
    for (uint32_t j = lo + lane; j < hi; j += 64) {
        const int2 r  = *(const int2 *)&rxy[2 * j];
        const int  dx = x - r.x, dy = y - r.y;
        if (!eligible_point(r.x, r.y, w, h, by2) || dx * dx + dy * dy > thresh_sqr)
            continue;
        const double ncc = cross_correlation(tpl, sum1, job.ref, job.ref_stride, r.x, r.y, sz);
        if (ncc > best.ncc)
            best.ncc = ncc, best.idx = j;
    }
    best = wave_best(best);
    const int template_norm = sumsq1 * (sz * sz) - sum1 * sum1;  // compute_variance
    if (best.idx == ~0u || !(best.ncc > (double)template_norm * 0.75 * 0.75)) {
        if (lane == 0)
            store_pts(out, i, -1, 0, 0, 0);
        return;
    }
    int rx = rxy[2 * best.idx], ry = rxy[2 * best.idx + 1], bx, by;
    // improve_correspondence, first loop: the reference point moves, the frame window is the template
    refine(tpl, sum1, job.ref, job.ref_stride, rx, ry, x, y, w, h, sz, thresh_sqr, bx, by);
    rx += bx, ry += by;
    // second loop: the frame point moves, the moved reference window is the template
    load_template(tpl, job.ref, job.ref_stride, rx, ry, sz, sum1, sumsq1);
    refine(tpl, sum1, job.frm, job.frm_stride, x, y, rx, ry, w, h, sz, thresh_sqr, bx, by);
    x += bx, y += by;
    if (lane == 0)
        store_pts(out, i, x, y, rx, ry);
}

// Closes the gaps of one job's record in frame-corner order.  A chunk's records are read before any of them is overwritten, and a
// record never moves up, so the chunks that follow are still intact.
__global__ __launch_bounds__(256) void gm_compact_kernel(const MatchArgs args, SvtHipGmMatches *__restrict__ d_out) {
    __shared__ uint32_t wave_n[4], total;
    const MatchJob     &job = args.j[blockIdx.x];
    SvtHipGmMatches    &out = d_out[blockIdx.x];
    const uint32_t      nf = min(job.fc->count, (uint32_t)SVT_HIP_GM_MAX_CORNERS) * job.fq / 4, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t            base = 0;
    for (uint32_t i0 = 0; i0 < nf; i0 += 256) {
        const uint32_t i = i0 + tid;
        int2           a = make_int2(-1, 0), b = make_int2(0, 0);
        if (i < nf)
            a = ((const int2 *)&out.pts[4 * i])[0], b = ((const int2 *)&out.pts[4 * i])[1];
        const bool               keep = a.x >= 0;
        const unsigned long long mask = __ballot(keep);
        if (lane == 0)
            wave_n[wave] = (uint32_t)__popcll(mask);
        __syncthreads();  // every record of the chunk is in registers, every count in LDS
        uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
        for (uint32_t v = 0; v < wave; v++) at += wave_n[v];
        if (keep)
            store_pts(out, at, a.x, a.y, b.x, b.y);
        if (tid == 0)
            total = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        __syncthreads();
        base += total;
    }
    __syncthreads();
    for (uint32_t i = base + tid; i < nf; i += 256) store_pts(out, i, 0, 0, 0, 0);
    if (tid == 0)
        out.count = base, out.pad_ = 0;
}

uint16_t narrow(int32_t status) { return SVT_HIP_GM_STATUS(status); }

// the byte score map, the survivor bit map and the row counts of a plane, each rounded up to 256
uint64_t plane_workspace(uint64_t width, uint64_t height) {
    return up256(width * height) + up256(height * words_per_row((uint32_t)width) * 8) + up256((height + 1) * 4);
}

const char *bad_plane(const SvtHipGmPlane &p) {
    if (!p.luma)
        return "NULL plane";
    if (!p.width || !p.height)
        return "empty plane";
    if (p.stride < p.width)
        return "stride smaller than the width";
    if (p.width > 16384 || p.height > 16384)  // the squared distances stay inside int, as the reference needs them to
        return "plane larger than 16384";
    return nullptr;
}

}  // namespace

extern "C" uint64_t svt_hip_gm_corners_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_planes) {
    return width && height ? (uint64_t)n_planes * plane_workspace(width, height) : 0;
}

extern "C" uint16_t svt_hip_gm_detect_corners(const SvtHipGmPlane *planes, uint32_t n, SvtHipGmCorners *d_out, void *workspace, uint64_t workspace_bytes,
                                              void *stream) {
    static const char *const fn = "svt_hip_gm_detect_corners";
    if (!planes || !d_out || !workspace)
        return narrow(refuse("%s: NULL argument", fn));
    if (n > SVT_HIP_GM_MAX_PLANES)
        return narrow(refuse("%s: %u planes, at most %d a call", fn, n, SVT_HIP_GM_MAX_PLANES));
    if (n == 0)
        return narrow(SVT_HIP_OK);
    if (((uintptr_t)workspace | (uintptr_t)d_out) & 7)
        return narrow(refuse("%s: records and workspace must be 8-byte aligned", fn));
    DetectArgs args = {};
    uint64_t   need = 0;
    uint32_t   max_w = 0, max_h = 0;
    for (uint32_t i = 0; i < n; i++) {
        const SvtHipGmPlane &p = planes[i];
        if (const char *why = bad_plane(p))
            return narrow(refuse("%s: plane %u: %s (%u x %u, stride %u)", fn, i, why, p.width, p.height, p.stride));
        uint8_t *const score = (uint8_t *)workspace + need, *const keep = score + up256((uint64_t)p.width * p.height);
        args.p[i] = DetectPlane{p.luma, score, (uint64_t *)keep, (uint32_t *)(keep + up256((uint64_t)p.height * words_per_row(p.width) * 8)),
                                p.width, p.height, p.stride, 0};
        need += plane_workspace(p.width, p.height);
        max_w = std::max(max_w, p.width), max_h = std::max(max_h, p.height);
    }
    if (workspace_bytes < need)
        return narrow(refuse("%s: workspace of %llu bytes, %llu needed", fn, (unsigned long long)workspace_bytes, (unsigned long long)need));
    TierBCall c(fn, stream);
    if (!c.ok())
        return narrow(c.status());
    hipLaunchKernelGGL(gm_score_kernel, dim3((max_w + TILE_W - 1) / TILE_W, (max_h + TILE_H - 1) / TILE_H, n), dim3(256), 0, c.stream(), args);
    hipLaunchKernelGGL(gm_rows_kernel, dim3(max_h, n), dim3(64), 0, c.stream(), args);
    hipLaunchKernelGGL(gm_offsets_kernel, dim3(n), dim3(256), 0, c.stream(), args, d_out);
    hipLaunchKernelGGL(gm_emit_kernel, dim3(max_h, n), dim3(64), 0, c.stream(), args, d_out);
    return narrow(c.finish());
}

extern "C" uint16_t svt_hip_gm_match_corners(const SvtHipGmMatchJob *jobs, uint32_t n, SvtHipGmMatches *d_out, void *stream) {
    static const char *const fn = "svt_hip_gm_match_corners";
    if (!jobs || !d_out)
        return narrow(refuse("%s: NULL argument", fn));
    if (n > SVT_HIP_GM_MAX_PLANES)
        return narrow(refuse("%s: %u jobs, at most %d a call", fn, n, SVT_HIP_GM_MAX_PLANES));
    if (n == 0)
        return narrow(SVT_HIP_OK);
    if ((uintptr_t)d_out & 7)
        return narrow(refuse("%s: records must be 8-byte aligned", fn));
    MatchArgs args = {};
    for (uint32_t i = 0; i < n; i++) {
        const SvtHipGmMatchJob &j = jobs[i];
        if (const char *why = bad_plane(j.frm))
            return narrow(refuse("%s: job %u: frame: %s (%u x %u, stride %u)", fn, i, why, j.frm.width, j.frm.height, j.frm.stride));
        if (const char *why = bad_plane(j.ref))
            return narrow(refuse("%s: job %u: reference: %s (%u x %u, stride %u)", fn, i, why, j.ref.width, j.ref.height, j.ref.stride));
        if (j.frm.width != j.ref.width || j.frm.height != j.ref.height)
            return narrow(refuse("%s: job %u: frame %u x %u, reference %u x %u", fn, i, j.frm.width, j.frm.height, j.ref.width, j.ref.height));
        if (!j.frm_corners || !j.ref_corners || (((uintptr_t)j.frm_corners | (uintptr_t)j.ref_corners) & 7))
            return narrow(refuse("%s: job %u: NULL or misaligned corner record", fn, i));
        if (j.frm_quarters < 1 || j.frm_quarters > 4 || j.ref_quarters < 1 || j.ref_quarters > 4)
            return narrow(refuse("%s: job %u: quarters %u and %u, 1 .. 4 allowed", fn, i, j.frm_quarters, j.ref_quarters));
        if (!(j.match_sz & 1) || j.match_sz < 3 || j.match_sz > SVT_HIP_GM_MAX_MATCH_SZ)
            return narrow(refuse("%s: job %u: match_sz %u, odd values 3 .. %d allowed", fn, i, j.match_sz, SVT_HIP_GM_MAX_MATCH_SZ));
        args.j[i] = MatchJob{j.frm.luma, j.ref.luma, j.frm_corners, j.ref_corners, j.frm.width, j.frm.height, j.frm.stride, j.ref.stride,
                             j.frm_quarters, j.ref_quarters, j.match_sz, 0};
    }
    TierBCall c(fn, stream);
    if (!c.ok())
        return narrow(c.status());
    hipLaunchKernelGGL(gm_match_kernel, dim3(SVT_HIP_GM_MAX_CORNERS, n), dim3(64), 0, c.stream(), args, d_out);
    hipLaunchKernelGGL(gm_compact_kernel, dim3(n), dim3(256), 0, c.stream(), args, d_out);
    return narrow(c.finish());
}

SVT_HIP_MODULE_WARMUP(inter_gm)
