// loopfilter_wiener_pick.hip — the Wiener decision of one plane on the device (restoration_pick.c: search_wiener_seg :1296-1378,
// search_wiener_finish :1380-1431, rest_finish_search :1555-1625 for NONE against WIENER), between svt_hip_wiener_stats (M and H in
// device memory) and svt_hip_restoration_filter_frame (units from device memory).  DESIGN.md section 4 has the design and why.
//
//   wpick_solve    workgroup per unit: wiener_decompose_sep_sym (:906-936), finalize_sym_filter (:977-1006), compute_score
//                  (:937-975).  All of it is the reference's int64 arithmetic with truncating division.  Every term of A, B, P
//                  and Q is divided before it is added, so the sums commute: the win^4 terms are spread over the threads and
//                  meet in LDS by 64-bit atomic adds (one per thread); one thread does the 3 (2) unknown linsolve_wiener literally.
//   wpick_trial    ONE trial filter of every unit that is still searching (finer_tile_search_wiener_seg :1042-1147): workgroup per
//                  64 x 64 tile of a unit, the separable filter in LDS, the squared difference against the source, one 64-bit
//                  atomic add per workgroup into the unit's sum.  The workgroup that arrives LAST at a unit (a ticket counter,
//                  nobody waits) advances that unit's state machine by one step: keep or undo the move, pick the next candidate.
//                  The host enqueues the largest number of trials the controls and the tap ranges allow, up front; the
//                  workgroups of a unit that has finished return at once.  The order of the launches is the stream's alone.
//   wpick_decide   one workgroup: the unit records, the raster-order chain of search_wiener_finish (`ref` follows the last unit
//                  that chose Wiener), the two RDCOST_DBL of the plane, the units for svt_hip_restoration_filter_frame.
// A trial is try_restoration_unit_seg (:129-165) with use_boundaries_in_rest_search == 0 (enc_handle.c:4127): the filter reads
// the picture's own samples, replicated outside the cropped plane as svt_extend_frame leaves them.
#include "lr_pick.hpp"

using namespace svthip;
using namespace svthip::lr;

namespace {

constexpr int       W2MAX = 49;
constexpr long long SCALE = 65536;  // WIENER_TAP_SCALE_FACTOR

struct State {  // the search of one unit between two launches: the workspace
    int16_t            h[8], v[8];  // the filter of the trial that runs next (the best one once phase is DONE)
    long long          err, none;   // smallest error so far; sse[RESTORE_NONE]
    unsigned long long acc, accn;   // sums of the running trial: filtered, unfiltered
    long long          score;       // compute_score (0 for previous-frame taps)
    int32_t            status;      // 0 rejected by the score, 1 solved, 2 taps of the previous frame
    int32_t            phase;       // FIRST: the trial of the start filter runs next; MOVE: the trial of a move; DONE
    int32_t            s, f, p, dir, skip;  // where the search stands: step size, h / v filter, tap, -1 / +1, the visit's skip flag
    int32_t            trials;
    uint32_t           arrived;     // workgroups of the running trial that have added their sum
    int32_t            pad_;
};
static_assert(sizeof(State) == 112, "workspace record");
constexpr int FIRST = 0, MOVE = 1, DONE = 2;

__device__ __forceinline__ int init_tap(int i) { return i == 3 ? 106 : (i == 0 || i == 6 ? 3 : (i == 1 || i == 5 ? -7 : 15)); }

// linsolve_wiener (:766-803), literally; A is the matrix (the caller's B), b the right-hand side (the caller's A)
template <int N, int STRIDE> __device__ int linsolve(long long *A, long long *b, int32_t *x) {
    auto mag = [](long long v) { return v < 0 ? -v : v; };
    for (int k = 0; k < N - 1; k++) {
        for (int i = N - 1; i > k; i--) {
            if (mag(A[(i - 1) * STRIDE + k]) < mag(A[i * STRIDE + k])) {
                for (int j = 0; j < N; j++) {
                    const long long c     = A[i * STRIDE + j];
                    A[i * STRIDE + j]       = A[(i - 1) * STRIDE + j];
                    A[(i - 1) * STRIDE + j] = c;
                }
                const long long c = b[i];
                b[i] = b[i - 1], b[i - 1] = c;
            }
        }
        for (int i = k; i < N - 1; i++) {
            if (A[k * STRIDE + k] == 0)
                return 0;
            const long long c = A[(i + 1) * STRIDE + k], cd = A[k * STRIDE + k];
            for (int j = 0; j < N; j++) A[(i + 1) * STRIDE + j] -= c / 256 * A[k * STRIDE + j] / cd * 256;
            b[i + 1] -= c * b[k] / cd;
        }
    }
    for (int i = N - 1; i >= 0; i--) {
        if (A[i * STRIDE + i] == 0)
            return 0;
        long long c = 0;
        for (int j = i + 1; j <= N - 1; j++) c += A[i * STRIDE + j] * x[j] / SCALE;
        x[i] = (int32_t)(SCALE * (b[i] - c) / A[i * STRIDE + i]);
    }
    return 1;
}

// finalize_sym_filter (:977-1006)
template <int WIN> __device__ void finalize(const int32_t *f, int16_t *fi) {
    for (int i = 0; i < WIN / 2; i++) {
        const long long dividend = (long long)f[i] * 128;
        fi[i] = (int16_t)(dividend < 0 ? (dividend - SCALE / 2) / SCALE : (dividend + SCALE / 2) / SCALE);
    }
    auto clip = [](int v, int lo, int hi) { return (int16_t)(v < lo ? lo : (v > hi ? hi : v)); };
    if (WIN == 7) {
        fi[0] = clip(fi[0], tap_min(0), tap_max(0)), fi[1] = clip(fi[1], tap_min(1), tap_max(1)), fi[2] = clip(fi[2], tap_min(2), tap_max(2));
    } else {
        fi[2] = clip(fi[1], tap_min(2), tap_max(2));
        fi[1] = clip(fi[0], tap_min(1), tap_max(1));
        fi[0] = 0;
    }
    fi[6] = fi[0], fi[5] = fi[1], fi[4] = fi[2];
    fi[3] = (int16_t)(-2 * (fi[0] + fi[1] + fi[2]));
    fi[7] = 0;
}

template <int WIN>
__global__ __launch_bounds__(256) void wpick_solve(const long long *__restrict__ M, const long long *__restrict__ H, const SvtHipLrUnit *__restrict__ prev,
                                                   State *__restrict__ start) {
    constexpr int W2 = WIN * WIN, HW1 = WIN / 2 + 1, OFF = (7 - WIN) / 2, PARTS = 256 / W2;
    __shared__ long long sA[HW1], sB[HW1 * HW1], sPQ[2];
    __shared__ int32_t   sa[7], sb[7], sS[7];  // a: the vertical filter, b: the horizontal one (:1349)
    __shared__ int16_t   sv[8], sh[8];
    const int unit = blockIdx.x, tid = threadIdx.x;
    State    &out  = start[unit];
    if (tid == 0)  // every field: a call starts from its own clean state
        out.err = out.none = 0, out.acc = out.accn = 0, out.phase = FIRST, out.s = out.f = out.p = out.dir = out.skip = out.trials = 0, out.arrived = 0, out.pad_ = 0;
    // use_prev_frame_coeffs (:1312-1317): no solver, no score.  The number of launches is derived from the taps' coded ranges, so a record
    // whose taps lie outside them (no decision of the encoder leaves one) is not taken: the unit is solved like any other.
    bool take_prev = prev && prev[unit].restoration_type == RESTORE_WIENER;
    if (take_prev)
        for (int p = 0; p < 3; p++) {
            const int h = prev[unit].hfilter[p], v = prev[unit].vfilter[p];
            take_prev = take_prev && (p < OFF ? h == 0 && v == 0 : h >= tap_min(p) && h <= tap_max(p) && v >= tap_min(p) && v <= tap_max(p));
        }
    if (take_prev) {
        if (tid < 8)
            out.h[tid] = prev[unit].hfilter[tid], out.v[tid] = prev[unit].vfilter[tid];
        if (tid == 0)
            out.score = 0, out.status = 2;
        return;
    }
    const long long *Mu = M + (size_t)unit * W2MAX, *Hu = H + (size_t)unit * W2MAX * W2MAX;
    auto wrap = [](int i) { return i >= HW1 ? WIN - 1 - i : i; };
    if (tid < WIN)
        sa[tid] = sb[tid] = (int32_t)(SCALE / 128) * init_tap(tid + OFF);
    for (int round = 0; round < 2 * 4; round++) {  // NUM_WIENER_ITERS - 1 times update_a_sep_sym, update_b_sep_sym
        const bool upd_a = !(round & 1);
        __syncthreads();
        if (tid < HW1)
            sA[tid] = 0;
        if (tid < HW1 * HW1)
            sB[tid] = 0;
        __syncthreads();
        if (tid < W2) {
            const int i = tid / WIN, j = tid - i * WIN;
            if (upd_a)
                lds_add(&sA[wrap(j)], Mu[i * WIN + j] * sb[i] / SCALE);
            else
                lds_add(&sA[wrap(i)], Mu[i * WIN + j] * sa[j] / SCALE);
        }
        if (tid < W2 * PARTS) {  // a thread sums a share of the win^2 terms of ONE element of B privately: one atomic add per thread
            const int q = tid / PARTS, q0 = q / WIN, q1 = q - q0 * WIN;
            long long sum = 0;
            for (int r = tid - q * PARTS; r < W2; r += PARTS) {
                const int r0 = r / WIN, r1 = r - r0 * WIN;
                if (upd_a)  // (k, l) = q, (i, j) = r: hc[j * win + i][k * win2 + l] * b[i] / S * b[j] / S  (:826)
                    sum += Hu[r1 * WIN * W2 + r0 * WIN + q0 * W2 + q1] * sb[r0] / SCALE * sb[r1] / SCALE;
                else        // (i, j) = q, (k, l) = r: hc[i * win + j][k * win2 + l] * a[k] / S * a[l] / S  (:877)
                    sum += Hu[q0 * WIN * W2 + q1 * WIN + r0 * W2 + r1] * sa[r0] / SCALE * sa[r1] / SCALE;
            }
            lds_add(&sB[wrap(q1) * HW1 + wrap(q0)], sum);  // B[wrap(l)][wrap(k)] / B[wrap(j)][wrap(i)]
        }
        __syncthreads();
        if (tid == 0) {  // in place in LDS: no private arrays, no scratch
            long long *A = sA, *B = sB;
            int32_t   *S = sS;
            const long long a_last = A[HW1 - 1];  // normalisation enforcement (:834-845)
            for (int i = 0; i < HW1 - 1; i++) A[i] -= a_last * 2 + B[i * HW1 + HW1 - 1] - 2 * B[(HW1 - 1) * HW1 + (HW1 - 1)];
            for (int i = 0; i < HW1 - 1; i++)
                for (int j = 0; j < HW1 - 1; j++)
                    B[i * HW1 + j] -= 2 * (B[i * HW1 + (HW1 - 1)] + B[(HW1 - 1) * HW1 + j] - 2 * B[(HW1 - 1) * HW1 + (HW1 - 1)]);
            if (linsolve<HW1 - 1, HW1>(B, A, S)) {
                uint32_t mid = (uint32_t)SCALE;
                for (int i = HW1; i < WIN; i++) S[i] = S[WIN - 1 - i], mid -= 2u * (uint32_t)S[i];
                S[HW1 - 1] = (int32_t)mid;
                int32_t *dst = upd_a ? sa : sb;
                for (int i = 0; i < WIN; i++) dst[i] = S[i];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        finalize<WIN>(sa, sv), finalize<WIN>(sb, sh);
        sPQ[0] = sPQ[1] = 0;
    }
    __syncthreads();
    // compute_score (:937-975): every term divided before it is added
    auto full = [](const int16_t *f, int i) { return i == 3 ? (int)(int16_t)(128 - 2 * (f[0] + f[1] + f[2])) : (int)f[i < 3 ? i : 6 - i]; };
    auto ab   = [&](int k) { return (int32_t)(full(sv, k % WIN + OFF) * full(sh, k / WIN + OFF)); };
    if (tid < W2)
        lds_add(&sPQ[0], (long long)ab(tid) * Mu[tid] / 128 / 128);
    if (tid < W2 * PARTS) {
        const int k = tid / PARTS;
        long long sum = 0;
        for (int l = tid - k * PARTS; l < W2; l += PARTS) sum += (long long)ab(k) * Hu[k * W2 + l] * ab(l) / 128 / 128 / 128 / 128;
        lds_add(&sPQ[1], sum);
    }
    __syncthreads();
    const long long score = (sPQ[1] - 2 * sPQ[0]) - (Hu[(W2 >> 1) * W2 + (W2 >> 1)] - 2 * Mu[W2 >> 1]);
    const bool      keep  = !(score > 0);
    if (tid < 8)
        out.h[tid] = keep ? sh[tid] : (int16_t)0, out.v[tid] = keep ? sv[tid] : (int16_t)0;
    if (tid == 0)
        out.score = score, out.status = keep ? 1 : 0;
}

struct SearchPrm {
    int plane_w, plane_h, is16, bd, r0, r1, plane_off, use_refinement, max_one_step;
};

// One step of finer_tile_search_wiener_seg for one unit, by one thread, after the sums of a trial are complete.
__device__ void advance(State &st, const SearchPrm &prm, long long err2, long long none) {
    auto done = [&]() { st.phase = DONE; };
    if (st.status == 0) {  // rejected by the score (:1361-1364): sse[RESTORE_NONE] alone (search_norestore_seg)
        st.none = none, st.trials = 0;
        return done();
    }
    auto move = [&](int d) {
        int16_t *f = st.f ? st.v : st.h;
        f[st.p] += (int16_t)d, f[6 - st.p] += (int16_t)d, f[3] -= (int16_t)(2 * d);
    };
    const int end_step = prm.max_one_step ? 4 : 1;
    auto next_f = [&]() {
        st.f++, st.p = prm.plane_off, st.dir = -1, st.skip = 0;
        if (st.f >= 2) {
            st.f = 0, st.s >>= 1;
            if (st.s < end_step)
                done();
        }
    };
    auto end_dir = [&]() {  // the `break` out of a do-while (:1076, :1097)
        if (st.dir < 0) {
            if (st.skip)  // `if (skip) break;` leaves the loop over p (:1078)
                next_f();
            else
                st.dir = 1;
        } else {
            st.p++, st.dir = -1, st.skip = 0;
            if (st.p >= 3)
                next_f();
        }
    };
    if (st.phase == FIRST) {
        st.err = err2, st.none = none, st.trials = 1;
        if (!prm.use_refinement)
            return done();
        st.phase = MOVE, st.s = 4, st.f = 0, st.p = prm.plane_off, st.dir = -1, st.skip = 0;
    } else {
        st.trials++;
        if (err2 > st.err) {
            move(-st.dir * st.s);
            end_dir();
        } else {
            st.err = err2;
            if (st.dir < 0)
                st.skip = 1;
            if (!(st.s == 4 && !prm.max_one_step))  // at the highest step size continue moving in the same direction
                end_dir();
        }
    }
    while (st.phase != DONE) {  // the next move that stays inside the tap's limits
        const int cur = (st.f ? st.v : st.h)[st.p];
        if (st.dir < 0 ? cur - st.s >= tap_min(st.p) : cur + st.s <= tap_max(st.p))
            return move(st.dir * st.s);
        end_dir();
    }
}

// grid (tiles of the largest unit, units)
__global__ __launch_bounds__(256) void wpick_trial(const SvtHipWienerUnit *__restrict__ units, State *__restrict__ states, SearchPrm prm) {
    constexpr int IP = WIENER_IP, NT = 256;
    __shared__ alignas(4) uint16_t in[(64 + 7) * IP + WIENER_IN_SLACK];
    __shared__ uint16_t            tmp[(64 + 7) * 64];
    __shared__ long long           s_sum[2];
    const int tid = threadIdx.x;
    State    &st  = states[blockIdx.y];
    if (st.phase == DONE)
        return;
    const SvtHipWienerUnit u = units[blockIdx.y];
    const int uw = u.h_end - u.h_start, uh = u.v_end - u.v_start, gx = (uw + 63) >> 6, n_tiles = gx * ((uh + 63) >> 6);
    if ((int)blockIdx.x >= n_tiles)
        return;
    const int  is16 = prm.is16, bd = prm.bd, r0 = prm.r0, r1 = prm.r1;
    const bool filter = st.status != 0, with_none = st.phase == FIRST;
    const int  y0 = ((int)blockIdx.x / gx) * 64, x0 = ((int)blockIdx.x % gx) * 64, tw = min(64, uw - x0), th = min(64, uh - y0);
    int16_t    fx[8], fy[8];
#pragma unroll
    for (int k = 0; k < 8; k++) fx[k] = st.h[k], fy[k] = st.v[k];
    if (tid < 2)
        s_sum[tid] = 0;
    // the picture's own samples, replicated outside the cropped plane
    load_tile_clamped(in, IP, u.dgd, u.dgd_stride, is16, prm.plane_w, prm.plane_h, u.v_start + y0 - 3, u.h_start + x0 - 3, th + 7, tw + 7, NT);
    __syncthreads();
    long long acc = 0, accn = 0;
    auto source = [&](int r, int c) { return ldpx(u.src, (size_t)(u.v_start + y0 + r) * u.src_stride + (u.h_start + x0 + c), is16); };
    if (filter) {  // the filter of lr_device.hpp, the store replaced by the squared differences against the source
        wiener_tile_filter_to<NT>(in, tmp, tid, tw, th, fx, fy, bd, r0, r1, [&](int r, int c, int32_t v) {
            const int32_t s = source(r, c);
            acc += (long long)((v - s) * (v - s));
            if (with_none) {
                const int32_t d = (int32_t)in[(r + 3) * IP + c + 3] - s;
                accn += (long long)(d * d);
            }
        });
    } else {
        for (int idx = tid; idx < th * tw; idx += NT) {
            const int     r = idx / tw, c = idx - r * tw;
            const int32_t d = (int32_t)in[(r + 3) * IP + c + 3] - source(r, c);
            accn += (long long)(d * d);
        }
    }
    acc = wave_sum64(acc), accn = wave_sum64(accn);
    if ((tid & 63) == 0)
        lds_add(&s_sum[0], acc), lds_add(&s_sum[1], accn);
    __syncthreads();  // every thread of this workgroup has read the state
    if (tid == 0) {
        atomicAdd(&st.acc, (unsigned long long)s_sum[0]);
        if (with_none)
            atomicAdd(&st.accn, (unsigned long long)s_sum[1]);
        __threadfence();
        if (atomicAdd(&st.arrived, 1u) == (uint32_t)n_tiles - 1) {  // the last to arrive: every sum is in, every workgroup has read the state
            __threadfence();
            const long long err2 = (long long)atomicExch(&st.acc, 0ull), none = (long long)atomicExch(&st.accn, 0ull);
            atomicExch(&st.arrived, 0u);
            advance(st, prm, err2, none);
        }
    }
}

// The trials the host enqueues: the start filter, then, per filter and tap of the window, at step 4 one failed move down, the moves up
// the tap's range allows and one failed one (a visit that moves down instead ends the filter's taps for this step size and costs
// less), and two per visit at steps 2 and 1; with max_one_refinement_step two per visit at step 4 alone.
int trial_bound(int plane_off, int use_refinement, int max_one_step) {
    int t = 1;
    if (use_refinement)
        for (int p = plane_off; p < 3; p++) {
            const int range = p == 0 ? 15 : (p == 1 ? 31 : 63);  // WIENER_FILT_TAPn_MAXV - _MINV
            t += 2 * (max_one_step ? 2 : 2 + range / 4 + 2 + 2);
        }
    return t;
}

// One thread walks the units in raster order, so everything that does not depend on `ref` is done beside it: the records and the
// NONE cost of 256 units at a time by 256 threads into LDS, the bit counts as a table of every (tap, reference, value) triple.  A
// dependent read of device memory per unit would cost more than the whole chain does from LDS.
__global__ __launch_bounds__(256) void wpick_decide(const State *__restrict__ states, SvtHipWienerPickUnit *__restrict__ recs, int n_units, int win, int rdmult,
                                                    int cost0, int cost1, SvtHipWienerPickResult *__restrict__ res, SvtHipLrUnit *__restrict__ lr_units) {
    constexpr int CH = 256, T1 = 16 * 16, T2 = T1 + 32 * 32, TN = T2 + 64 * 64;
    __shared__ uint8_t   s_count[TN];  // count_refsubexpfin of tap p: [ref - min][value - min]
    __shared__ long long s_sse[2][CH], s_bits[CH];
    __shared__ double    s_cost_none[CH], s_dist_w[CH];
    __shared__ int16_t   s_taps[CH][6];  // vfilter[0..2], hfilter[0..2]
    __shared__ int       s_best[CH], s_type;
    const int tid = threadIdx.x;
    for (int e = tid; e < TN; e += 256) {
        const int p = e < T1 ? 0 : (e < T2 ? 1 : 2), o = e - (p == 0 ? 0 : (p == 1 ? T1 : T2)), n = 16 << p;
        s_count[e] = (uint8_t)count_refsubexpfin(n, p + 1, o / n, o % n);
    }
    auto count = [&](int p, int ref, int v) {  // taps outside their range (a previous frame's record can hold anything) are counted directly
        const int n = 16 << p, r = ref - tap_min(p), x = v - tap_min(p);
        return (unsigned)r < (unsigned)n && (unsigned)x < (unsigned)n ? (int)s_count[(p == 0 ? 0 : (p == 1 ? T1 : T2)) + r * n + x] : wiener_tap_bits(p, ref, v);
    };
    int ref[6], n_wiener = 0;  // thread 0's alone
    set_default_wiener(ref);
    long long       sse_n = 0, sse_w = 0, bits_w = 0;
    const long long bits_none = cost0;
    for (int base = 0; base < n_units; base += CH) {
        const int i = base + tid;
        if (i < n_units) {
            const State          &st = states[i];
            SvtHipWienerPickUnit &r  = recs[i];
            const bool            keep = st.status != 0;
            const long long       sse0 = st.none, sse1 = keep ? st.err : SSE_REJECTED;
            r.sse[0] = sse0, r.sse[1] = sse1, r.trials = st.trials;
            for (int k = 0; k < 8; k++) r.hfilter[k] = keep ? st.h[k] : (int16_t)0, r.vfilter[k] = keep ? st.v[k] : (int16_t)0;
            s_sse[0][tid] = sse0, s_sse[1][tid] = sse1;
            for (int k = 0; k < 3; k++) s_taps[tid][k] = st.v[k], s_taps[tid][3 + k] = st.h[k];
            s_cost_none[tid] = rdcost_dbl(rdmult, bits_none >> 4, sse0), s_dist_w[tid] = (double)sse1 * 128.0;
        }
        __syncthreads();
        if (tid == 0) {
            const int n = min(CH, n_units - base);
            for (int k = 0; k < n; k++) {  // search_wiener_finish (:1380-1431)
                sse_n += s_sse[0][k];
                if (s_sse[1][k] == SSE_REJECTED) {
                    bits_w += bits_none, sse_w += s_sse[0][k];
                    s_bits[k] = bits_none, s_best[k] = RESTORE_NONE;
                    continue;
                }
                const long long bits_wiener = cost1 + (count_wiener_bits(win, s_taps[k], ref, count) << 9);
                const double    cost_wiener = (((double)(bits_wiener >> 4) * (double)rdmult) / 512.0) + s_dist_w[k];  // RDCOST_DBL, the distortion term from above
                const bool      wiener      = cost_wiener < s_cost_none[k];
                s_bits[k] = bits_wiener, s_best[k] = wiener ? RESTORE_WIENER : RESTORE_NONE;
                sse_w += wiener ? s_sse[1][k] : s_sse[0][k], bits_w += wiener ? bits_wiener : bits_none;
                if (wiener) {
                    n_wiener++;
                    for (int t = 0; t < 6; t++) ref[t] = s_taps[k][t];
                }
            }
        }
        __syncthreads();
        if (i < n_units)
            recs[i].bits = s_bits[tid], recs[i].best_rtype = s_best[tid];
        __syncthreads();  // the next 256 units overwrite the arrays
    }
    if (tid == 0) {  // search_rest_type_finish (:1456-1465) of both types, rest_finish_search (:1612-1617)
        const double c_none = rdcost_dbl(rdmult, 0, sse_n), c_wiener = rdcost_dbl(rdmult, bits_w >> 4, sse_w);
        const int    type   = c_wiener < c_none ? RESTORE_WIENER : RESTORE_NONE;
        res->frame_restoration_type = type, res->n_wiener = n_wiener;
        res->sse[0] = sse_n, res->sse[1] = sse_w, res->bits[0] = 0, res->bits[1] = bits_w;
        res->cost[0] = c_none, res->cost[1] = c_wiener;
        s_type = type;
    }
    __syncthreads();
    for (int i = tid; i < n_units; i += 256) {  // a thread reads back what it wrote itself
        const SvtHipWienerPickUnit &r = recs[i];
        const bool                  w = s_type == RESTORE_WIENER && r.best_rtype == RESTORE_WIENER;
        SvtHipLrUnit                o{};
        o.restoration_type = w ? RESTORE_WIENER : RESTORE_NONE;
        for (int k = 0; k < 8; k++) o.hfilter[k] = w ? r.hfilter[k] : (int16_t)0, o.vfilter[k] = w ? r.vfilter[k] : (int16_t)0;
        lr_units[i] = o;
    }
}

}  // namespace

extern "C" uint64_t svt_hip_wiener_pick_workspace_bytes(uint32_t n_units) { return n_units ? up256((size_t)n_units * sizeof(State)) : 0; }

extern "C" int svt_hip_wiener_pick_plane(const SvtHipWienerPickParams *prm, const SvtHipWienerUnit *units, uint32_t n_units, const int64_t *d_M,
                                             const int64_t *d_H, const SvtHipLrUnit *d_prev_units, SvtHipWienerPickUnit *d_unit_records,
                                             SvtHipWienerPickResult *d_result, SvtHipLrUnit *d_lr_units, void *d_workspace, uint64_t workspace_bytes,
                                             void *stream) {
    static_assert(sizeof(SvtHipWienerPickUnit) == SVT_HIP_WIENER_PICK_UNIT_BYTES, "record size stated in the header");
    if (!prm || !units || !d_M || !d_H || !d_unit_records || !d_result || !d_lr_units || !d_workspace)
        return refuse("svt_hip_wiener_pick_plane: NULL argument");
    if (n_units == 0 || n_units > 65535)
        return refuse("svt_hip_wiener_pick_plane: %u units (1..65535)", n_units);
    if (prm->wiener_win != 7 && prm->wiener_win != 5)
        return refuse("svt_hip_wiener_pick_plane: wiener_win %d is neither 7 nor 5", prm->wiener_win);
    if (const int32_t rc = pick_plane_ok("svt_hip_wiener_pick_plane", prm->bit_depth, prm->is_16bit, prm->plane_width, prm->plane_height); rc != SVT_HIP_OK)
        return rc;
    int max_tiles = 0;
    if (const int32_t rc = pick_units_ok("svt_hip_wiener_pick_plane", units, n_units, prm->plane_width, prm->plane_height, 4096,
                                         [&](uint32_t, const SvtHipWienerUnit &, int uw, int uh) { max_tiles = std::max(max_tiles, ((uw + 63) >> 6) * ((uh + 63) >> 6)); });
        rc != SVT_HIP_OK)
        return rc;
    if (workspace_bytes < svt_hip_wiener_pick_workspace_bytes(n_units) || ((uintptr_t)d_workspace & 7) || ((uintptr_t)d_result & 7) ||
        ((uintptr_t)d_unit_records & 7))
        return refuse("svt_hip_wiener_pick_plane: workspace of %llu bytes, %llu needed (workspace, records and result 8-byte aligned)",
                      (unsigned long long)workspace_bytes, (unsigned long long)svt_hip_wiener_pick_workspace_bytes(n_units));
    TierBCall               c("svt_hip_wiener_pick_plane", stream);
    const SvtHipWienerUnit *d_units = (const SvtHipWienerUnit *)c.stage(units, sizeof(SvtHipWienerUnit) * n_units);
    if (!c.ok())
        return c.status();
    hipStream_t st    = c.stream();
    State      *start = (State *)d_workspace;
    if (prm->wiener_win == 7)
        hipLaunchKernelGGL(wpick_solve<7>, dim3(n_units), dim3(256), 0, st, (const long long *)d_M, (const long long *)d_H, d_prev_units, start);
    else
        hipLaunchKernelGGL(wpick_solve<5>, dim3(n_units), dim3(256), 0, st, (const long long *)d_M, (const long long *)d_H, d_prev_units, start);
    SearchPrm sp{(int)prm->plane_width, (int)prm->plane_height, prm->is_16bit ? 1 : 0, prm->bit_depth, 3, 11, (7 - prm->wiener_win) >> 1,
                 prm->use_refinement ? 1 : 0, prm->max_one_refinement_step ? 1 : 0};
    const int range = prm->bit_depth + 7 - sp.r0 + 2;  // get_conv_params_wiener (convolve.h:70-86)
    if (range > 16)
        sp.r0 += range - 16, sp.r1 -= range - 16;
    const int trials = trial_bound(sp.plane_off, sp.use_refinement, sp.max_one_step);
    for (int t = 0; t < trials; t++) hipLaunchKernelGGL(wpick_trial, dim3((unsigned)max_tiles, n_units), dim3(256), 0, st, d_units, start, sp);
    hipLaunchKernelGGL(wpick_decide, dim3(1), dim3(256), 0, st, (const State *)start, d_unit_records, (int)n_units, prm->wiener_win, prm->rdmult,
                       prm->wiener_restore_cost[0], prm->wiener_restore_cost[1], d_result, d_lr_units);
    return c.finish();
}

SVT_HIP_MODULE_WARMUP(loopfilter_wiener_pick)
