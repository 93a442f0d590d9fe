"""Seeded cases for svt_hip_wiener_pick_plane and a plain Python driver of the Wiener decision of one plane (restoration_pick.c:
search_wiener_seg :1296-1378 with wiener_decompose_sep_sym, finalize_sym_filter, compute_score and finer_tile_search_wiener_seg;
search_wiener_finish :1380-1431; rest_finish_search :1555-1625 for NONE against WIENER) (test infrastructure).  The driver works in
Python integers with C's truncating division and asserts that nothing leaves the int64 range; the leaves under it -- statistics,
the separable filter, the SSE -- are functions it is GIVEN: the reference's own through its dispatch pointers, or the oracle's.
Planes are regenerated from the seeds; tests/golden/wiener_pick.npz stores results only."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

import lf_cases as L
import sgr_cases as G
from lf_cases import P, V
from svtav1_hip import abi

I64 = 1 << 63
SCALE, STEP = 1 << 16, 128                     # WIENER_TAP_SCALE_FACTOR, WIENER_FILT_STEP
TAP_MIN, TAP_MAX = (-5, -23, -17), (10, 8, 46)  # WIENER_FILT_TAPn_MINV / _MAXV (restoration.h:143-149)
INIT = (3, -7, 15, 106, 15, -7, 3)            # WIENER_FILT_TAPn_MIDV
NONE, WIENER = 0, 1
INT64_MAX = I64 - 1
B = G.B                                       # border of the degraded plane, edge-replicated as svt_extend_frame leaves it
UNIT_DTYPE, RESULT_DTYPE, LR_DTYPE = abi.WIENER_PICK_UNIT_DTYPE, abi.WIENER_PICK_RESULT_DTYPE, abi.LR_UNIT_DTYPE
# wn_filter_lvl -> (use_refinement, max_one_refinement_step, use_prev_frame_coeffs) (enc_mode_config.c:1330-1385)
LEVELS = {1: (1, 0, 0), 2: (1, 1, 0), 4: (0, 1, 0), 5: (0, 1, 0), 6: (0, 1, 1)}
# what a unit's rectangle of the degraded plane holds, one letter per unit in raster order (cycled):
#   b  the source blurred, plus noise: the filter helps, moves are accepted      s  the source itself: NONE wins
#   f  one value (and three samples around the unit): zero statistics, zero pivot, the taps stay at their start values
#   h  the source blurred hard: the solver's taps reach their clip limits        u  noise unrelated to the source
#   n  the source plus strong noise                                              i  the source inverted
#   p  one value with a few samples one step above it, unrelated to the source    q  the source with a few samples changed
#      (p and q leave statistics so small or so close to the identity that the quantised filter can score worse than none)
Case = namedtuple("Case", "name w h unit bd is16 win lvl rdmult cost kinds seed")
CASES = [
    Case("luma8_w7_l1", 200, 136, 64, 8, 0, 7, 1, 900, (180, 1100), "bnhsfp", 1),
    Case("luma10_w7_l2", 200, 136, 64, 10, 1, 7, 2, 2500, (200, 1000), "hbfnqp", 101),
    Case("luma8_w5_l4", 200, 136, 64, 8, 0, 5, 4, 1200, (150, 1200), "bqupnhf", 3),
    Case("luma10_w5_l6", 200, 136, 64, 10, 1, 5, 6, 4000, (256, 900), "bbnhsf", 4),
    Case("chroma8_w5_l1", 100, 68, 32, 8, 0, 5, 1, 700, (300, 800), "nbhfqp", 5),
    Case("chroma10_w5_l2", 100, 68, 32, 10, 1, 5, 2, 3000, (220, 1000), "sbpuhq", 110),
    Case("one8_w7_l1", 72, 40, 64, 8, 0, 7, 1, 600, (200, 1000), "b", 7),
    Case("one10_w5_l6", 72, 40, 64, 10, 1, 5, 6, 60000, (200, 1000), "n", 8),
    Case("tall8_w7_l2", 72, 150, 64, 8, 0, 7, 2, 1000, (190, 1050), "hn", 9),
    Case("tall10_w7_l1", 136, 150, 64, 10, 1, 7, 1, 8000, (170, 1150), "ipbq", 10),
    Case("none8_w7_l4", 200, 136, 64, 8, 0, 7, 4, 1 << 30, (100, 4000), "bnbhsb", 11),
    Case("luma8_w7_l6", 200, 136, 64, 8, 0, 7, 6, 1500, (180, 1100), "bnbhub", 12),
]


def unit_limits(w, h, unit, ss):
    """(h_start, h_end, v_start, v_end) of every restoration unit in raster order, the picture as one tile
    (foreach_rest_unit_in_tile, restoration.c:1250-1294)."""
    def spans(size):
        out, x0 = [], 0
        while x0 < size:
            n = size - x0 if size - x0 < unit * 3 // 2 else unit
            out.append((x0, x0 + n))
            x0 += n
        return out
    rows, off = [], 8 >> ss                      # RESTORATION_UNIT_OFFSET >> ss_y
    for y0, y1 in spans(h):
        rows.append((max(0, y0 - off), y1 - off if y1 < h else y1))
    return [(x0, x1, y0, y1) for y0, y1 in rows for x0, x1 in spans(w)]


class Inputs:
    """One case: src [h][w], dgd [h + 2B][w + 2B] (the plane with its replicated border), limits, prev (LR units or None)."""


def _blur(a, n):
    a = a.astype(np.float64)
    for _ in range(n):
        p = np.pad(a, 1, mode="edge")
        a = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + 4 * p[1:-1, 1:-1]) / 8.0
    return a


def make_inputs(case):
    rng = np.random.default_rng(8800 + case.seed)
    w, h, bd, top = case.w, case.h, case.bd, (1 << case.bd) - 1
    dt, sc = (np.uint16 if case.is16 else np.uint8), 1 << (bd - 8)
    src = np.clip(L.smooth_plane(rng, w, h, bd) + rng.integers(-24, 25, size=(h, w)) * sc, 0, top)
    x = Inputs()
    x.case, x.ss = case, int(case.name.startswith("chroma"))
    x.limits = unit_limits(w, h, case.unit, x.ss)
    kinds = {"b": _blur(src, 2) + rng.integers(-2, 3, size=(h, w)) * sc, "s": src, "f": np.full((h, w), float(rng.integers(top // 4, top // 2))),
             "h": _blur(src, 12), "u": rng.integers(0, top + 1, size=(h, w)).astype(np.float64),
             "n": src + rng.normal(0, 14 * sc, size=(h, w)), "i": top - src,
             "p": top // 2 + (rng.random((h, w)) < 0.02) * sc, "q": src + (rng.random((h, w)) < 0.01) * 3 * sc}
    dgd = np.zeros((h, w))
    x.kinds = [case.kinds[i % len(case.kinds)] for i in range(len(x.limits))]
    for (x0, x1, y0, y1), k in zip(x.limits, x.kinds):
        dgd[y0:y1, x0:x1] = kinds[k][y0:y1, x0:x1]
    for (x0, x1, y0, y1), k in zip(x.limits, x.kinds):           # flat units last, with the three samples the window reaches
        if k == "f":
            dgd[max(y0 - 3, 0):y1 + 3, max(x0 - 3, 0):x1 + 3] = kinds[k][0, 0]
    x.src = np.ascontiguousarray(src.astype(dt))
    x.dgd = np.ascontiguousarray(np.pad(np.clip(np.rint(dgd), 0, top).astype(dt), B, mode="edge"))
    x.refine, x.max_one, use_prev = LEVELS[case.lvl]
    x.prev = None
    if use_prev:                                                 # the previous frame's units: every second one is Wiener
        x.prev = np.zeros(len(x.limits), LR_DTYPE)
        for i, u in enumerate(x.prev):
            u["restoration_type"] = (1, 0, 1, 2)[(i + case.seed) % 4]
            f = [G.wiener_filter(rng)[0].copy() for _ in range(2)]
            for t in f:
                if case.win == 5:
                    t[3] += 2 * t[0]
                    t[0] = t[6] = 0
            u["hfilter"], u["vfilter"] = f
            u["ep"], u["xqd"] = int(rng.integers(0, 16)), (int(rng.integers(-96, 32)), int(rng.integers(-32, 96)))
    return x


def params(x):
    c = x.case
    return abi.WienerPickParams(c.win, c.is16, c.bd, c.w, c.h, x.refine, x.max_one, c.rdmult, (C.c_int32 * 2)(*c.cost))


def wiener_units(x, dgd_ptr, src_ptr):
    """The host array both svt_hip_wiener_stats and svt_hip_wiener_pick_plane take; the pointers are sample (0, 0) of the planes."""
    arr = (abi.WienerUnit * len(x.limits))()
    for i, (hs, he, vs, ve) in enumerate(x.limits):
        arr[i] = abi.WienerUnit(dgd_ptr, src_ptr, x.dgd.shape[1], x.src.shape[1], hs, he, vs, ve)
    return arr


# ------------------------------------------------------------------------------------------------ the leaves
def _enc(addr, is16):
    return V(addr >> 1) if is16 else V(addr)            # CONVERT_TO_BYTEPTR


def _aligned_kernel(f):
    buf = np.zeros(8 + 128, np.int16)
    off = (-buf.ctypes.data % 256) // 2                  # the reference reads its kernels through a 256-byte aligned base (convolve.c:45-54)
    buf[off:off + 8] = f
    return buf[off:off + 8], buf


class Leaves:
    """stats(limits) -> (M, H); filtered(hf, vf, limits) -> the unit's rectangle filtered in 64 x 64 tiles; sse(a, b) -> int."""

    def __init__(self, x):
        self.x, c = x, x.case
        self.bd, self.is16, self.win = c.bd, c.is16, c.win
        self.r0, self.r1 = G.wiener_rounds(c.bd)
        self.dgd0 = G.at(x.dgd)

    def filtered(self, hf, vf, limits):
        hs, he, vs, ve = limits
        out = np.zeros((ve - vs, he - hs + 16), self.x.dgd.dtype)
        fx, keepx = _aligned_kernel(hf)
        fy, keepy = _aligned_kernel(vf)
        isz, ds = out.itemsize, self.x.dgd.shape[1]
        for y in range(vs, ve, 64):
            for xx in range(hs, he, 64):
                self.convolve(self.dgd0 + (y * ds + xx) * isz, ds, out.ctypes.data + ((y - vs) * out.shape[1] + xx - hs) * isz, out.shape[1],
                              fx, fy, min(64, he - xx), min(64, ve - y))
        return out[:, :he - hs]


class RefLeaves(Leaves):
    """The reference's own functions through its dispatch pointers (oracle/_ref/libsvtref.so)."""

    def __init__(self, x, ref):
        super().__init__(x)
        i32, sz = C.c_int32, C.c_ssize_t
        if self.is16:
            self.f_stats = L.rtcd(ref, "svt_av1_compute_stats_highbd", None, i32, V, V, i32, i32, i32, i32, i32, i32, V, V, i32)
            self.f_conv = L.rtcd(ref, "svt_av1_highbd_wiener_convolve_add_src", None, V, sz, V, sz, V, V, i32, i32, V, i32)
            self.f_sse = L.rtcd(ref, "svt_aom_highbd_sse", C.c_int64, V, C.c_int, V, C.c_int, C.c_int, C.c_int)
        else:
            self.f_stats = L.rtcd(ref, "svt_av1_compute_stats", None, i32, V, V, i32, i32, i32, i32, i32, i32, V, V)
            self.f_conv = L.rtcd(ref, "svt_av1_wiener_convolve_add_src", None, V, sz, V, sz, V, V, i32, i32, V)
            self.f_sse = L.rtcd(ref, "svt_aom_sse", C.c_int64, V, C.c_int, V, C.c_int, C.c_int, C.c_int)
        self.cp = abi.ConvolveParams(round_0=self.r0, round_1=self.r1)

    def stats(self, limits):
        M, H = np.zeros(49, np.int64), np.zeros(49 * 49, np.int64)
        extra = (self.bd,) if self.is16 else ()
        self.f_stats(self.win, _enc(self.dgd0, self.is16), _enc(self.x.src.ctypes.data, self.is16), *limits, self.x.dgd.shape[1], self.x.src.shape[1],
                     P(M), P(H), *extra)
        return M, H

    def convolve(self, src, ss, dst, ds, fx, fy, w, h):
        extra = (self.bd,) if self.is16 else ()
        self.f_conv(_enc(src, self.is16), ss, _enc(dst, self.is16), ds, P(fx), P(fy), w, h, C.byref(self.cp), *extra)

    def sse(self, a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return int(self.f_sse(P(a), a.shape[1], P(b), b.shape[1], a.shape[1], a.shape[0]))   # the high-bit-depth one casts plain addresses


class OrcLeaves(Leaves):
    """The oracle's restatements (orc_wiener_compute_stats, orc_wiener_convolve_add_src); the SSE is the plain sum."""

    def __init__(self, x, orc):
        super().__init__(x)
        self.orc = orc

    def stats(self, limits):
        M, H = np.zeros(49, np.int64), np.zeros(49 * 49, np.int64)
        self.orc.orc_wiener_compute_stats(self.win, V(self.dgd0), P(self.x.src), *limits, self.x.dgd.shape[1], self.x.src.shape[1], P(M), P(H),
                                          self.is16, self.bd)
        return M, H

    def convolve(self, src, ss, dst, ds, fx, fy, w, h):
        self.orc.orc_wiener_convolve_add_src(V(src), ss, V(dst), ds, P(fx), P(fy), w, h, self.r0, self.r1, self.bd, self.is16)

    def sse(self, a, b):
        d = a.astype(np.int64) - b.astype(np.int64)
        return int((d * d).sum())


# ------------------------------------------------------------------------------------------------ the solver, in C's integers
def chk(v):
    assert -I64 <= v < I64, "an intermediate leaves the int64 range"
    return v


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def i16(v):
    v &= 0xFFFF
    return v - (1 << 16) if v >> 15 else v


def _tdiv_arr(a, d):
    """Truncating division of an int64 array by a positive constant."""
    return np.sign(a) * (np.abs(a) // d)


def _mul(a, b):
    """Elementwise int64 product, asserted to stay in range."""
    assert int(np.abs(a).max(initial=0)) * int(np.abs(b).max(initial=0)) < I64, "an intermediate leaves the int64 range"
    return a * b


def _bins(terms, idx, n):
    assert int(np.abs(terms).sum(dtype=object)) < I64, "an intermediate leaves the int64 range"
    out = [0] * n
    for t, i in zip(terms.ravel().tolist(), np.broadcast_to(idx, terms.shape).ravel().tolist()):
        out[i] += t
    return out


def linsolve(n, A, stride, b, x):
    """linsolve_wiener (:766-803), literally.  A and b are modified; 0 = a zero pivot, x untouched from there on."""
    for k in range(n - 1):
        for i in range(n - 1, k, -1):
            if abs(A[(i - 1) * stride + k]) < abs(A[i * stride + k]):
                for j in range(n):
                    A[i * stride + j], A[(i - 1) * stride + j] = A[(i - 1) * stride + j], A[i * stride + j]
                b[i], b[i - 1] = b[i - 1], b[i]
        for i in range(k, n - 1):
            if A[k * stride + k] == 0:
                return 0
            c, cd = A[(i + 1) * stride + k], A[k * stride + k]
            for j in range(n):
                A[(i + 1) * stride + j] = chk(A[(i + 1) * stride + j] - chk(tdiv(chk(tdiv(c, 256) * A[k * stride + j]), cd) * 256))
            b[i + 1] = chk(b[i + 1] - tdiv(chk(c * b[k]), cd))
    for i in range(n - 1, -1, -1):
        if A[i * stride + i] == 0:
            return 0
        c = 0
        for j in range(i + 1, n):
            c = chk(c + tdiv(chk(A[i * stride + j] * x[j]), SCALE))
        x[i] = i32(tdiv(chk(SCALE * chk(b[i] - c)), A[i * stride + i]))
    return 1


def _update(win, M, H, fixed, which):
    """update_a_sep_sym (which = 0: `fixed` is b) / update_b_sep_sym (which = 1: `fixed` is a) (:805-904) -> the new vector or None."""
    w2, hw1 = win * win, (win >> 1) + 1
    wrap = np.array([win - 1 - i if i >= hw1 else i for i in range(win)])
    f = np.array(fixed[:win], np.int64)
    M2, H4 = M[:w2].reshape(win, win), H[:w2 * w2].reshape(win, win, win, win)
    if which == 0:      # A[wrap(j)] += M[i][j] * b[i] / S;  B[wrap(l)][wrap(k)] += H4[j, k, i, l] * b[i] / S * b[j] / S
        A = _bins(_tdiv_arr(_mul(M2, f[:, None]), SCALE), wrap[None, :], hw1)
        t = _tdiv_arr(_mul(_tdiv_arr(_mul(H4, f[None, None, :, None]), SCALE), f[:, None, None, None]), SCALE)
        Bm = _bins(t, (wrap[None, None, None, :] * hw1 + wrap[None, :, None, None]), hw1 * hw1)
    else:               # A[wrap(i)] += M[i][j] * a[j] / S;  B[wrap(j)][wrap(i)] += H4[i, k, j, l] * a[k] / S * a[l] / S
        A = _bins(_tdiv_arr(_mul(M2, f[None, :]), SCALE), wrap[:, None], hw1)
        t = _tdiv_arr(_mul(_tdiv_arr(_mul(H4, f[None, :, None, None]), SCALE), f[None, None, None, :]), SCALE)
        Bm = _bins(t, (wrap[None, None, :, None] * hw1 + wrap[:, None, None, None]), hw1 * hw1)
    last = hw1 - 1
    a_last = A[last]
    for i in range(last):
        A[i] = chk(A[i] - chk(a_last * 2 + Bm[i * hw1 + last] - 2 * Bm[last * hw1 + last]))
    for i in range(last):
        for j in range(last):
            Bm[i * hw1 + j] = chk(Bm[i * hw1 + j] - 2 * chk(Bm[i * hw1 + last] + Bm[last * hw1 + j] - 2 * Bm[last * hw1 + last]))
    S = [0] * 7
    if not linsolve(last, Bm, hw1, A, S):
        return None
    S[last] = SCALE
    for i in range(hw1, win):
        S[i] = S[win - 1 - i]
        S[last] = i32(S[last] - 2 * S[i])
    return S[:win]


def finalize(win, f):
    """finalize_sym_filter (:977-1006) -> the 8 stored coefficients."""
    fi = [0] * 8
    for i in range(win >> 1):
        d = f[i] * STEP
        fi[i] = i16(tdiv(d - SCALE // 2, SCALE) if d < 0 else tdiv(d + SCALE // 2, SCALE))
    clip = lambda v, p: min(max(v, TAP_MIN[p]), TAP_MAX[p])
    if win == 7:
        fi[0], fi[1], fi[2] = clip(fi[0], 0), clip(fi[1], 1), clip(fi[2], 2)
    else:
        fi[2] = clip(fi[1], 2)
        fi[1] = clip(fi[0], 1)
        fi[0] = 0
    fi[6], fi[5], fi[4] = fi[0], fi[1], fi[2]
    fi[3] = -2 * (fi[0] + fi[1] + fi[2])
    return fi


def compute_score(win, M, H, vfilt, hfilt):
    """compute_score (:937-975)"""
    w2, off = win * win, (7 - win) >> 1
    a, b = list(vfilt[:7]), list(hfilt[:7])
    a[3], b[3] = STEP - 2 * sum(vfilt[:3]), STEP - 2 * sum(hfilt[:3])
    ab = np.array([a[l + off] * b[k + off] for k in range(win) for l in range(win)], np.int64)
    P_ = int(_tdiv_arr(_tdiv_arr(_mul(ab, M[:w2]), STEP), STEP).sum(dtype=object))
    t = _mul(_mul(H[:w2 * w2].reshape(w2, w2), ab[:, None]), ab[None, :])
    for _ in range(4):
        t = _tdiv_arr(t, STEP)
    assert int(np.abs(t).sum(dtype=object)) < I64
    Q = int(t.sum(dtype=object))
    mid = w2 >> 1
    return chk(chk(Q - 2 * P_) - chk(int(H[mid * w2 + mid]) - 2 * int(M[mid])))


_solved = {}


def solve(win, M, H):
    """wiener_decompose_sep_sym + finalize_sym_filter + compute_score -> (vfilter[8], hfilter[8], score, zero pivots met)."""
    key = (win, M.tobytes(), H.tobytes())
    if key not in _solved:
        off = (7 - win) >> 1
        a = [SCALE // STEP * INIT[i + off] for i in range(win)]
        b = list(a)
        zero = 0
        for _ in range(4):                               # NUM_WIENER_ITERS - 1
            s = _update(win, M, H, b, 0)
            a, zero = (s, zero) if s else (a, zero + 1)
            s = _update(win, M, H, a, 1)
            b, zero = (s, zero) if s else (b, zero + 1)
        v, h = finalize(win, a), finalize(win, b)
        _solved[key] = (v, h, compute_score(win, M, H, v, h), zero)
    return _solved[key]


# ------------------------------------------------------------------------------------------------ the search and the decision
def count_refsubexpfin(n, k, ref, v):
    """svt_aom_count_primitive_refsubexpfin (entropy_coding.c:2805-2951)"""
    def recenter(r, v):
        return v if v > (r << 1) else ((v - r) << 1 if v >= r else ((r - v) << 1) - 1)
    v = recenter(ref, v) if (ref << 1) <= n else recenter(n - 1 - ref, n - 1 - v)
    count = i = mk = 0
    while True:
        b = k + i - 1 if i else k
        a = 1 << b
        if n <= mk + 3 * a:
            nn, vv = n - mk, v - mk
            if nn > 1:
                l = (nn - 1).bit_length()
                count += l - 1 if vv < (1 << l) - nn else l
            return count
        count += 1
        if v >= mk + a:
            i, mk = i + 1, mk + a
        else:
            return count + b


def count_wiener_bits(win, v, h, ref_v, ref_h):
    """count_wiener_bits (:1008-1037)"""
    return sum(count_refsubexpfin(TAP_MAX[p] - TAP_MIN[p] + 1, p + 1, r[p] - TAP_MIN[p], f[p] - TAP_MIN[p])
               for f, r in ((v, ref_v), (h, ref_h)) for p in range(0 if win == 7 else 1, 3))


def rdcost_dbl(rdmult, rate, dist):
    """RDCOST_DBL (restoration.h:346): IEEE doubles, no contraction"""
    return ((float(rate) * float(rdmult)) / 512.0) + (float(dist) * 128.0)


def finer_search(x, leaves, limits, hf, vf, cover):
    """finer_tile_search_wiener_seg (:1042-1147) -> (err, trials); hf / vf are moved in place."""
    hs, he, vs, ve = limits
    src = x.src[vs:ve, hs:he]
    trial = lambda: leaves.sse(leaves.filtered(hf, vf, limits), src)
    err, trials = trial(), 1
    if not x.refine:
        return err, trials
    off = (7 - x.case.win) >> 1

    def move(f, p, d):
        f[p] += d
        f[6 - p] += d
        f[3] -= 2 * d
    s = 4
    while s >= (4 if x.max_one else 1):
        for f in (hf, vf):
            for p in range(off, 3):
                skip = False
                for d in (-1, 1):
                    again = 0
                    while f[p] - s >= TAP_MIN[p] if d < 0 else f[p] + s <= TAP_MAX[p]:
                        move(f, p, d * s)
                        err2 = trial()
                        trials += 1
                        if err2 > err:
                            move(f, p, -d * s)
                            break
                        err, skip = err2, skip or d < 0
                        cover["move%d" % s] += 1
                        cover["repeat4"] += again > 0
                        if not (s == 4 and not x.max_one):
                            break
                        again += 1                      # at the highest step size continue moving in the same direction
                    if skip:
                        break
                if skip:
                    cover["break"] += p < 2             # taps of this filter are left unvisited at this step size
                    break
        s >>= 1
    return err, trials


def prev_usable(win, rec):
    """A previous-frame record the entry point takes: RESTORE_WIENER with every coded tap inside its range (the reference's records
    always are; the number of launches is derived from the ranges, so anything else is solved like a unit without a record)."""
    off = (7 - win) >> 1
    return bool(rec["restoration_type"] == WIENER and all(
        (f[p] == 0 if p < off else TAP_MIN[p] <= f[p] <= TAP_MAX[p]) for f in (rec["hfilter"], rec["vfilter"]) for p in range(3)))


COVER = ("break", "repeat4", "move4", "move2", "move1", "rejected", "zero_pivot", "clip", "prev")
FIELDS = ("units", "result", "lr_units", "cover")


def drive(x, leaves):
    """The whole decision of the plane of `x` -> dict: `units` (UNIT_DTYPE [n]), `result` (one RESULT_DTYPE record), `lr_units`
    (LR_DTYPE [n]) and, for the checks on the cases alone, `cover` (int32 [n][len(COVER)]: how often each thing happened in a unit)."""
    case, n = x.case, len(x.limits)
    units, lr, cover_out = np.zeros(n, UNIT_DTYPE), np.zeros(n, LR_DTYPE), np.zeros((n, len(COVER)), np.int32)
    res = np.zeros((), RESULT_DTYPE)
    ref_v, ref_h = list(INIT), list(INIT)                # set_default_wiener
    sse_n = sse_w = bits_w = 0
    bits_none = case.cost[0]
    for i, limits in enumerate(x.limits):
        cover = dict.fromkeys(COVER, 0)
        hs, he, vs, ve = limits
        u = units[i]
        u["sse"][NONE] = leaves.sse(x.dgd[B + vs:B + ve, B + hs:B + he], x.src[vs:ve, hs:he])
        keep = True
        if x.prev is not None and prev_usable(case.win, x.prev[i]):
            vf, hf = [int(t) for t in x.prev[i]["vfilter"]], [int(t) for t in x.prev[i]["hfilter"]]
            cover["prev"] = 1
        else:
            M, H = leaves.stats(limits)
            vf, hf, score, cover["zero_pivot"] = solve(case.win, M, H)
            vf, hf = list(vf), list(hf)
            cover["clip"] = sum(f[p] in (TAP_MIN[p], TAP_MAX[p]) for f in (vf, hf) for p in range((7 - case.win) >> 1, 3))
            keep = not score > 0
        sse_n += int(u["sse"][NONE])
        if not keep:
            cover["rejected"] = 1
            u["sse"][WIENER], u["bits"] = INT64_MAX, bits_none
            bits_w, sse_w = bits_w + bits_none, sse_w + int(u["sse"][NONE])
        else:
            err, trials = finer_search(x, leaves, limits, hf, vf, cover)
            u["sse"][WIENER], u["hfilter"], u["vfilter"], u["trials"] = err, hf, vf, trials
            bits_wiener = case.cost[1] + (count_wiener_bits(case.win, vf, hf, ref_v, ref_h) << 9)
            wiener = rdcost_dbl(case.rdmult, bits_wiener >> 4, err) < rdcost_dbl(case.rdmult, bits_none >> 4, int(u["sse"][NONE]))
            u["bits"], u["best_rtype"] = bits_wiener, int(wiener)
            sse_w, bits_w = sse_w + (err if wiener else int(u["sse"][NONE])), bits_w + (bits_wiener if wiener else bits_none)
            if wiener:
                ref_v, ref_h = vf, hf
        cover_out[i] = [cover[k] for k in COVER]
    res["sse"], res["bits"] = (chk(sse_n), chk(sse_w)), (0, chk(bits_w))
    res["cost"] = (rdcost_dbl(case.rdmult, 0, sse_n), rdcost_dbl(case.rdmult, bits_w >> 4, sse_w))
    res["frame_restoration_type"] = int(res["cost"][WIENER] < res["cost"][NONE])
    res["n_wiener"] = int(units["best_rtype"].sum())
    for i in range(n):
        if res["frame_restoration_type"] == WIENER and units[i]["best_rtype"] == WIENER:
            lr[i]["restoration_type"], lr[i]["hfilter"], lr[i]["vfilter"] = WIENER, units[i]["hfilter"], units[i]["vfilter"]
    return {"units": units, "result": res, "lr_units": lr, "cover": cover_out}


def same(a, b, fields=FIELDS):
    """The names of the fields in which two driver / fixture / device outputs differ, bit for bit (the doubles included)."""
    return [f for f in fields if not (a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes())]


_golden = {}


def golden(case):
    """The recorded results of one case (tests/golden/wiener_pick.npz, written by tests/golden/make_golden_wiener_pick.py)."""
    if not _golden:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wiener_pick.npz")) as g:
            _golden.update({k: g[k] for k in g.files})
    return {f: _golden[f"{case.name}_{f}"] for f in FIELDS}


class Pin:
    """tests/wiener_pick_pin_driver.c (the reference's own static solver, score, bit count and RDCOST_DBL) built into `directory`
    against oracle/_ref/libsvtref.so."""

    def __init__(self, ref, directory):
        from support import build_pin
        self.ref, self.lib = ref, build_pin(directory, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wiener_pick_pin_driver.c"))
        self.lib.pin_wiener_solve.restype, self.lib.pin_rdcost_dbl.restype = C.c_int64, C.c_double
        self.lib.pin_rdcost_dbl.argtypes = [C.c_int32, C.c_int64, C.c_int64]

    def constants(self):
        out = np.zeros(15, np.int64)
        self.lib.pin_constants(P(out))
        return [int(v) for v in out]

    def solve(self, win, M, H):
        """-> (vfilter[8], hfilter[8], score) as search_wiener_seg gets them (:1349-1361)"""
        out, taps = np.zeros(16, np.int16), np.zeros(14, np.int32)
        score = self.lib.pin_wiener_solve(win, P(M), P(H), P(out), P(taps))
        return [int(v) for v in out[:8]], [int(v) for v in out[8:]], int(score)

    def count_bits(self, win, v, h, ref_v, ref_h):
        a = [np.array(list(f[:7]) + [0], np.int16) for f in (v, h, ref_v, ref_h)]
        return int(self.lib.pin_count_wiener_bits(win, *[P(f) for f in a]))

    def rdcost_dbl(self, rdmult, rate, dist):
        return float(self.lib.pin_rdcost_dbl(rdmult, rate, dist))


ARGS = ("prm", "units", "d_M", "d_H", "d_unit_records", "d_result", "d_lr_units", "d_workspace")


def rejections(x):
    """(label, change of the parameters, change of unit 0's limits, argument to pass as NULL, n_units or None, bytes to take off the
    workspace size): every call svt_hip_wiener_pick_plane must refuse with SVT_HIP_ERR_BAD_PARAMETER."""
    for a in ARGS:
        yield f"NULL {a}", {}, {}, a, None, 0
    yield "no units", {}, {}, None, 0, 0
    for v in (3, 6, 9, 0):
        yield f"window {v}", {"wiener_win": v}, {}, None, None, 0
    yield "bit depth 9", {"bit_depth": 9}, {}, None, None, 0
    yield "10 bit in bytes", {"bit_depth": 10, "is_16bit": 0}, {}, None, None, 0
    yield "empty plane", {"plane_width": 0}, {}, None, None, 0
    yield "unit wider than 4096", {"plane_width": 5000}, {"h_end": 4097}, None, None, 0
    yield "unit taller than 4096", {"plane_height": 5000}, {"v_end": 4097}, None, None, 0
    yield "unit past the plane", {}, {"h_end": x.case.w + 1}, None, None, 0
    yield "empty unit", {}, {"v_end": 0}, None, None, 0
    yield "workspace short", {}, {}, None, None, 1
