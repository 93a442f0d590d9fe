"""Seeded cases for svt_hip_rest_pick_plane and a plain Python driver of the restoration decision of one plane with the self-guided
filter enabled (restoration_pick.c: search_sgrproj_seg :1220-1264 with search_selfguided_restoration, encode_xq and
finer_search_pixel_proj_error; try_restoration_unit_seg :129-165 without boundaries; search_wiener_finish :1380, search_sgrproj_finish
:1267, search_switchable :1148, rest_finish_search :1555-1625, copy_unit_info :1202) (test infrastructure).  The driver works in
Python integers; the leaves under it -- the self-guided filter, svt_get_proj_subspace, the projection error,
svt_apply_selfguided_restoration, the SSE -- are functions it is GIVEN: the reference's own through its dispatch pointers, or the
oracle's.  The Wiener side of a plane is wiener_pick_cases.drive.  Planes are regenerated from the seeds; tests/golden/rest_pick.npz
stores results only."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

import lf_cases as L
import wiener_pick_cases as W
from lf_cases import P, V
from svtav1_hip import abi

NONE, WIENER, SGRPROJ, SWITCHABLE = 0, 1, 2, 3
INT64_MAX = W.INT64_MAX
B = W.B
PRJ_BITS, PRJ_MIN, PRJ_MAX = 7, (-96, -32), (31, 95)            # SGRPROJ_PRJ_BITS, _MIN0 / _MIN1, _MAX0 / _MAX1 (restoration.h:94-104)
PRJ_DEFAULT = (-32, 31)                                         # set_default_sgrproj: (MIN + MAX) / 2 in C
SGR_R = [(2, 1)] * 10 + [(0, 1)] * 4 + [(2, 0)] * 2             # the radii of svt_aom_eb_sgr_params
UNIT_DTYPE, RESULT_DTYPE, LR_DTYPE = abi.REST_PICK_UNIT_DTYPE, abi.REST_PICK_RESULT_DTYPE, abi.LR_UNIT_DTYPE
EP_ALL, EP_STEP8, EP_4_5 = (0, 16, 1, 1), (0, 16, 8, 1), (4, 5, 1, 0)
# win: the window of the Wiener records, 0 = no records (Wiener not searched on this plane); ep = (start, end, inc, refine);
# cost_w / cost_s / cost_sw = x->wiener_restore_cost, sgrproj_restore_cost, switchable_restore_cost; kinds: as wiener_pick_cases
Case = namedtuple("Case", "name w h unit bd is16 ss win ep rdmult cost_w cost_s cost_sw kinds seed")
CASES = [
    Case("luma8_w7_all", 200, 136, 64, 8, 0, 0, 7, EP_ALL, 900, (180, 1100), (200, 1000), (300, 900, 1000), "mlhafg", 1),
    Case("luma10_w7_step8", 200, 136, 64, 10, 1, 0, 7, EP_STEP8, 2500, (200, 1000), (190, 1050), (280, 950, 900), "hbfnqp", 101),
    Case("luma8_now_all", 200, 136, 64, 8, 0, 0, 0, EP_ALL, 1200, (0, 0), (150, 1200), (0, 0, 0), "mlgunf", 3),
    Case("luma10_w5_45", 200, 136, 64, 10, 1, 0, 5, EP_4_5, 4000, (256, 900), (220, 1000), (320, 880, 960), "bbnhsf", 4),
    Case("chroma8_w5_all", 100, 68, 32, 8, 0, 1, 5, EP_ALL, 700, (300, 800), (260, 900), (350, 850, 900), "mahflg", 5),
    Case("chroma10_now_45", 100, 68, 32, 10, 1, 1, 0, EP_4_5, 3000, (0, 0), (220, 1000), (0, 0, 0), "sbpuhq", 110),
    Case("chroma10_w5_step8", 100, 68, 32, 10, 1, 1, 5, EP_STEP8, 2000, (220, 1000), (200, 1000), (300, 900, 950), "sbpuhq", 110),
    Case("one8_w7_all", 72, 40, 64, 8, 0, 0, 7, EP_ALL, 600, (200, 1000), (200, 1000), (300, 900, 900), "b", 7),
    Case("one10_now_step8", 72, 40, 64, 10, 1, 0, 0, EP_STEP8, 60000, (0, 0), (200, 1000), (0, 0, 0), "n", 8),
    Case("wide8_now_step8", 383, 40, 256, 8, 0, 0, 0, EP_STEP8, 1000, (0, 0), (190, 1050), (0, 0, 0), "h", 9),
    Case("wide10_w7_45", 383, 40, 256, 10, 1, 0, 7, EP_4_5, 8000, (170, 1150), (180, 1100), (290, 940, 920), "n", 10),
    Case("luma12_now_all", 200, 136, 64, 12, 1, 0, 0, EP_ALL, 20000, (0, 0), (200, 1000), (0, 0, 0), "bmfhul", 12),
    Case("none8_w7_45", 200, 136, 64, 8, 0, 0, 7, EP_4_5, 1 << 30, (100, 4000), (100, 4000), (100, 4000, 4000), "bnbhsb", 11),
    Case("wiener8_w7_45", 200, 136, 64, 8, 0, 0, 7, EP_4_5, 1500, (180, 1100), (180, 60000), (6000, 1100, 60000), "bhbhbh", 13),
    Case("sgr8_w7_step8", 200, 136, 64, 8, 0, 0, 7, EP_STEP8, 100000, (180, 60000), (180, 1100), (600, 60000, 1100), "nmsnam", 14),
]


def wiener_case(c):
    """The case wiener_pick_cases builds the planes (and, with a window, the Wiener records) from: level 2, one refinement step."""
    return W.Case(("chroma_" if c.ss else "plane_") + c.name, c.w, c.h, c.unit, c.bd, c.is16, c.win or 7, 2, c.rdmult, c.cost_w, c.kinds, c.seed)


EXTRA = "mlga"      # kinds beyond wiener_pick_cases': m / l  the source plus moderate / light noise (the 3 x 3 filter alone, or a mild
#                     projection, is best); g  the source quantised to steps of 4; a  the source with one sample in 20 pushed up


def make_inputs(case):
    """wiener_pick_cases.Inputs (src, dgd with its replicated border, limits, kinds) with .case replaced by `case` and .wcase added.
    Units of a kind in EXTRA are filled here, from a generator of their own, over what wiener_pick_cases put there."""
    wc = wiener_case(case)
    x = W.make_inputs(wc._replace(kinds="".join("s" if k in EXTRA else k for k in wc.kinds)))
    x.wcase, x.case = wc, case
    assert x.ss == case.ss
    rng = np.random.default_rng(9900 + case.seed)
    src, sc, top = x.src.astype(np.float64), 1 << (case.bd - 8), (1 << case.bd) - 1
    extra = {"m": src + rng.normal(0, 5 * sc, size=src.shape), "l": src + rng.normal(0, 2 * sc, size=src.shape),
             "g": np.floor(src / (4 * sc)) * 4 * sc + 2 * sc, "a": src + (rng.random(src.shape) < 0.05) * 60 * sc}
    inner = x.dgd[B:-B, B:-B].copy()
    x.kinds = [case.kinds[i % len(case.kinds)] for i in range(len(x.limits))]
    for (x0, x1, y0, y1), k in zip(x.limits, x.kinds):
        if k in extra:
            inner[y0:y1, x0:x1] = np.clip(np.rint(extra[k][y0:y1, x0:x1]), 0, top)
    x.dgd = np.ascontiguousarray(np.pad(inner, B, mode="edge"))
    return x


def n_ep(case):
    s, e, inc, _ = case.ep
    return (e - s + inc - 1) // inc


def params(x):
    c = x.case
    i2, i3 = C.c_int32 * 2, C.c_int32 * 3
    return abi.RestPickParams(c.is16, c.bd, c.w, c.h, c.ss, c.ss, c.win, *c.ep, c.rdmult, i2(*c.cost_w), i2(*c.cost_s), i3(*c.cost_sw))


def wiener_units(x, dgd_ptr, src_ptr):
    return W.wiener_units(x, dgd_ptr, src_ptr)


def wiener_records(x, leaves):
    """The unit records svt_hip_wiener_pick_plane leaves for this plane (None without a window), from wiener_pick_cases.drive."""
    if not x.case.win:
        return None
    x.case, keep = x.wcase, x.case
    try:
        return W.drive(x, leaves)["units"]
    finally:
        x.case = keep


def wiener_leaves(x, lib, kind):
    x.case, keep = x.wcase, x.case
    try:
        return (W.RefLeaves if kind == "ref" else W.OrcLeaves)(x, lib)
    finally:
        x.case = keep


# ------------------------------------------------------------------------------------------------ the leaves
def _enc(addr, is16):
    return V(addr >> 1) if is16 else V(addr)            # CONVERT_TO_BYTEPTR


class SgrParams(C.Structure):                            # SgrParamsType (definitions.h:1758-1761)
    _fields_ = [("r", C.c_int32 * 2), ("s", C.c_int32 * 2)]


class RefLeaves:
    """The reference's own functions through its dispatch pointers (oracle/_ref/libsvtref.so).  Addresses are plain; every call
    encodes them as the reference expects."""

    def __init__(self, x, ref):
        c, i32, ci = x.case, C.c_int32, C.c_int
        self.bd, self.is16 = c.bd, c.is16
        self.f_filter = L.rtcd(ref, "svt_av1_selfguided_restoration", None, V, i32, i32, i32, V, V, i32, i32, i32, i32)
        self.f_apply = L.rtcd(ref, "svt_apply_selfguided_restoration", None, V, i32, i32, i32, i32, V, V, i32, V, i32, i32)
        self.f_err = L.rtcd(ref, "svt_av1_highbd_pixel_proj_error" if c.is16 else "svt_av1_lowbd_pixel_proj_error", C.c_int64, V, i32, i32, i32,
                            V, i32, V, i32, V, i32, V, V)
        self.f_sub = L.rtcd(ref, "svt_get_proj_subspace", None, V, ci, ci, ci, V, ci, ci, V, ci, V, ci, V, V)
        self.f_sse = L.rtcd(ref, "svt_aom_highbd_sse" if c.is16 else "svt_aom_sse", C.c_int64, V, ci, V, ci, ci, ci)
        self.prm = (SgrParams * 16).in_dll(ref, "svt_aom_eb_sgr_params")
        self.tmp = np.zeros(2 * 161 * 1024, np.int32)    # SGRPROJ_TMPBUF_SIZE (restoration.h:84-87)

    def filter(self, dat, w, h, stride, f0, f1, fs, ep):
        self.f_filter(_enc(dat, self.is16), w, h, stride, V(f0), V(f1), fs, ep, self.bd, self.is16)

    def subspace(self, src, w, h, ss, dat, ds, f0, f1, fs, ep):
        xq = np.zeros(2, np.int32)
        self.f_sub(_enc(src, self.is16), w, h, ss, _enc(dat, self.is16), ds, self.is16, P(f0), fs, P(f1), fs, P(xq), C.addressof(self.prm[ep]))
        return [int(xq[0]), int(xq[1])]

    def error(self, src, w, h, ss, dat, ds, f0, f1, fs, xq, ep):
        q = np.array(xq, np.int32)
        return int(self.f_err(_enc(src, self.is16), w, h, ss, _enc(dat, self.is16), ds, P(f0), fs, P(f1), fs, P(q), C.addressof(self.prm[ep])))

    def apply(self, dat, w, h, stride, ep, xqd, dst, ds):
        q = np.array(xqd, np.int32)
        self.f_apply(_enc(dat, self.is16), w, h, stride, ep, P(q), _enc(dst, self.is16), ds, P(self.tmp), self.bd, self.is16)

    def sse(self, a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return int(self.f_sse(P(a), a.shape[1], P(b), b.shape[1], a.shape[1], a.shape[0]))   # the high-bit-depth one casts plain addresses


class OrcLeaves:
    """The oracle's restatements: orc_selfguided_restoration, orc_get_proj_subspace, orc_sgr_pixel_proj_error,
    orc_apply_selfguided_restoration; the SSE is the plain sum."""

    def __init__(self, x, orc):
        self.orc, self.bd, self.is16 = orc, x.case.bd, x.case.is16
        orc.orc_sgr_pixel_proj_error.restype = C.c_int64

    def filter(self, dat, w, h, stride, f0, f1, fs, ep):
        self.orc.orc_selfguided_restoration(V(dat), w, h, stride, V(f0), V(f1), fs, ep, self.bd, self.is16)

    def subspace(self, src, w, h, ss, dat, ds, f0, f1, fs, ep):
        xq = np.zeros(2, np.int32)
        self.orc.orc_get_proj_subspace(V(src), w, h, ss, V(dat), ds, self.is16, P(f0), fs, P(f1), fs, P(xq), ep)
        return [int(xq[0]), int(xq[1])]

    def error(self, src, w, h, ss, dat, ds, f0, f1, fs, xq, ep):
        q = np.array(xq, np.int32)
        return int(self.orc.orc_sgr_pixel_proj_error(V(src), w, h, ss, V(dat), ds, P(f0), fs, P(f1), fs, P(q), ep, self.is16))

    def apply(self, dat, w, h, stride, ep, xqd, dst, ds):
        q = np.array(xqd, np.int32)
        self.orc.orc_apply_selfguided_restoration(V(dat), w, h, stride, ep, P(q), V(dst), ds, self.bd, self.is16)

    def sse(self, a, b):
        d = a.astype(np.int64) - b.astype(np.int64)
        return int((d * d).sum())


# ------------------------------------------------------------------------------------------------ the search of one unit
def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def encode_xq(xq, ep):
    """encode_xq (:508-519)"""
    r = SGR_R[ep]
    if r[0] == 0:
        return [0, clamp((1 << PRJ_BITS) - xq[1], PRJ_MIN[1], PRJ_MAX[1])]
    x0 = clamp(xq[0], PRJ_MIN[0], PRJ_MAX[0])
    if r[1] == 0:
        return [x0, clamp((1 << PRJ_BITS) - x0, PRJ_MIN[1], PRJ_MAX[1])]
    return [x0, clamp((1 << PRJ_BITS) - x0 - xq[1], PRJ_MIN[1], PRJ_MAX[1])]


def decode_xq(xqd, ep):
    """svt_decode_xq (restoration.c:634-645)"""
    r = SGR_R[ep]
    if r[0] == 0:
        return [0, (1 << PRJ_BITS) - xqd[1]]
    if r[1] == 0:
        return [xqd[0], 0]
    return [xqd[0], (1 << PRJ_BITS) - xqd[0] - xqd[1]]


COVER = ("clamp", "full_tie", "keep2", "step1_only", "improved")


def finer_search(error, xqd, ep, refine):
    """finer_search_pixel_proj_error (:320-411) with start_step 2 -> (err, trials, cover); xqd is moved in place; error(xqd) -> int.
    cover: full_tie = a walk at step 2 whose every move tied and which ended at the clamp; keep2 = the longest run of accepted moves at
    step 2 in one direction; step1_only = strictly better moves were found at step 1 and none at step 2."""
    err, trials = error(xqd), 1
    better = {2: 0, 1: 0}
    cover = dict.fromkeys(COVER, 0)
    if refine:
        s = 2
        while s >= 1:
            for p in range(2):
                if SGR_R[ep][p] == 0:
                    continue
                skip = False
                for d in (-1, 1):
                    run, ties = 0, 0
                    while xqd[p] - s >= PRJ_MIN[p] if d < 0 else xqd[p] + s <= PRJ_MAX[p]:
                        xqd[p] += d * s
                        err2 = error(xqd)
                        trials += 1
                        if err2 > err:
                            xqd[p] -= d * s
                            break
                        better[s] += err2 < err
                        ties += err2 == err
                        err, skip, run = err2, skip or d < 0, run + 1
                        if s != 2:
                            break                        # only at the highest step size continue moving in the same direction
                    else:
                        if s == 2 and run >= 1 and ties == run:
                            cover["full_tie"] = 1       # the loop ended on the clamp, not on a worse error
                    if s == 2:
                        cover["keep2"] = max(cover["keep2"], run)
                    if skip:
                        break
                if skip:
                    break                               # `if (skip) break;` leaves the loop over p
            s >>= 1
    cover["clamp"] = sum(SGR_R[ep][p] > 0 and xqd[p] in (PRJ_MIN[p], PRJ_MAX[p]) for p in range(2))
    cover["step1_only"], cover["improved"] = int(better[1] > 0 and better[2] == 0), int(better[1] + better[2] > 0)
    return err, trials, cover


def _addr(a, y, x):
    return a.ctypes.data + (y * a.shape[1] + x) * a.itemsize


def search_unit(x, lv, limits):
    """search_selfguided_restoration (:550-652) over the candidates of the case -> (ep, xqd, err, trials, cover)"""
    hs, he, vs, ve = limits
    w, h, pu = he - hs, ve - vs, 64 >> x.ss
    fs = ((w + 7) & ~7) + 8
    f0, f1 = np.zeros((h, fs), np.int32), np.zeros((h, fs), np.int32)
    dat, src = _addr(x.dgd, B + vs, B + hs), _addr(x.src, vs, hs)
    ds, ss = x.dgd.shape[1], x.src.shape[1]
    start, end, inc, refine = x.case.ep
    best = None
    for ep in range(start, end, inc):
        for i in range(0, h, pu):                       # apply_sgr (:523-548): processing units from the unit's top-left
            for j in range(0, w, pu):
                lv.filter(_addr(x.dgd, B + vs + i, B + hs + j), min(pu, w - j), min(pu, h - i), ds, _addr(f0, i, j), _addr(f1, i, j), fs, ep)
        xqd = encode_xq(lv.subspace(src, w, h, ss, dat, ds, f0, f1, fs, ep), ep)
        err, trials, cover = finer_search(lambda q: lv.error(src, w, h, ss, dat, ds, f0, f1, fs, decode_xq(q, ep), ep), xqd, ep, refine)
        if best is None or err < best[2]:
            best = (ep, xqd, err, trials, cover)
    return best


def trial_sse(x, lv, limits, ep, xqd):
    """try_restoration_unit_seg (:129-165) without boundaries: svt_av1_loop_restoration_filter_unit's stripes (restoration.c:1094-1134) and
    svt_aom_sgrproj_filter_stripe's tiles over the picture's own samples, then the SSE against the source."""
    hs, he, vs, ve = limits
    w, h, pu, sh, off = he - hs, ve - vs, 64 >> x.ss, 64 >> x.ss, 8 >> x.ss
    out = np.zeros((h, w + 16), x.dgd.dtype)
    i = 0
    while i < h:
        v = vs + i
        n = min(((v + off) // sh + 1) * sh - off, ve) - v
        for j in range(0, w, pu):
            lv.apply(_addr(x.dgd, B + v, B + hs + j), min(pu, w - j), n, x.dgd.shape[1], ep, xqd, _addr(out, i, j), out.shape[1])
        i += n
    return lv.sse(out[:, :w], x.src[vs:ve, hs:he])


# ------------------------------------------------------------------------------------------------ the decision
def count_sgrproj_bits(ep, xqd, ref):
    """count_sgrproj_bits (:655-669)"""
    return 4 + sum(W.count_refsubexpfin(PRJ_MAX[p] - PRJ_MIN[p] + 1, 4, ref[p] - PRJ_MIN[p], xqd[p] - PRJ_MIN[p]) for p in range(2) if SGR_R[ep][p] > 0)


def decide(case, sse, taps, wbest, ep, xqd):
    """The finish visitors in raster order and rest_finish_search, from per-unit sse[n][3], Wiener taps[n] = (vfilter, hfilter) and
    best_rtype[WIENER - 1], ep[n], xqd[n] -> (best_rtype[n][3], tested mask, sse[4], bits[4], cost[4], plane type, ref changes of the
    sgrproj pass, ref changes of the switchable pass)."""
    n, rd = len(sse), case.rdmult
    with_w = bool(case.win)
    with_sw = with_w and n > 1
    best = [[0, 0, 0] for _ in range(n)]
    tot_s, tot_b = [0] * 4, [0] * 4
    ref_w = (list(W.INIT), list(W.INIT))
    ref_s, sw_w, sw_s = list(PRJ_DEFAULT), (list(W.INIT), list(W.INIT)), list(PRJ_DEFAULT)
    chg_s, chg_sw = [], []
    for k in range(n):
        s0, s1, s2 = sse[k]
        tot_s[NONE] += s0
        if with_w:                                      # search_wiener_finish: the comparison of the two costs is the Wiener call's
            if s1 == INT64_MAX:
                tot_b[WIENER], tot_s[WIENER] = tot_b[WIENER] + case.cost_w[0], tot_s[WIENER] + s0
            else:
                bits_wiener = case.cost_w[1] + (W.count_wiener_bits(case.win, taps[k][0], taps[k][1], *ref_w) << 9)
                best[k][0] = int(wbest[k] == WIENER)
                tot_s[WIENER] += s1 if best[k][0] else s0
                tot_b[WIENER] += bits_wiener if best[k][0] else case.cost_w[0]
                if best[k][0]:
                    ref_w = taps[k]
        bits_none, bits_sgr = case.cost_s[0], case.cost_s[1] + (count_sgrproj_bits(ep[k], xqd[k], ref_s) << 9)      # search_sgrproj_finish
        sgr = W.rdcost_dbl(rd, bits_sgr >> 4, s2) < W.rdcost_dbl(rd, bits_none >> 4, s0)
        best[k][1] = SGRPROJ if sgr else NONE
        tot_s[SGRPROJ], tot_b[SGRPROJ] = tot_s[SGRPROJ] + (s2 if sgr else s0), tot_b[SGRPROJ] + (bits_sgr if sgr else bits_none)
        if sgr:
            chg_s.append(k)
            ref_s = list(xqd[k])
        if with_sw:                                     # search_switchable
            best_cost = best_bits = 0
            for r in range(3):
                if r > NONE and best[k][r - 1] == NONE:
                    continue
                pcost = 0 if r == NONE else (W.count_wiener_bits(case.win, taps[k][0], taps[k][1], *sw_w) if r == WIENER else count_sgrproj_bits(ep[k], xqd[k], sw_s))
                bits = case.cost_sw[r] + (pcost << 9)
                cost = W.rdcost_dbl(rd, bits >> 4, sse[k][r])
                if r == 0 or cost < best_cost:
                    best_cost, best_bits, best[k][2] = cost, bits, r
            tot_s[SWITCHABLE], tot_b[SWITCHABLE] = tot_s[SWITCHABLE] + sse[k][best[k][2]], tot_b[SWITCHABLE] + best_bits
            if best[k][2] == WIENER:
                sw_w = taps[k]
            if best[k][2] == SGRPROJ:
                chg_sw.append(k)
                sw_s = list(xqd[k])
    tested = 1 | (with_w << WIENER) | 1 << SGRPROJ | (with_sw << SWITCHABLE)
    cost, plane_type, best_cost = [0.0] * 4, NONE, 0.0
    for r in range(4):
        if not tested >> r & 1:
            tot_s[r] = tot_b[r] = 0
            continue
        cost[r] = W.rdcost_dbl(rd, W.chk(tot_b[r]) >> 4, W.chk(tot_s[r]))
        if r == 0 or cost[r] < best_cost:
            best_cost, plane_type = cost[r], r
    return best, tested, tot_s, tot_b, cost, plane_type, chg_s, chg_sw


FIELDS = ("units", "result", "lr_units", "cover", "chains")


def drive(x, lv, wrecs):
    """The whole decision of the plane of `x` over the leaves `lv` and the Wiener unit records `wrecs` (None: no Wiener) -> dict: `units`
    (UNIT_DTYPE [n]), `result` (one RESULT_DTYPE record), `lr_units` (LR_DTYPE [n]) and, for the checks on the cases alone, `cover` (int32
    [n][len(COVER)]) and `chains` (int32 [2][n]: 1 where `ref` changes in the sgrproj pass / in the switchable pass)."""
    case, n = x.case, len(x.limits)
    units, lr, cover_out = np.zeros(n, UNIT_DTYPE), np.zeros(n, LR_DTYPE), np.zeros((n, len(COVER)), np.int32)
    res, chains = np.zeros((), RESULT_DTYPE), np.zeros((2, n), np.int32)
    assert (wrecs is not None) == bool(case.win)
    for i, limits in enumerate(x.limits):
        hs, he, vs, ve = limits
        u = units[i]
        ep, xqd, err, trials, cover = search_unit(x, lv, limits)
        u["sse"] = (lv.sse(x.dgd[B + vs:B + ve, B + hs:B + he], x.src[vs:ve, hs:he]), int(wrecs[i]["sse"][1]) if case.win else INT64_MAX,
                    trial_sse(x, lv, limits, ep, xqd))
        u["search_err"], u["ep"], u["xqd"], u["trials"] = err, ep, xqd, trials
        cover_out[i] = [cover[k] for k in COVER]
        res["sg_frame_ep_cnt"][ep] += 1
    taps = [([int(t) for t in r["vfilter"]], [int(t) for t in r["hfilter"]]) for r in wrecs] if case.win else [None] * n
    wbest = [int(r["best_rtype"]) for r in wrecs] if case.win else [0] * n
    best, tested, tot_s, tot_b, cost, plane_type, chg_s, chg_sw = decide(
        case, [[int(v) for v in u["sse"]] for u in units], taps, wbest, [int(v) for v in units["ep"]], [[int(v) for v in u["xqd"]] for u in units])
    units["best_rtype"] = best
    res["frame_restoration_type"], res["tested"], res["sse"], res["bits"], res["cost"] = plane_type, tested, tot_s, tot_b, cost
    chains[0, chg_s], chains[1, chg_sw] = 1, 1
    for i in range(n):                                  # copy_unit_info (:1202) under the plane's type
        t = best[i][plane_type - 1] if plane_type else NONE
        lr[i]["restoration_type"] = t
        if t == WIENER:
            lr[i]["hfilter"], lr[i]["vfilter"] = wrecs[i]["hfilter"], wrecs[i]["vfilter"]
        if t == SGRPROJ:
            lr[i]["ep"], lr[i]["xqd"] = units[i]["ep"], units[i]["xqd"]
        res["n_units_of_type"][t] += 1
    return {"units": units, "result": res, "lr_units": lr, "cover": cover_out, "chains": chains}


def drive_ref(x, ref):
    return drive(x, RefLeaves(x, ref), wiener_records(x, wiener_leaves(x, ref, "ref")))


def drive_orc(x, orc):
    return drive(x, OrcLeaves(x, orc), wiener_records(x, wiener_leaves(x, orc, "orc")))


def same(a, b, fields=FIELDS):
    return W.same(a, b, fields)


_golden = {}


def golden(case):
    """The recorded results of one case (tests/golden/rest_pick.npz, written by tests/golden/make_golden_rest_pick.py)."""
    if not _golden:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rest_pick.npz")) as g:
            _golden.update({k: g[k] for k in g.files})
    out = {f: _golden[f"{case.name}_{f}"] for f in FIELDS}
    out["wiener"] = _golden.get(f"{case.name}_wiener")       # the Wiener unit records the plane was decided with (None without a window)
    return out


class Pin:
    """tests/rest_pick_pin_driver.c (the reference's own static finish visitors, bit count, encode_xq and finer search) built into
    `directory` against oracle/_ref/libsvtref.so."""

    def __init__(self, ref, directory):
        from support import build_pin
        self.lib = build_pin(directory, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rest_pick_pin_driver.c"))
        self.lib.pin_finer_search.restype = C.c_int64

    def constants(self):
        out = np.zeros(12, np.int64)
        self.lib.pin_rest_constants(P(out))
        return [int(v) for v in out]

    def encode_xq(self, xq, ep):
        a, b = np.array(xq, np.int32), np.zeros(2, np.int32)
        self.lib.pin_encode_xq(P(a), P(b), ep)
        return [int(b[0]), int(b[1])]

    def count_bits(self, ep, xqd, ref):
        a, b = np.array(xqd, np.int32), np.array(ref, np.int32)
        return int(self.lib.pin_count_sgrproj_bits(ep, P(a), P(b)))

    def finer_search(self, x, limits, f0, f1, fs, xqd, ep, refine):
        """-> (err, xqd) of the reference's finer_search_pixel_proj_error over the unit, from the same filtered planes"""
        hs, he, vs, ve = limits
        q = np.array(xqd, np.int32)
        err = self.lib.pin_finer_search(_enc(_addr(x.src, vs, hs), x.case.is16), he - hs, ve - vs, x.src.shape[1], _enc(_addr(x.dgd, B + vs, B + hs), x.case.is16),
                                        x.dgd.shape[1], x.case.is16, P(f0), fs, P(f1), fs, P(q), refine, ep)
        return int(err), [int(q[0]), int(q[1])]

    def decide(self, case, sse, taps, ep, xqd):
        """The reference's visitors in raster order, pass after pass as rest_finish_search runs them -> (best_rtype[n][3], sse[4], bits[4],
        cost[4] as bit patterns)"""
        n = len(sse)
        a_sse, a_ep, a_xqd = np.array(sse, np.int64).reshape(n, 3), np.array(ep, np.int32), np.array(xqd, np.int32).reshape(n, 2)
        a_taps = np.zeros((n, 2, 8), np.int16)
        for k in range(n):
            if taps[k] is not None:
                a_taps[k, 0, :len(taps[k][0])], a_taps[k, 1, :len(taps[k][1])] = taps[k][0][:8], taps[k][1][:8]
        costs = np.array([*case.cost_w, *case.cost_s, *case.cost_sw], np.int32)
        best, o_sse, o_bits, o_cost = np.zeros((n, 3), np.int32), np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(4, np.float64)
        tested = 1 | (bool(case.win) << WIENER) | 1 << SGRPROJ | ((bool(case.win) and n > 1) << SWITCHABLE)
        self.lib.pin_finish(n, P(a_sse), P(a_taps), P(a_ep), P(a_xqd), case.rdmult, P(costs), case.win or 7, tested, P(best), P(o_sse), P(o_bits), P(o_cost))
        return best.tolist(), o_sse.tolist(), o_bits.tolist(), o_cost.tobytes()


ARGS = ("prm", "units", "d_unit_records", "d_result", "d_lr_units", "d_workspace")


def rejections(x):
    """(label, change of the parameters, change of unit 0's limits, argument to pass as NULL or to misalign, n_units or None, bytes to take
    off the workspace size): every call svt_hip_rest_pick_plane must refuse with SVT_HIP_ERR_BAD_PARAMETER."""
    for a in ARGS:
        yield f"NULL {a}", {}, {}, a, None, 0
    for a in ARGS[2:]:
        yield f"misaligned {a}", {}, {}, "+" + a, None, 0
    yield "no units", {}, {}, None, 0, 0
    yield "too many units", {}, {}, None, 65536, 0
    yield "bit depth 9", {"bit_depth": 9}, {}, None, None, 0
    yield "10 bit in bytes", {"bit_depth": 10, "is_16bit": 0}, {}, None, None, 0
    yield "empty plane", {"plane_width": 0}, {}, None, None, 0
    yield "plane too tall", {"plane_height": 65537}, {}, None, None, 0
    yield "ss_x 2", {"ss_x": 2}, {}, None, None, 0
    yield "ss_y -1", {"ss_y": -1}, {}, None, None, 0
    yield "empty ep range", {"sg_start_ep": 5, "sg_end_ep": 5}, {}, None, None, 0
    yield "ep past 16", {"sg_end_ep": 17}, {}, None, None, 0
    yield "negative ep", {"sg_start_ep": -1}, {}, None, None, 0
    yield "ep step 0", {"sg_ep_inc": 0}, {}, None, None, 0
    yield "window 3 with records", {"wiener_win": 3}, {}, "records", None, 0
    yield "unit wider than 384", {"plane_width": 500}, {"h_end": 385}, None, None, 0
    yield "unit taller than 384", {"plane_height": 500}, {"v_end": 385}, None, None, 0
    yield "unit past the plane", {}, {"h_end": x.case.w + 1}, None, None, 0
    yield "empty unit", {}, {"v_end": 0}, None, None, 0
    yield "unit without src", {}, {"src": None}, None, None, 0
    yield "workspace short", {}, {}, None, None, 1


def call_rejection(lib, x, rej, good, n_units, records, workspace_bytes):
    """Makes the call of one rejections() entry with the pointers of `good` (a dict over ARGS; prm / units are filled in here) -> the
    int64 the call returns.  `records`: a non-NULL d_wiener_records for the entry that needs one."""
    label, change, limits, null, count, short = rej
    prm, units = params(x), wiener_units(x, good["dgd"], good["src"])
    for k, v in change.items():
        setattr(prm, k, v)
    for k, v in limits.items():
        setattr(units[0], k, v)
    a = dict(good, prm=C.addressof(prm), units=C.addressof(units))
    rec = None
    if null == "records":
        rec = records
    elif null and null[0] == "+":
        a[null[1:]] += 4
    elif null:
        a[null] = None
    return lib.svt_hip_rest_pick_plane(a["prm"], a["units"], n_units if count is None else count, rec, a["d_unit_records"], a["d_result"], a["d_lr_units"],
                                       a["d_workspace"], workspace_bytes - short, None)
