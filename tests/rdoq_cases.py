"""TEST INFRASTRUCTURE — cases, coefficient generator, Python restatement and arena / descriptor builder for the RDOQ stage of the
quantiser (svt_hip_rdoq_batch, include/svt_hip_txfm.h).

The stage is svt_aom_quantize_inv_quantize (full_loop.c:1462-1686) behind its first quantiser.  The quantiser tables, the
quantisation matrices and every case's expected result live in tests/golden/rdoq.npz (written by tests/golden/make_golden_rdoq.py);
the rate tables and the scans are those of tests/golden/txb_cost.npz.  tests/test_rdoq_abi.py pins fixture and restatement to the
reference's own function through tests/rdoq_pin_driver.c wherever oracle/_ref/libsvtref.so has been built.  The first quantiser and the
quantize_b family of the restatement are the oracle's (tx_cases.orc_quant); everything behind them is restated here."""
import collections
import ctypes as C
import hashlib
import os

import numpy as np

import tx_cases
import txb_cost_cases as T
from arena import PATTERN, Arena
from svtav1_hip import abi
from tx_cases import SIZES

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "rdoq.npz")
BIT_DEPTHS = (8, 10)
QM_LEVEL, NO_QM_LEVEL = 4, 15     # the level the cases with matrices use; NUM_QM_LEVELS - 1 means none
QT_FIELDS = ("zbin", "round", "quant", "qshift", "round_fp", "quant_fp", "dequant")   # the rows of Golden.quant[bd][table]
# the levels the generator aims at: the base levels, both sides of the Golomb switch (15), r = level - 14 = 31, 32 (a power of two
# in the r >= 32 branch), 33, both sides of the level clamp, and 2^15 and above
MAGNITUDES = (1, 2, 3, 14, 15, 16, 45, 46, 47, 127, 128, (1 << 15) + 300, 40000)
LAMBDAS = (0, 40, 900, 20000, 500000, 30000000)

Case = collections.namedtuple("Case", "group w h tx_type plane is_inter bd table qm lam skip_ctx dc_sign_ctx perform fast sharp eob_th eob_fast_th "
                                      "satd_factor early_exit_th sq_size fp_q eob dc recipe pic_bd")


def _cases():
    out = []

    def add(group, w, h, tx_type, eob, **kw):
        i = len(out)
        d = dict(plane=i % 2, is_inter=(i // 2) % 2, bd=BIT_DEPTHS[(i // 3) % 2], table=(i // 5) % 2, qm=int(i % 3 == 0),
                 lam=LAMBDAS[i % len(LAMBDAS)], skip_ctx=i % 13, dc_sign_ctx=i % 3, perform=1, fast=0, sharp=0, eob_th=255, eob_fast_th=255,
                 satd_factor=255, early_exit_th=0, sq_size=(8, 16, 32, 64)[i % 4], fp_q=1, dc=("neg", "pos", "zero")[(i // 2) % 3], recipe="mix")
        d.update(kw)
        d.setdefault("pic_bd", d["bd"])   # the picture's bit depth: the same unless mode decision runs at 8 bit on a 10-bit picture
        d["qm"] = int(d["qm"] and tx_type < T.IDTX)   # IS_2D_TRANSFORM: the reference uses the matrices for these types only
        out.append(Case(group, w, h, tx_type, eob=eob, **d))

    for w, h in SIZES:
        n = min(w, 32) * min(h, 32)
        big = n >= 512
        # every class the size allows x both planes x the eob edges; everything else takes turns
        for tx_type in T.size_types(w, h):
            for plane in (0, 1):
                for eob in T.eob_edges(n):
                    if big and eob == n and plane:
                        continue
                    add("grid", w, h, tx_type, eob, plane=plane)
        types = T.size_types(w, h)
        # short heads: 1 .. 7 non-zeros of magnitude 1 .. 3, spread over an eob; every lambda
        for k, lam in enumerate(LAMBDAS):
            for nnz in (1, 2, 3, 4, 5, 7):
                add("head", w, h, types[(k + nnz) % len(types)], min(n, nnz + (0, 2, 9)[(k + nnz) % 3]), lam=lam, recipe=f"head{nnz}")
        # the switches
        for k in range(4):
            e = (2, n // 8 + 1, n // 2, n)[k]
            tt = types[k % len(types)]
            add("sharp", w, h, tt, e, plane=0, sharp=1, lam=LAMBDAS[2 + k % 3])
            add("fast", w, h, tt, e, fast=1, recipe="tail")
            add("fast", w, h, tt, 1, fast=1, recipe="tail")
            for fast_th in (0, 30):
                add("eob_fast_th", w, h, tt, e, eob_fast_th=fast_th, recipe="tail")
            add("eob_th", w, h, tt, e, eob_th=85, eob_fast_th=(255, 30)[k % 2])
            add("satd", w, h, tt, e, satd_factor=(1, 60)[k % 2], recipe=("mix", "small")[k // 2])
            # skip context 1 is one where skipping is the cheaper flag in every table; 12 is one where it never is
            add("early", w, h, tt, e, early_exit_th=(200, 2, 200, 40)[k], sq_size=(8, 64, 8, 16)[k], skip_ctx=(1, 7, 12, 1)[k])
            add("unflagged", w, h, tt, e, perform=0)
            add("b_family", w, h, tt, e, fp_q=0, eob_th=(255, 85)[k % 2])
        # no size's batch ends on a full wavefront (64 lanes, min(n, 64) lanes to a block)
        per_wave = 64 // min(n, 64)
        if sum((c.w, c.h) == (w, h) for c in out) % per_wave == 0:
            add("ragged", w, h, T.DCT_DCT, 2)
    # every magnitude on its own, in the head and behind it, 10 bit for the ones only the high-bit-depth quantiser reaches
    for w, h in ((4, 4), (8, 8), (16, 16), (8, 16), (32, 32)):
        n = min(w, 32) * min(h, 32)
        for m in MAGNITUDES:
            for k, lam in enumerate((0, 900, 500000, 30000000)):
                add("magnitude", w, h, T.size_types(w, h)[k % len(T.size_types(w, h))], min(n, 24), lam=lam, recipe=f"mag{m}",
                    bd=10 if m > 200 else BIT_DEPTHS[k % 2], table=0 if m > 200 else k % 2, qm=0 if m > 200 else k % 2)
    # 8-bit mode decision of a 10-bit picture (hbd_md = 0): the SATD gate scales by the picture's depth, not the block's
    for w, h in ((4, 4), (8, 8), (16, 16), (32, 32), (16, 64), (8, 32)):
        n = min(w, 32) * min(h, 32)
        for k, factor in enumerate((2, 6, 12, 25, 60, 120)):
            add("satd_pic10", w, h, T.size_types(w, h)[k % len(T.size_types(w, h))], (n // 8 + 1, n // 2, n)[k % 3], bd=8, pic_bd=10, satd_factor=factor,
                recipe=("mix", "small")[k % 2])
    return out


CASES = _cases()


def digest(a):
    """64 bits of an int32 array"""
    return int.from_bytes(hashlib.blake2b(np.ascontiguousarray(a, np.int32).tobytes(), digest_size=8).digest(), "little")


class Golden:
    def __init__(self, path=GOLD):
        self.txb = T.Golden()
        self.tables = self.txb.tables
        z = np.load(path)
        self.quant = z["quant"]     # [bit depth][table][QT_FIELDS][DC, AC]
        self.qms = {(int(p), int(s)): (z["qm"][o:o + n], z["iqm"][o:o + n]) for p, s, o, n in z["qm_index"]}
        self.eob, self.cul_level, self.path, self.changed = z["eob"], z["cul_level"], z["path"], z["changed"]
        self.q_digest, self.dq_digest = z["q_digest"], z["dq_digest"]
        assert len(self.eob) == len(CASES)

    def iscan(self, w, h, tx_type):
        return self.txb.iscan(w, h, tx_type)

    def qt(self, c):
        return quant_dict(self.quant[BIT_DEPTHS.index(c.bd)][c.table])

    def qm(self, c):
        return self.qms[(c.plane, T.TX_INDEX[(c.w, c.h)])] if c.qm else (None, None)


def quant_dict(rows):
    """[7][2] of the fixture as the table dictionary tx_cases.orc_quant takes"""
    return {k: np.array(list(rows[i]) + [rows[i][1]] * 6, np.int16) for i, k in enumerate(QT_FIELDS)}


def coefficients(i, c, iscan, qt, qm):
    """The transform coefficients of case i: aimed at levels of its recipe below eob in scan order (a level L with rounding
    remainder u becomes about (L + u) quantiser steps), a non-zero level at eob - 1, the DC the case asks for, zero beyond eob."""
    n = len(iscan)
    rng = np.random.default_rng(5000 + i)
    co = np.zeros(n, np.int64)
    if not c.eob:
        return co.astype(np.int32)
    scan = T.scan_of(iscan)
    e, r = c.eob, c.recipe
    if r.startswith("head"):
        level = np.zeros(e, np.int64)
        level[rng.choice(e, size=min(int(r[4:]), e), replace=False)] = rng.choice((1, 1, 2, 3), size=min(int(r[4:]), e))
    elif r.startswith("mag"):
        level = np.where(rng.random(e) < 0.8, int(r[3:]), 0)
    elif r == "small":
        level = rng.choice((0, 1), size=e, p=(0.7, 0.3))
    else:
        level = rng.choice((0,) + MAGNITUDES[:11], size=e, p=(0.34,) + (0.06,) * 11)
    u = rng.uniform(-0.49, 0.49, size=e)
    if r == "tail":   # a run of ones at the end of the scan that update_coeff_eob_fast trims: below 0.77 steps
        k = min(e, 1 + e // 3)
        level[e - k:], u[e - k:] = 1, rng.uniform(-0.45, -0.3, size=k)
        if e - k - 1 >= 0:
            level[e - k - 1], u[e - k - 1] = 2, 0.2
    if level[e - 1] == 0:
        level[e - 1] = 1
    if r != "tail":
        u[e - 1] = abs(u[e - 1])
    sign = rng.choice((-1, 1), size=e)
    if e > 1 or c.dc != "zero":
        if c.dc == "zero":
            level[0], u[0] = 0, 0.0
        else:
            level[0], u[0], sign[0] = max(level[0], 1), abs(u[0]), -1 if c.dc == "neg" else 1
    pos = scan[:e]
    step = qt["dequant"][(pos != 0).astype(int)].astype(np.float64)
    if qm is not None:
        step = step * 32.0 / qm[pos]
    mag = np.floor(np.maximum(level + u, 0) * step / (1 << T.tx_scale(c.w, c.h))).astype(np.int64)
    co[pos] = sign * mag
    assert np.abs(co).max() < 1 << 28
    return co.astype(np.int32)


def first_quant(orc, c, coeff, iscan, qt, qm, iqm):
    """What svt_hip_txfm_quant_batch leaves before the stage: (quant_mode, qcoeff, dqcoeff, eob, satd)"""
    fp = c.fp_q and c.perform   # without perform_rdoq the reference quantises with the quantize_b family at once
    mode = (abi.QUANT_FP_HBD if c.bd > 8 else abi.QUANT_FP) if fp else (abi.QUANT_B_HBD if c.bd > 8 else abi.QUANT_B)
    q, dq, eob = quant(orc, mode, c, coeff, iscan, qt, qm, iqm)
    return mode, q, dq, eob, int(np.abs(coeff.astype(np.int64)).sum())


def quant(orc, mode, c, coeff, iscan, qt, qm, iqm):
    which = {abi.QUANT_B: 1, abi.QUANT_B_HBD: 2, abi.QUANT_FP: 3, abi.QUANT_FP_HBD: 4}[mode]
    return tx_cases.orc_quant(orc, which, dict(n=len(iscan), ls=T.tx_scale(c.w, c.h), coeff=np.ascontiguousarray(coeff, np.int32),
                                                scan=T.scan_of(iscan).astype(np.int16), iscan=iscan, qm=qm, iqm=iqm, t=qt))


# ------------------------------------------------------------------------------------------------ the stage, restated
SQRT_TX_PIXELS = {s: int(np.ceil(np.sqrt(min(s[0], 32) * min(s[1], 32)))) for s in SIZES}   # sqrt_tx_pixels_2d (full_loop.c:1112): of the retained block
PLANE_RD_MULT = ((17, 20), (16, 20))                                                # plane_rd_mult[is_inter][plane_type]
_cost_lists = {}


def _cc(t, key, txs_ctx, plane):
    k = (key, txs_ctx, plane)
    if k not in _cost_lists:
        cc = t["coeff"][txs_ctx][plane]
        _cost_lists[k] = {f: cc[f].tolist() for f in ("txb_skip", "base_eob", "base", "eob_extra", "dc_sign", "lps")}
    return _cost_lists[k]


def golomb(level):
    return (2 * int(level - 14).bit_length() - 1) * 512 if level >= 15 else 0


def wrap64(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def neighbours(cls):
    """(dr, dc) of the levels get_nz_mag reads and of those get_br_ctx reads, by transform class"""
    nz = {0: ((0, 1), (1, 0), (1, 1), (0, 2), (2, 0)), 1: ((0, 1), (1, 0), (0, 2), (0, 3), (0, 4)), 2: ((0, 1), (1, 0), (2, 0), (3, 0), (4, 0))}[cls]
    br = {0: ((0, 1), (1, 0), (1, 1)), 1: ((0, 1), (1, 0), (0, 2)), 2: ((0, 1), (1, 0), (2, 0))}[cls]
    return nz, br


class Trellis:
    """svt_av1_optimize_b (full_loop.c:1124-1331) in Python integers on lists; `hit` counts the branches taken."""

    def __init__(self, c, t, coeff, q, dq, iscan, dqt, iqm, hit):
        self.iw, self.ih = T.retained(c.w, c.h)
        self.n = self.iw * self.ih
        self.cls, self.orient = T.tx_class(c.tx_type), (c.w > c.h) - (c.w < c.h)
        txs_ctx = (T.size_index(min(c.w, c.h)) + T.size_index(max(c.w, c.h)) + 1) >> 1
        self.cc = _cc(t, c.table, txs_ctx, c.plane)
        self.eob_bits = t["eob"][self.n.bit_length() - 5][c.plane].tolist()
        self.tc, self.q, self.dq = coeff, q, dq
        self.scan = T.scan_of(iscan).tolist()
        self.dequant, self.iqm = dqt, None if iqm is None else [int(v) for v in iqm]
        self.shift, self.c, self.hit = T.tx_scale(c.w, c.h), c, hit
        self.sharp = c.sharp
        self.rdmult = ((c.lam * PLANE_RD_MULT[c.is_inter][c.plane] * (0 if c.sharp else 100)) // 100 + 2) >> 2
        self.nz_off, self.br_off = neighbours(self.cls)
        self.lev = [[0] * (self.iw + 4) for _ in range(self.ih + 4)]
        for p in range(self.n):
            self.lev[p // self.iw][p % self.iw] = min(abs(q[p]), 127)

    def rdcost(self, rate, dist):
        return wrap64(((rate * self.rdmult + 256) >> 9) + dist * 128)

    def dist(self, t, d):
        return ((t - d) << self.shift) ** 2

    def dqv(self, ci):
        v = self.dequant[int(ci != 0)]
        return (self.iqm[ci] * v + 16) >> 5 if self.iqm is not None else v

    def set_level(self, ci, v):
        self.lev[ci // self.iw][ci % self.iw] = min(v, 127)

    def lower_ctx(self, ci):
        row, col = divmod(ci, self.iw)
        if self.cls == 0 and ci == 0:
            return 0
        mag = sum(min(self.lev[row + a][col + b], 3) for a, b in self.nz_off)
        ctx = min((mag + 1) >> 1, 4)
        if self.cls == 0:
            if self.orient < 0 and row < 2:
                return ctx + 11
            if self.orient > 0 and col < 2:
                return ctx + 16
            return ctx + (1 if row + col < 2 else 6 if row + col < 4 else 21)
        k = col if self.cls == 1 else row
        return ctx + (26 if k == 0 else 31 if k == 1 else 36)

    def near(self, ci):
        row, col = divmod(ci, self.iw)
        return (row < 2 and col < 2) if self.cls == 0 else col == 0 if self.cls == 1 else row == 0

    def br_ctx(self, ci):
        row, col = divmod(ci, self.iw)
        mag = min((sum(self.lev[row + a][col + b] for a, b in self.br_off) + 1) >> 1, 6)
        return mag if ci == 0 else mag + (7 if self.near(ci) else 14)

    def br_ctx_eob(self, ci):
        return 0 if ci == 0 else 7 if self.near(ci) else 14

    def eob_ctx(self, si):
        return 0 if si == 0 else 1 if si <= self.n // 8 else 2 if si <= self.n // 4 else 3

    def br_cost(self, level, ctx):
        return self.cc["lps"][ctx][min(level - 3, 12)] + golomb(level)

    def cost_general(self, is_last, ci, a, sign, ctx):
        cost = self.cc["base_eob"][ctx][min(a, 3) - 1] if is_last else self.cc["base"][ctx][min(a, 3)]
        if a:
            cost += self.cc["dc_sign"][self.c.dc_sign_ctx][sign] if ci == 0 else 512
            if a > 2:
                cost += self.br_cost(a, self.br_ctx_eob(ci) if is_last else self.br_ctx(ci))
        return cost

    def cost_eob(self, ci, a, sign, ctx):
        return self.cost_general(True, ci, a, sign, ctx)

    def eob_cost(self, eob):
        """get_eob_cost (full_loop.c:690-707), eob >= 1: the token of get_eob_pos_token is the bit length of eob - 1, plus one"""
        pt = eob if eob < 2 else (eob - 1).bit_length() + 1
        cost = self.eob_bits[int(self.cls != 0)][pt - 1]
        offset_bits = pt - 2
        if offset_bits > 0:
            extra = eob - ((1 << offset_bits) + 1)
            cost += self.cc["eob_extra"][pt - 3][(extra >> (offset_bits - 1)) & 1] + (offset_bits - 1) * 512
        return cost

    def two_cost_simple(self, ci, a, ctx):
        cost = self.cc["base"][ctx][min(a, 3)] + 512
        diff = self.cc["base"][ctx][a + 4] if a <= 3 else 0
        if a > 2:
            lps = self.cc["lps"][self.br_ctx(ci)]
            base_range = min(a - 3, 12)
            bits = 0
            if a <= 15:
                diff += lps[base_range + 13]
            if a >= 15:
                r = a - 14
                if r < 32:
                    bits = (2 * r.bit_length() - 1) * 512                              # golomb_bits_cost
                    diff += 512 if r == 1 else 1024 if r & (r - 1) == 0 else 0         # golomb_cost_diff
                    self.hit("golomb_table")
                else:
                    bits = golomb(a)
                    diff += 1024 if r & (r - 1) == 0 else 0
                    self.hit("golomb_r32", "pow2" if r & (r - 1) == 0 else "other")
            cost += lps[base_range] + bits
        return cost, cost - diff

    def low(self, ci, a, sign):
        adq = mul32(a - 1, self.dqv(ci)) >> self.shift
        return (-(a - 1), -adq) if sign else (a - 1, adq)

    def store_low(self, ci, a_low, q_low, dq_low):
        self.q[ci], self.dq[ci] = q_low, dq_low
        self.set_level(ci, a_low)

    def update_general(self, acc, si, eob, where):
        ci = self.scan[si]
        q = self.q[ci]
        is_last = si == eob - 1
        ctx = self.eob_ctx(si) if is_last else self.lower_ctx(ci)
        if where == "dc":
            self.hit("dc_sign", (q > 0) - (q < 0))
        if q == 0:
            acc[0] += self.cc["base"][ctx][0]
            self.hit(where, "zero")
            return
        sign, a, t = int(q < 0), abs(q), self.tc[ci]
        dist, dist0 = self.dist(t, self.dq[ci]), self.dist(t, 0)
        rate = self.cost_general(is_last, ci, a, sign, ctx)
        rd = self.rdcost(rate, dist)
        if a == 1:
            q_low = dq_low = 0
            dist_low, rate_low = dist0, self.cc["base"][ctx][0]
        else:
            q_low, dq_low = self.low(ci, a, sign)
            dist_low, rate_low = self.dist(t, dq_low), self.cost_general(is_last, ci, a - 1, sign, ctx)
        if self.rdcost(rate_low, dist_low) < rd:
            self.store_low(ci, a - 1, q_low, dq_low)
            acc[0] += rate_low
            acc[1] += dist_low - dist0
            self.hit(where, "lower")
        else:
            acc[0] += rate
            acc[1] += dist - dist0
            self.hit(where, "keep")

    def update_eob(self, acc, st, si):
        """st: [eob, nz_ci list]"""
        ci = self.scan[si]
        q = self.q[ci]
        ctx = self.lower_ctx(ci)
        if q == 0:
            acc[0] += self.cc["base"][ctx][0]
            self.hit("head", "zero")
            return
        sign, a, t = int(q < 0), abs(q), self.tc[ci]
        dist0 = self.dist(t, 0)
        dist = self.dist(t, self.dq[ci]) - dist0
        rate = self.cost_general(False, ci, a, sign, ctx)
        rd = self.rdcost(acc[0] + rate, acc[1] + dist)
        if a == 1:
            a_low = q_low = dq_low = 0
            dist_low, rate_low = 0, self.cc["base"][ctx][0]
            rd_low = self.rdcost(acc[0] + rate_low, acc[1])
        else:
            a_low = a - 1
            q_low, dq_low = self.low(ci, a, sign)
            dist_low = self.dist(t, dq_low) - dist0
            rate_low = self.cost_general(False, ci, a_low, sign, ctx)
            rd_low = self.rdcost(acc[0] + rate_low, acc[1] + dist_low)
        lower_new = False
        new_eob, ctx_new = si + 1, self.eob_ctx(si)
        new_eob_cost = self.eob_cost(new_eob)
        rate_new = new_eob_cost + self.cost_eob(ci, a, sign, ctx_new)
        dist_new, rd_new = dist, self.rdcost(new_eob_cost + self.cost_eob(ci, a, sign, ctx_new), dist)
        if a_low > 0:
            rate_new_low = new_eob_cost + self.cost_eob(ci, a_low, sign, ctx_new)
            rd_new_low = self.rdcost(rate_new_low, dist_low)
            if rd_new_low < rd_new:
                lower_new, rd_new, rate_new, dist_new = True, rd_new_low, rate_new_low, dist_low
        lower = False
        if rd_low < rd:
            lower, rd, rate, dist = True, rd_low, rate_low, dist_low
        if not self.sharp and rd_new < rd:
            for z in st[1]:
                self.set_level(z, 0)
                self.q[z] = self.dq[z] = 0
            st[0], st[1] = new_eob, []
            acc[0], acc[1] = rate_new, dist_new
            lower = lower_new
            self.hit("head", "new_eob_lower" if lower else "new_eob")
        else:
            acc[0] += rate
            acc[1] += dist
            self.hit("head", "lower" if lower else "keep")
        if lower:
            self.store_low(ci, a_low, q_low, dq_low)
        if self.q[ci]:
            st[1].append(ci)

    def update_simple(self, si):
        ci = self.scan[si]
        q = self.q[ci]
        if q == 0:
            return
        a, at, ad = abs(q), abs(self.tc[ci]), abs(self.dq[ci])
        rate, rate_low = self.two_cost_simple(ci, a, self.lower_ctx(ci))
        self.hit("simple_level", a if a in MAGNITUDES else "big" if a >= 1 << 15 else "other")
        if ad < at:
            self.hit("simple", "below")
            return
        rd = self.rdcost(rate, self.dist(at, ad))
        ad_low = mul32(a - 1, self.dqv(ci)) >> self.shift
        if self.rdcost(rate_low, self.dist(at, ad_low)) < rd:
            self.store_low(ci, a - 1, -(a - 1) if q < 0 else a - 1, -ad_low if q < 0 else ad_low)
            self.hit("simple", "lower")
        else:
            self.hit("simple", "keep")

    def walk(self, eob, eob_cost, fast_mode, skip_cost, non_skip_cost):
        """-> (eob, skipped)"""
        acc = [eob_cost, 0]
        si = eob - 1
        ci = self.scan[si]
        q = self.q[ci]
        st = [eob, [ci]]
        if abs(q) >= 2:
            self.update_general(acc, si, eob, "last")
        else:
            acc[0] += self.cost_eob(ci, 1, int(q < 0), self.eob_ctx(si))
            acc[1] += self.dist(self.tc[ci], self.dq[ci]) - self.dist(self.tc[ci], 0)
            self.hit("last", "one")
        si -= 1
        while si >= 0 and len(st[1]) <= 4 and not fast_mode:
            self.update_eob(acc, st, si)
            si -= 1
        skipped = False
        if si == -1 and len(st[1]) <= 4:
            self.hit("head_end", "skip_reached", len(st[1]))
            if not self.sharp and self.rdcost(skip_cost, 0) < self.rdcost(acc[0] + non_skip_cost, acc[1]):
                for z in st[1]:
                    self.q[z] = self.dq[z] = 0
                st[0], skipped = 0, True
                self.hit("skip", "taken")
            else:
                self.hit("skip", "not_taken")
        else:
            self.hit("head_end", "skip_not_reached", "fast" if fast_mode else len(st[1]))
        while si >= 1:
            self.update_simple(si)
            si -= 1
        if si == 0:
            self.update_general(acc, 0, st[0], "dc")
        return st[0], skipped


def mul32(a, b):
    """abs_qc_low * dqv in the reference's int (32-bit); the cases stay inside it"""
    v = a * b
    assert -(1 << 31) <= v < 1 << 31
    return v


def fast_trim(c, eob, coeff, q, dq, scan, dequant):
    """update_coeff_eob_fast (full_loop.c:1089-1108) -> new eob"""
    shift = T.tx_scale(c.w, c.h)
    zbin = [int(d) + ((int(d) * 70 + 64) >> 7) for d in dequant]
    for i in range(eob - 1, -1, -1):
        rc = scan[i]
        if (abs(coeff[rc]) << (1 + shift)) < zbin[int(rc != 0)] or q[rc] == 0:
            eob -= 1
            q[rc] = dq[rc] = 0
        else:
            break
    return eob


def cul_level(q, scan, eob):
    """svt_av1_compute_cul_level_c (full_loop.c:1444-1460)"""
    cul = min(63, sum(abs(q[scan[k]]) for k in range(eob)))
    return cul | 64 if q[0] < 0 else cul + 128 if q[0] > 0 else cul


def restate(c, t, coeff, mode, q, dq, eob, satd, iscan, qt, qm, iqm, quant_b, hit=lambda *k: None):
    """The stage on case c.  t: one record of abi.RATE_TABLES_DTYPE; coeff, q, dq, eob, satd, mode: what the first quantiser left
    (first_quant); quant_b(): the quantize_b family on coeff -> (q, dq, eob).  Returns (qcoeff, dqcoeff, eob, cul_level, path)."""
    n = len(iscan)
    scan = T.scan_of(iscan).tolist()
    coeff, q, dq = [int(v) for v in coeff], [int(v) for v in q], [int(v) for v in dq]
    eob = min(eob, n)
    dequant = [int(qt["dequant"][0]), int(qt["dequant"][1])]
    path, perform, requant = abi.RDOQ_PATH_NOT_FLAGGED, bool(c.perform), False
    if perform and c.satd_factor != 255:
        s = satd
        shift = 1 - T.tx_scale(c.w, c.h)
        s = s << -shift if shift < 0 else s >> shift
        limit = c.satd_factor * (dequant[1] >> dequant_shift(c)) * SQRT_TX_PIXELS[(c.w, c.h)]
        if s >> (c.pic_bd - 8) > limit:
            perform, requant, path = False, True, abi.RDOQ_PATH_REQUANT_SATD
        hit("satd", "refused" if requant else "passed")
        if c.pic_bd != c.bd:
            hit("satd_picture_depth", "decides" if (s >> (c.bd - 8) > limit) != requant else "agrees", "refused" if requant else "passed")
    if perform:
        if eob == 0:
            perform, path = False, abi.RDOQ_PATH_EOB_ZERO
        else:
            eob_perc = eob * 100 // (c.w * c.h)
            if eob_perc >= c.eob_th:
                perform, requant, path = False, True, abi.RDOQ_PATH_REQUANT_EOB
            elif eob_perc >= c.eob_fast_th:
                eob = fast_trim(c, eob, coeff, q, dq, scan, dequant)
                path |= abi.RDOQ_PATH_FAST_TRIM
                hit("trim", "eob_fast_th", c.eob_fast_th)
                if eob == 0:
                    perform, path = False, abi.RDOQ_PATH_EOB_ZERO | abi.RDOQ_PATH_FAST_TRIM
            if c.eob_th != 255:
                hit("eob_th", "above" if requant else "below")
            if c.eob_fast_th not in (0, 255) and not requant:
                hit("eob_fast_th", "above" if path & abi.RDOQ_PATH_FAST_TRIM else "below")
    if requant and mode not in (abi.QUANT_B, abi.QUANT_B_HBD):
        q2, dq2, eob = quant_b()
        q, dq = [int(v) for v in q2], [int(v) for v in dq2]
        hit("requant", "redone")
    elif requant:
        hit("requant", "kept")
    if perform:
        tr = Trellis(c, t, coeff, q, dq, iscan, dequant, iqm, hit)
        eob_cost = tr.eob_cost(eob)
        skip_cost, non_skip_cost = tr.cc["txb_skip"][c.skip_ctx][1], tr.cc["txb_skip"][c.skip_ctx][0]
        sq_size_idx = 7 - c.sq_size.bit_length() + 1
        trimmed = path & abi.RDOQ_PATH_FAST_TRIM
        if eob_cost < n * sq_size_idx * c.early_exit_th and skip_cost < non_skip_cost:
            path = abi.RDOQ_PATH_EARLY_EXIT | trimmed
            hit("early_exit", "taken")
        else:
            if c.early_exit_th:
                hit("early_exit", "not_taken")
            path = abi.RDOQ_PATH_TRELLIS | trimmed
            if c.fast:
                eob = fast_trim(c, eob, coeff, q, dq, scan, dequant)
                path |= abi.RDOQ_PATH_FAST_TRIM
                hit("trim", "fast_mode")
            if eob:
                hit("trellis", "iqm", tr.iqm is not None), hit("trellis", "class", tr.cls), hit("trellis", "bd", c.bd), hit("trellis", "sharp", c.sharp)
                hit("trellis", "log_scale", tr.shift), hit("trellis", "plane", c.plane), hit("trellis", "inter", c.is_inter)
                hit("trellis", "size", c.w, c.h, tr.cls, c.plane), hit("trellis", "eob", c.w, c.h, eob)
                for p in range(n):   # the levels after the trim
                    tr.set_level(p, abs(q[p]))
                eob, skipped = tr.walk(eob, eob_cost, bool(c.fast), skip_cost, non_skip_cost)
                path |= abi.RDOQ_PATH_SKIP if skipped else 0
            else:
                hit("trim", "emptied_in_trellis")
    return np.array(q, np.int32), np.array(dq, np.int32), eob, cul_level(q, scan, eob), path


def dequant_shift(c):
    """hbd_md ? bit depth of the picture - 5 : 3"""
    return c.pic_bd - 5 if c.bd > 8 else 3


def early_exit_limit(c):
    return (7 - c.sq_size.bit_length() + 1) * c.early_exit_th


class Block:
    """Everything of one case: its coefficients, what the first quantiser leaves, and the restated result."""

    def __init__(self, gold, orc, i, hit=lambda *k: None):
        c = self.c = CASES[i]
        self.iscan = gold.iscan(c.w, c.h, c.tx_type)
        self.qt = gold.qt(c)
        self.qm, self.iqm = gold.qm(c)
        self.coeff = coefficients(i, c, self.iscan, self.qt, self.qm)
        self.mode, self.q0, self.dq0, self.eob0, self.satd = first_quant(orc, c, self.coeff, self.iscan, self.qt, self.qm, self.iqm)
        b_mode = abi.QUANT_B_HBD if c.bd > 8 else abi.QUANT_B
        self.q, self.dq, self.eob, self.cul, self.path = restate(
            c, gold.tables[c.table], self.coeff, self.mode, self.q0, self.dq0, self.eob0, self.satd, self.iscan, self.qt, self.qm, self.iqm,
            lambda: quant(orc, b_mode, c, self.coeff, self.iscan, self.qt, self.qm, self.iqm), hit)
        self.changed = int((self.q != self.q0).sum() + (self.dq != self.dq0).sum())   # coefficients the stage changed, both arrays


# ------------------------------------------------------------------------------------------------ device input
def batch(blocks, w, h, order=None, repeat=1):
    """The blocks of size w x h as one launch: (indices into blocks, arena image, transform descriptors, RDOQ descriptors, transform
    results, the arena's named regions), the three as record arrays.  Every byte of the arena that is no input holds the pattern."""
    idx = [i for i, b in enumerate(blocks) if (b.c.w, b.c.h) == (w, h)]
    if order is not None:
        idx = [idx[k] for k in order(len(idx))]
    idx = idx * repeat
    ab = Arena(fill=PATTERN)
    shared = {}

    def once(key, arr):
        if key not in shared:
            shared[key] = ab.add(f"{key[0]} {key[1]}", arr)
        return shared[key]
    tdescs = np.zeros(len(idx), abi.TXFM_DESC_DTYPE)
    descs = np.zeros(len(idx), abi.RDOQ_DESC_DTYPE)
    results = np.zeros(len(idx), abi.TXFM_RESULT_DTYPE)
    for k, i in enumerate(idx):
        b, c = blocks[i], blocks[i].c
        d, r = tdescs[k], descs[k]
        d["coeff_off"], d["qcoeff_off"], d["dqcoeff_off"] = ab.add(f"coeff of block {k}", b.coeff), ab.add(f"qcoeff of block {k}", b.q0), ab.add(f"dqcoeff of block {k}", b.dq0)
        d["residual_off"] = d["pred_off"] = d["recon_off"] = abi.NO_OFFSET
        d["iscan_off"] = once(("iscan", c.tx_type), b.iscan)
        d["qm_off"] = once(("qm", c.plane), b.qm) if c.qm else abi.NO_OFFSET
        d["iqm_off"] = once(("iqm", c.plane), b.iqm) if c.qm else abi.NO_OFFSET
        fp = b.mode in (abi.QUANT_FP, abi.QUANT_FP_HBD)
        d["zbin"], d["round"], d["quant"] = b.qt["zbin"][:2], b.qt["round_fp" if fp else "round"][:2], b.qt["quant_fp" if fp else "quant"][:2]
        d["quant_shift"], d["dequant"] = b.qt["qshift"][:2], b.qt["dequant"][:2]
        d["tx_type"], d["bit_depth"], d["quant_mode"], d["log_scale"] = c.tx_type, c.bd, b.mode, T.tx_scale(w, h)
        r["table"], r["lambda"], r["early_exit_limit"] = c.table, c.lam, early_exit_limit(c)
        r["zbin"], r["round"], r["quant"], r["quant_shift"] = b.qt["zbin"][:2], b.qt["round"][:2], b.qt["quant"][:2], b.qt["qshift"][:2]
        r["plane_type"], r["txb_skip_ctx"], r["dc_sign_ctx"], r["is_inter"] = c.plane, c.skip_ctx, c.dc_sign_ctx, c.is_inter
        r["eob_th"], r["eob_fast_th"], r["satd_factor"], r["dequant_shift"] = c.eob_th, c.eob_fast_th, c.satd_factor, dequant_shift(c)
        r["pic_bit_depth"] = c.pic_bd if c.pic_bd != c.bd or k % 2 else 0     # 0: the transform descriptor's
        r["flags"] = abi.RDOQ_PERFORM * c.perform | abi.RDOQ_FAST_MODE * c.fast | abi.RDOQ_SHARPNESS * c.sharp
        results[k]["three_quad_energy"], results[k]["eob"], results[k]["pad_"], results[k]["satd"] = 0x1234567800000000 + i, b.eob0, 0xBEEF, b.satd
    return idx, ab.build(), tdescs, descs, results, ab.regions


# ------------------------------------------------------------------------------------------------ the reference, where it was built
class PinArgs(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("bit_depth", "qindex", "plane", "tx_size", "tx_type", "txb_skip_ctx", "dc_sign_ctx", "is_inter")] + \
               [("lam", C.c_uint32)] + \
               [(f, C.c_int32) for f in ("rdoq_level", "fast_mode", "sharpness", "eob_th", "eob_fast_th", "satd_factor", "early_exit_th", "sq_size",
                                         "qm_level", "fp_q", "pic_bd")]


class Pin:
    """tests/rdoq_pin_driver.c built into `directory` against oracle/_ref/libsvtref.so (ref: the loaded pyorc.ref(), whose ref_init
    has set the RTCD pointers the quantisers, svt_aom_satd and svt_av1_txb_init_levels go through)."""

    def __init__(self, ref, directory):
        from support import build_pin
        self.ref, self.lib = ref, build_pin(directory, os.path.join(HERE, "rdoq_pin_driver.c"))
        self.lib.pin_tables_new.restype, self.lib.pin_tables_new.argtypes = C.c_void_p, [C.c_int32]
        self.lib.pin_rdoq.argtypes = [C.c_void_p] * 5 + [C.c_void_p]
        self.handles = [self.lib.pin_tables_new(q) for q in T.QINDEX]

    def quant_tables(self):
        out = np.zeros((len(BIT_DEPTHS), len(T.QINDEX), len(QT_FIELDS), 2), np.int16)
        for b, bd in enumerate(BIT_DEPTHS):
            for k, qi in enumerate(T.QINDEX):
                self.lib.pin_quant_tables(bd, qi, C.c_void_p(out[b, k].ctypes.data))
        return out

    def qm(self, plane, w, h, level=QM_LEVEL):
        iw, ih = T.retained(w, h)
        qm, iqm = np.zeros(iw * ih, np.uint8), np.zeros(iw * ih, np.uint8)
        assert self.lib.pin_qm(level, plane, T.TX_INDEX[(w, h)], C.c_void_p(qm.ctypes.data), C.c_void_p(iqm.ctypes.data)) == iw * ih
        return qm, iqm

    @staticmethod
    def args(c):
        return PinArgs(c.bd, T.QINDEX[c.table], c.plane, T.TX_INDEX[(c.w, c.h)], c.tx_type, c.skip_ctx, c.dc_sign_ctx, c.is_inter, c.lam, c.perform, c.fast,
                       c.sharp, c.eob_th, c.eob_fast_th, c.satd_factor, c.early_exit_th, c.sq_size, QM_LEVEL if c.qm else NO_QM_LEVEL, c.fp_q, c.pic_bd)

    def iscan(self, w, h, tx_type):
        iw, ih = T.retained(w, h)
        out = np.zeros(iw * ih, np.int16)
        assert self.lib.pin_iscan(T.TX_INDEX[(w, h)], tx_type, C.c_void_p(out.ctypes.data)) == out.size
        return out

    def run_many(self, cases, coeffs):
        """The same over blocks of one size and table set in one call -> (qcoeff, dqcoeff, eob), each with a leading block axis"""
        co = np.ascontiguousarray(coeffs, np.int32)
        nb, n = co.shape
        a = (PinArgs * nb)(*[self.args(c) for c in cases])
        q, dq, eob = np.zeros((nb, n), np.int32), np.zeros((nb, n), np.int32), np.zeros(nb, np.uint16)
        self.lib.pin_rdoq_many(C.c_void_p(self.handles[cases[0].table]), a, C.c_void_p(co.ctypes.data), C.c_void_p(q.ctypes.data), C.c_void_p(dq.ctypes.data),
                               C.c_void_p(eob.ctypes.data), nb, n)
        return q, dq, eob

    def run(self, c, coeff):
        """svt_aom_quantize_inv_quantize on the coefficients of case c -> (qcoeff, dqcoeff, eob, cul_level)"""
        n = len(coeff)
        a = self.args(c)
        co = np.ascontiguousarray(coeff, np.int32).copy()
        q, dq, eob = np.full(n, 7, np.int32), np.full(n, 7, np.int32), C.c_uint16(9999)
        cul = self.lib.pin_rdoq(C.c_void_p(self.handles[c.table]), C.byref(a), C.c_void_p(co.ctypes.data), C.c_void_p(q.ctypes.data),
                                C.c_void_p(dq.ctypes.data), C.byref(eob))
        assert np.array_equal(co, coeff)
        return q, dq, eob.value, cul
