"""TEST INFRASTRUCTURE — cases, numpy restatement and arena / descriptor builder for the coefficient rate of transform blocks
(svt_hip_txb_cost_batch, include/svt_hip_txfm.h).

The rate tables and the scans are data the reference computes; they and every case's expected bits live in tests/golden/txb_cost.npz
(written by tests/golden/make_golden_txb_cost.py).  tests/test_txb_cost_abi.py pins fixture and restatement to the reference's own
svt_av1_cost_coeffs_txb through tests/txb_cost_pin_driver.c wherever oracle/_ref/libsvtref.so has been built."""
import collections
import ctypes as C
import os

import numpy as np

from arena import PATTERN, Arena
from svtav1_hip import abi
from tx_cases import SIZES

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "txb_cost.npz")
QINDEX = (40, 200)                 # two of the four base-qindex classes of svt_av1_default_coef_probs: table sets 0 and 1
TX_INDEX = {s: i for i, s in enumerate(SIZES)}          # TxSize of w x h
DCT_DCT, ADST_DCT, FLIPADST_ADST, IDTX, V_DCT, H_DCT, V_ADST, H_ADST = 0, 1, 8, 9, 10, 11, 12, 13
NEARESTMV, NEW_NEWMV, FILTER_INTRA_NONE = 13, 24, 5
# av1_ext_tx_used (definitions.h:1786-1793) as sets of TxType, by TxSetType
EXT_TX_USED = [{0}, {0, 9}, {0, 1, 2, 3, 9}, {0, 1, 2, 3, 9, 10, 11}, set(range(12)), set(range(16))]

Case = collections.namedtuple("Case", "group w h tx_type plane eob skip_ctx dc_sign_ctx pred_mode fim reduced fast step est_mode flags table "
                                      "lam dc beyond dist")


def retained(w, h):
    return min(w, 32), min(h, 32)


def size_index(v):
    return {4: 0, 8: 1, 16: 2, 32: 3, 64: 4}[v]


def tx_class(tx_type):
    """tx_type_to_class: 0 two-dimensional, 1 horizontal, 2 vertical"""
    return 0 if tx_type < 10 else (1 if tx_type & 1 else 2)


def ext_tx_set_type(w, h, is_inter, reduced):
    """get_ext_tx_set_type (definitions.h:1795-1810)"""
    sqr, sqr_up = size_index(min(w, h)), size_index(max(w, h))
    if sqr_up > 3:
        return 0
    if sqr_up == 3:
        return 1 if is_inter else 0
    if reduced:
        return 1 if is_inter else 2
    if is_inter:
        return 4 if sqr == 2 else 5
    return 2 if sqr == 2 else 3


def is_inter_mode(pred_mode):
    return 13 <= pred_mode < 25


def type_allowed(c):
    return c.tx_type in EXT_TX_USED[ext_tx_set_type(c.w, c.h, is_inter_mode(c.pred_mode), c.reduced)]


def eob_edges(n):
    """0, 1, 2, 3 and both sides of the thresholds of the eob context (n / 8, n / 4), and the full block"""
    return sorted({e for e in (0, 1, 2, 3, n // 8, n // 8 + 1, n // 4, n // 4 + 1, n) if e <= n})


def size_types(w, h):
    """One type of every class the size allows for an inter block without the reduced set (the widest set)."""
    used = EXT_TX_USED[ext_tx_set_type(w, h, 1, 0)]
    return [t for t in (DCT_DCT, FLIPADST_ADST if FLIPADST_ADST in used else IDTX, H_ADST if H_ADST in used else H_DCT, V_DCT) if t in used]


def _cases():
    out = []
    combos = [(f, s) for f in (1, 2, 3) for s in (0, 1, 2)]

    def add(group, w, h, tx_type, plane, eob, **kw):
        i = len(out)
        d = dict(skip_ctx=(0, 12)[i % 2], dc_sign_ctx=i % 3, pred_mode=NEARESTMV, fim=FILTER_INTRA_NONE, reduced=0, fast=1, step=0, est_mode=0,
                 flags=0, table=(i // 3) % 2, lam=1 + (i * 2654435761) % (1 << 22), dc=("neg", "pos", "zero")[(i // 2) % 3], beyond=0,
                 dist=(i * 0x9E3779B97F4A7C15) % (1 << 40))
        d.update(kw)
        out.append(Case(group, w, h, tx_type, plane, eob, **d))

    # every size x one type per class x both planes x the eob edges; contexts, rate controls and table sets take turns
    for w, h in SIZES:
        n = retained(w, h)[0] * retained(w, h)[1]
        for tx_type in size_types(w, h):
            for plane in (0, 1):
                for eob in eob_edges(n):
                    fast, step = combos[len(out) % 9]
                    add("grid", w, h, tx_type, plane, eob, fast=fast, step=step, flags=abi.TXB_COST_NO_SHIFT if plane and len(out) % 4 < 2 else 0)
    # c_start: every fast_coeff_est_level x subres_step, with eob = 2 (empty loop) and longer scans
    for w, h in ((4, 4), (16, 8), (32, 32)):
        n = retained(w, h)[0] * retained(w, h)[1]
        for fast, step in combos:
            for eob in (2, 3, n // 4 + 1, n):
                add("c_start", w, h, DCT_DCT, 0, eob, fast=fast, step=step)
    # the transform-type rate: intra with three modes, filter intra, inter, both sets; sizes of every set type (64 x 64: one type, rate 0)
    for w, h in ((4, 4), (8, 8), (16, 16), (16, 4), (8, 32), (32, 32), (64, 64), (16, 64)):
        n = retained(w, h)[0] * retained(w, h)[1]
        for pred_mode, fim in ((0, 5), (1, 5), (12, 5), (0, 3), (0, 1), (NEARESTMV, 5), (NEW_NEWMV, 5)):
            for reduced in (0, 1):
                used = sorted(EXT_TX_USED[ext_tx_set_type(w, h, is_inter_mode(pred_mode), reduced)])
                for tx_type in (used[0], used[-1]):
                    add("tx_type_rate", w, h, tx_type, 0, n // 8 + 1, pred_mode=pred_mode, fim=fim, reduced=reduced)
    # the closed forms, on both sides of eob < area / 64
    for w, h in ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (16, 64)):
        th = (w * h) >> 6
        for est_mode in (1, 2):
            for eob in sorted({max(th - 1, 0), th, th + 1, 0}):
                add("closed_form", w, h, DCT_DCT, 0, eob, est_mode=est_mode, step=1, fast=2)
    # a value beyond eob in scan order (the levels see it), on every class
    for w, h in ((4, 4), (8, 16), (32, 32), (64, 32)):
        n = retained(w, h)[0] * retained(w, h)[1]
        for tx_type in size_types(w, h):
            add("beyond_eob", w, h, tx_type, 0, n // 4, beyond=1)
            add("beyond_eob", w, h, tx_type, 1, 3, beyond=1)
    # no size's batch ends on a full workgroup (256 lanes, min(n, 64) lanes to a block)
    for w, h in SIZES:
        per_wg = 256 // min(retained(w, h)[0] * retained(w, h)[1], 64)
        if sum((c.w, c.h) == (w, h) for c in out) % per_wg == 0:
            add("ragged", w, h, DCT_DCT, 0, 2)
    return out


CASES = _cases()
# magnitudes a non-zero coefficient takes: the base levels, both sides of the Golomb switch at 1 + NUM_BASE_LEVELS + COEFF_BASE_RANGE
# = 15, both sides of the level clamp at 127, and 2^15 and above
MAGNITUDES = (1, 2, 3, 14, 15, 127, 128, 1 << 15, (1 << 15) + 5, 100000)


def scan_of(iscan):
    scan = np.empty(len(iscan), np.int64)
    scan[iscan] = np.arange(len(iscan))
    return scan


def coefficients(i, c, iscan):
    """The quantised block of case i: magnitudes of MAGNITUDES and zeros below eob in scan order, a non-zero value at eob - 1, the DC
    the case asks for, and with `beyond` one non-zero value past eob."""
    n = len(iscan)
    rng = np.random.default_rng(1000 + i)
    q = np.zeros(n, np.int64)
    if c.eob:
        scan = scan_of(iscan)
        mag = rng.choice((0,) + MAGNITUDES, size=c.eob, p=(0.3,) + (0.07,) * 10)
        mag[c.eob - 1] = rng.choice(MAGNITUDES)
        vals = mag * rng.choice((-1, 1), size=c.eob)
        if c.eob > 1 or c.dc != "zero":
            vals[0] = {"neg": -abs(vals[0]) or -2, "pos": abs(vals[0]) or 15, "zero": 0}[c.dc]
        q[scan[:c.eob]] = vals
        if c.beyond and c.eob < n:
            q[scan[rng.integers(c.eob, n)]] = rng.choice((-3, 1, 130))
    return q.astype(np.int32)


# ------------------------------------------------------------------------------------------------ the rate, restated
def golomb(level):
    """get_golomb_cost (rd_cost.c:90-97) of an integer array"""
    r = np.maximum(level - 14, 0)
    length = sum(((r >> k) > 0).astype(np.int64) for k in range(40))
    return np.where(level >= 15, (2 * length - 1) * 512, 0)


def eob_cost(t, n, plane, cc, eob, cls):
    """get_eob_cost (rd_cost.c:281-298)"""
    small = [0, 1, 2, 3, 3, 4, 4, 4, 4] + [5] * 8 + [6] * 16
    large = [6, 7, 8, 8, 9, 9, 9, 9] + [10] * 8 + [11]
    group_start = [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513]
    offset_bits = [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    pt = small[eob] if eob < 33 else large[min((eob - 1) >> 5, 16)]
    cost = int(t["eob"][n.bit_length() - 5][plane][int(cls != 0)][pt - 1])
    if offset_bits[pt] > 0:
        extra = eob - group_start[pt]
        cost += int(cc["eob_extra"][pt - 3][(extra >> (offset_bits[pt] - 1)) & 1])
        if offset_bits[pt] > 1:
            cost += (offset_bits[pt] - 1) * 512
    return cost


def tx_type_rate(t, c):
    """av1_transform_type_rate_estimation (rd_cost.c:113-158)"""
    is_inter = is_inter_mode(c.pred_mode)
    set_type = ext_tx_set_type(c.w, c.h, is_inter, c.reduced)
    if len(EXT_TX_USED[set_type]) <= 1:
        return 0
    ext_tx_set = ((0, -1, 2, 1, -1, -1), (0, 3, -1, -1, 2, 1))[is_inter][set_type]   # ext_tx_set_index
    sq = size_index(min(c.w, c.h))
    if is_inter:
        return int(t["inter_tx_type"][ext_tx_set][sq][c.tx_type])
    intra_dir = (0, 1, 2, 6, 0)[c.fim] if c.fim != FILTER_INTRA_NONE else c.pred_mode   # fimode_to_intradir
    return int(t["intra_tx_type"][ext_tx_set][sq][intra_dir][c.tx_type])


def restate_bits(t, c, q, iscan, eob=None):
    """bits of svt_hip_txb_cost_batch for case c on the block q (raster order) with the table set t (one record of
    abi.RATE_TABLES_DTYPE): svt_av1_cost_coeffs_txb + its caller, position by position in numpy."""
    iw, ih = retained(c.w, c.h)
    n = iw * ih
    eob = min(c.eob if eob is None else eob, n)
    th = (c.w * c.h) >> 6
    if c.est_mode >= 1 and eob < th:
        return 6000 + 1000 * eob
    if c.est_mode == 2:
        return 3000 + 100 * eob
    txs_ctx = (size_index(min(c.w, c.h)) + size_index(max(c.w, c.h)) + 1) >> 1
    cc = t["coeff"][txs_ctx][c.plane]
    if eob == 0:
        return int(cc["txb_skip"][c.skip_ctx][1])
    cls = tx_class(c.tx_type)
    cost = int(cc["txb_skip"][c.skip_ctx][0]) + (tx_type_rate(t, c) if c.plane == 0 else 0) + eob_cost(t, n, c.plane, cc, eob, cls)
    q = q.astype(np.int64)
    level = np.abs(q)
    base_range = np.minimum(level - 3, 12)
    if eob == 1:   # av1_cost_coeffs_txb_loop_cost_one_eob
        v, lv = int(q[0]), int(level[0])
        cost += int(cc["base_eob"][0][min(lv, 3) - 1])
        if v:
            cost += int(cc["dc_sign"][c.dc_sign_ctx][int(v < 0)])
            if lv > 2:
                cost += int(cc["lps"][0][base_range[0]]) + int(golomb(level[:1])[0])
        return cost << (0 if c.flags & abi.TXB_COST_NO_SHIFT else c.step)
    # svt_av1_txb_init_levels_c: clamped levels of the whole block, zero padding right and below
    lev = np.zeros((ih + 4, iw + 4), np.int64)
    lev[:ih, :iw] = np.minimum(level, 127).reshape(ih, iw)
    row, col = np.divmod(np.arange(n), iw)

    def at(dr, dc):
        return lev[row + dr, col + dc]
    c3 = lambda x: np.minimum(x, 3)   # noqa: E731
    # get_nz_mag / get_nz_map_ctx_from_stats
    mag = c3(at(0, 1)) + c3(at(1, 0))
    if cls == 0:
        mag = mag + c3(at(1, 1)) + c3(at(0, 2)) + c3(at(2, 0))
        if c.w < c.h:
            off = np.where(row < 2, 11, np.where(row + col < 2, 1, np.where(row + col < 4, 6, 21)))
        elif c.w > c.h:
            off = np.where(col < 2, 16, np.where(row + col < 2, 1, np.where(row + col < 4, 6, 21)))
        else:
            off = np.where(row + col < 2, 1, np.where(row + col < 4, 6, 21))
    elif cls == 2:
        mag = mag + c3(at(2, 0)) + c3(at(3, 0)) + c3(at(4, 0))
        off = np.where(row == 0, 26, np.where(row == 1, 31, 36))
    else:
        mag = mag + c3(at(0, 2)) + c3(at(0, 3)) + c3(at(0, 4))
        off = np.where(col == 0, 26, np.where(col == 1, 31, 36))
    nz_ctx = np.minimum((mag + 1) >> 1, 4) + off
    if cls == 0:
        nz_ctx[0] = 0
    # get_br_ctx
    bmag = at(0, 1) + at(1, 0) + (at(1, 1) if cls == 0 else at(0, 2) if cls == 1 else at(2, 0))
    near = ((row < 2) & (col < 2)) if cls == 0 else (col == 0) if cls == 1 else (row == 0)
    br_ctx = np.minimum((bmag + 1) >> 1, 6) + np.where(np.arange(n) == 0, 0, np.where(near, 7, 14))
    high = np.where(level > 2, cc["lps"][br_ctx, np.maximum(base_range, 0)] + golomb(level), 0)
    scan = scan_of(iscan)
    # scan position eob - 1
    p = scan[eob - 1]
    ctx = 1 if eob - 1 <= n // 8 else 2 if eob - 1 <= n // 4 else 3
    cost += int(cc["base_eob"][ctx][min(int(level[p]), 3) - 1]) + (512 if q[p] else 0) + int(high[p])
    # scan position 0
    cost += int(cc["base"][nz_ctx[0]][min(int(level[0]), 3)]) + (int(cc["dc_sign"][c.dc_sign_ctx][int(q[0] < 0)]) if q[0] else 0) + int(high[0])
    # scan positions c_start .. 1
    c_start = min(eob - 2, eob // max(1, c.fast - c.step))
    ps = scan[1:c_start + 1]
    cost += int((cc["base"][nz_ctx[ps], c3(level[ps])] + np.where(q[ps] != 0, 512, 0) + high[ps]).sum())
    cost = int(np.int32(cost))
    return cost << (0 if c.flags & abi.TXB_COST_NO_SHIFT else c.step)


def tx_scale(w, h):
    """av1_get_tx_scale_tab (full_loop.h:52)"""
    return 2 if w * h > 1024 else 1 if w * h > 256 else 0


def rd_cost(w, h, lam, bits, step, dist, three_quad_energy=0):
    """product_coding_loop.c:4737-4749 and RDCOST (rd_cost.h:37) in Python integers, as the uint64 the device stores"""
    shift = (1 - tx_scale(w, h)) * 2
    d = dist + three_quad_energy
    d = ((d << -shift) if shift < 0 else (d >> shift)) << step
    return (((bits * lam + 256) >> 9) + d * 128) & ((1 << 64) - 1)


# ------------------------------------------------------------------------------------------------ fixture and device input
class Golden:
    def __init__(self, path=GOLD):
        z = np.load(path)
        self.tables = z["tables"].view(np.dtype(abi.RATE_TABLES_DTYPE)).reshape(-1)
        self.bits = z["bits"]
        self.iscans = {(int(s), int(t)): z["iscan"][o:o + n] for s, t, o, n in z["iscan_index"]}
        assert len(self.bits) == len(CASES) and len(self.tables) == len(QINDEX)

    def iscan(self, w, h, tx_type):
        return self.iscans[(TX_INDEX[(w, h)], tx_type)]


def batch(gold, w, h, order=None):
    """The cases of size w x h as one launch: (case indices, arena image, descriptor record array, distortions [n][2], the arena's
    named regions).  Every byte of the arena that is no input holds the pattern."""
    idx = [i for i, c in enumerate(CASES) if (c.w, c.h) == (w, h)]
    if order is not None:
        idx = [idx[k] for k in order(len(idx))]
    ab = Arena(fill=PATTERN)
    iscan_off = {}
    descs = np.zeros(len(idx), np.dtype(abi.TXB_COST_DESC_DTYPE))
    dist = np.zeros((len(idx), 2), np.uint64)
    for k, i in enumerate(idx):
        c = CASES[i]
        iscan = gold.iscan(w, h, c.tx_type)
        if c.tx_type not in iscan_off:
            iscan_off[c.tx_type] = ab.add(f"iscan {c.tx_type}", iscan)
        d = descs[k]
        d["qcoeff_off"], d["iscan_off"] = ab.add(f"qcoeff of block {k}", coefficients(i, c, iscan)), iscan_off[c.tx_type]
        d["table"], d["lambda"], d["eob"], d["tx_type"], d["plane_type"] = c.table, c.lam, c.eob, c.tx_type, c.plane
        d["txb_skip_ctx"], d["dc_sign_ctx"], d["pred_mode"], d["filter_intra_mode"] = c.skip_ctx, c.dc_sign_ctx, c.pred_mode, c.fim
        d["reduced_tx_set"], d["fast_coeff_est_level"], d["subres_step"], d["est_mode"], d["flags"] = c.reduced, c.fast, c.step, c.est_mode, c.flags
        dist[k] = (c.dist, 0xDEAD)
    return idx, ab.build(), descs, dist, ab.regions


def expected_rd(i, bits):
    c = CASES[i]
    return rd_cost(c.w, c.h, c.lam, int(bits), c.step, c.dist)


# ------------------------------------------------------------------------------------------------ the reference, where it was built
class Pin:
    """tests/txb_cost_pin_driver.c built into `directory` against oracle/_ref/libsvtref.so (ref: the loaded pyorc.ref(), whose
    ref_init has set the RTCD pointers the rate estimation goes through)."""

    def __init__(self, ref, directory):
        from support import build_pin
        self.ref, self.lib = ref, build_pin(directory, os.path.join(HERE, "txb_cost_pin_driver.c"))
        self.lib.pin_tables_new.restype, self.lib.pin_tables_new.argtypes = C.c_void_p, [C.c_int32]
        self.lib.pin_tables_export.restype, self.lib.pin_tables_export.argtypes = C.c_size_t, [C.c_void_p, C.c_void_p]
        self.lib.pin_iscan.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        self.lib.pin_txb_bits.restype, self.lib.pin_txb_bits.argtypes = C.c_uint64, [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int32] * 11
        self.handles = [self.lib.pin_tables_new(q) for q in QINDEX]

    def tables(self):
        out = np.zeros(len(QINDEX), np.dtype(abi.RATE_TABLES_DTYPE))
        for k, h in enumerate(self.handles):
            assert self.lib.pin_tables_export(h, out[k:k + 1].ctypes.data) == out.itemsize
        return out

    def iscan(self, w, h, tx_type):
        iw, ih = retained(w, h)
        out = np.zeros(iw * ih, np.int16)
        assert self.lib.pin_iscan(TX_INDEX[(w, h)], tx_type, out.ctypes.data) == out.size
        return out

    def allowed(self, w, h, tx_type, is_inter, reduced):
        return bool(self.lib.pin_tx_type_allowed(TX_INDEX[(w, h)], tx_type, int(is_inter), int(reduced)))

    def bits(self, c, q):
        """What the encoder's own path gives for case c: svt_aom_txb_estimate_coeff_bits for a luma block, and for a chroma block that
        asks for no shift; svt_av1_cost_coeffs_txb itself, shifted as include/svt_hip_txfm.h defines, for a chroma block that asks
        for the shift; the closed forms of tx_type_search (product_coding_loop.c:4757-4762) are arithmetic on eob alone."""
        th = (c.w * c.h) >> 6
        if c.est_mode >= 1 and c.eob < th:
            return 6000 + 1000 * c.eob
        if c.est_mode == 2:
            return 3000 + 100 * c.eob
        direct = int(c.plane == 1 and not c.flags & abi.TXB_COST_NO_SHIFT)
        q = np.ascontiguousarray(q, np.int32)
        v = self.lib.pin_txb_bits(self.handles[c.table], q.ctypes.data, c.eob, c.plane, TX_INDEX[(c.w, c.h)], c.tx_type, c.skip_ctx, c.dc_sign_ctx,
                                  c.reduced, c.pred_mode, c.fim, c.fast, c.step, direct)
        return v << c.step if direct and c.eob else v
