"""Seeded cases for svt_hip_cdef_pick_strengths and a plain Python driver of finish_cdef_search (enc_cdef.c:728-926) for
use_reference_cdef_fs == 0 and 64x64 superblocks (test infrastructure).  The driver does the participation, the bias,
joint_strength_search_dual, the RD choice, the per-block index and the filter map; the leaf under it, svt_search_one_dual, is a
function it is GIVEN (the reference's own or the oracle's), called through leaf_cases.run_dual's convention.  Tables are
regenerated from the seeds; tests/golden/cdef_pick.npz stores results only."""
import ctypes as C
from collections import namedtuple

import numpy as np

from svtav1_hip import abi

M64 = (1 << 64) - 1
HUGE = 1 << 63
DEFAULT_MSE_UV = 1040400 * 64      # default_mse_uv * 64 (cdef_process.c:78, :251)
WIDTHS, LEVELS = abi.CDEF_PICK_WIDTHS, abi.CDEF_PICK_MAX_LEVELS
RESULT_DTYPE = np.dtype(abi.CDEF_PICK_RESULT_DTYPE)

# kind: plain = uniform below 1 << bits; quant = plain quantised to multiples of 64 (many equal sums); equal = one value everywhere;
#       wrap = every entry 1 << 62 (U + V = 1 << 63, totals wrap); classes3 = every block is served best by one of the pairs
#       (0,0), (1,1), (2,2) and by nothing else, so a fourth slot cannot gain
# part: all / half / one / none of the filter blocks have a filtered 8x8;  uv: the chroma list has -1 entries
Case = namedtuple("Case", "name cols rows n bits kind part uv bias lam seed")
CASES = [
    Case("g1x1_n1", 1, 1, 1, 8, "plain", "all", 0, 0, 50, 1),
    Case("g1x1_n4_quant", 1, 1, 4, 8, "quant", "all", 1, 62, 3, 2),
    Case("g4x3_n4_classes", 4, 3, 4, 24, "classes3", "all", 0, 0, 1000, 3),
    Case("g4x3_n9_half", 4, 3, 9, 24, "plain", "half", 1, 0, 1 << 30, 4),
    Case("g4x3_n16_b40", 4, 3, 16, 40, "plain", "all", 0, 63, 1 << 40, 5),
    Case("g4x3_n64_quant", 4, 3, 64, 24, "quant", "all", 1, 0, 1 << 20, 6),
    Case("g4x3_n16_equal", 4, 3, 16, 8, "equal", "all", 0, 0, 700, 7),
    Case("g4x3_n9_wrap", 4, 3, 9, 62, "wrap", "all", 0, 62, 12345, 8),
    Case("g4x3_n4_one", 4, 3, 4, 24, "plain", "one", 1, 0, 1 << 22, 9),
    Case("g4x3_n16_none", 4, 3, 16, 24, "plain", "none", 0, 63, 1 << 16, 10),
    Case("g17x15_n16", 17, 15, 16, 24, "plain", "all", 1, 0, 1 << 31, 11),
    Case("g17x15_n9_quant_b40", 17, 15, 9, 40, "quant", "half", 0, 62, 1 << 49, 12),
    Case("g17x15_n64_b40", 17, 15, 64, 40, "plain", "all", 1, 63, 1 << 45, 13),
    Case("g17x15_n4_b8", 17, 15, 4, 8, "plain", "half", 0, 0, 1 << 16, 14),
    Case("g17x15_n9_wrap_half", 17, 15, 9, 62, "wrap", "half", 1, 0, 99, 15),
    Case("g19x14_n16", 19, 14, 16, 24, "plain", "all", 0, 0, 1 << 33, 16),
    Case("g19x14_n9_quant_b8", 19, 14, 9, 8, "quant", "half", 1, 63, 1 << 14, 17),
    Case("g19x14_n1_b40", 19, 14, 1, 40, "plain", "all", 0, 0, 1 << 20, 18),
    Case("g19x14_n4_classes", 19, 14, 4, 24, "classes3", "all", 0, 0, 1 << 12, 19),
    Case("g60x34_n16", 60, 34, 16, 24, "plain", "half", 1, 62, 1 << 32, 20),
]
LUMA_LIST = [0, 4, 9, 1, 16, 63, 2, 22, 5, 36, 3, 48, 7, 12, 60, 33]   # pri * 4 + sec values the search lists draw from


class Inputs:
    """What the entry point is given for one case: mse [3][n_fb][n], filt8x8 [h8][w8], the two strength lists."""


def make_inputs(case):
    rng = np.random.default_rng(7000 + case.seed)
    n_fb, n = case.cols * case.rows, case.n
    x = Inputs()
    x.case, x.n_fb = case, n_fb
    x.w8, x.h8 = case.cols * 8 - case.seed % 4, case.rows * 8 - case.seed % 3
    if case.kind == "wrap":
        mse = np.full((3, n_fb, n), 1 << 62, np.uint64)
    elif case.kind == "equal":
        mse = np.full((3, n_fb, n), 123, np.uint64)
    elif case.kind == "classes3":
        cls = rng.integers(0, 3, size=n_fb)
        hi = rng.integers(1 << (case.bits - 1), 1 << case.bits, size=(3, n_fb, n)).astype(np.uint64)
        lo = rng.integers(0, 1 << (case.bits - 8), size=(3, n_fb)).astype(np.uint64)
        mse = hi
        mse[:, np.arange(n_fb), cls] = lo
    else:
        mse = rng.integers(0, 1 << case.bits, size=(3, n_fb, n)).astype(np.uint64)
        if case.kind == "quant":
            mse = mse // np.uint64(64) * np.uint64(64)
    x.mse = np.ascontiguousarray(mse)
    takes = {"all": np.ones(n_fb, bool), "none": np.zeros(n_fb, bool), "half": rng.random(n_fb) < 0.5,
             "one": np.arange(n_fb) == int(rng.integers(0, n_fb))}[case.part]
    filt = np.zeros((x.h8, x.w8), np.uint8)
    for fb in np.flatnonzero(takes):
        r0, c0 = fb // case.cols * 8, fb % case.cols * 8
        th, tw = min(8, x.h8 - r0), min(8, x.w8 - c0)
        tile = (rng.random((th, tw)) < 0.3).astype(np.uint8) * np.uint8(1 + fb % 200)
        tile[int(rng.integers(0, th)), int(rng.integers(0, tw))] = 1
        filt[r0:r0 + th, c0:c0 + tw] = tile
    x.filt = filt
    x.strengths = [LUMA_LIST[(gi + case.seed) % 16] if n <= 16 else (gi * 37 + case.seed) % 64 for gi in range(n)]
    x.strengths[0] = 0      # the lists start with (0, 0): the entry the zero-strength bias is about
    x.strengths_uv = [(-1 if case.uv and gi % 3 == 2 else x.strengths[gi] ^ (gi & 1)) for gi in range(n)]
    return x


def params(x):
    p = abi.CdefPickParams()
    p.n_strengths, p.fb_cols, p.fb_rows, p.w8, p.h8 = x.case.n, x.case.cols, x.case.rows, x.w8, x.h8
    p.zero_fs_cost_bias = x.case.bias
    setattr(p, "lambda", x.case.lam)      # a Python keyword
    for gi in range(x.case.n):
        p.strengths[gi], p.strengths_uv[gi] = x.strengths[gi], x.strengths_uv[gi]
    return p


def takes_part(filt, cols, rows):
    """!skip_cdef_seg per filter block: at least one 8x8 of its tile is filtered (the glue's rule)."""
    return np.array([bool(filt[r * 8:r * 8 + 8, c * 8:c * 8 + 8].any()) for r in range(rows) for c in range(cols)])


def rdcost(lam, rate, dist):
    """RDCOST (rd_cost.h:37-39) on 64-bit two's complement values."""
    prod = (rate * lam + 256) & M64
    prod = prod - (1 << 64) if prod >> 63 else prod
    return ((prod >> 9) + ((dist << 7) & M64)) & M64


def drive(x, search):
    """finish_cdef_search over the tables of `x`.  search((lev0, lev1, nb, mse[2][sb][64], start_gi, end_gi)) -> (total, lev0, lev1)
    is one svt_search_one_dual call (leaf_cases.run_dual / run_dual_orc with the function bound).  Returns a dict: `result` (one
    RESULT_DTYPE record), `fb_gi` [n_fb], `fb_strength` [2][n_fb], and what only the case checks read: `greedy0` / `greedy1`
    [4][8], the lists before the refinement, and `tied`, the number of pairs that share the smallest total of the first step."""
    case, n, n_fb = x.case, x.case.n, x.n_fb
    part = takes_part(x.filt, case.cols, case.rows)
    idx = np.flatnonzero(part)
    sb = len(idx)
    mse = np.zeros((2, sb, 64), np.uint64)         # TOTAL_STRENGTHS entries per block as in the reference
    mse[0, :, :n] = x.mse[0, idx]
    uv = x.mse[1, idx] + x.mse[2, idx]             # uint64: wraps as C does
    uv[:, np.array([gi for gi in range(n) if x.strengths_uv[gi] == -1], np.intp)] = DEFAULT_MSE_UV
    mse[1, :, :n] = uv
    if case.bias:
        mse[:, :, 0] = (np.uint64(case.bias) * mse[:, :, 0]) >> np.uint64(6)
    res = np.zeros((), RESULT_DTYPE)
    greedy = np.zeros((2, WIDTHS, LEVELS), np.int32)
    best = HUGE
    for i in range(WIDTHS):
        nbs = 1 << i
        l0, l1 = np.zeros(LEVELS, np.int32), np.zeros(LEVELS, np.int32)
        for k in range(nbs):
            tot, l0, l1 = search((l0, l1, k, mse, 0, n))
        greedy[0, i], greedy[1, i] = l0, l1
        for _ in range(4 * nbs):
            l0[:nbs - 1], l1[:nbs - 1] = l0[1:nbs].copy(), l1[1:nbs].copy()
            tot, l0, l1 = search((l0, l1, nbs - 1, mse, 0, n))
        res["joint_mse"][i], res["lev0"][i], res["lev1"][i] = tot, l0, l1
        total_bits = sb * i + nbs * 6 * 2
        rd = rdcost(case.lam, total_bits * 512, (tot * 16) & M64)
        res["rd_cost"][i] = rd
        if rd < best:
            best = rd
            res["cdef_bits"], res["best_cost"] = i, rd
            res["y_index"][:], res["uv_index"][:] = 0, 0
            res["y_index"][:nbs], res["uv_index"][:nbs] = l0[:nbs], l1[:nbs]
    nbs = 1 << int(res["cdef_bits"])
    res["nb_strengths"], res["sb_count"] = nbs, sb
    for g in range(nbs):
        res["y_strength"][g], res["uv_strength"][g] = x.strengths[res["y_index"][g]], x.strengths[res["uv_index"][g]]
    fb_gi, fb_strength = np.full(n_fb, 0xFF, np.uint8), np.zeros((2, n_fb), np.uint8)
    for b, fb in enumerate(idx):
        best_gi, best_mse = 0, HUGE
        for gi in range(nbs):
            cur = (int(mse[0, b, res["y_index"][gi]]) + int(mse[1, b, res["uv_index"][gi]])) & M64
            if cur < best_mse:
                best_gi, best_mse = gi, cur
        fb_gi[fb], fb_strength[0, fb], fb_strength[1, fb] = best_gi, res["y_strength"][best_gi], res["uv_strength"][best_gi]
    first = np.minimum(mse[0, :, :n, None] + mse[1, :, None, :n], np.uint64(HUGE)).sum(axis=0, dtype=np.uint64) if sb else np.zeros((n, n), np.uint64)
    return {"result": res, "fb_gi": fb_gi, "fb_strength": fb_strength, "greedy0": greedy[0], "greedy1": greedy[1],
            "tied": np.int32((first == first.min()).sum())}


def ref_search(ref):
    """The reference's svt_search_one_dual through its dispatch pointer (oracle/_ref/libsvtref.so), as make_golden_leaves.py takes it."""
    import leaf_cases as L
    from lf_cases import V, rtcd
    dual = rtcd(ref, "svt_search_one_dual", C.c_uint64, V, V, C.c_int, V, C.c_int, C.c_int, C.c_int)
    return lambda c: L.run_dual(dual, c)


def orc_search(orc):
    import leaf_cases as L
    return lambda c: L.run_dual_orc(orc, c)


FIELDS = ("result", "fb_gi", "fb_strength", "greedy0", "greedy1", "tied")


def same(a, b, fields=FIELDS):
    """The names of the fields in which two driver / fixture / device outputs differ."""
    return [f for f in fields if not (a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes())]


_golden = {}


def golden(case):
    """The recorded results of one case (tests/golden/cdef_pick.npz, written by tests/golden/make_golden_cdef_pick.py)."""
    import os
    if not _golden:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cdef_pick.npz")) as g:
            _golden.update({k: g[k] for k in g.files})
    return {f: _golden[f"{case.name}_{f}"] for f in FIELDS}


ARGS = ("prm", "d_mse", "d_filt8x8", "d_result", "d_fb_gi", "d_fb_strength", "d_workspace")


def rejections(x):
    """(label, change of the parameters, argument to pass as NULL, bytes to take off the workspace size): every call
    svt_hip_cdef_pick_strengths must refuse with SVT_HIP_ERR_BAD_PARAMETER."""
    n, cols, rows = x.case.n, x.case.cols, x.case.rows
    for a in ARGS:
        yield f"NULL {a}", {}, a, 0
    for v in (0, -1, 65):
        yield f"n_strengths {v}", {"n_strengths": v}, None, 0
    for v in (-1, 64, 127):
        yield f"strengths[{n - 1}] {v}", {"strengths": (n - 1, v)}, None, 0
    for v in (-2, 64, -128):
        yield f"strengths_uv[0] {v}", {"strengths_uv": (0, v)}, None, 0
    yield "no columns", {"fb_cols": 0}, None, 0
    yield "no rows", {"fb_rows": 0}, None, 0
    yield "w8 short", {"w8": (cols - 1) * 8}, None, 0
    yield "h8 short", {"h8": (rows - 1) * 8}, None, 0
    yield "workspace short", {}, None, 1


def rejected_params(x, change):
    p = params(x)
    for k, v in change.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p
