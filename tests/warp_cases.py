"""TEST INFRASTRUCTURE — warped prediction, the global-motion error and its refinement (include/svt_hip_inter.h): cases, input
generators, the oracle and the golden fixture of tests/test_warp_abi.py and tests/test_gpu_warp.py.

The oracle calls the reference's own exported functions (oracle/_ref/libsvtref.so through pyorc.ref()): svt_av1_warp_affine_c,
svt_aom_dec_svt_av1_highbd_warp_affine_c, svt_get_shear_params, svt_av1_warp_error and svt_av1_refine_integerized_param.
tests/golden/inter_warp.npz holds the filter table (svt_aom_warped_filter) as the reference has it, the expected blocks and the
error / refinement results; inputs are regenerated from seeds with integer arithmetic only.  Written by
`PYTHONPATH=oracle:svt-av1-mod-by-patman_amd python tests/warp_cases.py`.
"""
import ctypes as C
import os

import numpy as np

import blend_cases as B
import conv_cases as K
from svtav1_hip import abi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_warp.npz")
FULL_LIMIT = 1024    # expected blocks up to this many samples are kept in full, larger ones as sha256
INT64_MAX = (1 << 63) - 1
ONE = 1 << 16        # WARPEDMODEL_PREC_BITS
IDENTITY, TRANSLATION, ROTZOOM, AFFINE = range(4)   # TransformationType
FORMATS = ((8, 0), (10, 1), (12, 1))                # (bit depth, 16-bit samples)
LUMA, CHROMA = (64, 48), (32, 24)                   # reference planes (width, height)
WEIGHTS = ((9, 7), (11, 5), (13, 3))
# mat[2 .. 5] of models whose shear is just inside is_affine_shear_allowed (4|alpha| + 7|beta| or 4|gamma| + 4|delta| >= 65280)
LIMIT_MODELS = ((ONE, 9344, 0, ONE), (ONE, -9344, 0, ONE), (ONE, 0, 8128, 73728), (81856, 0, 0, ONE), (ONE, 0, -8128, 57344),
                (49216, 0, 0, ONE))
MODELS = ("trans", "rotzoom", "affine") + tuple(f"limit{k}" for k in range(len(LIMIT_MODELS)))
POSITIONS = ("inside", "left", "right", "top", "bottom", "out_tl", "out_tr", "out_bl", "out_br", "pcol")


class WarpedMotionParams(C.Structure):   # EbWarpedMotionParams (definitions.h:2004-2010)
    _fields_ = [("wmtype", C.c_int32), ("wmmat", C.c_int32 * 8), ("alpha", C.c_int16), ("beta", C.c_int16), ("gamma", C.c_int16),
                ("delta", C.c_int16), ("invalid", C.c_int8)]


def lib_shear(mat):
    """(ok, [alpha, beta, gamma, delta]) of svt_hip_warp_shear_params: a host function of the library, no device needed."""
    out = (C.c_int16 * 4)()
    ok = abi.load().svt_hip_warp_shear_params((C.c_int32 * 6)(*mat[:6]), out)
    return ok, list(out)


def ref_shear(ref, mat, prefill=(0, 0, 0, 0)):
    """(ok, [alpha, beta, gamma, delta]) of the reference's svt_get_shear_params."""
    wm = WarpedMotionParams(AFFINE, (C.c_int32 * 8)(*mat[:6], 0, 0), *prefill, 0)
    ok = B._fn(ref, "svt_get_shear_params", C.c_int, C.c_void_p)(C.addressof(wm))
    return ok, [wm.alpha, wm.beta, wm.gamma, wm.delta]


def ref_filter(ref):
    return np.ctypeslib.as_array((C.c_int16 * (abi.WARP_FILTER_ROWS * 8)).in_dll(ref, "svt_aom_warped_filter")).reshape(-1, 8).copy()


# ---- prediction cases -------------------------------------------------------------------------------------------------------
# (name, chroma, p_width, p_height, format index, compound, weight index, model, position, checkerboard, layout index)
def _warp_cases():
    """Every size under every (format, compound) pair.  j counts those pairs; model, window position, checkerboard and weights
    are indexed so that over its 12 cases each size meets all nine models and all ten positions (3 is coprime to 10) and every
    size gets checkerboards, instead of one position per size."""
    cases, k = [], 0
    sizes = [(0, 8, 8), (0, 8, 16), (0, 16, 8), (0, 32, 32), (0, 64, 64), (1, 4, 4), (1, 4, 8), (1, 8, 4), (1, 16, 16), (1, 32, 32)]
    for f in range(len(FORMATS)):
        for compound in range(4):
            j = 4 * f + compound
            for s, (chroma, w, h) in enumerate(sizes):
                model, pos = MODELS[(s + j) % 9], POSITIONS[(s + 3 * j) % 10]
                cases.append((f"{'c' if chroma else 'y'}{w}x{h}_bd{FORMATS[f][0]}_c{compound}_{model}_{pos}_{k}", chroma, w, h, f, compound,
                              (s + j) % 3, model, pos, (s + j) % 4 == 0, k))
                k += 1
    cases.append(("y128x128_bd8_c0_affine_inside", 0, 128, 128, 0, 0, 0, "affine", "inside", False, k))
    return cases


WARP_CASES = _warp_cases()


def rounds(bd, compound):
    return K.conv_rounds_compound(bd) if compound else K.conv_rounds(bd)


def case_model(case, index):
    """(mat[6], p_col, p_row) of a case: the translation puts the source window where `position` says."""
    _, chroma, w, h, _, _, _, model, pos, _, _ = case
    rng = np.random.default_rng(5200 + index)
    W, H = CHROMA if chroma else LUMA
    if model == "trans":
        m = [ONE, 0, 0, ONE]
    elif model == "rotzoom":
        a, b = (int(v) for v in rng.integers(-3000, 3001, 2))
        m = [ONE + a, b, -b, ONE + a]
    elif model == "affine":
        m = [int(v) + d for v, d in zip(rng.integers(-4096, 4097, 4), (ONE, 0, 0, ONE))]
    else:
        m = list(LIMIT_MODELS[int(model[5:])])
    p_col, p_row = (16, 8) if pos == "pcol" else (0, 0)
    tx, ty = (W - w) // 2, (H - h) // 2
    tx = {"left": -6, "right": W - w + 5, "out_tl": -300, "out_bl": -300, "out_tr": W + 300, "out_br": W + 300, "pcol": -10}.get(pos, tx)
    ty = {"top": -6, "bottom": H - h + 5, "out_tl": -300, "out_tr": -300, "out_bl": H + 300, "out_br": H + 300, "pcol": -4}.get(pos, ty)
    frac = [int(v) for v in rng.integers(1, ONE, 2)]
    return [((tx << chroma) << 16) + frac[0], ((ty << chroma) << 16) + frac[1]] + m, p_col, p_row


def block_windows(case, index):
    """(x0, x1, y0, y1) of the 15 x 15 source window of every 8 x 8 block of a case, before clamping."""
    _, chroma, w, h = case[:4]
    mat, p_col, p_row = case_model(case, index)
    out = []
    for i in range(p_row, p_row + h, 8):
        for j in range(p_col, p_col + w, 8):
            sx, sy = (j + 4) << chroma, (i + 4) << chroma
            ix4 = ((mat[2] * sx + mat[3] * sy + mat[0]) >> chroma) >> 16
            iy4 = ((mat[4] * sx + mat[5] * sy + mat[1]) >> chroma) >> 16
            out.append((ix4 - 7, ix4 + 7, iy4 - 7, iy4 + 7))
    return out


class WarpInputs:
    """Host buffers of one prediction case: the reference plane, dst and cbuf as blend_cases.Buf (guard rows, strides wider than
    the block, some at odd sample offsets), the model and its shear."""

    def __init__(self, case, index):
        name, chroma, w, h, f, compound, wt, model, pos, checker, lay = case
        rng = np.random.default_rng(5600 + index)
        self.case, (self.bd, self.is16) = case, FORMATS[f]
        self.r0, self.r1 = rounds(self.bd, compound)
        self.fwd, self.bck = WEIGHTS[wt] if compound == 3 else (0, 0)
        px = np.uint16 if self.is16 else np.uint8
        W, H = CHROMA if chroma else LUMA
        top = (1 << self.bd) - 1
        if checker:
            yy, xx = np.mgrid[0:H, 0:W]
            plane = np.where((xx // int(rng.integers(1, 4)) + yy // int(rng.integers(1, 4))) & 1, top, 0)
        else:
            plane = rng.integers(0, top + 1, (H, W))
        (e0, o0), (e1, o1), (e2, o2) = (B.LAYOUTS[(lay + j) % len(B.LAYOUTS)] for j in range(3))
        self.ref = B.Buf(plane.astype(px), e0, o0)
        self.dst = B.Buf(np.full((h, w), B.FILL * 0x0101 if self.is16 else B.FILL, px), e1, o1)
        # compound 2 / 3 read what a first prediction left; compound 0 / 1 find fill bytes
        first = B.conv_buf_block(rng, w, h, self.bd, False) if compound >= 2 else np.full((h, w), B.FILL * 0x0101, np.uint16)
        self.cbuf = B.Buf(first, e2, o2)
        self.mat, self.p_col, self.p_row = case_model(case, index)
        ok, self.shear = lib_shear(self.mat)
        assert ok == 1, (name, "the model must pass the shear check")

    def desc(self, ptrs=None):
        """abi.WarpDesc over the host buffers, or over device copies of them ({id(Buf): device pointer})."""
        _, chroma, w, h, _, compound = self.case[:6]
        p = (lambda b: ptrs[id(b)] + b.byte_offset) if ptrs is not None else (lambda b: b.ptr)
        return abi.WarpDesc(p(self.ref), p(self.dst), p(self.cbuf), self.ref.stride, self.dst.stride, self.cbuf.stride, self.ref.w, self.ref.h,
                            self.p_col, self.p_row, w, h, (C.c_int32 * 6)(*self.mat), *self.shear, chroma, chroma, self.r0, self.r1,
                            self.bd, self.is16, compound, self.fwd, self.bck)

    def buffers(self):
        return [self.ref, self.dst, self.cbuf]

    @property
    def out(self):
        """The buffer the case writes: cbuf of a first compound prediction, dst otherwise."""
        return self.cbuf if self.case[5] == 1 else self.dst


class RefWarp:
    """The reference's warp filters on host buffers."""

    def __init__(self, ref):
        V, i, i16 = C.c_void_p, C.c_int, C.c_int16
        self.ref = ref
        self.lb = B._fn(ref, "svt_av1_warp_affine_c", None, V, V, i, i, i, V, i, i, i, i, i, i, i, V, i16, i16, i16, i16)
        self.hb = B._fn(ref, "svt_aom_dec_svt_av1_highbd_warp_affine_c", None, V, V, i, i, i, V, i, i, i, i, i, i, i, i, V, i16, i16, i16, i16)

    def warp(self, mat, shear, plane, pred_ptr, pred_stride, p_col, p_row, w, h, ss, bd, is16, cp):
        """plane: a blend_cases.Buf"""
        m = (C.c_int32 * 6)(*mat)
        head = (C.addressof(m), plane.ptr, plane.w, plane.h, plane.stride, pred_ptr, p_col, p_row, w, h, pred_stride, ss, ss)
        self.hb(*head, bd, C.addressof(cp), *shear) if is16 else self.lb(*head, C.addressof(cp), *shear)

    def run(self, inp):
        _, chroma, w, h, _, compound = inp.case[:6]
        ok, shear = ref_shear(self.ref, inp.mat)
        assert ok == 1 and shear == inp.shear, (inp.case[0], "shear")
        cp = abi.ConvolveParams(do_average=int(compound >= 2), dst=inp.cbuf.ptr if compound else None, dst_stride=inp.cbuf.stride, round_0=inp.r0,
                                round_1=inp.r1, is_compound=int(compound > 0), use_jnt_comp_avg=int(compound == 3), fwd_offset=inp.fwd,
                                bck_offset=inp.bck)
        self.warp(inp.mat, shear, inp.ref, inp.dst.ptr, inp.dst.stride, inp.p_col, inp.p_row, w, h, chroma, inp.bd, inp.is16, cp)


def record(key, block):
    block = np.ascontiguousarray(block)
    return {key + "_sha256": np.array(B.digest(block))} if block.size > FULL_LIMIT else {key: block.copy()}


def warp_record(inp):
    return record(f"warp_{inp.case[0]}", inp.out.view)


# ---- interplay with svt_hip_convolve_batch and svt_hip_blend_batch --------------------------------------------------------------
# (name, kind, w, h, bit depth, is_16bit): "warp_conv": warp compound 1 then convolve compound 2; "conv_warp": the reverse;
# "warp_warp_wedge": two warp compound 1 blocks blended by SVT_HIP_BLEND_D16 under a wedge of the blend fixture
INTER_CASES = [(f"{kind}_bd{bd}", kind, 16, 16, bd, is16) for bd, is16 in ((8, 0), (10, 1)) for kind in ("warp_conv", "conv_warp", "warp_warp_wedge")]
INTER_WEDGE = 2 * 5 + 1      # mask index 5, sign 1 of the 16 x 16 wedges
INTER_POS = (24, 16)         # the block's position in the luma plane


class InterInputs:
    """Two 64 x 48 reference planes (contiguous), two warp models and one sub-pel phase pair."""

    def __init__(self, case, index):
        name, kind, w, h, bd, is16 = case
        rng = np.random.default_rng(6100 + index)
        px = np.uint16 if is16 else np.uint8
        self.case = case
        self.planes = [B.Buf(rng.integers(0, 1 << bd, (LUMA[1], LUMA[0])).astype(px)) for _ in range(2)]
        self.mats = [[int(rng.integers(-2 * ONE, 2 * ONE)), int(rng.integers(-2 * ONE, 2 * ONE))] +
                     [int(v) + d for v, d in zip(rng.integers(-3000, 3001, 4), (ONE, 0, 0, ONE))] for _ in range(2)]
        self.shears = [lib_shear(m)[1] for m in self.mats]
        self.phase = (int(rng.integers(1, 16)), int(rng.integers(1, 16)))
        self.r0, self.r1 = K.conv_rounds_compound(bd)

    def conv_src_offset(self, plane):
        """Sample offset of the block's (0, 0) in a plane, for the interpolation."""
        return INTER_POS[1] * plane.stride + INTER_POS[0]


class RefInter:
    def __init__(self, ref, wedges):
        V, i, i32, u32 = C.c_void_p, C.c_int, C.c_int32, C.c_uint32
        self.warp, self.wedges = RefWarp(ref), wedges
        self.jnt8 = B._fn(ref, "svt_av1_jnt_convolve_2d_c", None, V, i32, V, i32, i32, i32, V, V, i32, i32, V)
        self.jnt16 = B._fn(ref, "svt_av1_highbd_jnt_convolve_2d_c", None, V, i32, V, i32, i32, i32, V, V, i32, i32, V, i32)
        self.d16_lb = B._fn(ref, "svt_aom_lowbd_blend_a64_d16_mask_c", None, V, u32, V, u32, V, u32, V, u32, i, i, i, i, V)
        self.d16_hb = B._fn(ref, "svt_aom_highbd_blend_a64_d16_mask_c", None, V, u32, V, u32, V, u32, V, u32, i, i, i, i, V, i)
        self.tab = K.kernel_table("sub_pel_filters_8")

    def run(self, inp):
        name, kind, w, h, bd, is16 = inp.case
        px = np.uint16 if is16 else np.uint8
        dst, cb = np.zeros((h, w), px), [np.zeros((h, w), np.uint16) for _ in range(2)]

        def warp(j, cbuf, average):
            cp = abi.ConvolveParams(do_average=average, dst=cbuf.ctypes.data, dst_stride=w, round_0=inp.r0, round_1=inp.r1, is_compound=1)
            self.warp.warp(inp.mats[j], inp.shears[j], inp.planes[j], dst.ctypes.data, w, INTER_POS[0], INTER_POS[1], w, h, 0, bd, is16, cp)

        def conv(j, cbuf, average):
            fp = K.InterpFilterParams(self.tab[0].ctypes.data, 8, 16, 0)
            cp = abi.ConvolveParams(do_average=average, dst=cbuf.ctypes.data, dst_stride=w, round_0=inp.r0, round_1=inp.r1, is_compound=1)
            p = inp.planes[j]
            args = [p.ptr + inp.conv_src_offset(p) * p.a.itemsize, p.stride, dst.ctypes.data, w, w, h, C.addressof(fp), C.addressof(fp),
                    inp.phase[0], inp.phase[1], C.addressof(cp)]
            self.jnt16(*args, bd) if is16 else self.jnt8(*args)

        if kind == "warp_conv":
            warp(0, cb[0], 0), conv(1, cb[0], 1)
        elif kind == "conv_warp":
            conv(0, cb[0], 0), warp(1, cb[0], 1)
        else:
            warp(0, cb[0], 0), warp(1, cb[1], 0)
            cp = abi.ConvolveParams(round_0=inp.r0, round_1=inp.r1, is_compound=1)
            mask = np.ascontiguousarray(self.wedges["wedge_16x16"][INTER_WEDGE])
            io = (dst.ctypes.data, w, cb[0].ctypes.data, w, cb[1].ctypes.data, w, mask.ctypes.data, w, w, h, 0, 0, C.addressof(cp))
            self.d16_hb(*io, bd) if is16 else self.d16_lb(*io)
        return dst


# ---- pictures for the global-motion error and the refinement --------------------------------------------------------------------
def texture(rng, w, h):
    """An 8-bit picture with structure at several scales, integer arithmetic only."""
    coarse = np.kron(rng.integers(0, 256, (h // 8 + 2, w // 8 + 2)), np.ones((8, 8), np.int64))[:h + 4, :w + 4]
    fine = np.kron(rng.integers(0, 256, (h // 2 + 3, w // 2 + 3)), np.ones((2, 2), np.int64))[:h + 4, :w + 4]
    a = 3 * coarse + fine
    for _ in range(2):   # 3 x 3 box blur
        a = sum(a[dy:a.shape[0] - 2 + dy, dx:a.shape[1] - 2 + dx] for dy in range(3) for dx in range(3)) // 9
    return np.clip((a[:h, :w] + 2) // 4, 0, 255).astype(np.uint8)


def warp_picture(ref, mat, w, h):
    """`ref` sampled bilinearly (8-bit fractions, clamped coordinates) at the model's positions: a w x h picture."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    sx, sy = mat[2] * xx + mat[3] * yy + mat[0], mat[4] * xx + mat[5] * yy + mat[1]
    ix, iy, fx, fy = sx >> 16, sy >> 16, (sx & 65535) >> 8, (sy & 65535) >> 8
    r = ref.astype(np.int64)
    at = lambda y, x: r[np.clip(y, 0, r.shape[0] - 1), np.clip(x, 0, r.shape[1] - 1)]   # noqa: E731
    v = (at(iy, ix) * (256 - fx) + at(iy, ix + 1) * fx) * (256 - fy) + (at(iy + 1, ix) * (256 - fx) + at(iy + 1, ix + 1) * fx) * fy
    return ((v + 32768) >> 16).astype(np.uint8)


def picture_pair(seed, w, h, mat, noise=3):
    """(reference, current) as blend_cases.Buf with strides wider than the picture: current = reference warped by mat + noise."""
    rng = np.random.default_rng(seed)
    ref = texture(rng, w, h)
    cur = np.clip(warp_picture(ref, mat, w, h).astype(np.int64) + rng.integers(-noise, noise + 1, (h, w)), 0, 255).astype(np.uint8)
    return B.Buf(ref, 5, 3), B.Buf(cur, 8, 0)


def error_job(ref, cur, chess, filter_ptr, ptrs=None):
    """abi.WarpErrorJob over host or device copies of the pair; the workspace is the caller's."""
    p = (lambda b: ptrs[id(b)] + b.byte_offset) if ptrs is not None else (lambda b: b.ptr)
    return abi.WarpErrorJob(p(ref), p(cur), filter_ptr, None, 0, ref.stride, ref.w, ref.h, cur.stride, cur.w, cur.h, chess)


ERROR_PICTURES = ((104, 88), (32, 32), (24, 16), (96, 64))
ERROR_TRUE = [3 * ONE + 21000, -2 * ONE + 40000, ONE + 600, -900, 700, ONE - 400]
# valid models (the first is the one that made the picture) and two whose shear is refused
ERROR_MODELS = [ERROR_TRUE, [0, 0, ONE, 0, 0, ONE], [3 * ONE, -2 * ONE, ONE, 0, 0, ONE], [2 * ONE + 5000, -ONE, ONE + 500, -800, 800, ONE + 500],
                [4 * ONE, -3 * ONE + 9000, ONE - 2000, 1500, -1200, ONE + 2500], [3 * ONE, -2 * ONE] + list(LIMIT_MODELS[2]),
                [-40 * ONE, 30 * ONE, ONE, 9344, 0, ONE]]
ERROR_BAD_MODELS = [[0, 0, ONE + 20000, 0, 0, ONE], [ONE, 0, ONE, 0, 9000, ONE + 9000]]
THRESHOLDS = ("max", "E", "E-1", "E/2", "E/10", "0")


def error_pair(k):
    w, h = ERROR_PICTURES[k]
    return picture_pair(7300 + k, w, h, ERROR_TRUE)


def error_candidates(best_errors):
    """The candidate array of one picture: every valid model under every threshold, then the refused ones."""
    models = [m for m in ERROR_MODELS for _ in THRESHOLDS] + ERROR_BAD_MODELS
    cand = np.zeros(len(models), np.dtype(abi.WARP_CANDIDATE_DTYPE))
    for c, m, e in zip(cand, models, best_errors):
        c["mat"], (c["alpha"], c["beta"], c["gamma"], c["delta"]), c["best_error"] = m, lib_shear(m)[1], e
    return cand


def threshold(kind, e):
    return {"max": INT64_MAX, "E": e, "E-1": e - 1, "E/2": e // 2, "E/10": e // 10, "0": 0}[kind]


class RefError:
    def __init__(self, ref):
        V, i, u8, i64 = C.c_void_p, C.c_int, C.c_uint8, C.c_int64
        self.ref, self.warp = ref, RefWarp(ref)
        self.warp_error = B._fn(ref, "svt_av1_warp_error", i64, V, V, i, i, i, V, i, i, i, i, i, i, i, u8, i64)
        self.refine = B._fn(ref, "svt_av1_refine_integerized_param", i64, V, i, V, i, i, i, V, i, i, i, i, u8, i64)

    def error(self, mat, wmtype, ref, cur, chess, best):
        """svt_av1_warp_error over the whole current picture (it computes the shear itself)."""
        wm = WarpedMotionParams(wmtype, (C.c_int32 * 8)(*mat[:6], 0, 0))
        return int(self.warp_error(C.addressof(wm), ref.ptr, ref.w, ref.h, ref.stride, cur.ptr, 0, 0, cur.w, cur.h, cur.stride, 0, 0, chess, best))

    def block_sads(self, mat, ref, cur):
        """[rows][cols] SADs of the 32 x 32 error blocks, each warped by svt_av1_warp_affine_c as warp_error() calls it."""
        shear = ref_shear(self.ref, mat)[1]
        cp = abi.ConvolveParams(round_0=3, round_1=11)
        rows, cols = -(-cur.h // 32), -(-cur.w // 32)
        out, tmp = np.zeros((rows, cols), np.int64), np.zeros((32, 32), np.uint8)
        for r in range(rows):
            for c in range(cols):
                w, h = min(32, cur.w - 32 * c), min(32, cur.h - 32 * r)
                self.warp.warp(mat, shear, ref, tmp.ctypes.data, 32, 32 * c, 32 * r, w, h, 0, 8, 0, cp)
                out[r, c] = np.abs(tmp[:h, :w].astype(np.int64) - cur.view[32 * r:32 * r + h, 32 * c:32 * c + w]).sum()
        return out

    def walk(self, sads, chess, best):
        """(error, blocks summed) of warp_error()'s raster walk over the block SADs."""
        total = n = 0
        for r in range(sads.shape[0]):
            for c in range((0 if r & 1 else 1) if chess else 0, sads.shape[1], 2 if chess else 1):
                total, n = total + int(sads[r, c]), n + 1
                if total > best:
                    return total, n
        return (2 * total if chess else total), n

    def picture(self, k, chess):
        """(best_error of every candidate, results) of error picture k: the errors are svt_av1_warp_error's own, blocks_summed
        comes from the walk over the block SADs, which is checked to reproduce every one of those errors."""
        ref, cur = error_pair(k)
        best, res = [], []
        for m in ERROR_MODELS:
            full = self.error(m, AFFINE, ref, cur, chess, INT64_MAX)
            sads = self.block_sads(m, ref, cur)
            for kind in THRESHOLDS:
                t = threshold(kind, full)
                e = self.error(m, AFFINE, ref, cur, chess, t)
                assert self.walk(sads, chess, t)[0] == e, (k, chess, kind)
                best.append(t), res.append((e, self.walk(sads, chess, t)[1], 0, (0, 0, 0)))
        for m in ERROR_BAD_MODELS:
            assert ref_shear(self.ref, m)[0] == 0 and self.error(m, AFFINE, ref, cur, chess, INT64_MAX) == 1
            best.append(INT64_MAX), res.append((0, 0, abi.WARP_ERROR_BAD_SHEAR, (0, 0, 0)))
        return np.array(best, np.int64), np.array(res, np.dtype(abi.WARP_ERROR_RESULT_DTYPE))


# ---- refinement -----------------------------------------------------------------------------------------------------------------
REFINE_SIZE = (104, 88)
REFINE_TRUE = [[2 * ONE + 30000, -ONE + 12000, ONE + 700, -1100, 1100, ONE + 700], [-3 * ONE + 5000, 2 * ONE + 50000, ONE - 900, 600, -1300, ONE + 1200],
               [ONE + 44000, 3 * ONE + 9000, ONE + 300, 1400, -1400, ONE + 300]]
# (name, pair, wmtype, chess_refn, best_frame_error, perturbation of wmmat[0 .. 5])
REFINE_CASES = [("rotzoom_pair0", 0, ROTZOOM, 0, INT64_MAX, (30000, -25000, 260, -180, 0, 0)),
                ("affine_pair1_chess", 1, AFFINE, 1, INT64_MAX, (-20000, 33000, -150, 220, 190, -240)),
                ("rotzoom_pair2_chess", 2, ROTZOOM, 1, INT64_MAX, (-36000, 18000, -200, 150, 0, 0)),
                ("affine_pair0", 0, AFFINE, 0, 400000, (22000, 27000, 170, -130, -210, 160)),
                ("affine_pair2", 2, AFFINE, 0, INT64_MAX, (15000, -30000, 240, 110, -90, -260))]
N_REFINEMENTS = 5


def refine_pair(k):
    return picture_pair(7700 + k, *REFINE_SIZE, REFINE_TRUE[k], noise=2)


def refine_start(case):
    _, pair, wmtype, _, _, delta = case
    m = [a + b for a, b in zip(REFINE_TRUE[pair], delta)]
    if wmtype == ROTZOOM:
        m[4], m[5] = -m[3], m[2]
    return m + [0, 0]


def ref_refine(orc, case):
    """[wmmat[0 .. 5], wmtype, error] of svt_av1_refine_integerized_param, as one int64 array."""
    _, pair, wmtype, chess, best, _ = case
    ref, cur = refine_pair(pair)
    wm = WarpedMotionParams(wmtype, (C.c_int32 * 8)(*refine_start(case)))
    err = orc.refine(C.addressof(wm), wmtype, ref.ptr, ref.w, ref.h, ref.stride, cur.ptr, cur.w, cur.h, cur.stride, N_REFINEMENTS, chess, best)
    return np.array(list(wm.wmmat)[:6] + [wm.wmtype, int(err)], np.int64)


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def golden_entries(ref, log=None):
    """Every entry of the fixture, computed by the reference."""
    rec = {"warped_filter": ref_filter(ref)}
    orc = RefWarp(ref)
    for i, case in enumerate(WARP_CASES):
        inp = WarpInputs(case, i)
        orc.run(inp)
        rec.update(warp_record(inp))
    wedges = np.load(B.GOLD)
    inter = RefInter(ref, wedges)
    for i, case in enumerate(INTER_CASES):
        rec[f"inter_{case[0]}"] = inter.run(InterInputs(case, i))
    err = RefError(ref)
    for k in range(len(ERROR_PICTURES)):
        for chess in (0, 1):
            rec[f"error_{k}_{chess}_best"], rec[f"error_{k}_{chess}_results"] = err.picture(k, chess)
    for case in REFINE_CASES:
        rec[f"refine_{case[0]}"] = ref_refine(err, case)
        if log:
            log(f"refine {case[0]}: {refine_start(case)[:6]} -> {rec[f'refine_{case[0]}'].tolist()}")
    return rec


def main():
    import pyorc
    rec = golden_entries(pyorc.ref(), print)
    np.savez_compressed(GOLD, **rec)
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes,", len(rec), "entries")


if __name__ == "__main__":  # PYTHONPATH=oracle:svt-av1-mod-by-patman_amd python tests/warp_cases.py
    main()
