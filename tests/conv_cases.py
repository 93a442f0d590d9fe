"""Shared helpers for the inter-prediction interpolation tests (test infrastructure)."""
import collections
import ctypes as C

import numpy as np

V = C.c_void_p


class InterpFilterParams(C.Structure):     # definitions.h:750-755 (== SvtHipInterpFilterParams)
    _fields_ = [("filter_ptr", C.c_void_p), ("taps", C.c_uint16), ("subpel_shifts", C.c_uint16), ("interp_filter", C.c_int32)]


# The AV1 interpolation kernels (inter_prediction.c:223-300 holds the same tables): 16 phases x 8 taps.  Tests read the
# reference's own copies when oracle/_ref is present and check this restatement against them (test_convolve_oracle.py).
REGULAR = [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -6, 126, 8, -2, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0], [0, 2, -12, 116, 28, -8, 2, 0],
           [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -14, 102, 48, -12, 2, 0], [0, 2, -16, 94, 58, -12, 2, 0], [0, 2, -14, 84, 66, -12, 2, 0],
           [0, 2, -14, 76, 76, -14, 2, 0], [0, 2, -12, 66, 84, -14, 2, 0], [0, 2, -12, 58, 94, -16, 2, 0], [0, 2, -12, 48, 102, -14, 2, 0],
           [0, 2, -10, 38, 110, -14, 2, 0], [0, 2, -8, 28, 116, -12, 2, 0], [0, 0, -4, 18, 122, -10, 2, 0], [0, 0, -2, 8, 126, -6, 2, 0]]
SHARP = [[0, 0, 0, 128, 0, 0, 0, 0], [-2, 2, -6, 126, 8, -2, 2, 0], [-2, 6, -12, 124, 16, -6, 4, -2], [-2, 8, -18, 120, 26, -10, 6, -2],
         [-4, 10, -22, 116, 38, -14, 6, -2], [-4, 10, -22, 108, 48, -18, 8, -2], [-4, 10, -24, 100, 60, -20, 8, -2],
         [-4, 10, -24, 90, 70, -22, 10, -2], [-4, 12, -24, 80, 80, -24, 12, -4], [-2, 10, -22, 70, 90, -24, 10, -4],
         [-2, 8, -20, 60, 100, -24, 10, -4], [-2, 8, -18, 48, 108, -22, 10, -4], [-2, 6, -14, 38, 116, -22, 10, -4],
         [-2, 6, -10, 26, 120, -18, 8, -2], [-2, 4, -6, 16, 124, -12, 6, -2], [0, 2, -2, 8, 126, -6, 2, -2]]
BILINEAR = [[0, 0, 0, 128 - 8 * i, 8 * i, 0, 0, 0] for i in range(16)]
SMOOTH = [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, 28, 62, 34, 2, 0, 0], [0, 0, 26, 62, 36, 4, 0, 0], [0, 0, 22, 62, 40, 4, 0, 0],
          [0, 0, 20, 60, 42, 6, 0, 0], [0, 0, 18, 58, 44, 8, 0, 0], [0, 0, 16, 56, 46, 10, 0, 0], [0, -2, 16, 54, 48, 12, 0, 0],
          [0, -2, 14, 52, 52, 14, -2, 0], [0, 0, 12, 48, 54, 16, -2, 0], [0, 0, 10, 46, 56, 16, 0, 0], [0, 0, 8, 44, 58, 18, 0, 0],
          [0, 0, 6, 42, 60, 20, 0, 0], [0, 0, 4, 40, 62, 22, 0, 0], [0, 0, 4, 36, 62, 26, 0, 0], [0, 0, 2, 34, 62, 28, 2, 0]]
# the kernels the reference uses in a direction where the block is <= 4 samples (av1_get_4tap_interp_filter_params)
REGULAR4 = [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, -4, 126, 8, -2, 0, 0], [0, 0, -8, 122, 18, -4, 0, 0], [0, 0, -10, 116, 28, -6, 0, 0],
            [0, 0, -12, 110, 38, -8, 0, 0], [0, 0, -12, 102, 48, -10, 0, 0], [0, 0, -14, 94, 58, -10, 0, 0], [0, 0, -12, 84, 66, -10, 0, 0],
            [0, 0, -12, 76, 76, -12, 0, 0], [0, 0, -10, 66, 84, -12, 0, 0], [0, 0, -10, 58, 94, -14, 0, 0], [0, 0, -10, 48, 102, -12, 0, 0],
            [0, 0, -8, 38, 110, -12, 0, 0], [0, 0, -6, 28, 116, -10, 0, 0], [0, 0, -4, 18, 122, -8, 0, 0], [0, 0, -2, 8, 126, -4, 0, 0]]
SMOOTH4 = [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, 30, 62, 34, 2, 0, 0], [0, 0, 26, 62, 36, 4, 0, 0], [0, 0, 22, 62, 40, 4, 0, 0],
           [0, 0, 20, 60, 42, 6, 0, 0], [0, 0, 18, 58, 44, 8, 0, 0], [0, 0, 16, 56, 46, 10, 0, 0], [0, 0, 14, 54, 48, 12, 0, 0],
           [0, 0, 12, 52, 52, 12, 0, 0], [0, 0, 12, 48, 54, 14, 0, 0], [0, 0, 10, 46, 56, 16, 0, 0], [0, 0, 8, 44, 58, 18, 0, 0],
           [0, 0, 6, 42, 60, 20, 0, 0], [0, 0, 4, 40, 62, 22, 0, 0], [0, 0, 4, 36, 62, 26, 0, 0], [0, 0, 2, 34, 62, 30, 0, 0]]
# the first three keep their places: the first-pass tests and the committed fixtures index this dict by position
TABLES = {"sub_pel_filters_8": REGULAR, "sub_pel_filters_8sharp": SHARP, "bilinear_filters": BILINEAR,
          "sub_pel_filters_8smooth": SMOOTH, "sub_pel_filters_4": REGULAR4, "sub_pel_filters_4smooth": SMOOTH4}


def kernel_table(name):
    """256-byte aligned int16 [16][8] copy of a kernel table (what InterpFilterParams.filter_ptr points at)."""
    buf = np.zeros(16 * 8 + 128, np.int16)
    off = (-buf.ctypes.data % 256) // 2
    t = buf[off:off + 128].reshape(16, 8)
    t[:] = np.array(TABLES[name], np.int16)
    return t, buf


def conv_rounds(bd):
    """get_conv_params (convolve.h:40-68), non-compound"""
    r0, r1 = 3, 11
    rng = bd + 7 - r0 + 2
    if rng > 16:
        r0, r1 = r0 + rng - 16, r1 - (rng - 16)
    return r0, r1


def ref_plane(rng, w, h, bd, is16, kind):
    B = 8
    dt = np.uint16 if is16 else np.uint8
    if kind == 2:
        a = rng.integers(0, 1 << bd, size=(h + 2 * B, w + 2 * B))
    elif kind == 1:
        a = np.where(rng.random((h + 2 * B, w + 2 * B)) < 0.5, 0, (1 << bd) - 1)
    else:
        yy, xx = np.mgrid[0:h + 2 * B, 0:w + 2 * B]
        a = (1 << bd) * (0.5 + 0.4 * np.sin(xx / 5.0) * np.cos(yy / 7.0)) + rng.integers(-4, 5, size=xx.shape)
    a = np.clip(np.rint(a), 0, (1 << bd) - 1).astype(dt)
    return a, a.ctypes.data + (B * a.shape[1] + B) * a.itemsize


SIZES = [(4, 4), (8, 8), (16, 8), (8, 16), (32, 32), (64, 64), (128, 64), (64, 128), (128, 128), (4, 16), (16, 64)]


def conv_rounds_compound(bd):
    """get_conv_params_no_round with is_compound = 1 (convolve.h:39-63)"""
    r0, r1 = 3, 7
    rng = bd + 7 - r0 + 2
    if rng > 16:
        r0 += rng - 16
    return r0, r1


JNT_MODES = ("2d", "x", "y", "2d_copy")
# quant_dist_lookup_table weights (fwd, bck) the reference uses for distance-weighted compounds (inter_prediction.c: the
# pairs sum to 16)
DIST_WEIGHTS = [(9, 7), (11, 5), (12, 4), (13, 3), (7, 9), (5, 11), (4, 12), (3, 13), (8, 8)]


def jnt_cases(bd, is16, n=40, seed=0):
    """(w, h, mode, table index, sx, sy, plane0, at0, plane1, at1, averaging mode 2|3, fwd, bck)"""
    rng = np.random.default_rng(7000 + bd + seed)
    for trial in range(n):
        w, h = SIZES[trial % len(SIZES)]
        ti = trial % 3
        sx, sy = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        mode = trial % 4
        p0, a0 = ref_plane(rng, w, h, bd, is16, (0, 2, 1)[trial % 3])
        p1, a1 = ref_plane(rng, w, h, bd, is16, (2, 0, 1)[trial % 3])
        avg = 3 if trial % 2 else 2
        fwd, bck = DIST_WEIGHTS[trial % len(DIST_WEIGHTS)]
        yield w, h, mode, ti, sx, sy, p0, a0, p1, a1, avg, fwd, bck


# ---- extended cases: every table, different tables in x and y, every block shape, short kernels, adversarial planes ----------
MODES = ("2d", "x", "y", "2d_copy")      # index = ExtCase.mode; the sr leaves are named <mode>_sr
AV1_SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64),
             (64, 128), (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]      # BlockSize, w x h
CHROMA_SIZES = [(2, 2), (2, 4), (4, 2), (2, 8), (8, 2), (2, 16), (16, 2)]       # 4:2:0 chroma of the sub-8x8 inter blocks
ODD_SIZES = [(6, 10), (12, 12), (24, 40), (66, 70), (96, 127), (127, 3), (1, 1)]
TABLES4 = ("sub_pel_filters_4", "sub_pel_filters_4smooth")
KIND_SMOOTH, KIND_BINARY, KIND_UNIFORM, KIND_ADV, KIND_ADV_INV = range(5)


class ExtCase(collections.namedtuple("ExtCase", "w h mode tx ty sx sy taps kind bd")):
    """One block: w x h, mode (index into MODES), the names of the x and y tables, the x and y phases, taps = (taps of the x
    InterpFilterParams, taps of the y one), the plane kind (KIND_*) and the bit depth."""
    __slots__ = ()

    @property
    def is16(self):
        return int(self.bd > 8)

    @property
    def use(self):
        """(taps_x, taps_y) as the Tier B descriptor and the oracle take them: 0 in a direction the mode does not filter"""
        return (self.taps[0] if self.mode in (0, 1) else 0), (self.taps[1] if self.mode in (0, 2) else 0)


def min_taps(name):
    """the shortest even kernel length that holds every non-zero tap of a table, centred as the reference centres a kernel"""
    t = np.array(TABLES[name])
    return next(n for n in (2, 4, 6, 8) if not t[:, :(8 - n) // 2].any() and not t[:, 8 - (8 - n) // 2:].any())


_narrow = {}


def narrow_table(name, taps):
    """256-byte aligned int16 [16][taps]: a table without its (8 - taps) / 2 outer columns on either side, which must all be zero.
    With an InterpFilterParams of that `taps` this is the same filter, as the reference's generic C functions read it."""
    if (name, taps) not in _narrow:
        assert taps in (2, 4, 6, 8) and taps >= min_taps(name), (name, taps)
        buf = np.zeros(16 * taps + 128, np.int16)
        off = (-buf.ctypes.data % 256) // 2
        t = buf[off:off + 16 * taps].reshape(16, taps)
        t[:] = np.array(TABLES[name], np.int16)[:, (8 - taps) // 2:8 - (8 - taps) // 2]
        _narrow[(name, taps)] = (t, buf)
    return _narrow[(name, taps)][0]


def has_negative_tap(name, phase):
    return min(TABLES[name][phase]) < 0


def adv_pattern(name, phase, n):
    """+1 / -1 for the n + 16 samples of one direction of a plane with 8 samples of border: +1 where the tap that multiplies the
    sample in the output at block offset 0 (and 8, 16 ...: the pattern has period 8) is positive, -1 where it is negative or zero."""
    k = np.array(TABLES[name][phase])
    return np.where(k[(np.arange(n + 16) - 8 + 3) % 8] > 0, 1, -1)


def ext_plane(rng, c, second=False):
    """(plane, address of the block's first sample) of a case; `second`: the other reference of a compound (another draw for the
    random kinds, the same plane for the adversarial ones: both predictions sit at the same extreme)."""
    if c.kind < KIND_ADV:
        return ref_plane(rng, c.w, c.h, c.bd, c.is16, KIND_UNIFORM if second else c.kind)
    sx = adv_pattern(c.tx, c.sx, c.w) if c.mode != 2 else np.ones(c.w + 16, int)
    sy = adv_pattern(c.ty, c.sy, c.h) if c.mode != 1 else np.ones(c.h + 16, int)
    hi = (np.outer(sy, sx) > 0) != (c.kind == KIND_ADV_INV)
    a = np.where(hi, (1 << c.bd) - 1, 0).astype(np.uint16 if c.is16 else np.uint8)
    return a, a.ctypes.data + (8 * a.shape[1] + 8) * a.itemsize


def adv_kernels():
    """every (table, phase) whose kernel has a negative tap"""
    return [(n, p) for n in TABLES for p in range(16) if has_negative_tap(n, p)]


def adv_cases(bd):
    """Section "adversarial magnitudes": per kernel with a negative tap, an 8 x 8 block of a plane that puts the maximum sample under
    the positive taps and 0 under the others, and the inverse plane, in every mode.  The 2-D mode pairs the kernel (in x) with the
    next one of the list (in y) and uses the outer product of the two sign patterns."""
    ks = adv_kernels()
    for i, (n, p) in enumerate(ks):
        n2, p2 = ks[(i + 7) % len(ks)]
        for kind in (KIND_ADV, KIND_ADV_INV):
            yield ExtCase(8, 8, 0, n, n2, p, p2, (8, 8), kind, bd)
            yield ExtCase(8, 8, 1, n, n2, p, p2, (8, 8), kind, bd)
            yield ExtCase(8, 8, 2, n2, n, p2, p, (8, 8), kind, bd)
            yield ExtCase(8, 8, 3, n, n2, p, p2, (8, 8), kind, bd)


def shape_cases(bd):
    """Every block shape in every mode.  The x and y tables differ in three cases of four; a direction of <= 4 samples takes a
    4-tap table, as in the reference; the InterpFilterParams' taps cycle through every length the table allows (so 2, 4, 6 and 8
    all occur, in both directions); phases are random, 0 included."""
    rng = np.random.default_rng(9100 + bd)
    names = list(TABLES)
    for i, (w, h) in enumerate(AV1_SIZES + CHROMA_SIZES + ODD_SIZES):
        for mode in range(4):
            j = i * 4 + mode
            tx = names[j % 6]
            ty = names[(j + (0 if j % 4 == 3 else 1 + (j // 4) % 5)) % 6]
            if w <= 4 and tx not in TABLES4:
                tx = TABLES4[j % 2]
            if h <= 4 and ty not in TABLES4:
                ty = TABLES4[(j // 2) % 2]
            ax, ay = [n for n in (8, 6, 4, 2) if n >= min_taps(tx)], [n for n in (8, 6, 4, 2) if n >= min_taps(ty)]
            taps = (ax[(j // 6) % len(ax)], ay[(j // 7) % len(ay)])
            yield ExtCase(w, h, mode, tx, ty, int(rng.integers(0, 16)), int(rng.integers(0, 16)), taps, (0, 2, 1)[j % 3], bd)
    for mode in range(3):       # the shortest kernels in every filtering mode
        yield ExtCase(12, 6, mode, "bilinear_filters", "bilinear_filters", 5, 11, (2, 2), KIND_UNIFORM, bd)
        yield ExtCase(6, 10, mode, "bilinear_filters", "sub_pel_filters_4", 9, 3, (2, 4), KIND_BINARY, bd)
        yield ExtCase(10, 6, mode, "sub_pel_filters_4smooth", "bilinear_filters", 15, 1, (4, 2), KIND_UNIFORM, bd)


def ext_cases(bd):
    yield from shape_cases(bd)
    yield from adv_cases(bd)


def ext_avgs(i, c):
    """(averaging mode 2|3, fwd, bck) a compound case is run with: both averages on the adversarial planes, one otherwise"""
    fwd, bck = DIST_WEIGHTS[i % len(DIST_WEIGHTS)]
    return [(2, fwd, bck), (3, fwd, bck)] if c.kind >= KIND_ADV else [(2 + i % 2, fwd, bck)]


def ext_golden():
    """The cases of tests/golden/convolve_ext.npz (written from the real reference functions by make_golden_convolve_ext.py):
    (case, plane0, plane1, fwd, bck, sr pixels, conv buffer after the first prediction, pixels of the plain average, pixels of the
    distance-weighted average); the planes have 8 samples of border."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convolve_ext.npz"))
    names = list(TABLES)
    for i in range(int(g["n"])):
        w, h, mode, txi, tyi, sx, sy, tapx, tapy, kind, bd, fwd, bck = (int(v) for v in g[f"c{i}_meta"])
        c = ExtCase(w, h, mode, names[txi], names[tyi], sx, sy, (tapx, tapy), kind, bd)
        yield (c, g[f"c{i}_p0"].copy(), g[f"c{i}_p1"].copy(), fwd, bck) + tuple(g[f"c{i}_{k}"] for k in ("sr", "first", "avg", "wtd"))


def at_block(plane):
    return plane.ctypes.data + (8 * plane.shape[1] + 8) * plane.itemsize
