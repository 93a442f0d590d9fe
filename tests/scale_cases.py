"""Cases of reference scaling (include/svt_hip_scale.h): svt_hip_resize_planes, svt_hip_superres_upscale_planes, svt_hip_convolve_scale_batch
and the three host helpers; deterministic input makers; a numpy restatement of the reference functions they stand for
(svt_av1_resize_plane_c, svt_av1_upscale_normative_rows, svt_av1_convolve_2d_scale_c and the highbd twins, svt_av1_setup_scale_factors_for_frame,
the scaled branch of compute_subpel_params, calculate_scaled_size_helper); and the calls into the reference's own functions
(oracle/_ref/libsvtref.so and tests/scale_pin_driver.c).  tests/golden/scale.npz (tests/golden/make_golden_scale.py) holds what the
reference gave for every case: the array, or for a large case the SHA-256 of its bytes, and the reference's filter banks."""
import ctypes as C
import hashlib
import os
import zlib
from collections import namedtuple

import numpy as np

import conv_cases
from svtav1_hip import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "scale.npz")
GOLD_MAX_BYTES = 256 * 1024
ARRAY_MAX_BYTES = 3000         # an expected output above this is kept as a digest
BAD_PARAMETER, NO_DEVICE = abi.SVT_HIP_ERR_BAD_PARAMETER, abi.SVT_HIP_ERR_NO_DEVICE      # SVT_HIP_SCALE_STATUS keeps the SvtHipStatus whole
STATUS_NAMES = ("svt_hip_resize_planes", "svt_hip_superres_upscale_planes", "svt_hip_convolve_scale_batch")
BANK_NAMES = (1000, 875, 750, 625, 500)


def dtype_of(is16):
    return np.uint16 if is16 else np.uint8


def seed_of(case):
    """The seed of a case's generated input: of its name, so that a case keeps its input when the lists change"""
    return zlib.crc32(case.name.encode()) & 0x7FFFFFFF


# ---- the fixture ----------------------------------------------------------------------------------------------------------------

_gold = None


def golden():
    global _gold
    if _gold is None:
        with np.load(GOLD) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


def banks():
    """The reference's five 64 x 8 banks, in the order of BANK_NAMES, and its two half filters (symeven, symodd)."""
    g = golden()
    return g["banks"].astype(np.int64), g["half"].astype(np.int64)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(store, key, a):
    """What the fixture keeps of an expected output"""
    if a.nbytes <= ARRAY_MAX_BYTES:
        store["out/" + key] = a
    else:
        store["sha/" + key] = np.frombuffer(bytes.fromhex(digest(a)), np.uint8)


def expected(key, restated):
    """The reference's output of a case: the fixture's array, or the restatement once its digest is the fixture's."""
    g = golden()
    if "out/" + key in g:
        return g["out/" + key]
    assert digest(restated()) == g["sha/" + key].tobytes().hex(), key
    return restated()


# ---- helpers -------------------------------------------------------------------------------------------------------------------

def scaled_size(dim, denom):
    """calculate_scaled_size_helper (super_res.c:22)"""
    if denom != 8 and denom <= 16:
        return max((dim * 8 + denom // 2) // denom & 0xFFFF, min(16, dim))
    return (3 + dim * 3) >> 2 if denom == 17 else dim


def cdiv(a, b):
    """C's integer division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def scale_factors(other_w, other_h, this_w, this_h):
    """svt_av1_setup_scale_factors_for_frame: (x_scale_fp, y_scale_fp, x_step_q4, y_step_q4), or None for an invalid pair"""
    if not (2 * this_w >= other_w and 2 * this_h >= other_h and this_w <= 16 * other_w and this_h <= 16 * other_h):
        return None
    xf, yf = ((other_w << 14) + this_w // 2) // this_w, ((other_h << 14) + this_h // 2) // this_h
    return xf, yf, (xf + 8) >> 4, (yf + 8) >> 4


def _scaled(val, scale_fp):
    t = val * scale_fp + (scale_fp - (1 << 14)) * 8
    return -((-t + 128) >> 8) if t < 0 else (t + 128) >> 8


def scaled_block_position(sf, pre_x, pre_y, mv_col, mv_row, ss_x, ss_y, frame_w, frame_h, sb_size):
    """The scaled branch of compute_subpel_params: (pos_x, pos_y, subpel_x, subpel_y, xs, ys)"""
    pos_y = _scaled(pre_y * 16 + mv_row * (1 << (1 - ss_y)), sf[1]) + 32
    pos_x = _scaled(pre_x * 16 + mv_col * (1 << (1 - ss_x)), sf[0]) + 32
    border = sb_size * 2 + 32
    pos_y = min(max(pos_y, -(((border >> ss_y) - 8) << 10)), ((frame_h >> ss_y) + 4) << 10)
    pos_x = min(max(pos_x, -(((border >> ss_x) - 8) << 10)), ((frame_w >> ss_x) + 4) << 10)
    return pos_x >> 10, pos_y >> 10, pos_x & 1023, pos_y & 1023, sf[2], sf[3]


POSITION_SIZES = [(1920, 1080, 9), (1920, 1080, 16), (640, 360, 13), (300, 200, 17)]        # reference w, h and the denominator of this frame


def position_probes():
    """(other_w, other_h, this_w, this_h, sb_size, pre_x, pre_y, mv_col, mv_row, ss_x, ss_y): blocks at the four picture corners with
    vectors that stay inside and that hit each side of the clamp, both super-block sizes, luma and chroma"""
    for ow, oh, denom in POSITION_SIZES:
        tw, th = scaled_size(ow, denom), scaled_size(oh, denom)
        for sb in (64, 128):
            for ss in (0, 1):
                for px, py in ((0, 0), ((tw - 8) >> ss, 0), (0, (th - 8) >> ss), ((tw - 8) >> ss, (th - 8) >> ss)):
                    for mvc, mvr in ((0, 0), (13, -7), (-3000, 5), (5, -3000), (3000, -11), (-11, 3000), (-16384, -16384), (16383, 16383)):
                        yield ow, oh, tw, th, sb, px, py, mvc, mvr, ss, ss


# ---- resize --------------------------------------------------------------------------------------------------------------------

ResizeCase = namedtuple("ResizeCase", "name sw sh dw dh bd is16 kind sstride dstride")


def _rz(name, sw, sh, dw, dh, bd=8, is16=None, kind="noise", pad=(5, 3)):
    return ResizeCase(name, sw, sh, dw, dh, bd, int(bd > 8) if is16 is None else is16, kind, sw + pad[0], dw + pad[1])


def _denom_cases():
    depth = {9: (8, "stripes"), 11: (10, "noise"), 13: (12, "stripes"), 15: (8, "noise"), 16: (10, "stripes"), 17: (12, "noise")}
    for d in range(9, 18):
        bd, kind = depth.get(d, (8, "noise"))
        yield _rz(f"d{d}_131x37_{bd}bit", 131, 37, scaled_size(131, d), scaled_size(37, d), bd, kind=kind)


RESIZE = list(_denom_cases()) + [
    _rz("d16_130x38_even", 130, 38, 65, 19),                             # both axes halve with symeven
    _rz("d16_130x38_even_12bit", 130, 38, 65, 19, 12, kind="stripes"),
    _rz("up_66x19_to_131x37", 66, 19, 131, 37, kind="stripes"),          # an up-scale: bank 1000
    _rz("up_66x19_to_131x37_10bit", 66, 19, 131, 37, 10),
    _rz("halve_then_875_100x9", 100, 9, 45, 9),                          # horizontal only: 100 -> 50 -> 45
    _rz("vertical_only_40x50", 40, 50, 40, 33, 8, 1),                    # uint16 samples of 8 bit
    _rz("same_size_21x7", 21, 7, 21, 7),                                 # both axes copy
    _rz("tiny_5x3_to_4x3", 5, 3, 4, 3),
    _rz("tiny_9x2_to_7x2", 9, 2, 7, 2, 10),
    _rz("tiny_7x5_to_13x9", 7, 5, 13, 9),
    _rz("tiny_halve_6x5_to_3x3", 6, 5, 3, 3, 8, kind="stripes"),         # halvings of lengths below 8: the short-input branch
    _rz("d12_322x98_10bit", 322, 98, scaled_size(322, 12), scaled_size(98, 12), 10),     # several workgroups in both passes
]
RESIZE_BY_NAME = {c.name: c for c in RESIZE}
RESIZE_MIXED = ["d9_131x37_8bit", "tiny_9x2_to_7x2", "d16_131x37_10bit", "halve_then_875_100x9", "d13_131x37_12bit",
                "same_size_21x7", "vertical_only_40x50"]


def make_samples(seed, h, w, bd, is16, kind):
    """(h, w) samples: noise over the whole range, or columns that alternate between 0 and the maximum in runs of 1 .. 3 (every filter
    overshoots at both ends)"""
    rng = np.random.RandomState(seed)
    if kind == "noise":
        a = rng.randint(0, 1 << bd, (h, w))
    else:
        runs = np.repeat(np.arange(w) % 2, rng.randint(1, 4, w))[:w]
        a = np.where(runs[None, :] ^ (np.arange(h)[:, None] // 3 % 2), (1 << bd) - 1, 0)
    return a.astype(dtype_of(is16))


def padded(img, stride, seed):
    """(h, stride) buffer: the picture, and a pattern that is no part of it in the columns from its width on"""
    h, w = img.shape
    buf = ((np.arange(h * stride, dtype=np.uint32) * 29 + 7 + seed) & 0xFF).astype(img.dtype).reshape(h, stride)
    buf[:, :w] = img
    return buf


def resize_source(c):
    return padded(make_samples(seed_of(c), c.sh, c.sw, c.bd, c.is16, c.kind), c.sstride, 1)


def down2_steps(in_len, out_len):
    """get_down2_steps (resize.c:149)"""
    steps = 0
    while (in_len + 1) >> 1 >= out_len:
        steps, in_len = steps + 1, (in_len + 1) >> 1
        if in_len == 1:
            break
    return steps


def choose_bank(in_len, out_len):
    o16 = out_len * 16
    return 0 if o16 >= in_len * 16 else 1 if o16 >= in_len * 13 else 2 if o16 >= in_len * 11 else 3 if o16 >= in_len * 9 else 4


def interp_plan(in_len, out_len):
    """delta, offset, x1 and x2 of svt_av1_interpolate_core_c"""
    delta = ((in_len << 14) + out_len // 2) // out_len
    offset = cdiv(((in_len - out_len) << 13) + out_len // 2, out_len) if in_len > out_len else -cdiv(((out_len - in_len) << 13) + out_len // 2, out_len)
    x, y = 0, offset + 128
    while (y >> 14) < 3:
        x, y = x + 1, y + delta
    x1, x = x, out_len - 1
    y = delta * x + offset + 128
    while (y >> 14) + 4 >= in_len:
        x, y = x - 1, y - delta
    return delta, offset, x1, x


def _down2(a, bd, trace):
    """svt_av1_down2_symeven_c / down2_symodd along the last axis, tap indices clamped"""
    n, (even, odd) = a.shape[-1], banks()[1]
    i = np.arange(0, n, 2)
    if n & 1:
        trace["halve"].add("symodd" + ("_short" if 4 > n - 3 + ((n - 3) & 1) else ""))
        s = 64 + a[..., i] * odd[0]
        for j in range(1, 4):
            s = s + (a[..., np.maximum(i - j, 0)] + a[..., np.minimum(i + j, n - 1)]) * odd[j]
    else:
        trace["halve"].add("symeven" + ("_short" if 4 > n - 4 + ((n - 4) & 1) else ""))
        s = np.full(a.shape[:-1] + (i.size,), 64, np.int64)
        for j in range(4):
            s = s + (a[..., np.maximum(i - j, 0)] + a[..., np.minimum(i + 1 + j, n - 1)]) * even[j]
    return np.clip(s >> 7, 0, (1 << bd) - 1)


def _interp(a, out_len, bd, trace):
    n, bank = a.shape[-1], choose_bank(a.shape[-1], out_len)
    delta, offset, x1, x2 = interp_plan(n, out_len)
    y = offset + 128 + np.arange(out_len) * delta
    phase, taps = (y >> 8) & 63, banks()[0][bank]
    trace["phases"].setdefault(BANK_NAMES[bank], set()).update(phase.tolist())
    trace["x1_above_x2"] |= x1 > x2
    s = 0
    for k in range(8):
        s = s + taps[phase, k] * a[..., np.clip((y >> 14) - 3 + k, 0, n - 1)]
    return np.clip((s + 64) >> 7, 0, (1 << bd) - 1)


def new_trace():
    return {"phases": {}, "halve": set(), "x1_above_x2": False}


def resize_line(a, out_len, bd, trace=None):
    """resize_multistep along the last axis of an int64 array"""
    trace = new_trace() if trace is None else trace
    n = a.shape[-1]
    if n == out_len:
        return a
    steps = down2_steps(n, out_len)
    assert steps <= 1, "two halvings"
    if steps:
        a = _down2(a, bd, trace)
    return a if a.shape[-1] == out_len else _interp(a, out_len, bd, trace)


def resize_plane(img, dw, dh, bd, trace=None):
    """svt_av1_resize_plane_c: rows, then the columns of the clipped intermediate"""
    mid = resize_line(img.astype(np.int64), dw, bd, trace)
    return resize_line(mid.T, dh, bd, trace).T.astype(img.dtype)


def restate_resize(c, trace=None):
    return resize_plane(resize_source(c)[:, :c.sw], c.dw, c.dh, c.bd, trace)


def reference_resize(ref, c, src=None):
    """svt_av1_resize_plane_c or its highbd twin; with equal heights svt_av1_resize_plane_horizontal must give the same, and is checked"""
    src, outs = resize_source(c) if src is None else src, []
    names = ["svt_av1_highbd_resize_plane_c" if c.is16 else "svt_av1_resize_plane_c"]
    if c.sh == c.dh:
        names.append("svt_av1_highbd_resize_plane_horizontal" if c.is16 else "svt_av1_resize_plane_horizontal")
    for n in names:
        dst = np.zeros((c.dh, c.dstride), src.dtype)
        args = [src.ctypes.data_as(C.c_void_p), c.sh, c.sw, c.sstride, dst.ctypes.data_as(C.c_void_p), c.dh, c.dw, c.dstride] + ([c.bd] if c.is16 else [])
        assert getattr(ref, n)(*args) == 0, n
        outs.append(dst[:, :c.dw].copy())
    assert all(np.array_equal(outs[0], o) for o in outs[1:]), c.name
    return outs[0]


# ---- super-res -----------------------------------------------------------------------------------------------------------------

SuperresCase = namedtuple("SuperresCase", "name up_width denom sub_x starts bd is16 rows sstride dstride")
SR_MARGIN = 5                      # the columns the reference overwrites and restores on either side of a row
SR_UP_WIDTH = 300


def _sr_case(up_width, denom, sub_x, n_cols, bd, tag=""):
    fw = scaled_size(up_width, denom)
    mi_cols = 2 * ((fw + 7) >> 3)
    starts = [s for s in (0, 16, 48)[:n_cols] if s < mi_cols] + [mi_cols]
    down_end = mi_cols << (2 - sub_x)
    return SuperresCase(f"d{denom}_sub{sub_x}_{len(starts) - 1}cols_{bd}bit{tag}", up_width, denom, sub_x, tuple(starts), bd, int(bd > 8), 8,
                        down_end + 2 * SR_MARGIN + 3, ((up_width + sub_x) >> sub_x) + 7)


def _sr_cases():
    for i, denom in enumerate(range(9, 17)):
        for sub_x in (0, 1):
            yield _sr_case(SR_UP_WIDTH, denom, sub_x, 1 + (i + sub_x) % 3, 10 if (i + sub_x) % 2 else 8)
    # a frame of 297 down to 216 (a multiple of 8): the chroma's last tile column ends at 108 * 11 / 8 = 148, below the plane width of 149
    yield _sr_case(297, 11, 0, 2, 8, "_w297")
    yield _sr_case(297, 11, 1, 2, 10, "_w297")


SUPERRES = list(_sr_cases())
SUPERRES_BY_NAME = {c.name: c for c in SUPERRES}
SUPERRES_MIXED = [SUPERRES[i].name for i in (0, 3, 6, 9, 17)]


def sr_frame_width(c):
    return scaled_size(c.up_width, c.denom)


def sr_widths(c):
    """down-scaled and up-scaled plane widths, and the end of the last tile column in the down-scaled plane"""
    return (sr_frame_width(c) + c.sub_x) >> c.sub_x, (c.up_width + c.sub_x) >> c.sub_x, c.starts[-1] << (2 - c.sub_x)


def superres_source(c):
    """(rows, sstride) buffer; column 0 of the plane is at SR_MARGIN.  Everything is noise: the columns between the plane width and the
    end of the last tile column are read, as in the reference."""
    return make_samples(seed_of(c), c.rows, c.sstride, c.bd, c.is16, "noise")


def restate_superres(c, trace=None):
    down_w, up_w, _ = sr_widths(c)
    src = superres_source(c)[:, SR_MARGIN:].astype(np.int64)
    step = ((down_w << 14) + up_w // 2) // up_w
    err = up_w * step - (down_w << 14)
    x0_qn = (cdiv(-((up_w - down_w) << 13) + up_w // 2, up_w) + 128 - cdiv(err, 2)) & 16383
    taps, out, n = banks()[0][0], np.zeros((c.rows, up_w), np.int64), len(c.starts) - 1
    for j in range(n):
        d0, d1 = c.starts[j] << (2 - c.sub_x), c.starts[j + 1] << (2 - c.sub_x)
        u0, u1 = d0 * c.denom // 8, up_w if j == n - 1 else d1 * c.denom // 8
        if trace is not None and j == n - 1:
            trace["last_below_width"] = d1 * c.denom // 8 < up_w
        x_qn = x0_qn + np.arange(u1 - u0) * step
        at = d0 + (x_qn >> 14) - 4
        s = 0
        for k in range(8):
            col = at + k
            if j == 0:
                col = np.maximum(col, d0)              # the padded border columns read the edge sample
            if j == n - 1:
                col = np.minimum(col, d1 - 1)
            s = s + taps[(x_qn & 16383) >> 8, k] * src[:, col]
        out[:, u0:u1] = np.clip((s + 64) >> 7, 0, (1 << c.bd) - 1)
        x0_qn += (u1 - u0) * step - ((d1 - d0) << 14)
    return out.astype(dtype_of(c.is16))


def reference_superres(pin, c, src=None):
    src, (_, up_w, _) = superres_source(c) if src is None else src, sr_widths(c)
    before, dst = src.copy(), np.zeros((c.rows, c.dstride), src.dtype)
    starts = (C.c_uint16 * len(c.starts))(*c.starts)
    pin.pin_upscale_rows(C.c_void_p(src.ctypes.data + SR_MARGIN * src.itemsize), c.sstride, dst.ctypes.data_as(C.c_void_p), c.dstride, c.rows, c.sub_x,
                         c.bd, c.is16, sr_frame_width(c), c.up_width, c.denom, len(c.starts) - 1, starts)
    assert np.array_equal(src, before)       # it restores what it overwrote
    return dst[:, :up_w].copy()


# ---- prediction from a scaled reference ----------------------------------------------------------------------------------------------

ScaleCase = namedtuple("ScaleCase", "name w h xs ys sx sy tab_x tab_y taps compound bd fwd bck kind")
BLOCKS = [(2, 2), (4, 4), (8, 16), (20, 12), (64, 64), (128, 64), (128, 128)]
STEPS = [64, 512, 1024, 1152, 1365, 2048]
TABLES8 = ("sub_pel_filters_8", "sub_pel_filters_8smooth", "sub_pel_filters_8sharp")
TABLE4 = {"sub_pel_filters_8": "sub_pel_filters_4", "sub_pel_filters_8smooth": "sub_pel_filters_4smooth", "sub_pel_filters_8sharp": "sub_pel_filters_4"}
SC_MARGIN = 8


def _sc(i, w, h, xs, ys, compound, bd, taps=(8, 8), name=None, sx=None, sy=None):
    tab = TABLES8[i % 3]
    sx = (37 * i + 13) % 1024 if sx is None else sx          # never a multiple of 64 unless asked for
    sy = (53 * i + 29) % 1024 if sy is None else sy
    fwd, bck = conv_cases.DIST_WEIGHTS[i % len(conv_cases.DIST_WEIGHTS)]
    return ScaleCase(name or f"{i:02d}_{w}x{h}_x{xs}_y{ys}_c{compound}_{bd}bit", w, h, xs, ys, sx, sy, TABLE4[tab] if w <= 4 else tab,
                     TABLE4[tab] if h <= 4 else tab, taps, compound, bd, fwd, bck, i % 3)


def _sc_cases():
    for i in range(28):
        w, h = BLOCKS[i % 7]
        xs, ys = STEPS[i % 6], STEPS[(5 * i + 1) % 6]
        if xs == ys == 1024:
            ys = 1365
        yield _sc(i, w, h, xs, ys, i % 4, (8, 10, 12)[(i // 2) % 3])
    yield _sc(28, 64, 64, 1152, 1024, 0, 10, name="superres_pattern_64x64")                    # only the width is scaled
    yield _sc(29, 128, 128, 2048, 2048, 0, 8, name="largest_step_128x128", sx=1023, sy=1023)    # 134 intermediate rows per tile
    yield _sc(30, 128, 128, 1365, 1365, 2, 12, name="fractional_tile_row_128x128")
    yield _sc(31, 4, 4, 1152, 1365, 0, 8, taps=(4, 4), name="narrow_tables_4x4")                # [16][4] tables
    yield _sc(32, 8, 16, 512, 64, 1, 8, name="whole_sample_start_8x16", sx=0, sy=0)
    yield _sc(33, 20, 12, 1024, 2048, 3, 10, taps=(6, 8), name="six_tap_table_20x12")


SCALED = list(_sc_cases())
SCALED_BY_NAME = {c.name: c for c in SCALED}


def sc_rounds(c):
    return conv_cases.conv_rounds_compound(c.bd) if c.compound else conv_cases.conv_rounds(c.bd)


def sc_table(name, taps):
    """int16 [16][taps]"""
    return np.ascontiguousarray(np.array(conv_cases.narrow_table(name, taps), np.int16))


def sc_extent(c):
    """rows and columns of the reference plane around the block: SC_MARGIN above and to the left, what the taps reach below and to the right"""
    return (SC_MARGIN + (((c.h - 1) * c.ys + c.sy) >> 10) + 9, SC_MARGIN + (((c.w - 1) * c.xs + c.sx) >> 10) + 9)


def sc_is16(c):
    return int(c.bd > 8)


def scaled_source(c):
    """the reference plane (rows, stride); the block's sample (0, 0) is at [SC_MARGIN, SC_MARGIN]"""
    rows, cols = sc_extent(c)
    kind = ("noise", "stripes", "noise")[c.kind]
    return padded(make_samples(seed_of(c), rows, cols, c.bd, sc_is16(c), kind), cols + 3, 2)


def scaled_cbuf(c):
    """the ConvBufType block a compound 2 / 3 case averages with: what a first prediction of noise would have left"""
    r0, r1 = sc_rounds(c)
    bits, off = 14 - r0 - r1, c.bd + 14 - r0 - r1
    px = np.random.RandomState(seed_of(c) ^ 1).randint(0, 1 << c.bd, (c.h, c.w))
    return ((px << bits) + (1 << off) + (1 << (off - 1))).astype(np.uint16)


def restate_scaled(c, src=None, cbuf=None, trace=None):
    """svt_av1_convolve_2d_scale_c / svt_av1_highbd_convolve_2d_scale_c: the pixels (h, w), or for compound 1 the ConvBufType block"""
    src = (scaled_source(c) if src is None else src).astype(np.int64)
    tx, ty = c.taps
    fx, fy = sc_table(c.tab_x, tx).astype(np.int64), sc_table(c.tab_y, ty).astype(np.int64)
    r0, r1 = sc_rounds(c)
    im_h = (((c.h - 1) * c.ys + c.sy) >> 10) + ty
    x_qn, y_qn = c.sx + np.arange(c.w) * c.xs, c.sy + np.arange(c.h) * c.ys
    if trace is not None:
        trace["second_tile_row_fraction"] = int(y_qn[64]) & 1023 if c.h > 64 else 0
        trace["im_rows"] = im_h
    rows = SC_MARGIN - (ty // 2 - 1) + np.arange(im_h)
    s = np.full((im_h, c.w), 1 << (c.bd + 6), np.int64)
    for k in range(tx):
        s = s + fx[(x_qn & 1023) >> 6, k][None, :] * src[rows[:, None], (SC_MARGIN + (x_qn >> 10) - (tx // 2 - 1) + k)[None, :]]
    im = ((s + ((1 << r0) >> 1)) >> r0).astype(np.int16).astype(np.int64)
    offset_bits = c.bd + 14 - r0
    s = np.full((c.h, c.w), 1 << offset_bits, np.int64)
    for k in range(ty):
        s = s + fy[(y_qn & 1023) >> 6, k][:, None] * im[(y_qn >> 10) + k, :]
    res = ((s + ((1 << r1) >> 1)) >> r1) & 0xFFFF
    if c.compound == 1:
        return res.astype(np.uint16)
    if c.compound:
        prev = (scaled_cbuf(c) if cbuf is None else cbuf).astype(np.int64)
        res = (prev * c.fwd + res * c.bck) >> 4 if c.compound == 3 else (prev + res) >> 1
    bits = 14 - r0 - r1
    res = res - ((1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1)))
    return np.clip((res + ((1 << bits) >> 1)) >> bits, 0, (1 << c.bd) - 1).astype(dtype_of(sc_is16(c)))


def conv_params(c, cbuf):
    r0, r1 = sc_rounds(c)
    cp = abi.ConvolveParams()
    cp.do_average, cp.is_compound, cp.round_0, cp.round_1 = int(c.compound >= 2), int(c.compound != 0), r0, r1
    cp.use_jnt_comp_avg = cp.use_dist_wtd_comp_avg = int(c.compound == 3)
    cp.fwd_offset, cp.bck_offset = c.fwd, c.bck
    if cbuf is not None:
        cp.dst, cp.dst_stride = cbuf.ctypes.data, cbuf.shape[1]
    return cp


def reference_scaled(ref, c, src=None, cbuf=None):
    src = scaled_source(c) if src is None else src
    tabs = [sc_table(c.tab_x, c.taps[0]), sc_table(c.tab_y, c.taps[1])]
    fp = [conv_cases.InterpFilterParams(t.ctypes.data, t.shape[1], 16, 0) for t in tabs]
    cb = (scaled_cbuf(c) if cbuf is None else cbuf.copy()) if c.compound >= 2 else np.zeros((c.h, c.w), np.uint16) if c.compound else None
    cp = conv_params(c, cb)
    dst = np.zeros((c.h, c.w), src.dtype)
    at = C.c_void_p(src.ctypes.data + (SC_MARGIN * src.shape[1] + SC_MARGIN) * src.itemsize)
    args = [at, src.shape[1], dst.ctypes.data_as(C.c_void_p), c.w, c.w, c.h, C.byref(fp[0]), C.byref(fp[1]), c.sx, c.xs, c.sy, c.ys, C.byref(cp)]
    if sc_is16(c):
        ref.svt_av1_highbd_convolve_2d_scale_c(*args, c.bd)
    else:
        ref.svt_av1_convolve_2d_scale_c(*args)
    return cb if c.compound == 1 else dst


# A scaled first prediction and an un-scaled second one of the same block.  The second is written as a ScaleCase with both steps 1024
# and whole sixteenths as phases: svt_av1_jnt_convolve_2d_c is svt_av1_convolve_2d_scale_c at that step, tap for tap, which the fixture
# (made with svt_av1_jnt_convolve_2d_c) confirms for restate_chain.
ChainCase = namedtuple("ChainCase", "name first second")


def _chain(name, w, h, bd, xs, ys, second_compound):
    first = _sc(40, w, h, xs, ys, 1, bd, name=name + "_first")
    second = _sc(41, w, h, 1024, 1024, second_compound, bd, name=name + "_second", sx=5 << 6, sy=11 << 6)
    return ChainCase(name, first, second._replace(tab_x=TABLES8[0], tab_y=TABLES8[2]))


CHAINS = [_chain("chain_20x12_8bit", 20, 12, 8, 1152, 1365, 2), _chain("chain_64x64_10bit", 64, 64, 10, 2048, 1024, 3),
          _chain("chain_128x128_12bit", 128, 128, 12, 1365, 1152, 2)]


def restate_chain(ch):
    return restate_scaled(ch.second, cbuf=restate_scaled(ch.first))


def reference_chain(ref, ch):
    """svt_av1_convolve_2d_scale_c into the ConvBufType block, then svt_av1_jnt_convolve_2d_c averaging with it (or the highbd twins)"""
    c, cb = ch.second, reference_scaled(ref, ch.first)
    src = scaled_source(c)
    tabs = [sc_table(c.tab_x, 8), sc_table(c.tab_y, 8)]
    fp = [conv_cases.InterpFilterParams(t.ctypes.data, 8, 16, 0) for t in tabs]
    cp, dst = conv_params(c, cb), np.zeros((c.h, c.w), src.dtype)
    at = C.c_void_p(src.ctypes.data + (SC_MARGIN * src.shape[1] + SC_MARGIN) * src.itemsize)
    args = [at, src.shape[1], dst.ctypes.data_as(C.c_void_p), c.w, c.w, c.h, C.byref(fp[0]), C.byref(fp[1]), c.sx >> 6, c.sy >> 6, C.byref(cp)]
    if sc_is16(c):
        ref.svt_av1_highbd_jnt_convolve_2d_c(*args, c.bd)
    else:
        ref.svt_av1_jnt_convolve_2d_c(*args)
    return dst


# ---- the pin driver --------------------------------------------------------------------------------------------------------------

def build_pin(tmp_dir):
    import support
    pin = support.build_pin(tmp_dir, os.path.join(HERE, "scale_pin_driver.c"))
    pin.pin_upscale_rows.restype = None
    return pin


def reference_banks(pin):
    b, h = np.zeros((5, 64, 8), np.int16), np.zeros((2, 4), np.int16)
    pin.pin_filter_banks(b.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p))
    return b, h
