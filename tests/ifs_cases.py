"""The cases of the interpolation filter search (svt_hip_ifs_search_batch, include/svt_hip_inter.h), their seeded integer pictures, a numpy
restatement of the whole search (interpolation_filter_search, enc_inter_prediction.c:2413-2543, with model_rd_for_sb / model_rd_from_sse)
and the builder of descriptors over one device arena (test infrastructure).  tests/golden/ifs.npz (tests/golden/make_golden_ifs.py) holds
what the reference's own functions leave on every case, driven by tests/ifs_pin_driver.c; tests/test_ifs_abi.py pins fixture and
restatement to them wherever oracle/_ref/libsvtref.so has been built.

A call has one job (bit depth, dual filter, controls, quantizer, lambda, rate table), so the cases are grouped by job: JOBS[c.job]."""
import collections
import ctypes as C
import os
import zlib

import numpy as np

import conv_cases
from arena import GUARD, Arena, check_containment, rows
from svtav1_hip import abi, device

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ifs.npz")
BORDER = 8
ONES = (1 << 64) - 1
SIZES = conv_cases.AV1_SIZES
FILTER_SETS = [(fy, fx) for fy in range(3) for fx in range(3)]      # filter_sets: [0] the y filter, [1] the x filter
BANKS = np.array([conv_cases.REGULAR, conv_cases.SMOOTH, conv_cases.SHARP, conv_cases.REGULAR4, conv_cases.SMOOTH4], np.int16)   # d_filters
WEIGHTS = [(9, 7), (11, 5), (12, 4), (13, 3)]                        # quant_dist_lookup_table pairs (fwd, bck)

Job = collections.namedtuple("Job", "name bd dual sub skip bias q lam rates")
Case = collections.namedtuple("Case", "group job w h compound fwd bck phases ctx kind seed")


def rate_table(kind):
    """switchable_interp_fac_bitss stand-ins, int32 [16][3]: "random" has context k favour filter k % 3 by a wide margin; "equal" is flat"""
    if kind == "equal":
        return np.full((16, 3), 700, np.int32)
    t = np.random.RandomState(41).randint(300, 1500, (16, 3)).astype(np.int32)
    t[np.arange(16), np.arange(16) % 3] = 20 + np.arange(16)
    return t


# y_dequant_qtx[q][1] at q = 0, mid, 255: 8 bit 4 .. 1828 (qstep 0 .. 228), 10 bit 4 .. 7312 (qstep 0 .. 228)
JOBS = [Job("main8", 8, 1, 0, 0, 0, 366, 3100, "random"), Job("main10", 10, 1, 0, 0, 0, 1451, 3100, "random"),
        Job("nodual8", 8, 0, 0, 0, 0, 366, 3100, "random"), Job("nodual10", 10, 0, 0, 0, 0, 1451, 3100, "random"),
        Job("sub8", 8, 1, 1, 0, 0, 366, 3100, "random"), Job("sub10", 10, 0, 1, 0, 0, 1451, 3100, "random"),
        Job("skip8", 8, 1, 0, 1, 0, 366, 3100, "random"), Job("skip10", 10, 1, 0, 1, 0, 1451, 3100, "random"),
        Job("level5_10", 10, 1, 1, 1, 0, 1451, 3100, "random"),
        Job("bias110_8", 8, 1, 0, 0, 110, 366, 3100, "random"), Job("bias130_10", 10, 1, 0, 0, 130, 1451, 3100, "random"),
        Job("bias130_nodual8", 8, 0, 0, 0, 130, 366, 3100, "random"),
        Job("qlow8", 8, 1, 0, 0, 0, 4, 3100, "random"), Job("qhigh8", 8, 1, 0, 0, 0, 1828, 3100, "random"),
        Job("qlow10", 10, 1, 0, 0, 0, 4, 3100, "random"), Job("qhigh10", 10, 1, 0, 0, 0, 7312, 3100, "random"),
        Job("lam_small8", 8, 1, 0, 0, 0, 366, 3, "random"), Job("lam_large8", 8, 1, 0, 0, 0, 366, 1 << 27, "random"),
        Job("lam_large10", 10, 1, 0, 0, 0, 1451, 1 << 27, "random"),
        Job("equal8", 8, 1, 0, 0, 0, 366, 3100, "equal")]
JOB = {j.name: i for i, j in enumerate(JOBS)}


def _cases():
    out = []

    def add(group, job, w, h, compound=0, fwd=0, bck=0, phases=(5, 11, 9, 2), ctx=None, kind="smooth"):
        i = len(out)
        ctx = ctx if ctx is not None else ((i * 5) % 16, (i * 7 + 3) % 16)
        out.append(Case(group, JOB[job], w, h, compound, fwd, bck, tuple(phases), tuple(ctx), kind, 1000 + i))

    # every size, single and compound, both components of every phase fractional
    for job in ("main8", "main10"):
        for k, (w, h) in enumerate(SIZES):
            add("size", job, w, h, phases=(3 + 2 * (k % 6), 1 + 2 * (k % 7), 0, 0), kind=("smooth", "busy")[k % 2])
            add("size", job, w, h, 2 + k % 2, *WEIGHTS[k % 4], phases=(1 + k % 15, 15 - k % 15, 2 + k % 13, 1 + (3 * k) % 15), kind=("busy", "smooth")[k % 2])
    # the 8 x 8 even phases: copy, x, y, 2d in sr and in jnt form
    for job, (w, h) in (("main8", (8, 8)), ("main10", (4, 16))):
        for px in range(0, 16, 2):
            for py in range(0, 16, 2):
                add("phase", job, w, h, phases=(px, py, 0, 0), kind="busy")
                add("phase", job, w, h, 2 + (px // 2 + py // 2) % 2, 11, 5, phases=(px, py, py, (px + 6) % 16), kind="busy")
    # the weight pairs and their reverses; the two references at different phases, one of them at zero phases
    for job in ("main8", "main10"):
        for k, (a, b) in enumerate(WEIGHTS + [(b, a) for a, b in WEIGHTS]):
            add("weights", job, (16, 16, 32, 8)[k % 4], (16, 8, 32, 32)[k % 4], 3, a, b, phases=((0, 0, 7, 12) if k % 2 else (13, 4, 0, 0)), kind="smooth")
        add("weights", job, 16, 16, 2, phases=(0, 0, 0, 0))
        add("weights", job, 16, 16, 2, phases=(6, 0, 0, 10))
    for job in ("nodual8", "nodual10"):
        for k, (w, h) in enumerate(((4, 4), (8, 8), (16, 16), (64, 64), (16, 4), (4, 16), (32, 64))):
            add("nodual", job, w, h, (0, 2, 3)[k % 3], 12, 4, phases=((5, 9, 3, 14), (0, 6, 0, 6), (10, 0, 4, 0), (0, 0, 0, 0))[k % 4], kind=("busy", "smooth", "flat")[k % 3])
    # sub-sampled distortion: h == 16 is not sub-sampled, h >= 32 is
    for job in ("sub8", "sub10", "level5_10"):
        for k, (w, h) in enumerate(((16, 16), (64, 16), (8, 16), (32, 32), (8, 32), (16, 64), (128, 128), (64, 128))):
            add("sub", job, w, h, (0, 2)[k % 2], phases=(4 + k, 15 - k, 1 + k, 2 * k), kind=("busy", "smooth")[k % 2])
    for job in ("skip8", "skip10"):
        for k, (w, h) in enumerate(((8, 8), (32, 16), (64, 64), (4, 8))):
            add("skip", job, w, h, (0, 3)[k % 2], 4, 12, kind=("busy", "smooth")[k % 2])
    for job in ("bias110_8", "bias130_10", "bias130_nodual8"):
        for k, (w, h) in enumerate(((8, 8), (16, 16), (32, 32), (16, 8), (8, 4), (64, 32))):
            add("bias", job, w, h, (0, 2)[k % 2], phases=(2 + k, 13 - k, 7, 7), kind=("smooth", "busy", "flat")[k % 3])
    for job in ("qlow8", "qhigh8", "qlow10", "qhigh10"):
        for k, (w, h) in enumerate(((8, 8), (32, 32), (16, 16), (4, 4), (128, 64))):
            add("quantizer", job, w, h, (0, 2)[k % 2], kind=("busy", "smooth", "flat", "busy", "smooth")[k])
    for job in ("qhigh8", "qhigh10"):            # a small sse under a large qstep: the MAX_XSQ_Q10 clamp
        for w, h in ((8, 8), (16, 16), (64, 64)):
            add("clamp", job, w, h, phases=(0, 0, 0, 0), kind="near")
    for job in ("lam_small8", "lam_large8", "lam_large10"):
        for k, (w, h) in enumerate(((8, 8), (16, 16), (32, 32), (16, 32))):
            add("lambda", job, w, h, (0, 3)[k % 2], 7, 9, kind=("busy", "smooth")[k % 2])
    for job in ("main8", "main10", "nodual8", "skip10"):      # source equal to the reference at zero phases
        add("zero", job, 16, 16, phases=(0, 0, 0, 0), kind="same")
        add("zero", job, 64, 32, phases=(0, 0, 0, 0), kind="same")
    add("contrast", "main10", 128, 128, phases=(8, 8, 0, 0), kind="contrast")      # sse above 2^32
    add("contrast", "skip10", 128, 128, 2, phases=(2, 12, 0, 0), kind="contrast")
    # flat references: every filter predicts the same, the nine SSEs are equal
    for job in ("main8", "main10", "equal8", "lam_large8"):
        for k, (w, h) in enumerate(((8, 8), (16, 16), (32, 8))):
            add("flat", job, w, h, (0, 2, 3)[k], 5, 11, kind="flat")
    # the rate decides on flat content under the large lambda: context k favours filter k % 3, so every pair wins once
    for fy in range(3):
        for fx in range(3):
            add("winner", "lam_large8", 8, 8, ctx=(fy + 3 * fx, fx + 6), kind="flat")
            add("winner", "lam_large10", 16, 8, 2, ctx=(fy + 9, fx + 3 * fy), kind="flat")
    return out


CASES = _cases()


def _texture(rs, H, W, cell, hi):
    """a coarse random grid interpolated in integers to (H + 4) x (W + 4)"""
    gh, gw = (H + 4) // cell + 3, (W + 4) // cell + 3
    grid = rs.randint(hi // 16, hi - hi // 16, (gh, gw)).astype(np.int64)
    yy, xx = np.arange(H + 4), np.arange(W + 4)
    a, u, b, v = yy // cell, yy % cell, xx // cell, xx % cell
    top = grid[a][:, b] * (cell - v) + grid[a][:, b + 1] * v
    bot = grid[a + 1][:, b] * (cell - v) + grid[a + 1][:, b + 1] * v
    return (top * (cell - u)[:, None] + bot * u[:, None] + cell * cell // 2) // (cell * cell)


def pictures(c):
    """(src [h][w], ref0, ref1 [(h + 2 BORDER)][(w + 2 BORDER)] with the block at (BORDER, BORDER)) as int64, samples of the job's bit depth"""
    bd = JOBS[c.job].bd
    rs, hi = np.random.RandomState(c.seed), 1 << bd
    H, W, B = c.h + 2 * BORDER, c.w + 2 * BORDER, BORDER
    if c.kind == "flat":
        ref0, ref1 = np.full((H, W), 90 << (bd - 8), np.int64), np.full((H, W), 101 << (bd - 8), np.int64)
        src = (93 << (bd - 8)) + rs.randint(0, 3, (c.h, c.w))
    elif c.kind == "contrast":
        cells = rs.randint(0, 2, (H // 16 + 1, W // 16 + 1)) * (hi - 1)
        ref0 = np.kron(cells, np.ones((16, 16), np.int64))[:H, :W]
        ref1 = ref0.copy()
        src = (hi - 1) - ref0[B:B + c.h, B:B + c.w]
    else:
        base = _texture(rs, H, W, 4 if c.kind == "busy" else 12, hi)
        n = (2, 5)[c.kind == "busy"] << (bd - 8)
        ref0 = base[0:H, 0:W] + rs.randint(-n, n + 1, (H, W))
        ref1 = base[2:H + 2, 1:W + 1] + rs.randint(-n, n + 1, (H, W))
        src = base[1:H + 1, 1:W + 1][B:B + c.h, B:B + c.w] + rs.randint(-n, n + 1, (c.h, c.w))
        if c.kind in ("same", "near"):
            src = ref0[B:B + c.h, B:B + c.w].copy()
        if c.kind == "near":
            src[::3, 1::4] += 1 << (bd - 8)
    return tuple(np.clip(p, 0, hi - 1).astype(np.int64) for p in (src, ref0, ref1))


def sample_dtype(c):
    return np.uint16 if JOBS[c.job].bd > 8 else np.uint8


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _rnd(v, n):
    return (v + ((1 << n) >> 1)) >> n


def _u16(v):
    return v & 0xFFFF


def _i16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def bank_of(f, side):
    """av1_get_interp_filter_params_with_block_size as an index into BANKS"""
    return (4 if f == 1 else 3) if side <= 4 else f


def _h(P, w, rows_, kx):
    win = P[rows_, BORDER - 3:BORDER + w + 4]
    return sum(int(kx[k]) * win[:, k:k + w] for k in range(8))


def _v(a, h, ky):
    return sum(int(ky[k]) * a[k:k + h] for k in range(8))


def predict_sr(P, w, h, sx, sy, kx, ky, bd):
    """svt_av1_(highbd_)convolve_{2d, x, y, 2d_copy}_sr with the ConvolveParams of get_conv_params_no_round(.., is_compound = 0, bd)"""
    B, hi = BORDER, (1 << bd) - 1
    if sx and sy:
        im = _i16(_u16(_rnd(_h(P, w, slice(B - 3, B + h + 4), kx) + (1 << (bd + 6)), 3)))
        res = _rnd(_v(im, h, ky) + (1 << (bd + 11)), 11) - ((1 << bd) + (1 << (bd - 1)))
        return np.clip(_i16(res) if bd == 8 else res, 0, hi)
    if sx:
        return np.clip(_rnd(_rnd(_h(P, w, slice(B, B + h), kx), 3), 4), 0, hi)
    if sy:
        return np.clip(_rnd(_v(P[B - 3:B + h + 4, B:B + w], h, ky), 7), 0, hi)
    return P[B:B + h, B:B + w].copy()


def predict_jnt(P, w, h, sx, sy, kx, ky, bd):
    """svt_av1_(highbd_)jnt_convolve_{2d, x, y, 2d_copy}: what goes to the ConvBufType plane (round_0 3, round_1 7)"""
    B, off = BORDER, (1 << (bd + 4)) + (1 << (bd + 3))
    if sx and sy:
        im = _i16(_u16(_rnd(_h(P, w, slice(B - 3, B + h + 4), kx) + (1 << (bd + 6)), 3)))
        return _u16(_rnd(_v(im, h, ky) + (1 << (bd + 11)), 7))
    if sy:
        return _rnd(_v(P[B - 3:B + h + 4, B:B + w], h, ky) * 16, 7) + off
    if sx:
        return _rnd(_h(P, w, slice(B, B + h), kx), 3) + off
    return _u16(_u16(P[B:B + h, B:B + w] << 4) + off)


def predict(c, ref0, ref1, fy, fx, banks=BANKS):
    """the luma prediction of one filter pair, [h][w] int64"""
    bd = JOBS[c.job].bd
    x0, y0, x1, y1 = c.phases
    taps = lambda f, side, phase: banks[bank_of(f, side)][phase]
    if not c.compound:
        return predict_sr(ref0, c.w, c.h, x0, y0, taps(fx, c.w, x0), taps(fy, c.h, y0), bd)
    a = _u16(predict_jnt(ref0, c.w, c.h, x0, y0, taps(fx, c.w, x0), taps(fy, c.h, y0), bd))
    b = predict_jnt(ref1, c.w, c.h, x1, y1, taps(fx, c.w, x1), taps(fy, c.h, y1), bd)
    tmp = (a * c.fwd + b * c.bck) >> 4 if c.compound == 3 else (a + b) >> 1
    return np.clip(_rnd(tmp - ((1 << (bd + 4)) + (1 << (bd + 3))), 4), 0, (1 << bd) - 1)


RATE_TAB = [65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376, 3307,
            3244, 3186, 3133, 3037, 2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001, 1928, 1862,
            1802, 1748, 1698, 1651, 1608, 1530, 1460, 1398, 1342, 1290, 1243, 1199, 1159, 1086, 1021, 963, 911, 864, 821, 781, 745, 680, 623,
            574, 530, 490, 455, 424, 395, 345, 304, 269, 239, 213, 190, 171, 154, 126, 104, 87, 73, 61, 52, 44, 38, 28, 21, 16, 12, 10, 8, 6,
            5, 3, 2, 1, 1, 1, 0, 0]
DIST_TAB = [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 7, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 21, 24, 26, 29, 31, 34, 36, 39, 44, 49, 54, 59, 64,
            69, 73, 78, 88, 97, 106, 115, 124, 133, 142, 151, 167, 184, 200, 215, 231, 245, 260, 274, 301, 327, 351, 375, 397, 418, 439, 458,
            495, 528, 559, 587, 613, 637, 659, 680, 717, 749, 777, 801, 823, 842, 859, 874, 899, 919, 936, 949, 960, 969, 977, 983, 994, 1001,
            1006, 1010, 1013, 1015, 1017, 1018, 1020, 1022, 1022, 1023, 1023, 1023, 1024]
XSQ_IQ = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96, 112, 128, 144, 160, 176, 192, 208, 224, 256, 288, 320, 352, 384, 416,
          448, 480, 544, 608, 672, 736, 800, 864, 928, 992, 1120, 1248, 1376, 1504, 1632, 1760, 1888, 2016, 2272, 2528, 2784, 3040, 3296, 3552,
          3808, 4064, 4576, 5088, 5600, 6112, 6624, 7136, 7648, 8160, 9184, 10208, 11232, 12256, 13280, 14304, 15328, 16352, 18400, 20448, 22496,
          24544, 26592, 28640, 30688, 32736, 36832, 40928, 45024, 49120, 53216, 57312, 61408, 65504, 73696, 81888, 90080, 98272, 106464, 114656,
          122848, 131040, 147424, 163808, 180192, 196576, 212960, 229344, 245728]
MAX_XSQ_Q10 = 245727


def _i32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def model_rd_from_sse(n_log2, quantizer, bd, sse):
    """(rate as the int32 the function writes, dist after its << 4, whether MAX_XSQ_Q10 clamped): model_rd_from_sse(.., 0) in Python ints"""
    qstep = quantizer >> (bd - 5)
    if sse == 0:
        return 0, 0, False
    xsq64 = ((qstep * qstep << (n_log2 + 10)) + (sse >> 1)) // sse
    xsq = min(xsq64, MAX_XSQ_Q10)
    tmp = (xsq >> 2) + 8
    k = tmp.bit_length() - 1 - 3
    xq = (k << 3) + ((tmp >> k) & 7)
    a = ((xsq - XSQ_IQ[xq]) << 10) >> (2 + k)
    b = 1024 - a
    r_q10 = (RATE_TAB[xq] * b + RATE_TAB[xq + 1] * a) >> 10
    d_q10 = (DIST_TAB[xq] * b + DIST_TAB[xq + 1] * a) >> 10
    return _i32(((r_q10 << n_log2) + 1) >> 1), (((sse * d_q10 + 512) >> 10) << 4) & ONES, xsq64 > MAX_XSQ_Q10


Found = collections.namedtuple("Found", "sse rd best filters rate pred clamped")


def search(c, pics=None, banks=BANKS):
    """The whole search on one case: Found(sse[9], rd[9] (ONES where a pair is not tested), index of the winner, its packed filters, its
    switchable rate, its prediction [h][w], whether the MAX_XSQ_Q10 clamp applied to any pair)"""
    j = JOBS[c.job]
    src, ref0, ref1 = pics if pics is not None else pictures(c)
    rates = rate_table(j.rates)
    anyx, anyy = bool(c.phases[0] or (c.compound and c.phases[2])), bool(c.phases[1] or (c.compound and c.phases[3]))
    shift = 1 if j.sub and c.h > 16 else 0
    sse, rd, preds, best, clamped = [ONES] * 9, [ONES] * 9, {}, None, False
    for i, (fy, fx) in enumerate(FILTER_SETS):
        if not j.dual and fy != fx:
            continue
        rs = int(rates[c.ctx[0]][fy]) + (int(rates[c.ctx[1]][fx]) if j.dual else 0)
        key = (fy if anyy else 0, fx if anyx else 0)       # a direction without a phase ignores its filter
        if key not in preds:
            preds[key] = predict(c, ref0, ref1, key[0], key[1], banks)
        d = src[::1 + shift] - preds[key][::1 + shift]
        s = int((d * d).sum()) << shift
        if j.skip:
            rate, dist = 0, s * 10
        else:
            rate, dist, cl = model_rd_from_sse((c.w * c.h).bit_length() - 1, j.q, j.bd, _rnd(s, 2 * (j.bd - 8)))
            clamped |= cl
        cost = ((_i32(rs + rate) * j.lam + 256) >> 9) + dist * 128
        cost &= ONES
        if j.bias and (fy == 1 or fx == 1):
            cost = (cost * j.bias) // 100
        sse[i], rd[i] = s, cost
        if best is None or cost < rd[best]:
            best = i
    fy, fx = FILTER_SETS[best]
    rs = int(rates[c.ctx[0]][fy]) + (int(rates[c.ctx[1]][fx]) if j.dual else 0)
    return Found(sse, rd, best, fy | fx << 16, rs, preds[(fy if anyy else 0, fx if anyx else 0)], clamped)


def checksum(pred, c):
    return zlib.crc32(np.ascontiguousarray(pred.astype(sample_dtype(c))).tobytes())


def found_tuple(f, c):
    """what the fixture holds of a case"""
    return tuple(f.sse), tuple(f.rd), (f.best, f.filters, f.rate), checksum(f.pred, c)


class Golden:
    def __init__(self):
        g = np.load(GOLDEN)
        self.banks, self.sse, self.rd, self.rec, self.crc = g["banks"], g["sse"], g["rd"], g["rec"], g["crc"]
        assert len(self.sse) == len(CASES), "tests/golden/ifs.npz is not of this case list: run tests/golden/make_golden_ifs.py"

    def record(self, i):
        return tuple(int(v) for v in self.sse[i]), tuple(int(v) for v in self.rd[i]), tuple(int(v) for v in self.rec[i]), int(self.crc[i])


# ---- the reference's own functions ------------------------------------------------------------------------------------------------------
class PinCase(C.Structure):      # PinIfsCase of tests/ifs_pin_driver.c
    _fields_ = [("src", C.c_void_p), ("ref0", C.c_void_p), ("ref1", C.c_void_p), ("src_stride", C.c_int32), ("ref0_stride", C.c_int32),
                ("ref1_stride", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("bd", C.c_int32), ("phase", C.c_int32 * 4), ("compound", C.c_int32),
                ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32), ("ctx", C.c_int32 * 2), ("rates", C.c_void_p), ("full_lambda", C.c_uint32),
                ("quantizer", C.c_int32), ("dual", C.c_int32), ("subsampled", C.c_int32), ("skip_model", C.c_int32), ("bias", C.c_int32)]


class Pin:
    """tests/ifs_pin_driver.c built into `directory` against oracle/_ref/libsvtref.so (pyorc.ref() has set the reference's function tables up)"""

    def __init__(self, directory):
        import pyorc
        from support import build_pin
        self.ref, self.lib = pyorc.ref(), build_pin(directory, os.path.join(HERE, "ifs_pin_driver.c"))
        self.lib.pin_ifs_search.restype = C.c_uint64

    def banks(self):
        out = np.zeros((5, 16, 8), np.int16)
        self.lib.pin_ifs_filter_banks(out.ctypes.data_as(C.c_void_p))
        return out

    def search(self, c):
        j, dt = JOBS[c.job], sample_dtype(c)
        src, ref0, ref1 = (np.ascontiguousarray(p.astype(dt)) for p in pictures(c))
        rates = np.ascontiguousarray(rate_table(j.rates))
        at = lambda p: p.ctypes.data + (BORDER * p.shape[1] + BORDER) * p.itemsize
        pc = PinCase(src.ctypes.data, at(ref0), at(ref1), c.w, ref0.shape[1], ref1.shape[1], c.w, c.h, j.bd, (C.c_int32 * 4)(*c.phases), c.compound,
                     c.fwd, c.bck, (C.c_int32 * 2)(*c.ctx), rates.ctypes.data, j.lam, j.q, j.dual, j.sub, j.skip, j.bias)
        sse, rd, rec, pred = np.zeros(9, np.uint64), np.zeros(9, np.uint64), np.zeros(3, np.int32), np.zeros((c.h, c.w), dt)
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        best_rd = self.lib.pin_ifs_search(C.byref(pc), P(sse), P(rd), P(rec), P(pred))
        assert best_rd == int(rd[rec[0]])
        return tuple(int(v) for v in sse), tuple(int(v) for v in rd), tuple(int(v) for v in rec), zlib.crc32(pred.tobytes())


# ---- descriptors over one device arena ----------------------------------------------------------------------------------------------------
def make_job(j, d_rates, d_filters):
    return abi.IfsJob(d_switchable_rate=d_rates, d_filters=d_filters, full_lambda=j.lam, quantizer=j.q, bit_depth=j.bd, enable_dual_filter=j.dual,
                      subsampled_distortion=j.sub, skip_sse_rd_model=j.skip, smooth_bias_pct=j.bias)


class Loaded:
    """The pictures of a list of cases OF ONE JOB in one guarded arena on the device (fill GUARD), with the job's tables, and one descriptor
    per case.  layout(i) -> (byte skew of every plane of case i, samples of stride padding).  With dst, every case has a w x h output inside
    its own guarded region."""

    def __init__(self, lib, cases, layout=lambda i: (0, 0), dst=True):
        assert len({c.job for c in cases}) == 1
        self.lib, self.cases, self.j = lib, cases, JOBS[cases[0].job]
        px = 2 if self.j.bd > 8 else 1
        ar, self.descs, self.declared = Arena(fill=GUARD, tail=4096), np.zeros(len(cases), abi.IFS_DESC_DTYPE), []
        o_rates, o_filters = ar.add("rates", rate_table(self.j.rates)), ar.add("filters", BANKS)
        self.dst_at = []
        for i, c in enumerate(cases):
            skew, pad = layout(i)
            dt = sample_dtype(c)
            src, ref0, ref1 = pictures(c)
            d = self.descs[i]

            def plane(name, a):
                wide = np.full((a.shape[0], a.shape[1] + pad), GUARD * 0x0101 & ((1 << self.j.bd) - 1), dt)
                wide[:, :a.shape[1]] = a
                return ar.add(f"{name} of case {i}", wide, skew=skew * px), a.shape[1] + pad
            o, d["src_stride"] = plane("src", src)
            d["src"] = o
            for k, p in enumerate((ref0, ref1)):
                o, d[f"ref{k}_stride"] = plane(f"ref{k}", p)
                d[f"ref{k}"] = o + (BORDER * int(d[f"ref{k}_stride"]) + BORDER) * px
            if dst:
                stride = c.w + 3 + pad
                o = ar.add(f"dst of case {i}", nbytes=stride * c.h * px, skew=skew * px)
                d["dst"], d["dst_stride"] = o, stride
                self.declared += rows(o, stride * px, c.w * px, c.h)
                self.dst_at.append((o, stride))
            d["w"], d["h"] = c.w, c.h
            d["subpel_x0"], d["subpel_y0"], d["subpel_x1"], d["subpel_y1"] = c.phases
            d["compound"], d["fwd_offset"], d["bck_offset"], d["ctx"] = c.compound, c.fwd, c.bck, c.ctx
        self.regions, self.before = ar.regions, ar.build()
        self.buf = device.DeviceBuffer(lib, self.before.nbytes)
        self.buf.upload(self.before)
        for f in ("src", "ref0", "ref1") + (("dst",) if dst else ()):
            self.descs[f] += self.buf.ptr
        self.job = make_job(self.j, self.buf.ptr + o_rates, self.buf.ptr + o_filters)

    def run(self, descs, trace=True):
        """One call over `descs` (rows of self.descs): (records, trace, clean) -- clean: the guards around the records and the trace are
        untouched and, in the arena, nothing but the dst rectangles of self.descs changed"""
        out, tr, guards = device.ifs_search_batch(self.lib, self.job, descs, trace=trace, fill=GUARD)
        self.after = self.buf.download(np.uint8, (self.before.nbytes,))
        check_containment(self.before, self.after, self.regions, self.declared, "svt_hip_ifs_search_batch")
        return out, tr, bool((guards == GUARD).all())

    def dst(self, i):
        """what the last run left in the dst rectangle of case i"""
        c, px, (o, stride) = self.cases[i], 2 if self.j.bd > 8 else 1, self.dst_at[i]
        return self.after[o:o + stride * c.h * px].view(sample_dtype(c)).reshape(c.h, stride)[:, :c.w]

    def reset(self):
        self.buf.upload(self.before)


def record_tuple(r, t):
    """a device record and its trace in the form of Golden.record without the checksum"""
    return tuple(int(v) for v in t["sse"]), tuple(int(v) for v in t["rd"]), (int(r["best"]), int(r["interp_filters"]), int(r["switchable_rate"]))
