"""Cases of the global-motion front end (svt_hip_gm_detect_corners / svt_hip_gm_match_corners), a numpy restatement of the two reference
functions they stand for, svt_av1_fast_corner_detect (corner_detect.c:19-30 over third_party/fastfeat) and svt_av1_determine_correspondence
with improve_correspondence (corner_match.c:87-218), and the calls into the reference's own functions (oracle/_ref/libsvtref.so).
tests/golden/gm_corners.npz (tests/golden/make_golden_gm_corners.py) holds every plane and what the reference gave for it."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from svtav1_hip import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "gm_corners.npz")
MAX_CORNERS, FAST_BARRIER, SEARCH_BY2, THRESHOLD_NCC = abi.GM_MAX_CORNERS, 18, 4, 0.75
BAD_PARAMETER, NO_DEVICE = abi.gm_status(abi.SVT_HIP_ERR_BAD_PARAMETER), abi.gm_status(abi.SVT_HIP_ERR_NO_DEVICE)
STATUS_NAMES = ("svt_hip_gm_detect_corners", "svt_hip_gm_match_corners")

# fast_9.c:2941-2956: the ring as (dx, dy)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

Plane = namedtuple("Plane", "name kind w h stride seed shift")           # shift: where the content of the frame of the same seed appears
MatchCase = namedtuple("MatchCase", "name frm ref match_sz frm_quarters ref_quarters")


def _p(name, kind, w, h, stride=None, seed=0, shift=(0, 0)):
    return Plane(name, kind, w, h, stride or w, seed, shift)


PLANES = [
    # detection: the smallest shapes at which it can still go wrong
    _p("noise_64x48", "noise", 64, 48, 80, 1),
    _p("blocks3_131x97", "blocks3", 131, 97, 136, 2),
    _p("tiny_7x7", "noise", 7, 7, 7, 8),                     # one pixel is tested, (3, 3): no corner in this one ...
    _p("tiny_7x7_corner", "centre", 7, 7, 12),               # ... and a corner in this one
    _p("tiny_9x6", "noise", 9, 6, 16, 4),
    _p("flat_20x20", "flat", 20, 20),
    _p("hand_32x24", "hand", 32, 24, 40),
    _p("dots_300x300", "dots", 300, 300, 304),
    # matching
    _p("b2_frm", "blocks2", 64, 48, 64, 5),
    _p("b2_ref", "blocks2", 64, 48, 72, 5, (2, 1)),
    _p("b2_other", "blocks2", 64, 48, 64, 5, (-1, 2)),
    _p("b3_frm", "blocks3", 200, 72, 208, 6),
    _p("b3_ref", "blocks3", 200, 72, 200, 6, (9, -3)),
    _p("sparse_frm", "sparse", 120, 96, 128),
    _p("sparse_ref", "sparse", 120, 96, 120, 0, (3, 2)),
    _p("flat_64x48", "flat", 64, 48),
]
PLANE = {p.name: p for p in PLANES}
DETECT_LISTED = ["noise_64x48", "blocks3_131x97", "tiny_7x7", "tiny_7x7_corner", "tiny_9x6", "flat_20x20", "hand_32x24", "dots_300x300"]
DETECT_BATCH = ["blocks3_131x97", "tiny_9x6", "noise_64x48"]            # three planes of different sizes in one call

MATCHES = [
    MatchCase("b2_sz7_q4", "b2_frm", "b2_ref", 7, 4, 4),
    MatchCase("b2_sz13_q4", "b2_frm", "b2_ref", 13, 4, 4),
    MatchCase("b2_sz7_q2", "b2_frm", "b2_ref", 7, 2, 2),
    MatchCase("b2_sz13_q2", "b2_frm", "b2_ref", 13, 2, 2),
    MatchCase("b2_other_sz7", "b2_frm", "b2_other", 7, 4, 3),
    MatchCase("b3_sz7", "b3_frm", "b3_ref", 7, 4, 4),
    MatchCase("b3_sz13", "b3_frm", "b3_ref", 13, 4, 4),
    MatchCase("dots_self", "dots_300x300", "dots_300x300", 7, 4, 4),
    MatchCase("sparse_sz7", "sparse_frm", "sparse_ref", 7, 4, 4),
    MatchCase("empty_frm", "flat_64x48", "b2_ref", 7, 4, 4),
    MatchCase("empty_ref", "b2_frm", "flat_64x48", 7, 4, 4),
]
MATCH = {m.name: m for m in MATCHES}
NOISE_MATCHES = [m.name for m in MATCHES if m.name.startswith(("b2_", "b3_"))]
SHARED = ["b2_sz7_q4", "b2_other_sz7", "b2_sz13_q2"]                     # one call: three jobs share the frame's record
HAND_CORNERS = [(3, 3), (28, 3), (19, 15), (28, 20)]                    # what the hand-made picture must give, in raster order


# ---- pictures ---------------------------------------------------------------------------------------------------------------

def _cells(rng, w, h, cell):
    g = rng.randint(0, 256, (-(-h // cell), -(-w // cell))).astype(np.uint8)
    return np.kron(g, np.ones((cell, cell), np.uint8))[:h, :w]


def make_plane(p):
    """The (h, stride) uint8 buffer of a plane; the columns from w on hold a pattern that is no part of the picture."""
    rng, m = np.random.RandomState(1000 + p.seed), 16
    dx, dy = p.shift
    if p.kind == "noise":
        img = rng.randint(0, 256, (p.h, p.w)).astype(np.uint8)
    elif p.kind in ("blocks2", "blocks3"):
        canvas = _cells(rng, p.w + 2 * m, p.h + 2 * m, int(p.kind[-1]))
        img = canvas[m - dy:m - dy + p.h, m - dx:m - dx + p.w].astype(np.int32)
        if p.shift != (0, 0):       # the reference of a pair: its own noise of +-6 on top
            img = img + np.random.RandomState(2000 + p.seed + 7 * dx + dy).randint(-6, 7, img.shape)
        img = np.clip(img, 0, 255).astype(np.uint8)
    elif p.kind == "flat":
        img = np.full((p.h, p.w), 128, np.uint8)
    elif p.kind == "centre":
        img = np.full((p.h, p.w), 128, np.uint8)
        img[p.h // 2, p.w // 2] = 255
    elif p.kind == "dots":
        img = np.zeros((p.h, p.w), np.uint8)
        img[4::4, 4::4] = 200
    elif p.kind == "sparse":        # three-pixel marks every 24 pixels on a background of 40
        img = np.full((p.h, p.w), 40, np.uint8)
        for y in range(10 + dy, p.h - 8, 24):
            for x in range(10 + dx, p.w - 8, 24):
                img[y, x], img[y, x + 1], img[y + 1, x] = 220, 150, 150
    elif p.kind == "hand":
        img = np.full((p.h, p.w), 50, np.uint8)
        for x, y in ((3, 3), (28, 3), (28, 20), (5, 21)):       # the first and last tested column and row; (5, 21) is outside them
            img[y, x] = 200
        img[10, 12] = img[10, 13] = 200                          # a bar of two equal pixels: both go
        img[14, 18], img[15, 19] = 200, 201                      # a diagonal pair: the larger stays
    else:
        raise ValueError(p.kind)
    buf = ((np.arange(p.h * p.stride, dtype=np.uint32) * 29 + 7) & 0xFF).astype(np.uint8).reshape(p.h, p.stride)
    buf[:, :p.w] = img
    return buf


# ---- the fixture --------------------------------------------------------------------------------------------------------------

_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLD) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


def plane_buf(name):
    """The plane as the fixture holds it: (h, stride) uint8"""
    return gold()["plane_" + name]


def golden_corners(name):
    """(count, found, xy[count, 2]) of the reference's svt_av1_fast_corner_detect"""
    g = gold()
    return int(g["count_" + name]), int(g["found_" + name]), g["xy_" + name].astype(np.int32).reshape(-1, 2)


def golden_matches(name):
    """pts[count, 4] of the reference's svt_av1_determine_correspondence"""
    return gold()["pts_" + name].astype(np.int32).reshape(-1, 4)


# ---- the restatement: detection -------------------------------------------------------------------------------------------------

def score_map(img):
    """fast9_score of every pixel that svt_aom_fast9_detect takes for a corner at barrier 18, 0 elsewhere.  The bisection between 18 and
    255 ends at min(254, m - 1), m the largest over the 16 arcs of nine ring pixels and over both signs of the smallest +-(ring - centre)."""
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    c = img[3:h - 3, 3:w - 3].astype(np.int32)
    d = np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int32) - c for dx, dy in RING])

    def arcs(v):
        vv = np.concatenate([v, v[:8]])
        return np.max(np.stack([vv[k:k + 9].min(axis=0) for k in range(16)]), axis=0)
    m = np.maximum(arcs(d), arcs(-d))
    out[3:h - 3, 3:w - 3] = np.where(m > FAST_BARRIER, np.minimum(254, m - 1), 0)
    return out


def suppress(score):
    """nonmax.c: a corner goes when one of its eight neighbours is a corner with a score >= its own.  The survivors as (x, y) in raster order."""
    h, w = score.shape
    pad = np.zeros((h + 2, w + 2), np.int32)
    pad[1:-1, 1:-1] = score
    top = np.max(np.stack([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]), axis=0)
    ys, xs = np.nonzero((score > 0) & (top < score))
    return np.stack([xs, ys], axis=1).astype(np.int32)


def detect(buf, w):
    """(count, found, xy[count, 2]) of the picture in the first w columns of buf"""
    xy = suppress(score_map(buf[:, :w]))
    return min(len(xy), MAX_CORNERS), len(xy), xy[:MAX_CORNERS]


# ---- the restatement: matching --------------------------------------------------------------------------------------------------

def _windows(img, sz):
    return np.lib.stride_tricks.sliding_window_view(img, (sz, sz))       # [y - by2][x - by2] is the window centred at (x, y)


def _eligible(x, y, w, h, by2):
    return (x >= by2) & (y >= by2) & (x + by2 < w) & (y + by2 < h)


def _ncc(tpl, wins, sz):
    """svt_av1_compute_cross_correlation_c of one template against n windows: int sums (nothing overflows up to match_sz 13), one float64
    multiply, one float64 divide; 0 for a negative covariance, nan for 0 / 0"""
    t, v = tpl.astype(np.int64), wins.astype(np.int64)
    sum1, sum2, sumsq2, cross = t.sum(), v.sum(axis=(1, 2)), (v * v).sum(axis=(1, 2)), (v * t).sum(axis=(1, 2))
    var2, cov = sumsq2 * sz * sz - sum2 * sum2, cross * sz * sz - sum1 * sum2
    assert max(np.abs(var2).max(initial=0), np.abs(cov).max(initial=0)) < 2 ** 31
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cov < 0, 0.0, cov.astype(np.float64) * cov.astype(np.float64) / var2.astype(np.float64))


def _first_best(ncc):
    """(index, value) of the first candidate that a `> best` scan from 0.0 ends on; index -1 when none exceeds 0"""
    if len(ncc) == 0:
        return -1, 0.0
    n = np.where(np.isnan(ncc), -1.0, ncc)
    k = int(np.argmax(n))
    return (k, float(n[k])) if n[k] > 0.0 else (-1, 0.0)


def correspond(frm, fxy, ref, rxy, w, h, sz, trace=None):
    """svt_av1_determine_correspondence: pts[n, 4].  frm, ref: (h, >= w) buffers; fxy, rxy: the corners the call is given.
    trace, a dict, receives what the generator's conditions ask about."""
    frm, ref, by2 = frm[:, :w], ref[:, :w], (sz - 1) // 2
    fw, rw = _windows(frm, sz), _windows(ref, sz)
    thresh_sqr = (max(w, h) >> 4) ** 2
    rxy = np.asarray(rxy, np.int64).reshape(-1, 2)
    r_ok = _eligible(rxy[:, 0], rxy[:, 1], w, h, by2)
    off = np.array([(dx, dy) for dy in range(-SEARCH_BY2, SEARCH_BY2 + 1) for dx in range(-SEARCH_BY2, SEARCH_BY2 + 1)], np.int64)
    out, skipped, moved1, moved2, nan = [], 0, 0, 0, 0
    for x, y in np.asarray(fxy, np.int64).reshape(-1, 2):
        if not _eligible(x, y, w, h, by2):
            skipped += 1
            continue
        tpl = fw[y - by2, x - by2]
        cand = np.flatnonzero(r_ok & ((rxy[:, 0] - x) ** 2 + (rxy[:, 1] - y) ** 2 <= thresh_sqr))
        k, best = _first_best(_ncc(tpl, rw[rxy[cand, 1] - by2, rxy[cand, 0] - by2], sz))
        t = tpl.astype(np.int64)
        template_norm = int((t * t).sum() * sz * sz - t.sum() ** 2)
        if not best > template_norm * THRESHOLD_NCC * THRESHOLD_NCC:
            continue
        rx, ry = rxy[cand[k]]
        # improve_correspondence, first loop: the reference point moves
        px, py = rx + off[:, 0], ry + off[:, 1]
        ok = np.flatnonzero(_eligible(px, py, w, h, by2) & ((x - px) ** 2 + (y - py) ** 2 <= thresh_sqr))
        ncc = _ncc(tpl, rw[py[ok] - by2, px[ok] - by2], sz)
        nan += int(np.isnan(ncc).sum())
        k, _ = _first_best(ncc)
        if k >= 0:
            moved1 += bool(off[ok[k]].any())
            rx, ry = rx + off[ok[k], 0], ry + off[ok[k], 1]
        # second loop: the frame point moves, the reference window is the template
        tpl = rw[ry - by2, rx - by2]
        px, py = x + off[:, 0], y + off[:, 1]
        ok = np.flatnonzero(_eligible(px, py, w, h, by2) & ((px - rx) ** 2 + (py - ry) ** 2 <= thresh_sqr))
        ncc = _ncc(tpl, fw[py[ok] - by2, px[ok] - by2], sz)
        nan += int(np.isnan(ncc).sum())
        k, _ = _first_best(ncc)
        if k >= 0:
            moved2 += bool(off[ok[k]].any())
            x, y = x + off[ok[k], 0], y + off[ok[k], 1]
        out.append((x, y, rx, ry))
    if trace is not None:
        trace.update(skipped=skipped, moved1=moved1, moved2=moved2, nan=nan)
    return np.array(out, np.int32).reshape(-1, 4)


def used(count, quarters):
    """The corners of a record that a job uses (gm_ctrls.corners)"""
    return count * quarters // 4


def restated_matches(m, trace=None):
    """The restatement on a case, from the fixture's planes and the fixture's corners"""
    f, r = PLANE[m.frm], PLANE[m.ref]
    (fc, _, fxy), (rc, _, rxy) = golden_corners(m.frm), golden_corners(m.ref)
    return correspond(plane_buf(m.frm), fxy[:used(fc, m.frm_quarters)], plane_buf(m.ref), rxy[:used(rc, m.ref_quarters)], f.w, f.h, m.match_sz, trace)


# ---- the reference's own functions ----------------------------------------------------------------------------------------------

def ref_detect(ref, buf, w):
    """svt_av1_fast_corner_detect of oracle/_ref/libsvtref.so: (count, xy[count, 2]); and `found` from a second call without the cap"""
    buf = np.ascontiguousarray(buf)
    h, stride = buf.shape
    big = np.zeros(2 * w * h + 2, np.int32)
    found = ref.svt_av1_fast_corner_detect(buf.ctypes.data_as(C.c_void_p), w, h, stride, big.ctypes.data_as(C.c_void_p), w * h)
    pts = np.full(2 * MAX_CORNERS, -1, np.int32)
    n = ref.svt_av1_fast_corner_detect(buf.ctypes.data_as(C.c_void_p), w, h, stride, pts.ctypes.data_as(C.c_void_p), MAX_CORNERS)
    assert n == min(found, MAX_CORNERS) and np.array_equal(pts[:2 * n], big[:2 * n])
    return n, found, pts[:2 * n].reshape(-1, 2).copy()


def ref_correspond(ref, frm, fxy, rbuf, rxy, w, h, sz):
    """svt_av1_determine_correspondence of oracle/_ref/libsvtref.so (ref_init() has set the correlation pointer to the C function)"""
    frm, rbuf = np.ascontiguousarray(frm), np.ascontiguousarray(rbuf)
    fxy, rxy = np.ascontiguousarray(fxy, np.int32).reshape(-1), np.ascontiguousarray(rxy, np.int32).reshape(-1)
    out = np.zeros(4 * max(1, len(fxy) // 2), np.int32)
    n = ref.svt_av1_determine_correspondence(frm.ctypes.data_as(C.c_void_p), fxy.ctypes.data_as(C.c_void_p), len(fxy) // 2, rbuf.ctypes.data_as(C.c_void_p),
                                             rxy.ctypes.data_as(C.c_void_p), len(rxy) // 2, w, h, frm.shape[1], rbuf.shape[1],
                                             out.ctypes.data_as(C.c_void_p), C.c_uint8(sz))
    return out[:4 * n].reshape(-1, 4).copy()


def ref_matches(ref, m, corners=None):
    """The reference on a case; corners: {plane: (count, found, xy)}, the fixture's by default"""
    f = PLANE[m.frm]
    (fc, _, fxy), (rc, _, rxy) = (corners or {}).get(m.frm) or golden_corners(m.frm), (corners or {}).get(m.ref) or golden_corners(m.ref)
    fbuf, rbuf = (make_plane(PLANE[n]) if corners else plane_buf(n) for n in (m.frm, m.ref))
    return ref_correspond(ref, fbuf, fxy[:used(fc, m.frm_quarters)], rbuf, rxy[:used(rc, m.ref_quarters)], f.w, f.h, m.match_sz)


# ---- building the calls -----------------------------------------------------------------------------------------------------

def gm_plane(ptr, p):
    return abi.GmPlane(ptr, p.w, p.h, p.stride, 0)


def match_job(m, frm_ptr, ref_ptr, frm_corners, ref_corners):
    f, r = PLANE[m.frm], PLANE[m.ref]
    return abi.GmMatchJob(gm_plane(frm_ptr, f), gm_plane(ref_ptr, r), frm_corners, ref_corners, m.frm_quarters, m.ref_quarters, m.match_sz)


def workspace_bytes(lib, names):
    """What one detect call over these planes needs"""
    return sum(lib.svt_hip_gm_corners_workspace_bytes(PLANE[n].w, PLANE[n].h, 1) for n in names)
