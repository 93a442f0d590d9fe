"""Shared case builders for the in-loop filter parity tests (test infrastructure)."""
import ctypes as C

import numpy as np

from svtav1_hip import abi

BS, VL, VB, HB = 144, 0x7F7F, 3, 8
V = C.c_void_p


def P(a):
    return V(a.ctypes.data)


def cdef_tile(rng, bd, edge=0):
    """A CDEF input tile (u16, stride 144, 64+6 rows) as cdef_seg_search builds it; `edge` bit-mask puts
    CDEF_VERY_LARGE on the top/left/bottom/right borders like at picture boundaries."""
    t = rng.integers(0, 1 << bd, size=(64 + 2 * VB, BS)).astype(np.uint16)
    if edge & 1:
        t[:VB, :] = VL
    if edge & 2:
        t[:, :HB] = VL
    if edge & 4:
        t[VB + 64:, :] = VL
    if edge & 8:
        t[:, HB + 64:] = VL
    return t


def smooth_plane(rng, w, h, bd):
    """Picture-like content (edges + gradients + noise) so that CDEF directions and clamps are exercised."""
    y, x = np.mgrid[0:h, 0:w]
    img = 0.5 * (1 << bd) + 0.3 * (1 << bd) * np.sin(x / 9.0 + y / 17.0) + 0.15 * (1 << bd) * ((x // 16 + y // 24) % 2)
    img += rng.normal(0, (1 << bd) / 64.0, size=(h, w))
    return np.clip(np.rint(img), 0, (1 << bd) - 1)


# ---- harsh whole-picture CDEF content.  smooth_plane only ever yields directions 0 and 7 and filter-block distortions below
# 2^17; these fill all eight directions (every row of the tap table, odd offsets included) and drive the distortion sums to
# 2^25 .. 2^28.  Each generator returns (recon, source) as integer arrays clipped to the bit depth.
CONTENTS = ("oriented", "noise", "ends", "checker", "saturated", "stripes")
STRENGTHS16 = [0, 1, 2, 3, 4, 9, 18, 27, 35, 44, 52, 63, -1, 60, 15, 7]   # both classes; five zero-primary entries (> one group)


def content_plane(kind, rng, w, h, bd):
    top, sc = (1 << bd) - 1, 1 << (bd - 8)
    y, x = np.mgrid[0:h, 0:w]

    def noise():
        return rng.integers(0, top + 1, size=(h, w))

    if kind == "oriented":
        # every 16x16 tile: a sinusoidal edge pattern at its own angle k * pi / 8, a small jitter, a little noise
        tx, ty = x // 16, y // 16
        nty, ntx = (h + 15) // 16, (w + 15) // 16
        ang = ((tx + 3 * ty) % 8) * np.pi / 8 + rng.uniform(-0.04, 0.04, size=(nty, ntx))[ty, tx]
        phase = rng.uniform(0, 2 * np.pi, size=(nty, ntx))[ty, tx]
        u = (x % 16) * np.cos(ang) + (y % 16) * np.sin(ang)
        recon = np.rint(top * (0.5 + 0.35 * np.sin(2 * np.pi * u / 7.0 + phase))) + rng.integers(-3 * sc, 3 * sc + 1, size=(h, w))
        source = recon + rng.integers(-40 * sc, 40 * sc + 1, size=(h, w))
    elif kind == "noise":
        recon, source = noise(), noise()
    elif kind == "ends":
        recon, source = rng.choice(np.array([0, 1, top - 1, top]), size=(h, w)), noise()
    elif kind == "checker":
        recon = ((x + y) & 1) * top
        source = top - recon
    elif kind == "saturated":
        recon, source = np.zeros((h, w), np.int64), np.full((h, w), top)
    elif kind == "stripes":
        recon, source = ((x // 3 + y // 5) & 1) * top, noise()
    else:
        raise ValueError(kind)
    return np.clip(recon, 0, top).astype(np.int64), np.clip(source, 0, top).astype(np.int64)


def content_planes(kind, lw, lh, bd, is16, fmt, seed):
    """The three planes of one picture of `kind`, chroma from the same generator with another seed:
    [(pli, xdec, ydec, w, h, recon, source)], rows 11 samples longer than the picture like the other CDEF cases."""
    dt = np.uint16 if is16 else np.uint8
    planes = []
    for pli in range(3):
        xdec, ydec = int(pli > 0 and fmt != 444), int(pli > 0 and fmt == 420)
        w, h = lw >> xdec, lh >> ydec
        recon, source = content_plane(kind, np.random.default_rng(seed + 1000 * pli), w + 11, h, bd)
        planes.append((pli, xdec, ydec, w, h, recon.astype(dt), source.astype(dt)))
    return planes


def content_filt(lw, lh, kind, seed):
    """filt8x8 of a picture: all ones, or the random 75 % map with one whole filter block cleared."""
    w8, h8 = (lw + 7) // 8, (lh + 7) // 8
    if kind == "ones":
        return np.ones((h8, w8), np.uint8)
    filt = (np.random.default_rng(seed + 77).random((h8, w8)) < 0.75).astype(np.uint8)
    filt[0:8, 8:16] = 0
    return filt


def real_blocks(ldir, lw, lh):
    """The direction (or variance) entries of the 8x8 blocks inside the picture, out of a [n_fb][64] array."""
    w8, h8, nhfb = (lw + 7) // 8, (lh + 7) // 8, (lw + 63) // 64
    return np.array([ldir[(r // 8) * nhfb + c // 8, (r % 8) * 8 + c % 8] for r in range(h8) for c in range(w8)])


def cdef_plane(recon, source, pli, xdec, ydec, is16):
    return abi.CdefPlane(recon.ctypes.data, source.ctypes.data, recon.strides[0] // recon.itemsize,
                         source.strides[0] // source.itemsize, recon.shape[1] if False else 0, 0, is16, xdec, ydec, pli)


def search_params(strengths, damping, coeff_shift, sub):
    p = abi.CdefSearchParams()
    p.n_strengths = len(strengths)
    for i, s in enumerate(strengths):
        p.strengths[i] = s
    p.pri_damping = p.sec_damping = damping
    p.coeff_shift, p.subsampling_factor = coeff_shift, sub
    return p


def rtcd(ref, name, restype, *argtypes):
    p = C.c_void_p.in_dll(ref, name).value
    assert p, name
    return C.CFUNCTYPE(restype, *argtypes)(p)


def ref_cdef_plane(ref, recon, source, w, h, is16, xdec, ydec, pli, filt, strengths, fbs, damping, cs, sub, ldir, lvar):
    """One plane through the REFERENCE's own per-filter-block functions (svt_aom_cdef_find_dir, svt_cdef_filter_fb,
    svt_compute_cdef_dist_*), tiles built as cdef_seg_search (cdef_process.c:204-221) builds them.
    Luma fills ldir/lvar [n_fb][64]; chroma reads them.  Returns (mse[n_fb][n_strengths], applied plane)."""
    lw, lh = w << xdec, h << ydec
    w8, h8, nhfb, nvfb = (lw + 7) // 8, (lh + 7) // 8, (lw + 63) // 64, (lh + 63) // 64
    stride = recon.shape[1]
    fdir = rtcd(ref, "svt_aom_cdef_find_dir", C.c_uint8, V, C.c_int32, V, C.c_int32)
    f16 = rtcd(ref, "svt_compute_cdef_dist_16bit", C.c_uint64, V, C.c_int32, V, V, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint8)
    f8 = rtcd(ref, "svt_compute_cdef_dist_8bit", C.c_uint64, V, C.c_int32, V, V, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint8)
    bsz = 3 if (xdec, ydec) == (0, 0) else 0 if (xdec, ydec) == (1, 1) else 1 if xdec else 2
    eff_sub = min(sub, 4) if bsz == 3 else 1 if bsz == 0 else min(sub, 2)
    bw, bh = 64 >> xdec, 64 >> ydec
    mse = np.full((nhfb * nvfb, len(strengths)), 0xABCD, np.uint64)
    applied = np.zeros_like(recon)
    applied[:, :w] = recon[:, :w]
    for fby in range(nvfb):
        for fbx in range(nhfb):
            fb = fby * nhfb + fbx
            dl = (abi.CdefList * 64)()
            n = 0
            for r in range(8):
                for c in range(8):
                    if fby * 8 + r < h8 and fbx * 8 + c < w8 and filt[fby * 8 + r, fbx * 8 + c]:
                        dl[n].by, dl[n].bx = r, c
                        n += 1
            if n == 0:
                continue
            tile = np.full((64 + 2 * VB, BS), VL, np.uint16)
            for y in range(-VB, bh + VB):
                py = fby * bh + y
                if 0 <= py < h:
                    x0, x1 = max(fbx * bw - HB, 0), min(fbx * bw + bw + HB, w)
                    tile[VB + y, HB + x0 - fbx * bw:HB + x1 - fbx * bw] = recon[py, x0:x1]
            inp = tile.ctypes.data + 2 * (VB * BS + HB)
            if pli == 0:
                for i in range(n):
                    v = C.c_int32(0)
                    ldir[fb, dl[i].by * 8 + dl[i].bx] = fdir(inp + 2 * (8 * dl[i].by * BS + 8 * dl[i].bx), BS, C.addressof(v), cs)
                    lvar[fb, dl[i].by * 8 + dl[i].bx] = v.value
            d16, v16 = np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.int32)
            d16[:8, :8], v16[:8, :8] = ldir[fb].reshape(8, 8), lvar[fb].reshape(8, 8)
            soff = (fby * bh) * stride + fbx * bw
            for gi, s in enumerate(strengths):
                if s < 0:
                    continue
                pri, sec = s // 4, s % 4
                tmp = np.zeros(64 * 64, np.uint16)
                dirinit = C.c_int32(1)
                ref.svt_cdef_filter_fb(None if is16 else P(tmp), P(tmp) if is16 else None, 0, V(inp), xdec, ydec, P(d16), C.byref(dirinit),
                                       P(v16), pli, C.byref(dl), n, pri, sec + (sec == 3), damping, damping, cs, C.c_uint8(eff_sub))
                m = (f16 if is16 else f8)(source.ctypes.data + soff * source.itemsize, stride, tmp.ctypes.data, C.addressof(dl), n, bsz, cs,
                                          pli, eff_sub)
                mse[fb, gi] = m * eff_sub
            s = int(fbs[fb])
            pri, sec = s // 4, s % 4
            if pri or sec:
                dirinit = C.c_int32(1)
                dst = applied.ctypes.data + soff * recon.itemsize
                ref.svt_cdef_filter_fb(None if is16 else V(dst), V(dst) if is16 else None, stride, V(inp), xdec, ydec, P(d16),
                                       C.byref(dirinit), P(v16), pli, C.byref(dl), n, pri, sec + (sec == 3), damping, damping, cs,
                                       C.c_uint8(1))
    return mse, applied


GOLDEN_CDEF = [  # key, luma w, luma h, bd, is16, fmt, sub, seed, content (None: smooth_plane)
    ("a_420_8", 200, 136, 8, 0, 420, 2, 5, None), ("b_420_10", 136, 72, 10, 1, 420, 1, 6, None),
    ("c_444_8in16", 72, 136, 8, 1, 444, 4, 7, None), ("d_420_10_tall", 72, 200, 10, 1, 420, 4, 8, None),
    ("e_oriented_420_8", 136, 72, 8, 0, 420, 1, 9, "oriented"), ("f_noise_420_10", 136, 72, 10, 1, 420, 1, 10, "noise")]


def golden_cdef_inputs(lw, lh, bd, is16, fmt, sub, seed, content=None):
    """Seeded inputs of one golden picture: yields per plane (pli, xdec, ydec, w, h, recon, source) + shared parameters."""
    rng = np.random.default_rng(seed)
    w8, h8, nhfb, nvfb = lw // 8, lh // 8, (lw + 63) // 64, (lh + 63) // 64
    filt = (rng.random((h8, w8)) < 0.75).astype(np.uint8)
    if content:     # harsh content: the 16-entry strength list over both classes, every strength kind among the applied ones
        fbs = rng.permutation(np.array([2, 37, 63, 0, 1, 22], np.uint8))
        return filt, STRENGTHS16, 3 + seed % 4, fbs, content_planes(content, lw, lh, bd, is16, fmt, seed)
    strengths = [0, 5, 18, 35, 63, -1, 12, 2]
    damping = 3 + seed % 4
    fbs = rng.choice(np.array([s for s in strengths if s >= 0], np.uint8), size=nhfb * nvfb).astype(np.uint8)
    dt = np.uint16 if is16 else np.uint8
    planes = []
    for pli in range(3):
        xdec, ydec = int(pli > 0 and fmt != 444), int(pli > 0 and fmt == 420)
        w, h = lw >> xdec, lh >> ydec
        recon = smooth_plane(rng, w + 11, h, bd).astype(dt)
        source = np.clip(recon.astype(np.int32) + rng.integers(-6, 7, size=recon.shape), 0, (1 << bd) - 1).astype(dt)
        planes.append((pli, xdec, ydec, w, h, recon, source))
    return filt, strengths, damping, fbs, planes


# ------------------------------------------------------------------------------------------------ deblocking
# BlockSize enum (definitions.h): value by (width, height)
BSIZE = {(4, 4): 0, (4, 8): 1, (8, 4): 2, (8, 8): 3, (8, 16): 4, (16, 8): 5, (16, 16): 6, (16, 32): 7, (32, 16): 8, (32, 32): 9,
         (32, 64): 10, (64, 32): 11, (64, 64): 12, (64, 128): 13, (128, 64): 14, (128, 128): 15, (4, 16): 16, (16, 4): 17,
         (8, 32): 18, (32, 8): 19, (16, 64): 20, (64, 16): 21}


class RefLfModeInfo(C.Structure):   # oracle/ref_harness_lf.c
    _fields_ = [(n, C.c_void_p) for n in ("bsize", "tx_depth", "skip", "ref_frame0", "mode", "segment_id")]


class RefLfHeader(C.Structure):
    _fields_ = [("filter_level", C.c_int32 * 2), ("filter_level_u", C.c_int32), ("filter_level_v", C.c_int32),
                ("sharpness_level", C.c_int32), ("mode_ref_delta_enabled", C.c_uint8), ("ref_deltas", C.c_int8 * 8),
                ("mode_deltas", C.c_int8 * 2), ("segmentation_enabled", C.c_uint8), ("seg_lf_data", (C.c_int16 * 4) * 8),
                ("seg_lf_enabled", (C.c_uint8 * 4) * 8)]


def random_mode_info(rng, mi_rows, mi_cols, mi_stride, sb=64, p_skip=0.45, p_intra=0.3, max_depth=2):
    """A random but structurally valid block partition of the picture: per-4x4 arrays of the fields
    set_lpf_parameters reads (bsize, tx_depth, skip, ref_frame[0], mode, segment_id)."""
    f = {k: np.zeros((mi_rows, mi_stride), np.uint8) for k in ("bsize", "tx_depth", "skip", "ref_frame0", "mode", "segment_id")}

    def leaf(x, y, w, h):
        if x >= mi_cols * 4 or y >= mi_rows * 4:
            return
        intra = rng.random() < p_intra
        vals = dict(bsize=BSIZE[(w, h)], tx_depth=int(rng.integers(0, max_depth + 1)), skip=int(rng.random() < p_skip),
                    ref_frame0=0 if intra else int(rng.integers(1, 8)), mode=int(rng.integers(0, 13)) if intra else int(rng.integers(13, 25)),
                    segment_id=int(rng.integers(0, 8)))
        for k, v in vals.items():
            f[k][y // 4:min((y + h) // 4, mi_rows), x // 4:min((x + w) // 4, mi_cols)] = v

    def part(x, y, s):
        if x >= mi_cols * 4 or y >= mi_rows * 4:
            return
        kinds = ["none", "split", "horz", "vert"] if s > 4 else ["none"]
        if 16 <= s <= 64:
            kinds += ["horz4", "vert4"]
        if s >= 16:
            kinds += ["horz_a", "horz_b", "vert_a", "vert_b"]
        w = [3 if k == "split" and s > 16 else 1 for k in kinds]
        k = kinds[int(rng.choice(len(kinds), p=np.array(w) / sum(w)))]
        hs = s // 2
        if k == "none":
            leaf(x, y, s, s)
        elif k == "split":
            for dy in (0, hs):
                for dx in (0, hs):
                    part(x + dx, y + dy, hs)
        elif k == "horz":
            leaf(x, y, s, hs), leaf(x, y + hs, s, hs)
        elif k == "vert":
            leaf(x, y, hs, s), leaf(x + hs, y, hs, s)
        elif k == "horz4":
            for i in range(4):
                leaf(x, y + i * s // 4, s, s // 4)
        elif k == "vert4":
            for i in range(4):
                leaf(x + i * s // 4, y, s // 4, s)
        elif k == "horz_a":
            leaf(x, y, hs, hs), leaf(x + hs, y, hs, hs), leaf(x, y + hs, s, hs)
        elif k == "horz_b":
            leaf(x, y, s, hs), leaf(x, y + hs, hs, hs), leaf(x + hs, y + hs, hs, hs)
        elif k == "vert_a":
            leaf(x, y, hs, hs), leaf(x, y + hs, hs, hs), leaf(x + hs, y, hs, s)
        elif k == "vert_b":
            leaf(x, y, hs, s), leaf(x + hs, y, hs, hs), leaf(x + hs, y + hs, hs, hs)

    for y in range(0, mi_rows * 4, sb):
        for x in range(0, mi_cols * 4, sb):
            part(x, y, sb)
    return f


BW = {v: k[0] for k, v in BSIZE.items()}
BH = {v: k[1] for k, v in BSIZE.items()}
TX = {(4, 4): 0, (8, 8): 1, (16, 16): 2, (32, 32): 3, (64, 64): 4, (4, 8): 5, (8, 4): 6, (8, 16): 7, (16, 8): 8, (16, 32): 9, (32, 16): 10,
      (32, 64): 11, (64, 32): 12, (4, 16): 13, (16, 4): 14, (8, 32): 15, (32, 8): 16, (16, 64): 17, (64, 16): 18}   # TxSize by (w, h)
TXW = {v: k[0] for k, v in TX.items()}
TXH = {v: k[1] for k, v in TX.items()}
TX_UV = sorted({TX[(min(max(w // 2, 4), 32), min(max(h // 2, 4), 32))] for w, h in BSIZE})    # the 14 chroma sizes of 4:2:0
INTER_MODES_WITH_DELTA = (13, 14, 16, 17, 18, 19, 20, 21, 22, 24)     # mode_lf_lut == 1: every inter mode but the two GLOBAL ones


def split_tx(w, h):
    """One step of the transform split of the AV1 specification: a square halves, 2:1 becomes the square of its short side, 4:1 halves
    its long side."""
    if w == h:
        return max(w // 2, 4), max(h // 2, 4)
    if w > h:
        return (w // 2, h) if w == 4 * h else (h, h)
    return (w, h // 2) if h == 4 * w else (w, w)


def max_depth_of(bsize):
    """The depths a block can have: none above 64 samples or for the 4x8 / 8x4 / 4x4 blocks, one for 8x8, two otherwise."""
    w, h = BW[bsize], BH[bsize]
    return 0 if max(w, h) > 64 or w * h <= 32 else 1 if (w, h) == (8, 8) else 2


def flat_mode_info(minfo, mi_rows, mi_stride):
    """The SvtHipLfMi grid of a partition (what INTEGRATION's gather loop builds), tx_depth limited to what the block can have in
    `minfo` itself.  test_dlf_pick_abi.py checks the grid against the reference's gather (ref_lf_gather)."""
    flat = np.zeros((mi_rows, mi_stride), abi.LF_MI_DTYPE)
    for r in range(mi_rows):
        for c in range(mi_stride):
            b = int(minfo["bsize"][r, c])
            minfo["tx_depth"][r, c] = min(int(minfo["tx_depth"][r, c]), max_depth_of(b))
            skip_inter = bool(minfo["skip"][r, c]) and minfo["ref_frame0"][r, c] > 0
            w, h = min(BW[b], 64), min(BH[b], 64)
            for _ in range(0 if skip_inter else int(minfo["tx_depth"][r, c])):
                w, h = split_tx(w, h)
            flat[r, c] = (b, TX[(w, h)], TX[(min(max(BW[b] // 2, 4), 32), min(max(BH[b] // 2, 4), 32))], skip_inter,
                          minfo["segment_id"][r, c], minfo["ref_frame0"][r, c], int(minfo["mode"][r, c]) in INTER_MODES_WITH_DELTA, 0)
    return flat


# ---- the catalogue partition.  A layout is a nested tuple: a partition type of the AV1 specification followed by the transform
# depths of its blocks in coding order (0 where left out), or "split" followed by the layouts of the four quarters.  A 64x64
# region takes its layout by its place in the picture, LAYOUTS64[(row * whole regions per row + column) % 12].  Together the
# twelve hold every block size up to 64x64 with every depth it can have.  On a picture four regions wide the first two rows
# alone hold every size at depth 0 (transform = block) at a place with a left and at one with an upper neighbour: the
# regions that a block fills from side to side (5, 1, 2) or from top to bottom (5, 4, 6) lie off the left or upper border, the
# smaller ones in the right or lower quarters.  No region is like the one beside or below it.
_Q16 = ("split", ("horz", 0, 1), ("vert", 0, 1), ("horz4", 0, 1, 2, 0), ("vert4", 0, 1, 2, 0))   # 16x8, 8x16, 16x4, 4x16
_Q8 = ("split", ("horz_a", 0, 1, 2), ("vert_a", 0, 1, 2), ("split", ("none", 1), ("horz",), ("vert",), ("split",) + (("none",),) * 4),
       ("none", 0))                                                                               # 8x8 .. 4x4, 16x8 / 8x16 depth 2, 16x16
LAYOUTS64 = [
    ("split", ("horz_b", 2, 1, 2), ("vert_b", 2, 1, 2), ("horz4", 1, 2, 0, 1), ("none", 0)),
    ("horz", 1, 0), ("horz4", 0, 1, 2, 0), ("split", ("vert4", 1, 2, 0, 1), ("none", 1), _Q16, _Q8),
    ("vert", 1, 0), ("none", 0), ("vert4", 0, 1, 2, 0), ("split", ("horz", 0, 1), ("vert", 0, 1), ("horz4", 0, 1, 2, 0), ("vert4", 0, 1, 2, 0)),
    ("none", 1), ("horz_a", 1, 2, 2), ("none", 2), ("vert_a", 0, 2, 2)]
LAYOUTS128 = [("split",), ("split",), ("vert",), ("none",), ("horz",), ("split",)]      # per superblock, in raster order


def _leaves(layout, x, y, s):
    """The (x, y, w, h, depth) blocks of one layout of a square of `s` samples at (x, y), in coding order."""
    k, hs, qs = layout[0], s // 2, s // 4
    if k == "split":
        return [b for i, sub in enumerate(layout[1:]) for b in _leaves(sub, x + (i & 1) * hs, y + (i >> 1) * hs, hs)]
    blocks = {"none": [(x, y, s, s)], "horz": [(x, y, s, hs), (x, y + hs, s, hs)], "vert": [(x, y, hs, s), (x + hs, y, hs, s)],
              "horz4": [(x, y + i * qs, s, qs) for i in range(4)], "vert4": [(x + i * qs, y, qs, s) for i in range(4)],
              "horz_a": [(x, y, hs, hs), (x + hs, y, hs, hs), (x, y + hs, s, hs)],
              "horz_b": [(x, y, s, hs), (x, y + hs, hs, hs), (x + hs, y + hs, hs, hs)],
              "vert_a": [(x, y, hs, hs), (x, y + hs, hs, hs), (x + hs, y, hs, s)],
              "vert_b": [(x, y, hs, s), (x + hs, y, hs, hs), (x + hs, y + hs, hs, hs)]}[k]
    return [b + (d,) for b, d in zip(blocks, layout[1:] + (0,) * len(blocks))]


def catalogue_mode_info(mi_rows, mi_cols, mi_stride, sb, seed, p_skip=0.45, p_intra=0.3):
    """A deterministic partition: every 64x64 region has the layout and the transform depths that LAYOUTS64 gives its place,
    and with sb == 128 the superblocks walk LAYOUTS128 in raster order, "split" standing for four such regions.  The first
    block of each size above 64 samples is a skipped inter block (its 64-sample interior transform edges are the ones
    set_lpf_parameters refuses); the other fields (skip, reference, mode, segment) are seeded random as in random_mode_info."""
    rng = np.random.default_rng(seed)
    f = {k: np.zeros((mi_rows, mi_stride), np.uint8) for k in ("bsize", "tx_depth", "skip", "ref_frame0", "mode", "segment_id")}
    W, H = mi_cols * 4, mi_rows * 4
    big = set()

    def leaf(x, y, w, h, depth):
        intra, skip = rng.random() < p_intra, int(rng.random() < p_skip)     # drawn for every block, inside the picture or not
        ref0, mode_intra, mode_inter, seg = int(rng.integers(1, 8)), int(rng.integers(0, 13)), int(rng.integers(13, 25)), int(rng.integers(0, 8))
        if x >= W or y >= H:
            return
        b = BSIZE[(w, h)]
        if max(w, h) > 64 and b not in big:
            big.add(b)
            intra, skip = False, 1
        vals = dict(bsize=b, tx_depth=min(depth, max_depth_of(b)), skip=skip, ref_frame0=0 if intra else ref0,
                    mode=mode_intra if intra else mode_inter, segment_id=seg)
        for k, v in vals.items():
            f[k][y // 4:min((y + h) // 4, mi_rows), x // 4:min((x + w) // 4, mi_cols)] = v

    def region(x, y):
        for b in _leaves(LAYOUTS64[(y // 64 * max(W // 64, 1) + x // 64) % len(LAYOUTS64)], x, y, 64):
            leaf(*b)

    n_sb = 0
    for y in range(0, H, sb):
        for x in range(0, W, sb):
            if sb == 64:
                region(x, y)
                continue
            layout = LAYOUTS128[n_sb % len(LAYOUTS128)]
            n_sb += 1
            if layout[0] == "split":
                for i in range(4):
                    region(x + (i & 1) * 64, y + (i >> 1) * 64)
            else:
                for b in _leaves(layout, x, y, 128):
                    leaf(*b)
    return f


def lf_header(rng, variant):
    """Frame-header loop-filter parameters; `variant` walks through the branches of svt_av1_loop_filter_frame_init."""
    h = RefLfHeader()
    h.filter_level[0], h.filter_level[1] = int(rng.integers(1, 64)), int(rng.integers(1, 64))
    h.filter_level_u, h.filter_level_v = int(rng.integers(1, 64)), int(rng.integers(1, 64))
    h.sharpness_level = (0, 3, 7, 5)[variant % 4]
    if variant % 3 == 1:
        h.mode_ref_delta_enabled = 1
        for i, v in enumerate((1, 0, 0, 0, -1, 0, -1, -1)):      # the AV1 default ref deltas
            h.ref_deltas[i] = v + int(rng.integers(-2, 3))
        h.mode_deltas[0], h.mode_deltas[1] = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
    if variant % 3 == 2:
        h.segmentation_enabled = 1
        for s in range(8):
            for k in range(4):
                h.seg_lf_enabled[s][k] = int(rng.random() < 0.6)
                h.seg_lf_data[s][k] = int(rng.integers(-40, 41))
    if variant == 5:
        h.filter_level_u = 0                                      # plane switched off
    if variant == 7:
        h.filter_level[0] = h.filter_level[1] = 0                 # luma off => everything off (the `break`, :570-572)
    return h


PAD = 32


def lf_planes(rng, w, h, bd, is16):
    """Three padded 4:2:0 planes with blocky content (so that every filter and both flat branches fire)."""
    dt = np.uint16 if is16 else np.uint8
    out = []
    for pl in range(3):
        pw, ph = (w >> (pl > 0)) + 2 * PAD, (h >> (pl > 0)) + 2 * PAD
        yy, xx = np.mgrid[0:ph, 0:pw]
        img = (1 << bd) * (0.5 + 0.25 * np.sin(xx / 23.0) * np.cos(yy / 31.0))
        img += (1 << (bd - 8)) * rng.integers(-6, 7, size=(ph // 8 + 1, pw // 8 + 1)).repeat(8, 0).repeat(8, 1)[:ph, :pw]   # block steps
        img += (1 << (bd - 8)) * rng.integers(-40, 41, size=(ph // 32 + 1, pw // 32 + 1)).repeat(32, 0).repeat(32, 1)[:ph, :pw] * (rng.random() < 0.5)
        img += rng.integers(-1, 2, size=(ph, pw)) * (1 << (bd - 8)) * (rng.random((ph, pw)) < 0.3)
        out.append(np.clip(np.rint(img), 0, (1 << bd) - 1).astype(dt))
    return out


LF_CONTENTS = ("low", "high", "ends", "steps")


def lf_content_planes(kind, rng, w, h, bd, is16):
    """Three padded 4:2:0 planes whose samples sit at the ends of the range, where the signed clamps of filter4 act:
    `low` lf_planes moved down until its lower part clips at 0, `high` its mirror at the top value, `ends` 16x16 areas drawn
    from {0, 1, 2s} or from {top - 2s, top - 1, top}, `steps` steps of up to +-110 s per 8x8 block around mid-range with a
    little noise (s = 1 << (bd - 8))."""
    top, s = (1 << bd) - 1, 1 << (bd - 8)
    if kind in ("low", "high"):
        out = [np.clip(p.astype(np.int64) - 115 * s, 0, top) for p in lf_planes(rng, w, h, bd, is16)]
        return [(top - p if kind == "high" else p).astype(np.uint16 if is16 else np.uint8) for p in out]
    out = []
    for pl in range(3):
        pw, ph = (w >> (pl > 0)) + 2 * PAD, (h >> (pl > 0)) + 2 * PAD
        if kind == "ends":
            high = (rng.random((ph // 16 + 1, pw // 16 + 1)) < 0.5).repeat(16, 0).repeat(16, 1)[:ph, :pw]
            pick = rng.integers(0, 3, size=(ph, pw))
            img = np.where(high, np.array([top - 2 * s, top - 1, top])[pick], np.array([0, 1, 2 * s])[pick])
        elif kind == "steps":
            img = 128 * s + s * rng.integers(-110, 111, size=(ph // 8 + 1, pw // 8 + 1)).repeat(8, 0).repeat(8, 1)[:ph, :pw]
            img = img + rng.integers(-1, 2, size=(ph, pw)) * s * (rng.random((ph, pw)) < 0.3)
        else:
            raise ValueError(kind)
        out.append(np.clip(img, 0, top).astype(np.uint16 if is16 else np.uint8))
    return out


def lf_frame(planes, w, h, mi_ptr, mi_stride, mi_rows, mi_cols, hdr, bd, is16, plane_start=0, plane_end=3, lvl=None):
    f = abi.LfFrame()
    for i, p in enumerate(planes):
        if isinstance(p, np.ndarray):
            f.plane[i] = p.ctypes.data + (PAD * p.shape[1] + PAD) * p.itemsize
            f.stride[i] = p.shape[1]
        else:
            f.plane[i], f.stride[i] = p
    f.width, f.height, f.mi, f.mi_stride, f.mi_rows, f.mi_cols = w, h, mi_ptr, mi_stride, mi_rows, mi_cols
    f.filter_level[0], f.filter_level[1] = hdr.filter_level[0], hdr.filter_level[1]
    f.filter_level_u, f.filter_level_v, f.sharpness_level = hdr.filter_level_u, hdr.filter_level_v, hdr.sharpness_level
    f.bit_depth, f.is_16bit, f.plane_start, f.plane_end = bd, is16, plane_start, plane_end
    if lvl is not None:
        C.memmove(f.lvl, lvl.ctypes.data, 768)
    return f


def ref_deblock(ref, planes, w, h, minfo, mi_stride, mi_rows, mi_cols, hdr, bd, is16, sb_size=64, plane_start=0, plane_end=3):
    """Run the REAL svt_av1_loop_filter_frame in place on `planes`; returns (flat SvtHipLfMi array, lvl table)."""
    m = RefLfModeInfo(*[minfo[k].ctypes.data for k in ("bsize", "tx_depth", "skip", "ref_frame0", "mode", "segment_id")])
    flat = np.zeros((mi_rows, mi_stride), abi.LF_MI_DTYPE)
    ref.ref_lf_gather(mi_rows * mi_stride, C.byref(m), P(flat))
    f = lf_frame(planes, w, h, None, mi_stride, mi_rows, mi_cols, hdr, bd, is16, plane_start, plane_end)
    assert ref.ref_loop_filter_frame(C.byref(f), C.byref(m), C.byref(hdr), sb_size) == 0
    return flat, np.frombuffer(bytes(f.lvl), np.uint8).copy()


def random_levels(rng):
    """A level table drawn at random, one entry in seven 0: any table is a valid input of the frame filter (the reference's
    derivation of it from the frame header is control-plane code), and it needs no reference where there is none."""
    lvl = rng.integers(0, 64, size=(3, 8, 2, 8, 2)).astype(np.uint8)
    lvl[:, :, :, :, :] = np.where(rng.random(lvl.shape) < 0.15, 0, lvl)
    return lvl.reshape(-1)


class CatalogueCase:
    """One deblocking frame on the catalogue partition: the header of lf_header(variant) (variants 0..3: its four sharpness
    values, no plane switched off), a random level table, and lf_planes or one of LF_CONTENTS."""

    def __init__(self, w, h, bd, is16, sb, variant=0, content=None, seed=0):
        self.w, self.h, self.bd, self.is16, self.sb = w, h, bd, is16, sb
        rng = np.random.default_rng(7000 + seed)
        self.mi_cols, self.mi_rows = (w + 7) // 8 * 2, (h + 7) // 8 * 2
        self.mi_stride = self.mi_cols + 3
        self.minfo = catalogue_mode_info(self.mi_rows, self.mi_cols, self.mi_stride, sb, 7000 + seed)
        self.flat = flat_mode_info(self.minfo, self.mi_rows, self.mi_stride)
        self.hdr = lf_header(rng, variant)
        self.lvl = random_levels(rng)
        wa, ha = self.mi_cols * 4, self.mi_rows * 4
        self.planes = lf_planes(rng, wa, ha, bd, is16) if content is None else lf_content_planes(content, rng, wa, ha, bd, is16)

    def frame(self, planes, mi_ptr, plane_start=0, plane_end=3, lvl=None):
        return lf_frame(planes, self.w, self.h, mi_ptr, self.mi_stride, self.mi_rows, self.mi_cols, self.hdr, self.bd, self.is16,
                        plane_start, plane_end, self.lvl if lvl is None else lvl)

    def oracle(self, orc, plane_start=0, plane_end=3):
        out = [p.copy() for p in self.planes]
        orc.orc_loop_filter_frame(C.byref(self.frame(out, self.flat.ctypes.data, plane_start, plane_end)), self.sb)
        return out


DEPTHS = ((8, 0), (10, 1), (8, 1), (12, 1))
CATALOGUE_PARAMS = [(bd, is16, sb, variant) for bd, is16 in DEPTHS for sb in (64, 128) for variant in range(4)]
# kind, bit depth, is16, w, h, first plane; 130x258: the one size whose luma width is no multiple of 4
LF_CONTENT_PARAMS = [(kind, bd, int(bd > 8), w, h, 0) for kind in LF_CONTENTS for bd in (8, 10, 12) for w, h in ((200, 136), (130, 258))]
LF_CONTENT_PARAMS += [("steps", 10, 1, 200, 136, 1)]


def catalogue_case(bd, is16, sb, variant):
    """264 x 200.  The seeds are chosen: with them the level table of every case leaves each transform size a filtered edge
    (test_lf_oracle.py::test_catalogue_conditions); about one table in eight has the zeros in the wrong place."""
    return CatalogueCase(264, 200, bd, is16, sb, variant, None, 74000 + bd + is16 + sb + variant)


def lf_content_case(kind, bd, is16, w, h):
    """Superblock 128 on the tall picture, 64 on the wide one; the header variant (sharpness) follows the kind."""
    return CatalogueCase(w, h, bd, is16, 128 if h > w else 64, LF_CONTENTS.index(kind), kind, 100 + bd + w)


GOLDEN_DLF = [  # key, w, h, bd, is16, header variant, sb, seed, content (None: random partition and lf_planes; else catalogue partition)
    ("a_8bit", 200, 136, 8, 0, 1, 64, 21, None), ("b_10bit_seg", 136, 72, 10, 1, 2, 64, 22, None),
    ("c_8in16_sb128", 264, 136, 8, 1, 0, 128, 23, None), ("d_10bit_ends", 136, 72, 10, 1, 1, 64, 24, "ends")]


def golden_dlf_inputs(w, h, bd, is16, variant, sb, seed, content=None):
    rng = np.random.default_rng(seed)
    mi_cols, mi_rows = (w + 7) // 8 * 2, (h + 7) // 8 * 2
    mi_stride = mi_cols + 1
    if content:
        minfo = catalogue_mode_info(mi_rows, mi_cols, mi_stride, sb, seed)
        return mi_cols, mi_rows, mi_stride, minfo, lf_header(rng, variant), lf_content_planes(content, rng, mi_cols * 4, mi_rows * 4, bd, is16)
    minfo = random_mode_info(rng, mi_rows, mi_cols, mi_stride, sb=sb)
    hdr = lf_header(rng, variant)
    planes = lf_planes(rng, mi_cols * 4, mi_rows * 4, bd, is16)
    return mi_cols, mi_rows, mi_stride, minfo, hdr, planes


class GoldHdr:
    """The header fields lf_frame() needs, rebuilt from a golden fixture's meta row."""

    def __init__(self, meta):
        self.filter_level = [int(meta[7]), int(meta[8])]
        self.filter_level_u, self.filter_level_v, self.sharpness_level = int(meta[9]), int(meta[10]), int(meta[11])


def golden_dlf_cases():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dlf.npz"))
    for key in sorted(k[:-5] for k in g.files if k.endswith("_meta")):
        meta = g[key + "_meta"]
        w, h, bd, is16, mi_cols, mi_rows, mi_stride = (int(v) for v in meta[:7])
        flat = np.ascontiguousarray(g[key + "_mi"]).view(abi.LF_MI_DTYPE).reshape(mi_rows, mi_stride)
        yield (key, w, h, bd, is16, mi_cols, mi_rows, mi_stride, flat, g[key + "_lvl"].copy(), GoldHdr(meta),
               [g[f"{key}_in{i}"].copy() for i in range(3)], [g[f"{key}_out{i}"] for i in range(3)])
