"""CPU: the in-loop filter oracle against the REAL reference functions (oracle/_ref RTCD pointers / _c symbols)."""
import ctypes as C

import numpy as np
import pytest

import lf_cases as L
from lf_cases import BS, HB, P, V, VB, VL
from svtav1_hip import abi


def rtcd(ref, name, restype, *argtypes):
    p = C.c_void_p.in_dll(ref, name).value
    assert p, name
    return C.CFUNCTYPE(restype, *argtypes)(p)


def test_cdef_find_dir(orc, ref):
    rng = np.random.default_rng(1)
    fn = rtcd(ref, "svt_aom_cdef_find_dir", C.c_uint8, V, C.c_int32, V, C.c_int32)
    for trial in range(300):
        bd = (8, 10, 12)[trial % 3]
        img = rng.integers(0, 1 << bd, size=(8, 24)).astype(np.uint16)
        if trial % 7 == 0:
            img[:] = np.arange(24, dtype=np.uint16) * ((1 << bd) // 32)   # pure gradient
        if trial % 11 == 0:
            img[:] = 7
        v1, v2 = C.c_int32(-1), C.c_int32(-1)
        d1 = fn(img.ctypes.data, 24, C.addressof(v1), bd - 8)
        d2 = orc.orc_cdef_find_dir(P(img), 24, C.byref(v2), bd - 8)
        assert (d1, v1.value) == (d2, v2.value)


def test_cdef_filter_block(orc, ref):
    rng = np.random.default_rng(2)
    fn = rtcd(ref, "svt_cdef_filter_block", None, V, V, C.c_int32, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
              C.c_int32, C.c_int32, C.c_uint8)
    for trial in range(600):
        bd = (8, 10)[trial % 2]
        cs = bd - 8
        tile = L.cdef_tile(rng, bd, edge=trial % 16)
        if trial % 5 == 0:   # low-contrast content: the constrain() ramps matter
            tile = np.where(tile == VL, VL, (tile.astype(np.int32) // 64 + (1 << (bd - 1)))).astype(np.uint16)
        bsize = trial % 4
        by, bx = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        bw, bh = 4 << (bsize in (2, 3)), 4 << (bsize in (1, 3))
        off = (VB + by * bh) * BS + HB + bx * bw
        pri, sec = int(rng.integers(0, 16)) << cs, int(rng.choice([0, 1, 2, 4])) << cs
        d = int(rng.integers(0, 8))
        damp = int(rng.integers(3, 7)) + cs
        sub = (1, 2, 4)[trial % 3] if bsize == 3 else (1, 2)[trial % 2] if bsize in (1, 2) else 1
        for is16 in (0, 1):
            o1 = np.full((8, 16), 0xAAAA if is16 else 0xAA, np.uint16 if is16 else np.uint8)
            o2 = o1.copy()
            flat = tile.reshape(-1)
            inp = flat.ctypes.data + 2 * off
            fn(None if is16 else o1.ctypes.data, o1.ctypes.data if is16 else None, 16, inp, pri, sec, d, damp, damp, bsize, cs, sub)
            orc.orc_cdef_filter_block(None if is16 else P(o2), P(o2) if is16 else None, 16, V(inp), pri, sec, d, damp, damp, bsize,
                                      cs, C.c_uint8(sub))
            assert np.array_equal(o1, o2), (trial, is16)


def test_cdef_dist(orc, ref):
    rng = np.random.default_rng(3)
    f16 = rtcd(ref, "svt_compute_cdef_dist_16bit", C.c_uint64, V, C.c_int32, V, V, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint8)
    f8 = rtcd(ref, "svt_compute_cdef_dist_8bit", C.c_uint64, V, C.c_int32, V, V, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint8)
    orc.orc_compute_cdef_dist.restype = C.c_uint64
    for trial in range(200):
        is16 = trial % 2
        bd = 10 if is16 and trial % 4 == 1 else 8
        cs = bd - 8
        bsize, pli = trial % 4, int(trial % 3 == 0 and trial % 4 == 3) * 0 + (0 if trial % 4 == 3 and trial % 3 else 1)
        n = int(rng.integers(1, 65))
        dl = (abi.CdefList * 64)()
        cells = rng.permutation(64)[:n]
        for i, c in enumerate(sorted(cells)):
            dl[i].by, dl[i].bx = c // 8, c % 8
        dt = np.uint16 if is16 else np.uint8
        pic = rng.integers(0, 1 << bd, size=(64, 80)).astype(dt)
        packed = np.clip(pic[:64, :64].astype(np.int32) + rng.integers(-9, 10, size=(64, 64)), 0, (1 << bd) - 1).astype(dt).reshape(-1)
        sub = (1, 2, 4)[trial % 3] if bsize == 3 else 1
        a = (f16 if is16 else f8)(pic.ctypes.data, 80, packed.ctypes.data, C.addressof(dl), n, bsize, cs, pli, sub)
        b = orc.orc_compute_cdef_dist(P(pic), 80, P(packed), C.byref(dl), n, bsize, cs, pli, C.c_uint8(sub), is16)
        assert a == b, (trial, a, b)


@pytest.mark.parametrize("is16,bd,pli", [(0, 8, 0), (1, 10, 0), (0, 8, 1), (1, 10, 2)])
def test_cdef_search_and_apply_vs_filter_fb(orc, ref, is16, bd, pli):
    """Per filter block, orc_cdef_search_plane / orc_cdef_apply_plane must equal the reference's svt_cdef_filter_fb
    (+ svt_compute_cdef_dist) run on a tile built the way cdef_seg_search / svt_av1_cdef_frame build it."""
    rng = np.random.default_rng(10 + pli + bd)
    xdec = ydec = int(pli != 0)
    lw, lh = 200, 136                           # luma size: partial filter blocks at right / bottom
    w, h = lw >> xdec, lh >> ydec
    cs = bd - 8
    dt = np.uint16 if is16 else np.uint8
    recon = L.smooth_plane(rng, w + 11, h, bd).astype(dt)
    source = np.clip(recon.astype(np.int32) + rng.integers(-6, 7, size=recon.shape), 0, (1 << bd) - 1).astype(dt)
    w8, h8 = (lw + 7) // 8, (lh + 7) // 8
    filt = (rng.random((h8, w8)) < 0.7).astype(np.uint8)
    filt[0:8, 8:16] = 0                          # one filter block entirely skipped
    nhfb, nvfb = (lw + 63) // 64, (lh + 63) // 64
    strengths = [0, 5, 18, 35, 63, -1, 12]
    damping, sub = 5, 2
    prm = L.search_params(strengths, damping, cs, sub)
    pl = abi.CdefPlane(recon.ctypes.data, source.ctypes.data, w + 11, w + 11, w, h, is16, xdec, ydec, pli)
    mse = np.full((nhfb * nvfb, len(strengths)), 0xABCD, np.uint64)
    # luma direction data: chroma needs the luma pass first (run it on a luma plane of the same picture)
    ldir, lvar = np.zeros((nhfb * nvfb, 64), np.uint8), np.zeros((nhfb * nvfb, 64), np.int32)
    lrecon = L.smooth_plane(np.random.default_rng(99), lw + 5, lh, bd).astype(dt)
    lpl = abi.CdefPlane(lrecon.ctypes.data, lrecon.ctypes.data, lw + 5, lw + 5, lw, lh, is16, 0, 0, 0)
    lmse = np.zeros((nhfb * nvfb, len(strengths)), np.uint64)
    orc.orc_cdef_search_plane(C.byref(lpl if pli else pl), P(filt), C.byref(prm), P(lmse if pli else mse), P(ldir), P(lvar))
    if pli:
        orc.orc_cdef_search_plane(C.byref(pl), P(filt), C.byref(prm), P(mse), P(ldir), P(lvar))
    # ---- reference, filter block by filter block
    ffb = rtcd(ref, "svt_cdef_filter_fb", None, V, V, C.c_int32, V, C.c_int32, C.c_int32, V, V, V, C.c_int32, V, C.c_int32,
               C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint8) if False else ref.svt_cdef_filter_fb
    f16 = rtcd(ref, "svt_compute_cdef_dist_16bit", C.c_uint64, V, C.c_int32, V, V, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint8)
    f8 = rtcd(ref, "svt_compute_cdef_dist_8bit", C.c_uint64, V, C.c_int32, V, V, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint8)
    bsz = 0 if pli else 3
    eff_sub = min(sub, 4) if bsz == 3 else 1
    bw, bh = 64 >> xdec, 64 >> ydec
    out_apply = recon.copy()
    want_apply = recon.copy()
    fbs = np.array([strengths[(i * 3 + 1) % 5] for i in range(nhfb * nvfb)], np.uint8)
    orc.orc_cdef_apply_plane(C.byref(abi.CdefPlane(recon.ctypes.data, out_apply.ctypes.data, w + 11, w + 11, w, h, is16, xdec, ydec, pli)),
                             P(filt), P(fbs), damping, cs, P(ldir), P(lvar))
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
                assert (mse[fb] == 0xABCD).all()
                continue
            tile = np.full((64 + 2 * VB, BS), VL, np.uint16)
            for y in range(-VB, bh + VB):
                py = fby * bh + y
                if 0 <= py < h:
                    x0, x1 = max(fbx * bw - HB, 0), min(fbx * bw + bw + HB, w)
                    tile[VB + y, HB + x0 - fbx * bw:HB + x1 - fbx * bw] = recon[py, x0:x1]
            inp = tile.ctypes.data + 2 * (VB * BS + HB)
            d = np.ascontiguousarray(ldir[fb].reshape(8, 8))
            d16 = np.zeros((16, 16), np.uint8)
            d16[:8, :8] = d
            v16 = np.zeros((16, 16), np.int32)
            v16[:8, :8] = lvar[fb].reshape(8, 8)
            for gi, s in enumerate(strengths):
                if s < 0:
                    assert mse[fb, gi] == 0xABCD
                    continue
                pri, sec = s // 4, s % 4
                tmp = np.zeros(64 * 64, np.uint16)
                dirinit = C.c_int32(1)
                ref.svt_cdef_filter_fb(None if is16 else P(tmp), P(tmp) if is16 else None, 0, V(inp), xdec, ydec, P(d16), C.byref(dirinit),
                                       P(v16), pli, C.byref(dl), n, pri, sec + (sec == 3), damping, damping, cs, C.c_uint8(eff_sub))
                soff = (fby * bh) * (w + 11) + fbx * bw
                m = (f16 if is16 else f8)(source.ctypes.data + soff * source.itemsize, w + 11, tmp.ctypes.data, C.addressof(dl), n, bsz, cs, pli, eff_sub)
                assert mse[fb, gi] == m * eff_sub, (fb, gi, mse[fb, gi], m)
            # apply
            s = int(fbs[fb])
            pri, sec = s // 4, s % 4
            if pri or sec:
                dirinit = C.c_int32(1)
                dst = want_apply.ctypes.data + ((fby * bh) * (w + 11) + fbx * bw) * recon.itemsize
                ref.svt_cdef_filter_fb(None if is16 else V(dst), V(dst) if is16 else None, w + 11, V(inp), xdec, ydec, P(d16), C.byref(dirinit),
                                       P(v16), pli, C.byref(dl), n, pri, sec + (sec == 3), damping, damping, cs, C.c_uint8(1))
    assert np.array_equal(out_apply[:, :w], want_apply[:, :w])


def content_search(orc, kind, bd, is16, strengths, lw=136, lh=72, fmt=420, filt_kind="ones", seed=40):
    """Oracle search of one harsh-content picture (lf_cases.content_planes): (planes, filt, [mse per plane], dir, var)."""
    n_fb = ((lw + 63) // 64) * ((lh + 63) // 64)
    planes, filt = L.content_planes(kind, lw, lh, bd, is16, fmt, seed), L.content_filt(lw, lh, filt_kind, seed)
    prm = L.search_params(strengths, 5, bd - 8, 1)
    ldir, lvar = np.zeros((n_fb, 64), np.uint8), np.zeros((n_fb, 64), np.int32)
    out = []
    for pli, xdec, ydec, w, h, recon, source in planes:
        st = recon.shape[1]
        mse = np.full((n_fb, len(strengths)), 0xABCD, np.uint64)
        orc.orc_cdef_search_plane(C.byref(abi.CdefPlane(recon.ctypes.data, source.ctypes.data, st, st, w, h, is16, xdec, ydec, pli)),
                                  P(filt), C.byref(prm), P(mse), P(ldir), P(lvar))
        out.append(mse)
    return planes, filt, out, ldir, lvar


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1)])
def test_cdef_content_conditions(orc, bd, is16):
    """Conditions on the INPUTS of the whole-picture content tests (test_gpu_lf.py), asserted on the oracle alone: `oriented`
    spreads the real luma 8x8 blocks over all eight directions (at least 8 % each) and gives every luma filter block at least 32
    distinct mse values over the 64 strengths; `noise` reaches every direction.  If a re-seeded generator misses these, change the
    generator, not the bounds."""
    lw, lh = 136, 72
    _, _, mse, ldir, _ = content_search(orc, "oriented", bd, is16, list(range(64)))
    d = L.real_blocks(ldir, lw, lh)
    assert d.size == 17 * 9
    hist = np.bincount(d, minlength=8)
    assert (hist >= 0.08 * d.size).all(), hist
    for fb in range(mse[0].shape[0]):
        assert len(set(mse[0][fb].tolist())) >= 32, (fb, mse[0][fb])
    _, _, _, ldir, _ = content_search(orc, "noise", bd, is16, [0])
    assert (np.bincount(L.real_blocks(ldir, lw, lh), minlength=8) > 0).all()


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1)])
@pytest.mark.parametrize("kind", L.CONTENTS)
def test_cdef_content_vs_reference(orc, ref, kind, bd, is16):
    """The oracle's search and apply on every harsh content against the reference's own per-filter-block functions
    (lf_cases.ref_cdef_plane): pins the oracle for the inputs on which it judges the GPU kernels."""
    lw, lh, damping, cs = 136, 72, 5, bd - 8
    strengths = L.STRENGTHS16
    planes, filt, mse, ldir, lvar = content_search(orc, kind, bd, is16, strengths, filt_kind="map")
    n_fb = mse[0].shape[0]
    fbs = np.array([2, 37, 63, 0, 1, 22], np.uint8)
    rdir, rvar = np.zeros((n_fb, 64), np.uint8), np.zeros((n_fb, 64), np.int32)
    for (pli, xdec, ydec, w, h, recon, source), m in zip(planes, mse):
        want_mse, want = L.ref_cdef_plane(ref, recon, source, w, h, is16, xdec, ydec, pli, filt, strengths, fbs, damping, cs, 1, rdir, rvar)
        st = recon.shape[1]
        out = np.zeros_like(recon)
        orc.orc_cdef_apply_plane(C.byref(abi.CdefPlane(recon.ctypes.data, out.ctypes.data, st, st, w, h, is16, xdec, ydec, pli)),
                                 P(filt), P(fbs), damping, cs, P(ldir), P(lvar))
        assert np.array_equal(m, want_mse), (pli, np.argwhere(m != want_mse)[:5])
        assert np.array_equal(out[:, :w], want[:, :w]), pli
        if pli == 0:
            assert np.array_equal(ldir, rdir) and np.array_equal(lvar, rvar)


def test_cdef_oracle_vs_golden(orc):
    """No reference needed: the committed fixture (made by the reference, tests/golden/make_golden_lf.py) pins the oracle."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cdef.npz"))
    keys = sorted(k[:-6] for k in g.files if k.endswith("_recon"))
    assert len(keys) == 3 * len(L.GOLDEN_CDEF)
    for key in keys:
        recon, source, filt = g[key + "_recon"].copy(), g[key + "_source"].copy(), g[key + "_filt"].copy()
        w, h, is16, xdec, ydec, pli, damping, cs, sub = (int(v) for v in g[key + "_meta"])
        prm = L.search_params([int(s) for s in g[key + "_strengths"]], damping, cs, sub)
        n_fb = g[key + "_mse"].shape[0]
        ldir, lvar = g[key + "_dir"].copy(), g[key + "_var"].copy()
        if pli == 0:
            ldir[:], lvar[:] = 0, 0
        mse = np.full((n_fb, prm.n_strengths), 0xABCD, np.uint64)
        out = np.zeros_like(recon)
        fbs = g[key + "_fbs"].copy()
        st = recon.shape[1]
        orc.orc_cdef_search_plane(C.byref(abi.CdefPlane(recon.ctypes.data, source.ctypes.data, st, st, w, h, is16, xdec, ydec, pli)),
                                  P(filt), C.byref(prm), P(mse), P(ldir), P(lvar))
        orc.orc_cdef_apply_plane(C.byref(abi.CdefPlane(recon.ctypes.data, out.ctypes.data, st, st, w, h, is16, xdec, ydec, pli)),
                                 P(filt), P(fbs), damping, cs, P(ldir), P(lvar))
        assert np.array_equal(mse, g[key + "_mse"]), key
        assert np.array_equal(out[:, :w], g[key + "_applied"][:, :w]), key
        assert np.array_equal(ldir, g[key + "_dir"]) and np.array_equal(lvar, g[key + "_var"]), key


# ------------------------------------------------------------------------------------------------ deblocking
LPF = [(d, n) for d in ("horizontal", "vertical") for n in (4, 6, 8, 14)]


def lpf_block(rng, bd, trial):
    """A 16x16 neighbourhood around an edge: flat, stepped or noisy so all three filter branches are hit."""
    base = int(rng.integers(16 << (bd - 8), 240 << (bd - 8)))
    a = np.full((16, 16), base, np.int32)
    kind = trial % 4
    if kind == 0:
        a += rng.integers(-1, 2, size=a.shape) * (1 << (bd - 8))
        a[:, 8:] += int(rng.integers(-3, 4)) << (bd - 8)
    elif kind == 1:
        a[:, 8:] += int(rng.integers(-12, 13)) << (bd - 8)
        a += rng.integers(-2, 3, size=a.shape) << (bd - 8)
    elif kind == 2:
        a += rng.integers(-30, 31, size=a.shape) << (bd - 8)
    else:
        a = rng.integers(0, 1 << bd, size=a.shape)
    return np.clip(a, 0, (1 << bd) - 1)


@pytest.mark.parametrize("d,n", LPF)
def test_lpf_leaves(orc, ref, d, n):
    rng = np.random.default_rng(n + (d == "vertical"))
    f8 = L.rtcd(ref, f"svt_aom_lpf_{d}_{n}", None, V, C.c_int32, V, V, V)
    f16 = L.rtcd(ref, f"svt_aom_highbd_lpf_{d}_{n}", None, V, C.c_int32, V, V, V, C.c_int32)
    for trial in range(400):
        bd = (8, 10, 8, 12, 10)[trial % 5]      # 5 and the 4 kinds of lpf_block: every depth meets every kind
        is16 = int(trial % 5 != 0)
        a = lpf_block(rng, bd, trial)
        if d == "horizontal":
            a = a.T
        a = np.ascontiguousarray(a).astype(np.uint16 if is16 else np.uint8)
        level, sharp = int(rng.integers(0, 64)), int(rng.integers(0, 8))
        lim, mblim, hev = C.c_int(), C.c_int(), C.c_int()
        orc.orc_lf_thresholds(level, sharp, C.byref(lim), C.byref(mblim), C.byref(hev))
        th = [np.full(16, v.value, np.uint8) for v in (mblim, lim, hev)]
        b = a.copy()
        off = (8 * 16 + 4) if d == "horizontal" else (4 * 16 + 8)
        if is16:
            f16(a.ctypes.data + 2 * off, 16, P(th[0]), P(th[1]), P(th[2]), bd)
        else:
            f8(a.ctypes.data + off, 16, P(th[0]), P(th[1]), P(th[2]))
        orc.orc_lpf(V(b.ctypes.data + off * b.itemsize), 16, mblim.value, lim.value, hev.value, bd, is16, n, int(d == "vertical"))
        assert np.array_equal(a, b), (d, n, trial)


def test_lf_thresholds(orc, ref):
    """orc_lf_thresholds against the lfthr table svt_av1_loop_filter_init builds (read back through a frame run)."""
    # indirectly covered by test_loop_filter_frame (every level/sharpness pair used there goes through the real table);
    # here: the closed form for all 64 x 8 combinations against the published AV1 formula values at the corners.
    lim, mblim, hev = C.c_int(), C.c_int(), C.c_int()
    for level, sharp, want in ((0, 0, (1, 5, 0)), (63, 0, (63, 193, 3)), (63, 7, (2, 132, 3)), (32, 4, (5, 73, 2)), (10, 5, (2, 26, 0))):
        orc.orc_lf_thresholds(level, sharp, C.byref(lim), C.byref(mblim), C.byref(hev))
        assert (lim.value, mblim.value, hev.value) == want


@pytest.mark.parametrize("variant", range(8))
def test_loop_filter_frame(orc, ref, variant):
    """Whole-frame deblocking: oracle vs the REAL svt_av1_loop_filter_frame on random partitions."""
    rng = np.random.default_rng(100 + variant)
    w, h = ((200, 136), (328, 184), (64, 64), (136, 264), (196, 134), (322, 182), (264, 200), (130, 258))[variant]
    bd, is16 = ((8, 0), (10, 1), (8, 1))[variant % 3]
    sb = 128 if variant == 6 else 64
    mi_cols, mi_rows = (w + 7) // 8 * 2, (h + 7) // 8 * 2
    mi_stride = mi_cols + 3
    minfo = L.random_mode_info(rng, mi_rows, mi_cols, mi_stride, sb=sb)
    hdr = L.lf_header(rng, variant)
    planes = L.lf_planes(rng, mi_cols * 4, mi_rows * 4, bd, is16)
    p_ref = [p.copy() for p in planes]
    p_orc = [p.copy() for p in planes]
    ps, pe = (0, 3) if variant != 4 else (1, 3)
    flat, lvl = L.ref_deblock(ref, p_ref, w, h, minfo, mi_stride, mi_rows, mi_cols, hdr, bd, is16, sb, ps, pe)
    f = L.lf_frame(p_orc, w, h, flat.ctypes.data, mi_stride, mi_rows, mi_cols, hdr, bd, is16, ps, pe, lvl)
    orc.orc_loop_filter_frame(C.byref(f), sb)
    changed = 0
    for a, b, o in zip(p_ref, p_orc, planes):
        assert np.array_equal(a, b), np.argwhere(a != b)[:5]
        changed += int((a != o).sum())
    assert (changed > 0) == (variant != 7)


def test_loop_filter_oracle_vs_golden(orc):
    """No reference needed: tests/golden/dlf.npz (made by the real svt_av1_loop_filter_frame) pins the oracle."""
    n = 0
    for key, w, h, bd, is16, mi_cols, mi_rows, mi_stride, flat, lvl, hdr, planes, want in L.golden_dlf_cases():
        f = L.lf_frame(planes, w, h, flat.ctypes.data, mi_stride, mi_rows, mi_cols, hdr, bd, is16, 0, 3, lvl)
        orc.orc_loop_filter_frame(C.byref(f), 64)      # the schedule's SB size does not change the result
        for a, b in zip(planes, want):
            assert np.array_equal(a, b), key
        n += 1
    assert n == len(L.GOLDEN_DLF)


# ---- the catalogue partition and the range-end contents (lf_cases.CatalogueCase): conditions on the inputs, then the pin
_TXW_LOG2 = np.array([L.TXW[t].bit_length() - 1 for t in range(19)])
_TXH_LOG2 = np.array([L.TXH[t].bit_length() - 1 for t in range(19)])
_BW_LOG2 = np.array([L.BW[b].bit_length() - 1 for b in range(22)])
_BH_LOG2 = np.array([L.BH[b].bit_length() - 1 for b in range(22)])


def edge_census(c, plane, d, lvl=None):
    """set_lpf_parameters (deblocking_filter.c:162-282) restated in numpy for every 4-sample unit of one plane and direction
    (d 0: vertical edges) of a CatalogueCase: a dict of arrays [units down][units across] - `edge` the unit starts a transform
    and is not at the picture's border, `filtered` / `refused` of those with a level (refused: both sides skipped inter blocks and
    no block edge), `cur` / `prev` the transform sizes on both sides, `lc` / `lp` their levels, `len` and `level` of the filter."""
    ss = int(plane > 0)
    nx, ny = ((c.w >> ss) + 3) // 4, ((c.h >> ss) + 3) // 4
    rows, cols = ss | (np.arange(ny) * 4 << ss >> 2), ss | (np.arange(nx) * 4 << ss >> 2)
    mi = c.flat[np.ix_(rows, cols)]
    pv = c.flat[np.ix_(rows - (d == 1) * (1 << ss), cols - (d == 0) * (1 << ss))]      # wraps at coordinate 0, where no edge is
    coord = (np.arange(nx) * 4)[None, :] if d == 0 else (np.arange(ny) * 4)[:, None]
    key = "tx_size_uv" if plane else "tx_size_y"
    log2 = _TXW_LOG2 if d == 0 else _TXH_LOG2
    ts, pv_ts = log2[mi[key]], log2[pv[key]]
    table = (c.lvl if lvl is None else lvl).reshape(3, 8, 2, 8, 2)
    lc = table[plane, mi["segment_id"], d, mi["ref_frame0"], mi["mode_lf"]].astype(int)
    lp = table[plane, pv["segment_id"], d, pv["ref_frame0"], pv["mode_lf"]].astype(int)
    bdim = (_BW_LOG2 if d == 0 else _BH_LOG2)[mi["bsize"]]
    if ss:
        bdim = np.maximum(bdim - 1, 2)
    edge = ((coord & ((1 << ts) - 1)) == 0) & (coord > 0)
    pu_edge = (coord & ((1 << bdim) - 1)) == 0
    allowed = (pv["skip_inter"] == 0) | (mi["skip_inter"] == 0) | pu_edge
    on = edge & ((lc != 0) | (lp != 0))
    min_ts = np.minimum(ts, pv_ts)
    length = np.where(min_ts <= 2, 4, np.where(plane > 0, 6, np.where(min_ts == 3, 8, 14)))
    return dict(edge=edge, filtered=on & allowed, refused=on & ~allowed, cur=mi[key], prev=pv[key], lc=lc, lp=lp, len=length,
                level=np.where(lc != 0, lc, lp))


def branch_census(c, plane, d):
    """The branch each of the four lines of every filtered edge takes on the UNFILTERED picture (filter_mask / hev_mask /
    flat_mask of deblocking_common.c restated): the set of (length, branch), branch one of nomask, hev, nohev, flat, flat2."""
    e = edge_census(c, plane, d)
    uy, ux = np.nonzero(e["filtered"])
    if not uy.size:
        return set()
    pic = c.planes[plane].astype(np.int64)
    along, k = np.arange(4)[None, :, None], np.arange(-7, 7)[None, None, :]
    y0, x0 = (L.PAD + uy * 4)[:, None, None], (L.PAD + ux * 4)[:, None, None]
    s = pic[y0 + along, x0 + k] if d == 0 else pic[y0 + k, x0 + along]                 # [edge][line][p6 .. p0 q0 .. q6]
    p, q = (lambda i: s[:, :, 6 - i]), (lambda i: s[:, :, 7 + i])
    level, sharp, sh = e["level"][uy, ux], c.hdr.sharpness_level, c.bd - 8
    inside = level >> (int(sharp > 0) + int(sharp > 4))                                 # svt_aom_update_sharpness
    if sharp > 0:
        inside = np.minimum(inside, 9 - sharp)
    inside = np.maximum(inside, 1)
    lim, blim, thr = ((v << sh)[:, None] for v in (inside, 2 * (level + 2) + inside, level >> 4))
    one, n = 1 << sh, e["len"][uy, ux][:, None]
    a = np.abs
    mask = ~((a(p(1) - p(0)) > lim) | (a(q(1) - q(0)) > lim) | (a(p(0) - q(0)) * 2 + a(p(1) - q(1)) // 2 > blim))
    mask &= (n < 6) | ~((a(p(2) - p(1)) > lim) | (a(q(2) - q(1)) > lim))
    mask &= (n < 8) | ~((a(p(3) - p(2)) > lim) | (a(q(3) - q(2)) > lim))
    flat = (n >= 6) & ~((a(p(1) - p(0)) > one) | (a(q(1) - q(0)) > one) | (a(p(2) - p(0)) > one) | (a(q(2) - q(0)) > one))
    flat &= (n < 8) | ~((a(p(3) - p(0)) > one) | (a(q(3) - q(0)) > one))
    flat2 = (n == 14) & ~np.any([(a(p(i) - p(0)) > one) | (a(q(i) - q(0)) > one) for i in (4, 5, 6)], axis=0)
    hev = (a(p(1) - p(0)) > thr) | (a(q(1) - q(0)) > thr)
    branch = np.where(mask & flat & flat2, 4, np.where(mask & flat, 3, np.where(~mask, 0, np.where(hev, 1, 2))))
    names = ("nomask", "hev", "nohev", "flat", "flat2")
    return {(int(ln), names[b]) for ln, b in set(zip(np.broadcast_to(n, branch.shape).ravel().tolist(), branch.ravel().tolist()))}


BRANCHES = {4: ("nomask", "hev", "nohev"), 6: ("nomask", "hev", "nohev", "flat"), 8: ("nomask", "hev", "nohev", "flat"),
            14: ("nomask", "hev", "nohev", "flat", "flat2")}
_cases = {}


def cached(make, *args):
    """One CatalogueCase per argument list for the whole session, left unchanged by its users."""
    if (make, args) not in _cases:
        _cases[(make, args)] = make(*args)
    return _cases[(make, args)]


def blocks_of(minfo):
    return set(zip(minfo["bsize"].ravel().tolist(), minfo["tx_depth"].ravel().tolist(),
                   ((minfo["skip"] != 0) & (minfo["ref_frame0"] > 0)).ravel().tolist()))


def tx_census(c):
    """{(plane kind, direction, side): transform sizes seen on that side of a filtered edge}."""
    out = {}
    for plane in (0, 1, 2):
        for d in (0, 1):
            e = edge_census(c, plane, d)
            for side in ("cur", "prev"):
                out.setdefault((min(plane, 1), d, side), set()).update(e[side][e["filtered"]].tolist())
    return out


@pytest.mark.parametrize("sb", [64, 128])
def test_catalogue_partition(sb):
    """catalogue_mode_info holds every block size that fits the superblock with every depth it can have - at 264 x 200 for
    superblock 64, on a 512 x 384 grid for 128, where 264 x 200 has room for eight whole 64x64 regions only - and, for 128 at
    264 x 200, the three blocks above 64 samples as skipped inter blocks.  It is deterministic but for the seeded fields."""
    w, h = (264, 200) if sb == 64 else (512, 384)
    mi_cols, mi_rows = w // 4, h // 4
    m = L.catalogue_mode_info(mi_rows, mi_cols, mi_cols + 3, sb, 1)
    have = blocks_of({k: v[:, :mi_cols] for k, v in m.items()})
    for (bw, bh), b in L.BSIZE.items():
        if max(bw, bh) <= sb:
            for depth in range(L.max_depth_of(b) + 1):
                assert any(x[:2] == (b, depth) for x in have), (bw, bh, depth)
    m2 = L.catalogue_mode_info(mi_rows, mi_cols, mi_cols + 3, sb, 2)
    assert np.array_equal(m["bsize"], m2["bsize"]) and np.array_equal(m["tx_depth"], m2["tx_depth"])
    assert not np.array_equal(m["segment_id"], m2["segment_id"])
    if sb == 128:
        small = L.catalogue_mode_info(50, 66, 69, 128, 1)
        for size in ((128, 128), (128, 64), (64, 128)):
            assert (L.BSIZE[size], 0, True) in blocks_of(small), size


@pytest.mark.parametrize("bd,is16,sb,variant", L.CATALOGUE_PARAMS)
def test_catalogue_conditions(bd, is16, sb, variant):
    """Conditions on the INPUTS of every case of test_tier_b_deblock_catalogue (test_gpu_lf.py), from the mode info and the level
    table alone: per direction each of the 19 luma and 14 chroma transform sizes is the current unit of a filtered edge and the
    previous unit of one; superblock 128 has a luma transform edge refused because both sides are skipped inter blocks and it is
    no block edge, inside a block above 64 samples; an edge with level 0 takes its neighbour's, another has none.  If a changed
    catalogue or seed misses these, change that, not the conditions."""
    c = cached(L.catalogue_case, bd, is16, sb, variant)
    for (kind, d, side), seen in tx_census(c).items():
        want = set(L.TX_UV) if kind else set(range(19))
        assert seen == want, (kind, d, side, sorted(want - seen))
    e = [edge_census(c, plane, d) for plane in range(3) for d in (0, 1)]
    if sb == 128:
        big = np.isin(c.flat["bsize"], [L.BSIZE[s] for s in ((128, 128), (128, 64), (64, 128))])[:, :c.mi_cols]
        assert (c.flat["skip_inter"][:, :c.mi_cols][big] == 1).any() and (c.flat["tx_size_y"][:, :c.mi_cols][big] == L.TX[(64, 64)]).all()
        ny, nx = e[0]["refused"].shape
        assert sum(int((x["refused"] & big[:ny, :nx]).sum()) for x in e[:2]) > 0
    assert any((x["edge"] & (x["lc"] == 0) & (x["lp"] != 0)).any() for x in e)
    assert any((x["edge"] & (x["lc"] == 0) & (x["lp"] == 0)).any() for x in e)


def test_catalogue_conditions_need_the_catalogue():
    """The same census on random_mode_info partitions of the same picture misses transform sizes, whatever the seed: the
    conditions above do guard the catalogue."""
    c = L.catalogue_case(10, 1, 64, 1)
    for seed in range(4):
        c.minfo = L.random_mode_info(np.random.default_rng(seed), c.mi_rows, c.mi_cols, c.mi_stride, sb=64)
        c.flat = L.flat_mode_info(c.minfo, c.mi_rows, c.mi_stride)
        assert any(seen != (set(L.TX_UV) if kind else set(range(19))) for (kind, d, side), seen in tx_census(c).items()), seed


def range_ends(before, after, top):
    """Counts of samples the filter changed: that ended at 0, at the top value, that started at 0, at the top value."""
    ch = before != after
    return [int((ch & (after == 0)).sum()), int((ch & (after == top)).sum()), int((ch & (before == 0)).sum()), int((ch & (before == top)).sum())]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_deblock_content_conditions(orc, bd):
    """Conditions on the INPUTS of test_tier_b_deblock_content and _catalogue, per bit depth, from the inputs and the oracle's
    outputs: over these cases together every (luma / chroma, direction, length, branch) occurs (the horizontal pass taken on
    the unfiltered picture: a census of the inputs, not a check of outputs); `low` and `ends` have changed samples that end
    at 0 and others that started there, `high` and `ends` the same at the top value, on both sizes; at 130 x 258 every case
    has non-zero levels and changes samples in all three planes."""
    top = (1 << bd) - 1
    seen = {}
    cases = [(kind, cached(L.lf_content_case, kind, b, is16, w, h)) for kind, b, is16, w, h, ps in L.LF_CONTENT_PARAMS if b == bd and ps == 0]
    cases += [(None, cached(L.catalogue_case, b, is16, sb, v)) for b, is16, sb, v in L.CATALOGUE_PARAMS if b == bd and v == 1]
    for kind, c in cases:
        for plane in range(3):
            for d in (0, 1):
                seen.setdefault((min(plane, 1), d), set()).update(branch_census(c, plane, d))
        if kind is None:
            continue
        out = c.oracle(orc)
        ends = np.sum([range_ends(a, b, top) for a, b in zip(c.planes, out)], axis=0)
        if kind in ("low", "ends"):
            assert ends[0] > 0 and ends[2] > 0, (kind, c.w, ends)
        if kind in ("high", "ends"):
            assert ends[1] > 0 and ends[3] > 0, (kind, c.w, ends)
        if c.w == 130:
            assert c.w % 4 and c.lvl.any() and all((a != b).any() for a, b in zip(c.planes, out)), kind
    for (kind, d), got in seen.items():
        want = {(n, b) for n in ((4, 6) if kind else (4, 8, 14)) for b in BRANCHES[n]}
        assert got == want, (kind, d, sorted(want - got))


def test_deblock_content_conditions_need_the_content(orc):
    """With lf_planes in place of the range-end contents no changed sample ends or starts at either end of the range."""
    for bd, is16 in ((8, 0), (10, 1), (12, 1)):
        c = L.CatalogueCase(200, 136, bd, is16, 64, 0, None, 100 + bd + 200)
        assert not np.sum([range_ends(a, b, (1 << bd) - 1) for a, b in zip(c.planes, c.oracle(orc))]), bd


@pytest.mark.parametrize("bd,is16,sb,variant", L.CATALOGUE_PARAMS)
def test_loop_filter_frame_catalogue(orc, ref, bd, is16, sb, variant):
    """The oracle against the REAL svt_av1_loop_filter_frame on every case of the catalogue partition, 12 bit through the same
    frame call (the reference hands encoder_bit_depth to its highbd filters).  The mode info is the reference's own gather
    (tx_depth_to_tx_size, av1_get_max_uv_txsize), and flat_mode_info must equal it.  The level table is the one the reference
    derives from the case's header: the reference takes no table, so the random one of the GPU test is not pinned here."""
    c = cached(L.catalogue_case, bd, is16, sb, variant)
    p_ref = [p.copy() for p in c.planes]
    flat, lvl = L.ref_deblock(ref, p_ref, c.w, c.h, c.minfo, c.mi_stride, c.mi_rows, c.mi_cols, c.hdr, bd, is16, sb)
    assert flat.tobytes() == c.flat.tobytes()
    p_orc = [p.copy() for p in c.planes]
    orc.orc_loop_filter_frame(C.byref(c.frame(p_orc, flat.ctypes.data, lvl=lvl)), sb)
    for a, b, o in zip(p_ref, p_orc, c.planes):
        assert np.array_equal(a, b), np.argwhere(a != b)[:5]
        assert (a != o).any()


@pytest.mark.parametrize("kind,bd,is16,w,h,ps", L.LF_CONTENT_PARAMS)
def test_loop_filter_frame_content(orc, ref, kind, bd, is16, w, h, ps):
    """The same on the range-end contents, 130 x 258 and the chroma-only plane range included.  With the reference's level
    table too the changed samples reach the end of the range they are named for, so the clamps are pinned where they act."""
    c = cached(L.lf_content_case, kind, bd, is16, w, h)
    p_ref = [p.copy() for p in c.planes]
    flat, lvl = L.ref_deblock(ref, p_ref, w, h, c.minfo, c.mi_stride, c.mi_rows, c.mi_cols, c.hdr, bd, is16, c.sb, ps, 3)
    assert flat.tobytes() == c.flat.tobytes()
    p_orc = [p.copy() for p in c.planes]
    orc.orc_loop_filter_frame(C.byref(c.frame(p_orc, flat.ctypes.data, ps, 3, lvl)), c.sb)
    for i, (a, b, o) in enumerate(zip(p_ref, p_orc, c.planes)):
        assert np.array_equal(a, b), np.argwhere(a != b)[:5]
        assert (a != o).any() == (i >= ps)
    ends = np.sum([range_ends(o, a, (1 << bd) - 1) for o, a in zip(c.planes, p_ref)], axis=0)
    assert kind not in ("low", "ends") or (ends[0] > 0 and ends[2] > 0), ends
    assert kind not in ("high", "ends") or (ends[1] > 0 and ends[3] > 0), ends
