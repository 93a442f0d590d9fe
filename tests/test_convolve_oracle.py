"""CPU: the single-reference interpolation oracle against the REAL reference functions (oracle/_ref RTCD pointers)."""
import ctypes as C

import numpy as np
import pytest

import conv_cases as K
import lf_cases as L
from lf_cases import P, V
from test_wiener_oracle import ConvolveParams


def test_kernel_tables_match_reference(ref):
    for name, tab in K.TABLES.items():
        got = np.frombuffer((C.c_int16 * 128).in_dll(ref, name), np.int16).reshape(16, 8)
        assert np.array_equal(got, np.array(tab, np.int16)), name


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1), (12, 1)])
def test_convolve_sr(orc, ref, bd, is16):
    rng = np.random.default_rng(120 + bd)
    r0, r1 = K.conv_rounds(bd)
    sig8 = (V, C.c_int32, V, C.c_int32, C.c_int32, C.c_int32, V, V, C.c_int32, C.c_int32, V)
    fns = {}
    for mode in ("2d_sr", "x_sr", "y_sr", "2d_copy_sr"):
        name = f"svt_av1_highbd_convolve_{mode}" if is16 else f"svt_av1_convolve_{mode}"
        fns[mode] = L.rtcd(ref, name, None, *(sig8 + ((C.c_int32,) if is16 else ())))
    tabs = {n: K.kernel_table(n) for n in K.TABLES}
    for trial in range(66):
        w, h = K.SIZES[trial % len(K.SIZES)]
        name = list(K.TABLES)[trial % 3]
        tab = tabs[name][0]
        sx, sy = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        mode = ("2d_sr", "x_sr", "y_sr", "2d_copy_sr")[trial % 4]
        plane, at = K.ref_plane(rng, w, h, bd, is16, (0, 2, 1)[trial % 3])
        fp = K.InterpFilterParams(tab.ctypes.data, 8, 16, trial % 3)
        cp = ConvolveParams(round_0=r0, round_1=r1)
        o1, o2 = np.zeros((h, w + 3), plane.dtype), np.zeros((h, w + 3), plane.dtype)
        args = [V(at), plane.shape[1], P(o1), w + 3, w, h, C.byref(fp), C.byref(fp), sx, sy, C.byref(cp)] + ([bd] if is16 else [])
        fns[mode](*args)
        tx = 8 if mode in ("2d_sr", "x_sr") else 0
        ty = 8 if mode in ("2d_sr", "y_sr") else 0
        orc.orc_convolve_sr(V(at), plane.shape[1], P(o2), w + 3, w, h, V(tab[sx].ctypes.data), tx, V(tab[sy].ctypes.data), ty, r0, r1, bd, is16)
        assert np.array_equal(o1, o2), (trial, mode, w, h, sx, sy)
    # the extended cases: every table, x table != y table, every block shape, taps 2 / 4 / 6, the adversarial planes
    fns = [fns[m + "_sr"] for m in K.MODES]
    rng, n = np.random.default_rng(4120 + bd), 0
    for i, c in enumerate(K.ext_cases(bd)):
        plane, at = K.ext_plane(rng, c)
        o1, o2 = ext_run_fn_sr(fns, c, plane, at, ConvolveParams, K.InterpFilterParams), ext_run_orc_sr(orc, c, plane, at)
        assert np.array_equal(o1, o2), (i, c)
        n += 1
    print(f"convolve_sr bd {bd}: {n} extended cases")


def ext_filters(c):
    """the x and y tables of a case as its InterpFilterParams' taps see them: [16][taps]"""
    return K.narrow_table(c.tx, c.taps[0]), K.narrow_table(c.ty, c.taps[1])


def ext_run_orc_sr(orc, c, plane, at):
    """one extended case through the oracle; the result keeps 3 columns of padding, which must stay as they were"""
    tabx, taby = ext_filters(c)
    r0, r1 = K.conv_rounds(c.bd)
    o = np.full((c.h, c.w + 3), 0xA5, plane.dtype)
    orc.orc_convolve_sr(V(at), plane.shape[1], P(o), c.w + 3, c.w, c.h, V(tabx[c.sx].ctypes.data), c.use[0], V(taby[c.sy].ctypes.data), c.use[1],
                        r0, r1, c.bd, c.is16)
    return o


def ext_run_fn_sr(fns, c, plane, at, CP, FP):
    """the same through functions with the reference's signatures, fns[mode] (the reference's own, or the HIP Tier A leaves)"""
    tabx, taby = ext_filters(c)
    r0, r1 = K.conv_rounds(c.bd)
    fx, fy = FP(tabx.ctypes.data, c.taps[0], 16, 0), FP(taby.ctypes.data, c.taps[1], 16, 0)
    cp = CP(round_0=r0, round_1=r1)
    o = np.full((c.h, c.w + 3), 0xA5, plane.dtype)
    fns[c.mode](*([V(at), plane.shape[1], P(o), c.w + 3, c.w, c.h, C.byref(fx), C.byref(fy), c.sx, c.sy, C.byref(cp)] + ([c.bd] if c.is16 else [])))
    return o


def ext_run_orc_jnt(orc, c, p0, a0, p1, a1, avg, fwd, bck):
    """both predictions of an extended compound case through the oracle (the same kernels for both references): returns
    (conv buffer after the first, pixels after the second), both with padding columns"""
    tabx, taby = ext_filters(c)
    r0, r1 = K.conv_rounds_compound(c.bd)
    cb, out = np.full((c.h, c.w + 5), 0xA5A5, np.uint16), np.full((c.h, c.w + 3), 0xA5, p0.dtype)
    for at, plane, comp in ((a0, p0, 1), (a1, p1, avg)):
        orc.orc_convolve_jnt(V(at), plane.shape[1], P(out), c.w + 3, c.w, c.h, V(tabx[c.sx].ctypes.data), c.use[0], V(taby[c.sy].ctypes.data),
                             c.use[1], r0, r1, c.bd, c.is16, P(cb), c.w + 5, comp, fwd, bck)
        if comp == 1:
            first = cb.copy()
    return first, out


def ext_run_fn_jnt(fns, c, p0, a0, p1, a1, avg, fwd, bck, CP, FP):
    tabx, taby = ext_filters(c)
    r0, r1 = K.conv_rounds_compound(c.bd)
    cb, out = np.full((c.h, c.w + 5), 0xA5A5, np.uint16), np.full((c.h, c.w + 3), 0xA5, p0.dtype)
    fx, fy = FP(tabx.ctypes.data, c.taps[0], 16, 0), FP(taby.ctypes.data, c.taps[1], 16, 0)
    cp = CP(do_average=0, dst=cb.ctypes.data, dst_stride=c.w + 5, round_0=r0, round_1=r1, is_compound=1)
    tail = [c.bd] if c.is16 else []
    fns[c.mode](*([V(a0), p0.shape[1], P(out), c.w + 3, c.w, c.h, C.byref(fx), C.byref(fy), c.sx, c.sy, C.byref(cp)] + tail))
    first, dst_after_first = cb.copy(), out.copy()
    cp.do_average, cp.use_jnt_comp_avg, cp.fwd_offset, cp.bck_offset = 1, int(avg == 3), fwd, bck
    fns[c.mode](*([V(a1), p1.shape[1], P(out), c.w + 3, c.w, c.h, C.byref(fx), C.byref(fy), c.sx, c.sy, C.byref(cp)] + tail))
    assert (dst_after_first == 0xA5).all(), "the first prediction of a compound wrote pixels"
    assert np.array_equal(cb, first), "the second prediction of a compound wrote the conv buffer"
    return first, out


def test_convolve_oracle_vs_golden(orc):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convolve.npz"))
    for i in range(int(g["n"])):
        bd, is16, w, h, mode, ti, sx, sy = (int(v) for v in g[f"c{i}_meta"])
        plane = g[f"c{i}_plane"].copy()
        at = plane.ctypes.data + (8 * plane.shape[1] + 8) * plane.itemsize
        tab = np.array(K.TABLES[list(K.TABLES)[ti]], np.int16)
        r0, r1 = K.conv_rounds(bd)
        o = np.zeros((h, w), plane.dtype)
        tx, ty = (8 if mode in (0, 1) else 0), (8 if mode in (0, 2) else 0)
        orc.orc_convolve_sr(V(at), plane.shape[1], P(o), w, w, h, V(tab[sx].ctypes.data), tx, V(tab[sy].ctypes.data), ty, r0, r1, bd, is16)
        assert np.array_equal(o, g[f"c{i}_out"]), i


def run_orc_jnt(orc, c, bd, is16):
    """both predictions of one compound block through the oracle: returns (conv buffer after the first, pixels after the second)"""
    w, h, mode, ti, sx, sy, p0, a0, p1, a1, avg, fwd, bck = c
    tab = np.array(K.TABLES[list(K.TABLES)[ti]], np.int16)
    r0, r1 = K.conv_rounds_compound(bd)
    tx, ty = (8 if mode in (0, 1) else 0), (8 if mode in (0, 2) else 0)
    cb = np.zeros((h, w + 5), np.uint16)
    out = np.zeros((h, w + 3), p0.dtype)
    orc.orc_convolve_jnt(V(a0), p0.shape[1], P(out), w + 3, w, h, V(tab[sx].ctypes.data), tx, V(tab[sy].ctypes.data), ty, r0, r1, bd, is16,
                         P(cb), w + 5, 1, 0, 0)
    first = cb.copy()
    orc.orc_convolve_jnt(V(a1), p1.shape[1], P(out), w + 3, w, h, V(tab[sy].ctypes.data), tx, V(tab[sx].ctypes.data), ty, r0, r1, bd, is16,
                         P(cb), w + 5, avg, fwd, bck)
    return first, out


def run_fn_jnt(fns, c, bd, is16, CP, FP):
    """the same through functions with the reference's signatures (the reference's own, or the HIP Tier A leaves)"""
    w, h, mode, ti, sx, sy, p0, a0, p1, a1, avg, fwd, bck = c
    tab = K.kernel_table(list(K.TABLES)[ti])[0]
    r0, r1 = K.conv_rounds_compound(bd)
    cb = np.zeros((h, w + 5), np.uint16)
    out = np.zeros((h, w + 3), p0.dtype)
    fp = FP(tab.ctypes.data, 8, 16, ti)
    cp = CP(do_average=0, dst=cb.ctypes.data, dst_stride=w + 5, round_0=r0, round_1=r1, is_compound=1)
    tail = [bd] if is16 else []
    fns[mode](*([V(a0), p0.shape[1], P(out), w + 3, w, h, C.byref(fp), C.byref(fp), sx, sy, C.byref(cp)] + tail))
    first = cb.copy()
    cp.do_average, cp.use_jnt_comp_avg, cp.fwd_offset, cp.bck_offset = 1, int(avg == 3), fwd, bck
    fns[mode](*([V(a1), p1.shape[1], P(out), w + 3, w, h, C.byref(fp), C.byref(fp), sy, sx, C.byref(cp)] + tail))
    return first, out


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1), (12, 1)])
def test_convolve_jnt(orc, ref, bd, is16):
    sig8 = (V, C.c_int32, V, C.c_int32, C.c_int32, C.c_int32, V, V, C.c_int32, C.c_int32, V)
    fns = [L.rtcd(ref, (f"svt_av1_highbd_jnt_convolve_{m}" if is16 else f"svt_av1_jnt_convolve_{m}"), None,
                  *(sig8 + ((C.c_int32,) if is16 else ()))) for m in K.JNT_MODES]
    for i, c in enumerate(K.jnt_cases(bd, is16)):
        f1, o1 = run_fn_jnt(fns, c, bd, is16, ConvolveParams, K.InterpFilterParams)
        f2, o2 = run_orc_jnt(orc, c, bd, is16)
        assert np.array_equal(f1, f2) and np.array_equal(o1, o2), (i, c[:6])
    rng, n = np.random.default_rng(4130 + bd), 0
    for i, c in enumerate(K.ext_cases(bd)):
        (p0, a0), (p1, a1) = K.ext_plane(rng, c), K.ext_plane(rng, c, second=True)
        for avg, fwd, bck in K.ext_avgs(i, c):
            f1, o1 = ext_run_fn_jnt(fns, c, p0, a0, p1, a1, avg, fwd, bck, ConvolveParams, K.InterpFilterParams)
            f2, o2 = ext_run_orc_jnt(orc, c, p0, a0, p1, a1, avg, fwd, bck)
            assert np.array_equal(f1, f2) and np.array_equal(o1, o2), (i, c, avg)
            n += 1
    print(f"jnt_convolve bd {bd}: {n} extended cases")


def test_convolve_jnt_oracle_vs_golden(orc):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convolve_jnt.npz"))
    k = 0
    for bd, is16 in ((8, 0), (10, 1)):
        for c in K.jnt_cases(bd, is16, n=16, seed=1):
            f, o = run_orc_jnt(orc, c, bd, is16)
            assert np.array_equal(f[:, :c[0]], g[f"first{k}"]) and np.array_equal(o[:, :c[0]], g[f"out{k}"]), k
            k += 1


def test_convolve_ext_oracle_vs_golden(orc):
    """the oracle against the reference's recorded results on the extended cases (holds without oracle/_ref)"""
    n = 0
    for c, p0, p1, fwd, bck, sr, first, avg, wtd in K.ext_golden():
        a0, a1 = K.at_block(p0), K.at_block(p1)
        assert np.array_equal(ext_run_orc_sr(orc, c, p0, a0)[:, :c.w], sr), c
        for mode, want in ((2, avg), (3, wtd)):
            f, o = ext_run_orc_jnt(orc, c, p0, a0, p1, a1, mode, fwd, bck)
            assert np.array_equal(f[:, :c.w], first) and np.array_equal(o[:, :c.w], want), (c, mode)
        n += 1
    assert n == 16
