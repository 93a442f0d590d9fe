"""GPU parity: single-reference inter-prediction interpolation (through the C-ABI) against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import conv_cases as K
from arena import GUARD
from lf_cases import P, V
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
MODES = ("2d_sr", "x_sr", "y_sr", "2d_copy_sr")


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1), (12, 1)])
def test_tier_a(hip, orc, bd, is16):
    rng = np.random.default_rng(120 + bd)
    r0, r1 = K.conv_rounds(bd)
    tabs = {n: K.kernel_table(n) for n in K.TABLES}
    for trial in range(44):
        w, h = K.SIZES[trial % len(K.SIZES)]
        tab = tabs[list(K.TABLES)[trial % 3]][0]
        sx, sy = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        mode = MODES[trial % 4]
        plane, at = K.ref_plane(rng, w, h, bd, is16, (0, 2, 1)[trial % 3])
        fp = abi.InterpFilterParams(tab.ctypes.data, 8, 16, trial % 3)
        cp = abi.ConvolveParams(round_0=r0, round_1=r1)
        o1, o2 = np.zeros((h, w + 3), plane.dtype), np.zeros((h, w + 3), plane.dtype)
        tx = 8 if mode in ("2d_sr", "x_sr") else 0
        ty = 8 if mode in ("2d_sr", "y_sr") else 0
        orc.orc_convolve_sr(V(at), plane.shape[1], P(o1), w + 3, w, h, V(tab[sx].ctypes.data), tx, V(tab[sy].ctypes.data), ty, r0, r1, bd, is16)
        fn = getattr(hip, f"svt_av1_highbd_convolve_{mode}_hip" if is16 else f"svt_av1_convolve_{mode}_hip")
        fn(*([V(at), plane.shape[1], P(o2), w + 3, w, h, C.byref(fp), C.byref(fp), sx, sy, C.byref(cp)] + ([bd] if is16 else [])))
        assert np.array_equal(o1, o2), (trial, mode, w, h, sx, sy)


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1)])
def test_tier_b_batch(hip, orc, bd, is16):
    """A whole picture's worth of blocks (random sizes, phases, filters, modes) from one reference plane in one launch."""
    rng = np.random.default_rng(500 + bd)
    W, H = 640, 384
    plane, at0 = K.ref_plane(rng, W, H, bd, is16, 0)
    d_ref = device.DeviceBuffer(hip, plane.nbytes)
    d_ref.upload(plane)
    off0 = at0 - plane.ctypes.data
    out = np.zeros((H, W), plane.dtype)
    d_out = device.DeviceBuffer(hip, out.nbytes)
    d_out.fill(0)
    r0, r1 = K.conv_rounds(bd)
    tabs = [np.array(K.TABLES[n], np.int16) for n in K.TABLES]
    descs, want = [], np.zeros_like(out)
    for by in range(0, H, 128):
        for bx in range(0, W, 128):
            bs = int(rng.choice([16, 32, 64, 128]))
            for y in range(by, by + 128, bs):
                for x in range(bx, bx + 128, bs):
                    w, h = bs, bs
                    if rng.random() < 0.3 and bs > 16:
                        h = bs // 2        # a rectangular block; the lower half is predicted separately
                    for (yy, hh) in ((y, h),) + (((y + h, bs - h),) if h != bs else ()):
                        mvx, mvy = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))      # whole-sample part, stays inside the border
                        sx, sy = int(rng.integers(0, 16)), int(rng.integers(0, 16))
                        mode = int(rng.integers(0, 4))
                        tx = 8 if mode in (0, 1) else 0
                        ty = 8 if mode in (0, 2) else 0
                        t = tabs[int(rng.integers(0, 3))]
                        so = ((yy + mvy) * plane.shape[1] + x + mvx) * plane.itemsize
                        d = abi.ConvolveDesc(d_ref.ptr + off0 + so, d_out.ptr + (yy * W + x) * plane.itemsize, plane.shape[1], W, w, hh,
                                             (C.c_int16 * 8)(*t[sx]), (C.c_int16 * 8)(*t[sy]), tx, ty, r0, r1, bd, is16)
                        descs.append(d)
                        orc.orc_convolve_sr(V(at0 + so), plane.shape[1], V(want.ctypes.data + (yy * W + x) * plane.itemsize), W, w, hh,
                                            V(t[sx].ctypes.data), tx, V(t[sy].ctypes.data), ty, r0, r1, bd, is16)
    arr = (abi.ConvolveDesc * len(descs))(*descs)
    d_desc = device.DeviceBuffer(hip, C.sizeof(arr))
    d_desc.upload(np.frombuffer(arr, np.uint8))
    device.check(hip, hip.svt_hip_convolve_sr_batch(V(d_desc.ptr), len(descs), None), "convolve_sr_batch")
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert np.array_equal(d_out.download(plane.dtype, out.shape), want)
    assert hip.svt_hip_convolve_sr_batch(None, 0, None) == abi.SVT_HIP_ERR_BAD_PARAMETER


def test_golden(hip):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convolve.npz"))
    tabs = {n: K.kernel_table(n) for n in K.TABLES}
    for i in range(int(g["n"])):
        bd, is16, w, h, mode, ti, sx, sy = (int(v) for v in g[f"c{i}_meta"])
        plane = g[f"c{i}_plane"].copy()
        at = plane.ctypes.data + (8 * plane.shape[1] + 8) * plane.itemsize
        tab = tabs[list(K.TABLES)[ti]][0]
        r0, r1 = K.conv_rounds(bd)
        fp = abi.InterpFilterParams(tab.ctypes.data, 8, 16, ti)
        cp = abi.ConvolveParams(round_0=r0, round_1=r1)
        o = np.zeros((h, w), plane.dtype)
        fn = getattr(hip, f"svt_av1_highbd_convolve_{MODES[mode]}_hip" if is16 else f"svt_av1_convolve_{MODES[mode]}_hip")
        fn(*([V(at), plane.shape[1], P(o), w, w, h, C.byref(fp), C.byref(fp), sx, sy, C.byref(cp)] + ([bd] if is16 else [])))
        assert np.array_equal(o, g[f"c{i}_out"]), i


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1), (12, 1)])
def test_tier_a_compound(hip, orc, bd, is16):
    """svt_av1_(highbd_)jnt_convolve_{2d,x,y,2d_copy}_hip: first prediction into the ConvBufType buffer, second prediction
    averaged (plain / distance-weighted) into pixels — both steps against the oracle."""
    import test_convolve_oracle as T
    fns = [getattr(hip, f"svt_av1_highbd_jnt_convolve_{m}_hip" if is16 else f"svt_av1_jnt_convolve_{m}_hip") for m in K.JNT_MODES]
    for i, c in enumerate(K.jnt_cases(bd, is16)):
        f1, o1 = T.run_fn_jnt(fns, c, bd, is16, abi.ConvolveParams, abi.InterpFilterParams)
        f2, o2 = T.run_orc_jnt(orc, c, bd, is16)
        assert np.array_equal(f1, f2) and np.array_equal(o1, o2), (i, c[:6])


def test_compound_golden(hip):
    import test_convolve_oracle as T
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convolve_jnt.npz"))
    k = 0
    for bd, is16 in ((8, 0), (10, 1)):
        fns = [getattr(hip, f"svt_av1_highbd_jnt_convolve_{m}_hip" if is16 else f"svt_av1_jnt_convolve_{m}_hip") for m in K.JNT_MODES]
        for c in K.jnt_cases(bd, is16, n=16, seed=1):
            f, o = T.run_fn_jnt(fns, c, bd, is16, abi.ConvolveParams, abi.InterpFilterParams)
            assert np.array_equal(f[:, :c[0]], g[f"first{k}"]) and np.array_equal(o[:, :c[0]], g[f"out{k}"]), k
            k += 1


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1)])
def test_tier_b_compound_batch(hip, orc, bd, is16):
    """Compound prediction of a tiled picture: one launch for every block's first reference (into a picture-sized
    ConvBufType plane), one for the second reference with the average, both from device-resident reference planes."""
    rng = np.random.default_rng(640 + bd)
    W, H = 512, 256
    p0, a0 = K.ref_plane(rng, W, H, bd, is16, 0)
    p1, a1 = K.ref_plane(rng, W, H, bd, is16, 2)
    d0, d1 = device.DeviceBuffer(hip, p0.nbytes), device.DeviceBuffer(hip, p1.nbytes)
    d0.upload(p0), d1.upload(p1)
    o0, o1 = a0 - p0.ctypes.data, a1 - p1.ctypes.data
    d_out, d_cb = device.DeviceBuffer(hip, W * H * p0.itemsize), device.DeviceBuffer(hip, W * H * 2)
    d_out.fill(0), d_cb.fill(0)
    r0, r1 = K.conv_rounds_compound(bd)
    tabs = [np.array(K.TABLES[n], np.int16) for n in K.TABLES]
    first, second = [], []
    want, cb = np.zeros((H, W), p0.dtype), np.zeros((H, W), np.uint16)
    for y in range(0, H, 64):
        for x in range(0, W, 64):
            bs = int(rng.choice([8, 16, 32, 64]))
            for yy in range(y, y + 64, bs):
                for xx in range(x, x + 64, bs):
                    avg = int(rng.choice([2, 3]))
                    fwd, bck = K.DIST_WEIGHTS[int(rng.integers(0, len(K.DIST_WEIGHTS)))]
                    for ref_i, (dev, off, plane, at, lst) in enumerate(((d0, o0, p0, a0, first), (d1, o1, p1, a1, second))):
                        mvx, mvy = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
                        sx, sy = int(rng.integers(0, 16)), int(rng.integers(0, 16))
                        mode = int(rng.integers(0, 4))
                        tx, ty = (8 if mode in (0, 1) else 0), (8 if mode in (0, 2) else 0)
                        t = tabs[int(rng.integers(0, 3))]
                        so = ((yy + mvy) * plane.shape[1] + xx + mvx) * plane.itemsize
                        comp = 1 if ref_i == 0 else avg
                        lst.append(abi.ConvolveDesc(dev.ptr + off + so, d_out.ptr + (yy * W + xx) * plane.itemsize, plane.shape[1], W, bs, bs,
                                                    (C.c_int16 * 8)(*t[sx]), (C.c_int16 * 8)(*t[sy]), tx, ty, r0, r1, bd, is16, comp, fwd, bck,
                                                    (C.c_uint8 * 3)(), d_cb.ptr + (yy * W + xx) * 2, W, 0))
                        orc.orc_convolve_jnt(V(at + so), plane.shape[1], V(want.ctypes.data + (yy * W + xx) * plane.itemsize), W, bs, bs,
                                             V(t[sx].ctypes.data), tx, V(t[sy].ctypes.data), ty, r0, r1, bd, is16,
                                             V(cb.ctypes.data + (yy * W + xx) * 2), W, comp, fwd, bck)
    for lst in (first, second):
        arr = (abi.ConvolveDesc * len(lst))(*lst)
        d_desc = device.DeviceBuffer(hip, C.sizeof(arr))
        d_desc.upload(np.frombuffer(arr, np.uint8))
        device.check(hip, hip.svt_hip_convolve_batch(V(d_desc.ptr), len(lst), None), "convolve_batch")
        device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert np.array_equal(d_cb.download(np.uint16, (H, W)), cb)
    assert np.array_equal(d_out.download(p0.dtype, (H, W)), want)


# ---- extended net: every table / shape / phase / kernel length, adversarial planes, the Tier B contract ------------------------
BDS = [(8, 0), (10, 1), (12, 1)]


def _leaves(hip, is16, jnt):
    hb = "highbd_" if is16 else ""
    return [getattr(hip, f"svt_av1_{hb}jnt_convolve_{m}_hip" if jnt else f"svt_av1_{hb}convolve_{m}_sr_hip") for m in K.MODES]


@pytest.mark.parametrize("bd,is16", BDS)
def test_tier_a_ext(hip, orc, bd, is16):
    """The single-reference leaves over conv_cases.ext_cases: all 22 block sizes, the 2-wide / 2-high chroma sizes, sizes that are no
    power of two (1x1 .. 127x3), all six tables with x table != y table, InterpFilterParams of 2 / 4 / 6 / 8 taps, and per kernel
    with a negative tap the two planes that drive it to its extremes.  Padding columns of dst included."""
    import test_convolve_oracle as T
    fns, rng = _leaves(hip, is16, 0), np.random.default_rng(4120 + bd)
    for i, c in enumerate(K.ext_cases(bd)):
        plane, at = K.ext_plane(rng, c)
        got = T.ext_run_fn_sr(fns, c, plane, at, abi.ConvolveParams, abi.InterpFilterParams)
        assert np.array_equal(got, T.ext_run_orc_sr(orc, c, plane, at)), (i, c)


@pytest.mark.parametrize("bd,is16", BDS)
def test_tier_a_compound_ext(hip, orc, bd, is16):
    """The compound leaves over the same cases: conv buffer after the first prediction, pixels after the second (both averages on
    the adversarial planes); the first call leaves dst alone and the second the conv buffer (ext_run_fn_jnt asserts it)."""
    import test_convolve_oracle as T
    fns, rng = _leaves(hip, is16, 1), np.random.default_rng(4130 + bd)
    for i, c in enumerate(K.ext_cases(bd)):
        (p0, a0), (p1, a1) = K.ext_plane(rng, c), K.ext_plane(rng, c, second=True)
        for avg, fwd, bck in K.ext_avgs(i, c):
            f1, o1 = T.ext_run_fn_jnt(fns, c, p0, a0, p1, a1, avg, fwd, bck, abi.ConvolveParams, abi.InterpFilterParams)
            f2, o2 = T.ext_run_orc_jnt(orc, c, p0, a0, p1, a1, avg, fwd, bck)
            assert np.array_equal(f1, f2) and np.array_equal(o1, o2), (i, c, avg)


def test_ext_golden(hip):
    """the leaves against the reference's recorded results (tests/golden/convolve_ext.npz)"""
    import test_convolve_oracle as T
    for c, p0, p1, fwd, bck, sr, first, avg, wtd in K.ext_golden():
        a0, a1 = K.at_block(p0), K.at_block(p1)
        got = T.ext_run_fn_sr(_leaves(hip, c.is16, 0), c, p0, a0, abi.ConvolveParams, abi.InterpFilterParams)
        assert np.array_equal(got[:, :c.w], sr), c
        for mode, want in ((2, avg), (3, wtd)):
            f, o = T.ext_run_fn_jnt(_leaves(hip, c.is16, 1), c, p0, a0, p1, a1, mode, fwd, bck, abi.ConvolveParams, abi.InterpFilterParams)
            assert np.array_equal(f[:, :c.w], first) and np.array_equal(o[:, :c.w], want), (c, mode)


class Mirror:
    """A host array and its device copy.  The oracle works on the one and the library on the other, at the same offsets."""

    def __init__(self, hip, host):
        assert host.flags.c_contiguous
        self.host, self.dev = host, device.DeviceBuffer(hip, host.nbytes)
        self.push()

    def push(self):
        self.dev.upload(self.host)

    def pull(self):
        return self.dev.download(self.host.dtype, self.host.shape)

    def at(self, *idx):
        """(host address, device address) of an element"""
        off = int(np.ravel_multi_index(idx, self.host.shape)) * self.host.itemsize
        return self.host.ctypes.data + off, self.dev.ptr + off


def _kernel8(name, phase, taps):
    """filter_x / filter_y of a descriptor: the kernel in the first `taps` entries (its outer zero columns dropped); the library
    reads no further, so the rest holds junk"""
    k = np.full(8, 0x7fff, np.int16)
    k[:taps] = K.narrow_table(name, taps)[phase]
    return (C.c_int16 * 8)(*k)


class Batch:
    """The descriptors of one svt_hip_convolve_batch launch.  add() also runs the oracle with the same arguments on the host side
    of the mirrors, so after run() every device buffer must equal its mirror.  src / dst / cbuf: (host address, device address)."""

    def __init__(self, hip, orc):
        self.hip, self.orc, self.descs = hip, orc, []

    def add(self, c, src, dst, strides, cbuf=(0, 0), comp=0, fwd=0, bck=0):
        (r0, r1), (tx, ty) = (K.conv_rounds_compound if comp else K.conv_rounds)(c.bd), c.use
        kx, ky = _kernel8(c.tx, c.sx, c.taps[0]), _kernel8(c.ty, c.sy, c.taps[1])
        self.descs.append(abi.ConvolveDesc(src[1], dst[1], strides[0], strides[1], c.w, c.h, kx, ky, tx, ty, r0, r1, c.bd, c.is16, comp, fwd, bck,
                                           (C.c_uint8 * 3)(), cbuf[1], strides[2], 0))
        if comp:
            self.orc.orc_convolve_jnt(V(src[0]), strides[0], V(dst[0]), strides[1], c.w, c.h, kx, tx, ky, ty, r0, r1, c.bd, c.is16,
                                      V(cbuf[0]), strides[2], comp, fwd, bck)
        else:
            self.orc.orc_convolve_sr(V(src[0]), strides[0], V(dst[0]), strides[1], c.w, c.h, kx, tx, ky, ty, r0, r1, c.bd, c.is16)

    def add_skipped(self, w, h):
        """an unused slot: w == 0 or h == 0, every pointer null"""
        assert w == 0 or h == 0
        self.descs.append(abi.ConvolveDesc(w=w, h=h, taps_x=8, taps_y=8, bit_depth=8))

    def run(self):
        arr = (abi.ConvolveDesc * len(self.descs))(*self.descs)
        d_desc = device.DeviceBuffer(self.hip, C.sizeof(arr))
        d_desc.upload(np.frombuffer(arr, np.uint8))
        device.check(self.hip, self.hip.svt_hip_convolve_batch(V(d_desc.ptr), len(self.descs), None), "convolve_batch")
        device.check(self.hip, self.hip.svt_hip_stream_sync(None), "sync")


def _canary(shape, dtype):
    return np.full(shape, GUARD * (0x101 if np.dtype(dtype).itemsize == 2 else 1), dtype)


def _three_launches(hip, orc, cases, src, src_at, slot, strides):
    """cases through Tier B as single references, then as first and as second predictions of compounds (both from the same source;
    case i averaged as conv_cases.ext_avgs(i) says), block i at [i] of packed dst / cbuf arrays of `slot` = (rows, stride) per block.  Checks pixels and
    conv buffers against the oracle, the untouched rest of every slot included, and that a first prediction leaves dst alone and a
    second one the conv buffer."""
    n, dt = len(cases), src.host.dtype
    dst, cb = Mirror(hip, _canary((n,) + slot, dt)), Mirror(hip, _canary((n,) + slot, np.uint16))
    b = Batch(hip, orc)
    for i, c in enumerate(cases):
        b.add(c, src_at(i, c), dst.at(i, 0, 0), strides)
    b.run()
    got = dst.pull()
    bad = np.flatnonzero((got != dst.host).any(axis=(1, 2)))
    assert bad.size == 0, ("sr", cases[bad[0]])
    b = Batch(hip, orc)
    for i, c in enumerate(cases):
        b.add(c, src_at(i, c), dst.at(i, 0, 0), strides, cb.at(i, 0, 0), 1)
    b.run()
    first = cb.pull()
    bad = np.flatnonzero((first != cb.host).any(axis=(1, 2)))
    assert bad.size == 0, ("compound 1", cases[bad[0]])
    assert np.array_equal(dst.pull(), got), "a first prediction wrote pixels"
    for k in range(2):      # every case with one average; the adversarial ones with the other too
        dst.host[:] = _canary(dst.host.shape, dt)
        dst.push()
        b, ran = Batch(hip, orc), []
        for i, c in enumerate(cases):
            avgs = K.ext_avgs(i, c)
            if k < len(avgs):
                b.add(c, src_at(i, c), dst.at(i, 0, 0), strides, cb.at(i, 0, 0), *avgs[k])
                ran.append(i)
        if not ran:
            break
        b.run()
        got2 = dst.pull()
        bad = np.flatnonzero((got2 != dst.host).any(axis=(1, 2)))
        assert bad.size == 0, ("compound", K.ext_avgs(bad[0], cases[bad[0]])[k], cases[bad[0]])
        assert np.array_equal(cb.pull(), first), "a second prediction wrote the conv buffer"


@pytest.mark.parametrize("bd,is16", BDS)
def test_tier_b_adversarial(hip, orc, bd, is16):
    """conv_cases.adv_cases in Tier B launches: the planes that put the maximum sample under every positive tap of a kernel and 0
    under the others, and their inverses, in every sr and jnt mode with both averages.  These drive the int16 intermediate of the
    2-D pass, the uint16 ConvBufType store and the final clip to their bounds."""
    cases = list(K.adv_cases(bd))
    rng = np.random.default_rng(0)
    src = Mirror(hip, np.stack([K.ext_plane(rng, c)[0] for c in cases]))
    _three_launches(hip, orc, cases, src, lambda i, c: src.at(i, 8, 8), (8, 12), (24, 12, 12))


def _sweep_cases(bd):
    """(x table, x phase, y table, y phase) over all 6 x 16 x 6 x 16 combinations on 8 x 8 blocks, the 4-tap tables also on 2 x 8 and
    4 x 4.  A zero phase alternately runs as a filter (taps 8, the identity kernel) and as no filter (taps 0)."""
    names, zx, zy = list(K.TABLES), 0, 0
    for w, h, tabs in ((8, 8, names), (2, 8, K.TABLES4), (4, 4, K.TABLES4)):
        for tx in tabs:
            for sx in range(16):
                for ty in tabs:
                    for sy in range(16):
                        zx, zy = zx + (sx == 0), zy + (sy == 0)
                        x_on, y_on = sx != 0 or (zx // 16 + zx) % 2 == 0, sy != 0 or (zy // 2) % 2 == 0
                        yield K.ExtCase(w, h, (0 if y_on else 1) if x_on else (2 if y_on else 3), tx, ty, sx, sy, (8, 8), K.KIND_UNIFORM, bd)


def test_sweep_cases():
    cs = list(_sweep_cases(8))
    assert len(cs) == 6 * 16 * 6 * 16 + 2 * (2 * 16 * 2 * 16)
    for d, on in ((0, (0, 1)), (1, (0, 2))):       # direction: the modes that filter it
        zero = [c.mode in on for c in cs if (c.sx, c.sy)[d] == 0]
        assert abs(2 * sum(zero) - len(zero)) <= 2, (d, sum(zero), len(zero))
    assert {c.mode for c in cs if c.sx == 0 and c.sy == 0} == {0, 1, 2, 3}


@pytest.mark.parametrize("compound", [0, 1])
@pytest.mark.parametrize("bd,is16", BDS)
def test_tier_b_phase_sweep(hip, orc, bd, is16, compound):
    """Every (x table, x phase, y table, y phase) in one launch from one random reference plane; as a compound, a compound 1 launch
    and a compound 2 / 3 launch over DIST_WEIGHTS."""
    cases = list(_sweep_cases(bd))
    rng = np.random.default_rng(900 + bd)
    plane = K.ref_plane(rng, 96, 96, bd, is16, K.KIND_UNIFORM)[0]          # 112 x 112 with the border
    src = Mirror(hip, plane)
    dst = Mirror(hip, _canary((len(cases), 8, 12), plane.dtype))
    cb = Mirror(hip, _canary((len(cases), 8, 12), np.uint16))
    at = [src.at(8 + (i * 7) % 89, 8 + (i * 13) % 83) for i in range(len(cases))]       # blocks of <= 8 x 8 inside the 96 x 96
    b = Batch(hip, orc)
    for i, c in enumerate(cases):
        b.add(c, at[i], dst.at(i, 0, 0), (112, 12, 12), cb.at(i, 0, 0), compound)
    b.run()
    for m in ((cb, dst) if compound else (dst, cb)):      # what the launch writes, then what it must leave alone
        bad = np.flatnonzero((m.pull() != m.host).any(axis=(1, 2)))
        assert bad.size == 0, (compound, len(bad), cases[bad[0]])
    if compound:
        b = Batch(hip, orc)
        for i, c in enumerate(cases):
            b.add(c, at[(i * 31 + 5) % len(cases)], dst.at(i, 0, 0), (112, 12, 12), cb.at(i, 0, 0), 2 + i % 2, *K.DIST_WEIGHTS[i % len(K.DIST_WEIGHTS)])
        b.run()
        for m in (dst, cb):
            bad = np.flatnonzero((m.pull() != m.host).any(axis=(1, 2)))
            assert bad.size == 0, ("average", len(bad), bad[0], cases[bad[0]])


CONTAIN = [(128, 128, 8), (128, 64, 144), (64, 128, 280), (66, 70, 352), (2, 2, 426)]        # w, h, x of the block in dst / cbuf


@pytest.mark.parametrize("bd,is16", BDS)
def test_tier_b_containment(hip, orc, bd, is16):
    """Blocks with >= 8 samples between them and the buffer's edges, strides that differ from w and from each other: outside the
    w x h rectangles dst and cbuf keep their canary; a compound 1 launch leaves all of dst alone, a compound 2 / 3 launch all of cbuf."""
    rng = np.random.default_rng(77 + bd)
    sstride, dstride, cstride = 480, 448, 464
    src = Mirror(hip, K.ref_plane(rng, sstride - 16, 144, bd, is16, K.KIND_UNIFORM)[0])       # 160 x 480
    dst, cb = Mirror(hip, _canary((144, dstride), src.host.dtype)), Mirror(hip, _canary((144, cstride), np.uint16))
    inside = np.zeros((144, dstride), bool)
    for w, h, x in CONTAIN:
        inside[8:8 + h, x:x + w] = True
    for mode in range(4):
        cases = [K.ExtCase(w, h, mode, "sub_pel_filters_8sharp", "sub_pel_filters_8", 5 + i, 11 - i, (8, 8), K.KIND_UNIFORM, bd)
                 for i, (w, h, x) in enumerate(CONTAIN)]
        for comp in (0, 1, 2):
            if comp != 2:
                dst.host[:], cb.host[:] = _canary(dst.host.shape, dst.host.dtype), _canary(cb.host.shape, np.uint16)
                dst.push(), cb.push()
            cb_before = cb.host.copy()
            b = Batch(hip, orc)
            for i, ((w, h, x), c) in enumerate(zip(CONTAIN, cases)):
                b.add(c, src.at(12 + 3 * comp, x + 10 + comp), dst.at(8, x), (sstride, dstride, cstride), cb.at(8, x), comp + (comp == 2 and i % 2),
                      *K.DIST_WEIGHTS[i])
            b.run()
            got, got_cb = dst.pull(), cb.pull()
            assert (got[~inside] == dst.host[0, 0]).all(), (mode, comp, "dst outside the blocks")
            assert (got_cb[:, :dstride][~inside] == GUARD * 0x101).all() and (got_cb[:, dstride:] == GUARD * 0x101).all(), (mode, comp, "cbuf outside the blocks")
            assert np.array_equal(got, dst.host) and np.array_equal(got_cb, cb.host), (mode, comp)
            if comp == 1:
                assert (got == got[0, 0]).all(), (mode, "compound 1 wrote dst")
            if comp == 2:
                assert np.array_equal(got_cb, cb_before), (mode, "compound 2 / 3 wrote cbuf")


MARGIN_SHAPES = [(8, 8), (2, 2), (66, 70), (128, 128)]
MARGIN_FILTERS = [("sub_pel_filters_8sharp", 8), ("sub_pel_filters_8", 6), ("sub_pel_filters_4", 4), ("bilinear_filters", 2)]


@pytest.mark.parametrize("bd,is16", [(8, 0), (12, 1)])
def test_tier_b_source_margins(hip, orc, bd, is16):
    """The documented source region is all a block depends on: the block plus taps / 2 - 1 samples before and taps / 2 after, per
    direction, nothing more in a direction with taps == 0.  The library reads a copy of the plane where everything outside that
    region is a sentinel (0, then the maximum); the oracle reads the plane itself.  The buffers extend 32 samples and more beyond
    the region on all sides, so nothing here makes the kernel address unallocated memory."""
    rng = np.random.default_rng(310 + bd)
    cases = []
    for mode in range(4):
        for i, (w, h) in enumerate(MARGIN_SHAPES):
            (tx, tapx), (ty, tapy) = MARGIN_FILTERS[(i + mode) % 4], MARGIN_FILTERS[(i + mode // 2 + 1) % 4]
            cases.append(K.ExtCase(w, h, mode, tx, ty, 3 + 2 * i, 13 - 3 * i, (tapx, tapy), K.KIND_UNIFORM, bd))
    n, S = len(cases), 200
    real = rng.integers(0, 1 << bd, size=(n, S, S)).astype(np.uint16 if is16 else np.uint8)
    for sentinel in (0, (1 << bd) - 1):
        masked = np.full_like(real, sentinel)
        for i, c in enumerate(cases):
            (tx, ty) = c.use
            y0, y1 = 36 - (ty // 2 - 1 if ty else 0), 36 + c.h + ty // 2
            x0, x1 = 36 - (tx // 2 - 1 if tx else 0), 36 + c.w + tx // 2
            masked[i, y0:y1, x0:x1] = real[i, y0:y1, x0:x1]
        src = Mirror(hip, masked)
        host_at = lambda i, c: (real.ctypes.data + (i * S * S + 36 * S + 36) * real.itemsize, src.at(i, 36, 36)[1])  # noqa: E731
        _three_launches(hip, orc, cases, src, host_at, (128, 136), (S, 136, 136))


def test_tier_b_mixed_launch(hip, orc):
    """one launch: skipped descriptors (w == 0 or h == 0, null pointers) between live ones, 8-bit next to 10- and 12-bit, single
    references next to first predictions of compounds"""
    rng = np.random.default_rng(41)
    src = {bd: Mirror(hip, K.ref_plane(rng, 80, 80, bd, bd > 8, K.KIND_UNIFORM)[0]) for bd in (8, 10, 12)}
    dst = {bd: Mirror(hip, _canary((6, 70, 72), src[bd].host.dtype)) for bd in src}
    cb = {bd: Mirror(hip, _canary((6, 70, 72), np.uint16)) for bd in src}
    b, names = Batch(hip, orc), list(K.TABLES)
    b.add_skipped(0, 16)
    for i in range(18):
        bd, k = (8, 10, 12)[i % 3], i // 3
        w, h = [(8, 8), (66, 70), (2, 16), (16, 2), (32, 64), (64, 16)][k]
        c = K.ExtCase(w, h, i % 4, names[i % 6], names[(i + 1 + k) % 6], 1 + i % 15, 15 - i % 15, (8, 8), K.KIND_UNIFORM, bd)
        b.add(c, src[bd].at(10 + k, 9 + i % 5), dst[bd].at(k, 0, 0), (96, 72, 72), cb[bd].at(k, 0, 0), k % 2)
        if i % 4 == 1:
            b.add_skipped(0, 0)
        if i % 5 == 2:
            b.add_skipped(64, 0)
    b.add_skipped(0, 128)
    b.run()
    for bd in src:
        assert np.array_equal(dst[bd].pull(), dst[bd].host) and np.array_equal(cb[bd].pull(), cb[bd].host), bd


SEAM_SHAPES = [(128, 128), (128, 64), (64, 128), (65, 65), (127, 128)]


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1)])
def test_tier_b_tile_seams(hip, orc, bd, is16):
    """Blocks of more than one 64 x 64 tile in each sr mode and each jnt mode: rows and columns 63 / 64, where one tile's result ends
    and the next one's begins from its own staged copy of the source, are compared on their own (and then everything else)."""
    rng = np.random.default_rng(63 + bd)
    src = Mirror(hip, K.ref_plane(rng, 144, 144, bd, is16, K.KIND_UNIFORM)[0])         # 160 x 160
    names = list(K.TABLES)
    cases = [K.ExtCase(w, h, mode, names[(i + mode) % 6], names[(i + mode + 1 + i % 2) % 6], 1 + (3 * i + mode) % 15, 15 - (5 * i + mode) % 15,
                       (8, 8), K.KIND_UNIFORM, bd) for mode in range(4) for i, (w, h) in enumerate(SEAM_SHAPES)]
    n = len(cases)
    dst, cb = Mirror(hip, _canary((n, 128, 136), src.host.dtype)), Mirror(hip, _canary((n, 128, 136), np.uint16))
    at = [src.at(10 + i % 5, 12 + i % 7) for i in range(n)]

    def seams(m, what):
        got = m.pull()
        for i, c in enumerate(cases):
            for r in (63, 64):
                if r < c.h:
                    assert np.array_equal(got[i, r, :c.w], m.host[i, r, :c.w]), (what, "row", r, c)
                if r < c.w:
                    assert np.array_equal(got[i, :c.h, r], m.host[i, :c.h, r]), (what, "column", r, c)
        assert np.array_equal(got, m.host), what

    for comp in (0, 1, 2):
        b = Batch(hip, orc)
        for i, c in enumerate(cases):
            b.add(c, at[(i + comp) % n], dst.at(i, 0, 0), (160, 136, 136), cb.at(i, 0, 0), comp + (comp == 2 and i % 2), *K.DIST_WEIGHTS[i % 8])
        b.run()
        seams(cb if comp == 1 else dst, comp)
