"""GPU parity of reference scaling (include/svt_hip_scale.h): svt_hip_resize_planes, svt_hip_superres_upscale_planes and
svt_hip_convolve_scale_batch against the fixture of the reference's own svt_av1_resize_plane_c, svt_av1_upscale_normative_rows and
svt_av1_convolve_2d_scale_c with their highbd twins (tests/golden/scale.npz), byte for byte; a case the fixture keeps as a digest is
compared with the numpy restatement once that has the digest.  Every plane, table, descriptor, output and the workspace of a test live in
one guarded arena: a byte written outside the declared outputs and the workspace fails the test, and so does a source plane that
changed.  Every test makes its calls twice, and both runs must give the fixture."""
import ctypes as C

import numpy as np
import pytest

import conv_cases
import scale_cases as K
from arena import PATTERN, Arena, check_containment, rows
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu


class Board:
    """One device buffer: sources at ragged offsets, outputs with their stride padding guarded, everything else a pattern."""

    def __init__(self, hip):
        self.hip, self.arena, self.off, self.outputs, self.late, self.n = hip, Arena(fill=PATTERN, tail=512), {}, [], [], 0

    def source(self, key, arr, skew=0):
        self.off[key] = self.arena.add(str(key), arr, skew=skew)

    def output(self, key, nbytes, declared=None, **kw):
        off = self.off[key] = self.arena.add(str(key), nbytes=nbytes, **kw)
        self.outputs += declared(off) if declared else [(off, nbytes)]

    def plane_out(self, key, h, stride, w, px):
        self.output(key, h * stride * px, lambda off: rows(off, stride * px, w * px, h), skew=px * (1 + self.n % 3))
        self.n += 1

    def reserve(self, key, nbytes, fill):
        """An input whose bytes hold device addresses: written into the image once the buffer exists"""
        self.off[key] = self.arena.add(str(key), nbytes=nbytes)
        self.late.append((key, fill))

    def upload(self):
        self.before = self.arena.build()
        self.buf = device.DeviceBuffer(self.hip, self.before.nbytes)
        for key, fill in self.late:
            raw = fill()
            self.before[self.off[key]:self.off[key] + raw.size] = raw
        self.buf.upload(self.before)
        return self

    def at(self, key, offset=0):
        return self.buf.ptr + self.off[key] + offset

    def image(self):
        return self.buf.download(np.uint8, (self.before.nbytes,))

    def plane(self, image, key, h, stride, w, dtype):
        o = self.off[key]
        return image[o:o + h * stride * np.dtype(dtype).itemsize].view(dtype).reshape(h, stride)[:, :w]

    def contained(self, image, what):
        check_containment(self.before, image, self.arena.regions, self.outputs, what)


def run(hip, rc, what):
    device.check(hip, rc, what)


def px_of(is16):
    return 2 if is16 else 1


# ---- resize ---------------------------------------------------------------------------------------------------------------------

class ResizeCall:
    """Planes are keyed by their place in the call: a case may appear twice."""

    def __init__(self, hip, cases, board=None):
        self.hip, self.cases, self.b = hip, cases, board or Board(hip)
        for i, c in enumerate(cases):
            self.b.source(("rsrc", i), K.resize_source(c), skew=px_of(c.is16) * (1 + i % 7))
            self.b.plane_out(("rdst", i), c.dh, c.dstride, c.dw, px_of(c.is16))
        self.ws_bytes = hip.svt_hip_resize_workspace_bytes(self.jobs(lambda key: 256), len(cases))      # layout only: any address does
        if self.ws_bytes:
            self.b.output("resize workspace", self.ws_bytes)
        if board is None:
            self.b.upload()

    def jobs(self, at=None):
        at = at or self.b.at
        return (abi.ResizePlane * len(self.cases))(*[abi.ResizePlane(at(("rsrc", i)), at(("rdst", i)), c.sstride, c.dstride, c.sw, c.sh, c.dw, c.dh,
                                                                     c.is16, c.bd) for i, c in enumerate(self.cases)])

    def launch(self, stream=None):
        return self.hip.svt_hip_resize_planes(self.jobs(), len(self.cases), self.b.at("resize workspace") if self.ws_bytes else None, self.ws_bytes, stream)

    def verify(self, image):
        for i, c in enumerate(self.cases):
            got = self.b.plane(image, ("rdst", i), c.dh, c.dstride, c.dw, K.dtype_of(c.is16))
            assert np.array_equal(got, K.expected("resize/" + c.name, lambda: K.restate_resize(c))), c.name


@pytest.mark.parametrize("case", K.RESIZE, ids=lambda c: c.name)
def test_resize_equals_the_fixture(hip, case):
    call = ResizeCall(hip, [case])
    assert (call.ws_bytes > 0) == (case.sw != case.dw and case.sh != case.dh)
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_resize_planes")
        image = call.b.image()
        call.verify(image)
        call.b.contained(image, "svt_hip_resize_planes " + case.name)


def test_resize_planes_of_all_sizes_and_depths_in_one_call(hip):
    call = ResizeCall(hip, [K.RESIZE_BY_NAME[n] for n in K.RESIZE_MIXED])
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_resize_planes")
        image = call.b.image()
        call.verify(image)
        call.b.contained(image, "svt_hip_resize_planes, mixed planes")


def test_resize_batch_of_the_maximum(hip):
    call = ResizeCall(hip, (K.RESIZE * 2)[:abi.SCALE_MAX_PLANES])
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_resize_planes")
        image = call.b.image()
        call.verify(image)
        call.b.contained(image, "svt_hip_resize_planes, 24 planes")


# ---- super-res ------------------------------------------------------------------------------------------------------------------

class SuperresCall:
    def __init__(self, hip, cases, board=None):
        self.hip, self.cases, self.b = hip, cases, board or Board(hip)
        for i, c in enumerate(cases):
            self.b.source(("ssrc", c.name), K.superres_source(c), skew=px_of(c.is16) * (1 + i))
            self.b.plane_out(("sdst", c.name), c.rows, c.dstride, K.sr_widths(c)[1], px_of(c.is16))
        if board is None:
            self.b.upload()

    def job(self, c):
        j = abi.SuperresPlane(self.b.at(("ssrc", c.name), K.SR_MARGIN * px_of(c.is16)), self.b.at(("sdst", c.name)), c.sstride, c.dstride, c.rows,
                              K.sr_frame_width(c), c.up_width, c.denom, c.sub_x, c.is16, c.bd, len(c.starts) - 1)
        for k, s in enumerate(c.starts):
            j.tile_col_start_mi[k] = s
        return j

    def launch(self, stream=None):
        jobs = (abi.SuperresPlane * len(self.cases))(*[self.job(c) for c in self.cases])
        return self.hip.svt_hip_superres_upscale_planes(jobs, len(self.cases), stream)

    def verify(self, image):
        for c in self.cases:
            got = self.b.plane(image, ("sdst", c.name), c.rows, c.dstride, K.sr_widths(c)[1], K.dtype_of(c.is16))
            assert np.array_equal(got, K.expected("superres/" + c.name, lambda: K.restate_superres(c))), c.name


@pytest.mark.parametrize("case", K.SUPERRES, ids=lambda c: c.name)
def test_superres_equals_the_fixture(hip, case):
    call = SuperresCall(hip, [case])
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_superres_upscale_planes")
        image = call.b.image()
        call.verify(image)
        call.b.contained(image, "svt_hip_superres_upscale_planes " + case.name)      # the source's border columns included


def test_superres_planes_of_all_kinds_in_one_call(hip):
    call = SuperresCall(hip, [K.SUPERRES_BY_NAME[n] for n in K.SUPERRES_MIXED])
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_superres_upscale_planes")
        image = call.b.image()
        call.verify(image)
        call.b.contained(image, "svt_hip_superres_upscale_planes, mixed planes")


# ---- prediction from a scaled reference ---------------------------------------------------------------------------------------------

class ScaledCall:
    """cases: ScaleCase, or None for a descriptor that is skipped (w == 0, null pointers)"""

    def __init__(self, hip, cases, board=None, cbuf_of=None):
        self.hip, self.slots, self.b = hip, cases, board or Board(hip)
        self.cases = [c for c in cases if c is not None]
        for i, c in enumerate(self.cases):
            px = px_of(K.sc_is16(c))
            self.b.source(("csrc", c.name), K.scaled_source(c), skew=px * (1 + i % 5))
            for name, taps in ((c.tab_x, c.taps[0]), (c.tab_y, c.taps[1])):
                if ("tab", name, taps) not in self.b.off:
                    self.b.source(("tab", name, taps), K.sc_table(name, taps))
            if c.compound == 1:
                self.b.source(("cdst", c.name), np.full(64, 0x5A, np.uint8))        # a compound 1 descriptor never touches dst
                self.b.plane_out(("cbuf", c.name), c.h, c.w + 5, c.w, 2)
            else:
                self.b.plane_out(("cdst", c.name), c.h, c.w + 3, c.w, px)
                if c.compound:
                    self.b.source(("cbuf", c.name), K.scaled_cbuf(c) if cbuf_of is None else cbuf_of(c), skew=2)
        self.b.reserve("scale descriptors", len(cases) * C.sizeof(abi.ConvolveScaleDesc), self.descriptors)
        if board is None:
            self.b.upload()

    def desc(self, c):
        if c is None:
            return abi.ConvolveScaleDesc()
        r0, r1 = K.sc_rounds(c)
        src = K.scaled_source(c)
        d = abi.ConvolveScaleDesc(self.b.at(("csrc", c.name), (K.SC_MARGIN * src.shape[1] + K.SC_MARGIN) * src.itemsize), self.b.at(("cdst", c.name)),
                                  src.shape[1], c.w + 3, c.w, c.h, 0, self.b.at(("tab", c.tab_x, c.taps[0])), self.b.at(("tab", c.tab_y, c.taps[1])),
                                  c.sx, c.xs, c.sy, c.ys, c.taps[0], c.taps[1], r0, r1, c.bd, K.sc_is16(c), c.compound, c.fwd, c.bck)
        if c.compound:
            d.cbuf, d.cbuf_stride = self.b.at(("cbuf", c.name)), c.w + 5 if c.compound == 1 else c.w
        return d

    def descriptors(self):
        return np.frombuffer((abi.ConvolveScaleDesc * len(self.slots))(*[self.desc(c) for c in self.slots]), np.uint8)

    def launch(self, stream=None):
        return self.hip.svt_hip_convolve_scale_batch(self.b.at("scale descriptors"), len(self.slots), stream)

    def result(self, image, c):
        if c.compound == 1:
            return self.b.plane(image, ("cbuf", c.name), c.h, c.w + 5, c.w, np.uint16)
        return self.b.plane(image, ("cdst", c.name), c.h, c.w + 3, c.w, K.dtype_of(K.sc_is16(c)))

    def verify(self, image):
        for c in self.cases:
            assert np.array_equal(self.result(image, c), K.expected("scaled/" + c.name, lambda: K.restate_scaled(c))), c.name


@pytest.mark.parametrize("case", K.SCALED, ids=lambda c: c.name)
def test_scaled_prediction_equals_the_fixture(hip, case):
    call = ScaledCall(hip, [case])
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_convolve_scale_batch")
        image = call.b.image()
        call.verify(image)
        call.b.contained(image, "svt_hip_convolve_scale_batch " + case.name)


def test_one_batch_of_every_block_step_and_compound_kind_with_skipped_descriptors(hip):
    slots = []
    for i, c in enumerate(K.SCALED):
        slots += [c] + ([None] if i % 3 == 0 else [])
    call = ScaledCall(hip, [None] + slots)
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_convolve_scale_batch")
        image = call.b.image()
        call.verify(image)
        call.b.contained(image, "svt_hip_convolve_scale_batch, mixed batch")


@pytest.mark.parametrize("chain", K.CHAINS, ids=lambda ch: ch.name)
def test_scaled_first_and_unscaled_second_prediction_average_on_the_device(hip, chain):
    """A scaled compound 1 descriptor through svt_hip_convolve_scale_batch, then an un-scaled compound 2 / 3 descriptor of
    svt_hip_convolve_batch that reads its ConvBufType block: the reference's svt_av1_convolve_2d_scale_c and svt_av1_jnt_convolve_2d_c
    (or the highbd twins) in that order."""
    first, second = chain.first, chain.second
    call = ScaledCall(hip, [first], board=Board(hip))
    b, src2, px = call.b, K.scaled_source(second), px_of(K.sc_is16(second))
    b.source("second source", src2, skew=px)
    b.plane_out("chain dst", second.h, second.w + 3, second.w, px)
    r0, r1 = K.sc_rounds(second)

    def unscaled():
        d = abi.ConvolveDesc(b.at("second source", (K.SC_MARGIN * src2.shape[1] + K.SC_MARGIN) * px), b.at("chain dst"), src2.shape[1], second.w + 3,
                             second.w, second.h)
        d.filter_x[:] = conv_cases.TABLES[second.tab_x][second.sx >> 6]
        d.filter_y[:] = conv_cases.TABLES[second.tab_y][second.sy >> 6]
        d.taps_x = d.taps_y = 8
        d.round_0, d.round_1, d.bit_depth, d.is_16bit, d.compound = r0, r1, second.bd, K.sc_is16(second), second.compound
        d.fwd_offset, d.bck_offset, d.cbuf, d.cbuf_stride = second.fwd, second.bck, b.at(("cbuf", first.name)), first.w + 5
        return np.frombuffer(d, np.uint8)

    b.reserve("unscaled descriptor", C.sizeof(abi.ConvolveDesc), unscaled)
    b.upload()
    want = K.expected("chain/" + chain.name, lambda: K.restate_chain(chain))
    for _ in range(2):
        run(hip, call.launch(), "svt_hip_convolve_scale_batch")
        run(hip, hip.svt_hip_convolve_batch(b.at("unscaled descriptor"), 1, None), "svt_hip_convolve_batch")
        image = b.image()
        call.verify(image)
        assert np.array_equal(b.plane(image, "chain dst", second.h, second.w + 3, second.w, K.dtype_of(K.sc_is16(second))), want), chain.name
        b.contained(image, "scaled then un-scaled " + chain.name)


# ---- streams, empty and refused calls ----------------------------------------------------------------------------------------------

def test_three_entry_points_on_two_streams_at_once(hip):
    streams = []
    for _ in range(2):
        s = C.c_void_p()
        run(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
        streams.append(s)
    picks = [(["d9_131x37_8bit", "d12_322x98_10bit"], K.SUPERRES_MIXED[:2], K.SCALED[:8]),
             (["d16_131x37_10bit", "up_66x19_to_131x37", "tiny_7x5_to_13x9"], K.SUPERRES_MIXED[2:], K.SCALED[8:20])]
    sides = []
    for rz, sr, sc in picks:
        b = Board(hip)
        calls = [ResizeCall(hip, [K.RESIZE_BY_NAME[n] for n in rz], b), SuperresCall(hip, [K.SUPERRES_BY_NAME[n] for n in sr], b), ScaledCall(hip, sc, b)]
        b.upload()
        sides.append((b, calls))
    try:
        for _ in range(2):
            for k in range(3):                      # the two streams' calls alternate, nothing waits in between
                for (b, calls), s in zip(sides, streams):
                    run(hip, calls[k].launch(s), K.STATUS_NAMES[k])
            for s in streams:
                run(hip, hip.svt_hip_stream_sync(s), "svt_hip_stream_sync")
            for i, (b, calls) in enumerate(sides):
                image = b.image()
                for call in calls:
                    call.verify(image)
                b.contained(image, f"stream {i}")
    finally:
        for s in streams:
            hip.svt_hip_stream_destroy(s)


def test_empty_and_refused_calls_write_nothing(hip):
    case = K.RESIZE_BY_NAME["d9_131x37_8bit"]
    call = ResizeCall(hip, [case])
    before = call.b.image()
    jobs = call.jobs()
    assert hip.svt_hip_resize_planes(jobs, 0, None, 0, None) == 0
    assert hip.svt_hip_resize_planes(jobs, 1, call.b.at("resize workspace"), call.ws_bytes - 1, None) == K.BAD_PARAMETER
    assert b"svt_hip_resize_planes" in hip.svt_hip_last_error()
    jobs[0].dst_width = 20                          # 131 -> 20: three halvings
    assert hip.svt_hip_resize_planes(jobs, 1, call.b.at("resize workspace"), call.ws_bytes, None) == K.BAD_PARAMETER
    assert b"halvings" in hip.svt_hip_last_error()
    sr = SuperresCall(hip, [K.SUPERRES[0]])
    job = (abi.SuperresPlane * 1)(sr.job(K.SUPERRES[0]))
    sr_before = sr.b.image()
    assert hip.svt_hip_superres_upscale_planes(job, 0, None) == 0
    job[0].tile_cols = 0
    assert hip.svt_hip_superres_upscale_planes(job, 1, None) == K.BAD_PARAMETER
    assert hip.svt_hip_convolve_scale_batch(call.b.at("resize workspace"), 0, None) == 0
    assert hip.svt_hip_convolve_scale_batch(None, 1, None) == K.BAD_PARAMETER
    run(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    assert np.array_equal(call.b.image(), before) and np.array_equal(sr.b.image(), sr_before)
