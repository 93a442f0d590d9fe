"""GPU parity: svt_hip_palette_search_batch, svt_hip_palette_predict_batch and svt_hip_sc_classify against the fixture of the reference's
own search_palette_luma, rate functions and svt_aom_is_screen_content (tests/golden/palette.npz): records, maps, predictions and the
classifier's record byte for byte.  Every plane, table, record, map and prediction of a test lives in one guarded arena: a byte written
outside the declared outputs fails the test.  Every test makes its calls twice, and both runs must give the fixture."""
import ctypes as C

import numpy as np
import pytest

import palette_cases as K
from arena import PATTERN, Arena, check_containment, rows
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
REC = K.RECORD_BYTES
CAND0 = abi.PaletteRecord.cand.offset + abi.PaletteCand.palette_colors.offset       # palette_colors of candidate 0 inside a record


class Uploaded:
    """The rate table, the source of every case (a plane of its own at a ragged offset with an odd stride, or one plane per bit depth that
    all its cases share), one record and one map storage per case, and whatever `extra` adds, in ONE device buffer."""

    def __init__(self, hip, names, shared=False, extra=None):
        self.hip, self.cases = hip, [K.CASE[n] for n in names]
        a, self.off, self.src = Arena(fill=PATTERN, tail=512), {}, {}
        self.off["rates"] = a.add("rate table", np.frombuffer(K.rates_struct(*K.golden_rates()), np.uint8), skew=4)
        if shared:
            for bd in sorted({c.bd for c in self.cases}):
                mine = [c for c in self.cases if c.bd == bd]
                stride, x, y, put = 163, 1, 3, []
                for c in mine:              # left to right, a new band when the row is full; odd origins
                    if x + c.w > stride - 2:
                        x, y = 1, y + 64 + 1
                    put.append((c, x, y))
                    x += c.w + 2 * (len(put) % 2) + 2
                plane = np.full((y + 65, stride), 77, np.uint8 if bd == 8 else np.uint16)
                for c, x, y in put:
                    plane[y:y + c.h, x:x + c.w] = K.make_block(c)
                off = a.add(f"shared plane, {bd} bit", plane, skew=2 * (1 + bd % 3))
                for c, x, y in put:
                    self.src[c.name] = (off, stride, x, y)
        else:
            for i, c in enumerate(self.cases):
                blk = K.make_block(c)
                stride, x, y = c.w + 5 + 2 * (i % 3), 1 + i % 4, i % 3
                plane = np.full((c.h + y, stride), 33, blk.dtype)
                plane[y:, x:x + c.w] = blk
                self.src[c.name] = (a.add("plane " + c.name, plane, skew=2 * (i % 5)), stride, x, y)
        self.outputs = []
        for i, c in enumerate(self.cases):
            n_cands = len(K.golden_record(c.name)[1])
            self.off["rec", c.name] = a.add("record " + c.name, nbytes=REC, skew=8 * (i % 4))
            self.off["maps", c.name] = a.add("maps " + c.name, nbytes=K.MAX_CANDS * c.w * c.h, skew=4 * (i % 3))
            self.outputs += [(self.off["rec", c.name], REC), (self.off["maps", c.name], n_cands * c.w * c.h)]     # the unused slots stay
        if extra:
            extra(self, a)
        self.arena, self.before = a, a.build()
        self.buf = device.DeviceBuffer(hip, self.before.nbytes)
        self.buf.upload(self.before)

    def at(self, *key):
        return self.buf.ptr + self.off[key if len(key) > 1 else key[0]]

    def search(self, stream=None):
        """One call per (bit depth, step, max_itr) among the cases"""
        for (bd, step, max_itr), cases in K.groups([c.name for c in self.cases]).items():
            ctrls = abi.PaletteCtrls(self.at("rates"), step, bd, max_itr)
            descs = (abi.PaletteDesc * len(cases))(*[K.desc(c, self.buf.ptr + self.src[c.name][0], *self.src[c.name][1:], self.at("rec", c.name),
                                                            self.at("maps", c.name)) for c in cases])
            device.check(self.hip, self.hip.svt_hip_palette_search_batch(C.byref(ctrls), descs, len(cases), stream), "svt_hip_palette_search_batch")

    def image(self):
        return self.buf.download(np.uint8, (self.before.nbytes,))

    def assert_fixture(self, image):
        for c in self.cases:
            rec, maps = K.golden_record(c.name)
            o = self.off["rec", c.name]
            got = image[o:o + REC]
            assert np.array_equal(got, rec), (c.name, got.view(abi.PALETTE_RECORD_DTYPE), rec.view(abi.PALETTE_RECORD_DTYPE))
            o = self.off["maps", c.name]
            assert np.array_equal(image[o:o + maps.size], maps.reshape(-1)), c.name


def run_twice(u, what, stream=None):
    for _ in range(2):
        u.search(stream)
        if stream is not None:
            device.check(u.hip, u.hip.svt_hip_stream_sync(stream), "svt_hip_stream_sync")
        image = u.image()
        u.assert_fixture(image)
        check_containment(u.before, image, u.arena.regions, u.outputs, what)
    return image


@pytest.mark.parametrize("name", [c.name for c in K.CASES])
def test_search_equals_the_fixture(hip, name):
    run_twice(Uploaded(hip, [name]), "svt_hip_palette_search_batch " + name)


def test_one_batch_of_all_sizes_steps_and_candidate_counts(hip):
    names = [c.name for c in K.CASES if c.name.startswith("s")] + ["colors_1", "colors_2", "colors_65", "one_cand", "full_12", "full_12_10", "colors_8"]
    counts = {len(K.golden_record(n)[1]) for n in names}
    assert {0, 1, 12} <= counts and {K.CASE[n].step for n in names} == {1, 2} and {(K.CASE[n].w, K.CASE[n].h) for n in names} == set(K.SIZES)
    assert len(K.groups(names)) == 4         # 8 and 10 bit, both steps: four calls, each a batch of many sizes
    run_twice(Uploaded(hip, names), "svt_hip_palette_search_batch, mixed batch")


def test_descriptors_share_a_plane_at_ragged_offsets(hip):
    names = ["s64x64_8", "s8x8_8", "s16x64_8", "short_9x13", "short_3x5", "tie_top", "empties", "s32x8_8", "s64x16_10", "s16x32_10", "empties_10", "cache_10"]
    u = Uploaded(hip, names, shared=True)
    assert len({u.src[n][0] for n in names}) == 2 and all(u.src[n][1] % 2 and u.src[n][2] % 2 for n in names)
    run_twice(u, "svt_hip_palette_search_batch, shared planes")


def test_search_on_a_stream_of_the_callers(hip):
    s = C.c_void_p()
    device.check(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
    try:
        run_twice(Uploaded(hip, ["s32x32_8", "s64x32_10", "itr_1", "itr_2", "itr_50", "dups"]), "svt_hip_palette_search_batch, own stream", s)
    finally:
        device.check(hip, hip.svt_hip_stream_destroy(s), "svt_hip_stream_destroy")


def test_prediction_reads_what_the_search_left(hip):
    dst_stride = 70

    def extra(u, a):
        descs = np.zeros(len(K.PREDS), abi.PALETTE_PRED_DESC_DTYPE)
        for i, p in enumerate(K.PREDS):
            u.off["dst", p.name] = a.add("prediction " + p.name, nbytes=p.h * dst_stride * (1 + p.is_16bit), skew=2 * (i % 3))
            u.outputs += rows(u.off["dst", p.name], dst_stride * (1 + p.is_16bit), p.w * (1 + p.is_16bit), p.h)
        u.off["descs"] = a.add("prediction descriptors", descs)
        u.n_descs = len(descs)

    u = Uploaded(hip, list(dict.fromkeys(p.case for p in K.PREDS)), extra=extra)
    descs = np.zeros(len(K.PREDS), abi.PALETTE_PRED_DESC_DTYPE)
    for i, p in enumerate(K.PREDS):
        c = K.CASE[p.case]
        d = descs[i]
        d["map"], d["colors"] = u.at("maps", p.case) + p.cand * c.w * c.h, u.at("rec", p.case) + CAND0 + p.cand * C.sizeof(abi.PaletteCand)
        d["dst"], d["dst_stride"], d["map_width"], d["is_16bit"], d["bit_depth"] = u.at("dst", p.name), dst_stride, c.w, p.is_16bit, p.bd
        d["x"], d["y"], d["w"], d["h"] = p.x, p.y, p.w, p.h
    device.check(hip, hip.svt_hip_upload(u.at("descs"), descs.ctypes.data, descs.nbytes, None), "svt_hip_upload")
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    o = u.off["descs"]
    u.before[o:o + descs.nbytes] = descs.view(np.uint8).reshape(-1)
    for _ in range(2):
        u.search()          # the prediction follows on the same stream, nothing waited for
        device.check(hip, hip.svt_hip_palette_predict_batch(u.at("descs"), len(descs), None), "svt_hip_palette_predict_batch")
        image = u.image()
        u.assert_fixture(image)
        for p in K.PREDS:
            want, o = K.golden_pred(p), u.off["dst", p.name]
            got = image[o:o + p.h * dst_stride * want.itemsize].view(want.dtype).reshape(p.h, dst_stride)[:, :p.w]
            assert np.array_equal(got, want), p.name
        check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_palette_predict_batch")
    assert K.golden_pred(K.PREDS[5]).max() == 1023 and K.golden_pred(K.PREDS[6]).dtype == np.uint16


@pytest.mark.parametrize("plane", K.SC_PLANES, ids=lambda p: p.name)
def test_classifier_equals_the_fixture(hip, plane):
    a = Arena(fill=PATTERN, tail=512)
    off = a.add("plane", K.make_sc_plane(plane), skew=3)
    out = a.add("record", nbytes=C.sizeof(abi.ScClass), skew=4)
    before = a.build()
    buf = device.DeviceBuffer(hip, before.nbytes)
    buf.upload(before)
    for _ in range(2):
        device.check(hip, hip.svt_hip_sc_classify(buf.ptr + off, plane.w, plane.h, plane.stride, buf.ptr + out, None), "svt_hip_sc_classify")
        image = buf.download(np.uint8, (before.nbytes,))
        assert np.array_equal(image[out:out + C.sizeof(abi.ScClass)], K.gold()["sc_" + plane.name]), image[out:out + 24].view(abi.SC_CLASS_DTYPE)
        check_containment(before, image, a.regions, [(out, C.sizeof(abi.ScClass))], "svt_hip_sc_classify " + plane.name)


def test_refused_calls_write_nothing(hip):
    u = Uploaded(hip, ["colors_3"])
    c = K.CASE["colors_3"]
    before = u.image()
    good = K.desc(c, u.buf.ptr + u.src[c.name][0], *u.src[c.name][1:], u.at("rec", c.name), u.at("maps", c.name))
    for field, value in (("rows", 17), ("width", 12), ("left_n", 9)):
        d = abi.PaletteDesc.from_buffer_copy(good)
        setattr(d, field, value)
        ctrls = abi.PaletteCtrls(u.at("rates"), 1, 8, 50)
        assert hip.svt_hip_palette_search_batch(C.byref(ctrls), (abi.PaletteDesc * 2)(good, d), 2, None) == K.BAD_PARAMETER, field
        assert b"svt_hip_palette_search_batch: descriptor 1" in hip.svt_hip_last_error()
    assert hip.svt_hip_sc_classify(u.at("rates"), 64, 64, 63, u.at("rec", c.name), None) == K.BAD_PARAMETER
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    assert np.array_equal(u.image(), before)
