"""GPU parity: svt_hip_dlf_pick_levels (search_filter_level on the device, all planes, no host step) against the fixture of the
reference's own svt_av1_loop_filter_frame and full-distortion leaves and against the same driver over the oracle, bit-exact; and the
chain pick -> svt_hip_dlf_apply_picked with no host step in between."""
import ctypes as C

import numpy as np
import pytest

import dlf_pick_cases as K
from arena import PATTERN, Arena, check_containment
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
IDS = [c.name for c in K.CASES]
REC = ("record",)


class Uploaded:
    """One case in ONE device buffer: the six padded planes at ragged offsets, the mode info, the result record and the workspace,
    everything in between a pattern that nobody may change (arena.check_containment)."""

    def __init__(self, hip, x):
        self.hip, self.x = hip, x
        a, item = Arena(fill=PATTERN, tail=512), x.recon[0].itemsize
        self.off = {}
        for p in range(3):
            self.off["recon", p] = a.add(f"recon{p}", x.recon[p], skew=item * (3 + 2 * p))
            self.off["src", p] = a.add(f"src{p}", x.src[p], skew=item * (5 + p))
        self.off["mi"] = a.add("mi", x.flat.view(np.uint8))
        self.ws_bytes = hip.svt_hip_dlf_pick_workspace_bytes(x.case.w, x.case.h, x.case.is16)
        self.off["record"], self.off["ws"] = a.add("record", nbytes=abi.DLF_PICK_RESULT_BYTES), a.add("workspace", nbytes=self.ws_bytes)
        self.arena, self.before = a, a.build()
        self.buf = device.DeviceBuffer(hip, self.before.nbytes)
        self.buf.upload(self.before)
        self.pick = device.DeviceDlfPick(hip, x.case.w, x.case.h, x.case.is16, result=self.buf.ptr + self.off["record"],
                                         workspace=self.buf.ptr + self.off["ws"])
        self.outputs = [(self.off["record"], abi.DLF_PICK_RESULT_BYTES), (self.off["ws"], self.ws_bytes)]

    def at(self, kind, p):
        """(device address of the top-left picture sample, stride) of a plane"""
        a = self.x.recon[p]
        return self.buf.ptr + self.off[kind, p] + (K.PAD * a.shape[1] + K.PAD) * a.itemsize, a.shape[1]

    def params(self, **kw):
        return K.params(self.x, [self.at("recon", p) for p in range(3)], [self.at("src", p) for p in range(3)], self.buf.ptr + self.off["mi"], **kw)

    def run(self, stream=None, **kw):
        device.check(self.hip, self.pick.run(self.params(**kw), stream), "svt_hip_dlf_pick_levels")

    def image(self):
        return self.buf.download(np.uint8, (self.before.nbytes,))

    def record(self, image=None):
        image = self.image() if image is None else image
        return {"record": image[self.off["record"]:self.off["record"] + abi.DLF_PICK_RESULT_BYTES].view(K.RESULT_DTYPE)[0]}

    def plane(self, image, kind, p):
        a = self.x.recon[p]
        return image[self.off[kind, p]:self.off[kind, p] + a.nbytes].view(a.dtype).reshape(a.shape)


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The driver over the oracle's frame filter, computed once for all tests of the module."""
    out = {}
    for c in K.CASES:
        x = K.make_inputs(c)
        out[c.name] = K.drive(x, K.orc_filter(orc, x), K.numpy_sse(x))
    return out


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_case_equals_fixture_and_oracle(hip, oracle_results, case):
    u = Uploaded(hip, K.make_inputs(case))
    u.run()
    image = u.image()
    got, want = u.record(image), K.golden(case)
    assert K.same(got, want, REC) == [], (got["record"], want["record"])
    assert K.same(got, oracle_results[case.name], REC) == []
    # the planes, the mode info and everything around them are what they were: only the record and the workspace were written
    check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_dlf_pick_levels")
    u.run()      # a second call on the same record and workspace starts from its own clean state
    assert K.same(u.record(), want, REC) == []


def test_two_rounds_leave_the_search_unfinished(hip):
    case = K.CASE["tiles_8bit_harsh"]
    u = Uploaded(hip, K.make_inputs(case))
    u.run(max_rounds=2)
    image = u.image()
    short, full = u.record(image)["record"], K.golden(case)["record"]
    assert short["finished"] == 0 and (short["rounds"] == 2).all() and (full["rounds"] > 2).all()
    tried = short["ss_err"] >= 0
    assert (tried.sum(axis=1) == short["trials"]).all() and np.array_equal(short["ss_err"][tried], full["ss_err"][tried])
    assert (short["ss_err"][~tried] == -1).all()
    for p in range(3):      # the level is the best of what was measured, with its error
        assert short["ss_err"][p][short["level"][p]] >= 0 and short["best_err"][p] >= short["ss_err"][p][tried[p]].min()
    check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_dlf_pick_levels, two rounds")


def test_two_streams_do_not_disturb_each_other(hip):
    cases = [K.CASE[n] for n in ("tiles_8bit_blocky", "small_10bit_seg", "tiles_8in16_sb128", "tiles_10bit_chroma_only")]
    streams, ups = [], [Uploaded(hip, K.make_inputs(c)) for c in cases]
    for _ in range(2):
        s = C.c_void_p()
        device.check(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
        streams.append(s)
    try:
        for i, u in enumerate(ups):     # two calls per stream, enqueued alternately, nothing waited for in between
            u.run(streams[i % 2])
        for s in streams:
            device.check(hip, hip.svt_hip_stream_sync(s), "svt_hip_stream_sync")
        for c, u in zip(cases, ups):
            assert K.same(u.record(), K.golden(c), REC) == [], c.name
    finally:
        for s in streams:
            device.check(hip, hip.svt_hip_stream_destroy(s), "svt_hip_stream_destroy")


def test_rejections_launch_nothing(hip):
    x = K.make_inputs(K.CASE["small_10bit_seg"])
    u = Uploaded(hip, x)
    for label, change, null, short, applies in K.rejections(x):
        prm = u.params()
        if change:
            change(prm)
        args = [C.addressof(prm), u.pick.result, u.pick.workspace]
        if null:
            args[K.ARGS.index(null)] = None
        assert hip.svt_hip_dlf_pick_levels(*args, u.ws_bytes - short, None) == K.BAD_PARAMETER, label
        assert b"svt_hip_dlf_pick_levels" in hip.svt_hip_last_error(), label
        if applies:
            assert hip.svt_hip_dlf_apply_picked(*args[:2], None) == K.BAD_PARAMETER, label
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert np.array_equal(u.image(), u.before)      # record, workspace and planes untouched
    u.run()                                         # and the same buffers serve a good call afterwards
    assert K.same(u.record(), K.golden(x.case), REC) == []


@pytest.mark.parametrize("name", ["tiles_8bit_clean", "tiles_8bit_luma_only", "tiles_8in16_sb128"])
def test_pick_then_apply_stays_on_the_device(hip, orc, oracle_results, name):
    """svt_hip_dlf_pick_levels -> svt_hip_dlf_apply_picked on one stream with no host step; the planes must be the oracle's
    orc_loop_filter_frame at the levels the driver picks: the luma-0 case (nothing is filtered at all), a case whose chroma planes are
    not searched and take the host's levels, and a case with segment deltas."""
    case = K.CASE[name]
    x = K.make_inputs(case)
    want = oracle_results[name]["record"]
    levels = [int(v) for v in want["hdr_level"]]
    expected = [a.copy() for a in x.recon]
    K.orc_filter(orc, x)(expected, 0, 3, levels)
    u = Uploaded(hip, x)
    prm = u.params()
    device.check(hip, u.pick.run(prm), "svt_hip_dlf_pick_levels")
    device.check(hip, u.pick.apply(prm), "svt_hip_dlf_apply_picked")
    image = u.image()
    assert K.same(u.record(image), oracle_results[name], REC) == []
    for p in range(3):
        assert np.array_equal(u.plane(image, "recon", p), expected[p]), (name, p)
    if name == "tiles_8bit_clean":
        assert levels == [0, 0, 0, 0] and all(np.array_equal(expected[p], x.recon[p]) for p in range(3))
    else:
        assert all(not np.array_equal(expected[p], x.recon[p]) for p in range(3))
    if name == "tiles_8bit_luma_only":
        assert levels[2:] == list(K.HOST_LEVELS[2:]) and levels[0] == levels[1] == want["level"][0]
    # the source, the mode info and every byte around the planes are untouched; of the planes only picture samples may change
    planes = [(u.off["recon", p], x.recon[p].nbytes) for p in range(3)]
    check_containment(u.before, image, u.arena.regions, u.outputs + planes, "pick -> apply")
    for p in range(3):      # the padding of a filtered plane is the caller's
        mask = np.ones(x.recon[p].shape, bool)
        mask[K.PAD:K.PAD + (x.mi_rows * 4 >> (p > 0)), K.PAD:K.PAD + (x.mi_cols * 4 >> (p > 0))] = False
        assert np.array_equal(u.plane(image, "recon", p)[mask], x.recon[p][mask]), p
