"""GPU parity: svt_hip_wiener_pick_plane (the Wiener decision of a plane on the device) against the fixture of the reference's own
leaves and against the same driver over the oracle's leaves, bit-exact, the doubles by their bit patterns; and the chain
statistics -> pick -> frame filter with no host step in between."""
import ctypes as C

import numpy as np
import pytest

import lr_cases as R
import wiener_pick_cases as K
from lf_cases import V
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
OUT = ("units", "result", "lr_units")
IDS = [c.name for c in K.CASES]


class Uploaded:
    """The planes of one case in device memory, its statistics as svt_hip_wiener_stats leaves them, and the pick's buffers."""

    def __init__(self, hip, x, stream=None, stats=True):
        self.x, self.prm, self.n = x, K.params(x), len(x.limits)
        self.dgd, self.src = device.DeviceBuffer(hip, x.dgd.nbytes), device.DeviceBuffer(hip, x.src.nbytes)
        self.dgd.upload(x.dgd), self.src.upload(x.src)
        self.dgd0 = self.dgd.ptr + (K.B * x.dgd.shape[1] + K.B) * x.dgd.itemsize          # sample (0, 0) of the plane
        self.units = K.wiener_units(x, self.dgd0, self.src.ptr)
        self.M, self.H = device.DeviceBuffer(hip, self.n * 49 * 8), device.DeviceBuffer(hip, self.n * 49 * 49 * 8)
        self.prev = None
        if x.prev is not None:
            self.prev = device.DeviceBuffer(hip, x.prev.nbytes)
            self.prev.upload(x.prev)
        self.pick = device.DeviceWienerPick(hip, self.n)
        if stats:
            self.stats(hip, stream)
            device.check(hip, hip.svt_hip_stream_sync(stream), "sync")

    def stats(self, hip, stream=None):
        c = self.x.case
        device.check(hip, hip.svt_hip_wiener_stats(self.units, self.n, c.win, c.is16, c.bd, V(self.M.ptr), V(self.H.ptr), stream), "svt_hip_wiener_stats")

    def run(self, hip, stream=None):
        device.check(hip, self.pick.run(self.prm, self.units, self.M.ptr, self.H.ptr, self.prev.ptr if self.prev else None, stream),
                     "svt_hip_wiener_pick_plane")

    def moments(self):
        return self.M.download(np.int64, (self.n, 49)), self.H.download(np.int64, (self.n, 49 * 49))


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The driver over the oracle's leaves, computed once for all tests of the module."""
    out = {}
    for c in K.CASES:
        x = K.make_inputs(c)
        out[c.name] = K.drive(x, K.OrcLeaves(x, orc))
    return out


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_case_equals_fixture_and_oracle(hip, oracle_results, case):
    u = Uploaded(hip, K.make_inputs(case))
    M0, H0 = u.moments()
    u.run(hip)
    got = u.pick.download()
    assert K.same(got, K.golden(case), OUT) == [], (got["result"], K.golden(case)["result"], got["units"], K.golden(case)["units"])
    assert K.same(got, oracle_results[case.name], OUT) == []
    M1, H1 = u.moments()
    assert np.array_equal(M0, M1) and np.array_equal(H0, H1), "d_M / d_H were modified"
    u.run(hip)      # a second call on the same workspace and outputs starts from its own clean state
    assert K.same(u.pick.download(), K.golden(case), OUT) == []


def test_two_streams_do_not_disturb_each_other(hip):
    cases = [K.CASES[0], K.CASES[5], K.CASES[3], K.CASES[9]]      # different planes, windows, controls and search lengths
    ups = [Uploaded(hip, K.make_inputs(c)) for c in cases]
    streams = []
    for _ in range(2):
        s = C.c_void_p()
        device.check(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
        streams.append(s)
    try:
        for i, u in enumerate(ups):     # two calls per stream, enqueued alternately, nothing waited for in between
            u.run(hip, streams[i % 2])
        for s in streams:
            device.check(hip, hip.svt_hip_stream_sync(s), "svt_hip_stream_sync")
        for c, u in zip(cases, ups):
            assert K.same(u.pick.download(), K.golden(c), OUT) == [], c.name
    finally:
        for s in streams:
            device.check(hip, hip.svt_hip_stream_destroy(s), "svt_hip_stream_destroy")


@pytest.mark.parametrize("case", [K.CASES[0], K.CASES[5], K.CASES[10]], ids=lambda c: c.name)
def test_stats_pick_filter_chain_stays_on_the_device(hip, orc, case):
    """svt_hip_wiener_stats -> svt_hip_wiener_pick_plane -> svt_hip_restoration_filter_frame with d_lr_units, enqueued back to back
    on one stream with nothing downloaded in between; the restored plane is the oracle's frame filter run with the fixture's units."""
    x = K.make_inputs(case)
    gold = K.golden(case)
    hu, vu, dst_stride = R.units_in(case.w, case.unit), R.units_in(case.h, case.unit), case.w + R.DST_EXTRA
    assert hu * vu == len(x.limits)

    def plane(src, dst, units):
        return abi.LrPlane(src, dst, x.dgd.shape[1], dst_stride, case.w, case.h, x.ss, x.ss, case.is16, case.bd, case.unit, hu, vu, units, 0, 0, 0, 1)
    want = np.zeros((case.h + 2, dst_stride), x.dgd.dtype)
    units = np.ascontiguousarray(gold["lr_units"])
    arr = (abi.LrPlane * 1)(plane(K.G.at(x.dgd), want.ctypes.data, units.ctypes.data))
    orc.orc_restoration_filter_frame(arr, C.c_uint32(1))
    u = Uploaded(hip, x, stats=False)
    d_dst = device.DeviceBuffer(hip, want.nbytes)
    d_dst.fill(0)
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    s = C.c_void_p()
    device.check(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
    try:
        u.stats(hip, s)
        u.run(hip, s)
        arr = (abi.LrPlane * 1)(plane(u.dgd0, d_dst.ptr, u.pick.lr_units.ptr))
        device.check(hip, hip.svt_hip_restoration_filter_frame(arr, C.c_uint32(1), s), "svt_hip_restoration_filter_frame")
        device.check(hip, hip.svt_hip_stream_sync(s), "svt_hip_stream_sync")
    finally:
        device.check(hip, hip.svt_hip_stream_destroy(s), "svt_hip_stream_destroy")
    assert K.same(u.pick.download(), gold, OUT) == []
    got = d_dst.download(x.dgd.dtype, want.shape)
    assert np.array_equal(got[:case.h, :case.w], want[:case.h, :case.w])
    inner = x.dgd[K.B:-K.B, K.B:-K.B]
    for (hs, he, vs, ve), lr in zip(x.limits, gold["lr_units"]):      # RESTORE_NONE units come out as copies, Wiener ones do not
        same = np.array_equal(got[vs:ve, hs:he], inner[vs:ve, hs:he])
        assert same == (lr["restoration_type"] == 0 or not (lr["hfilter"].any() or lr["vfilter"].any())), (hs, vs)


def test_previous_taps_outside_their_ranges_are_not_taken(hip, orc):
    """The launches are counted from the taps' coded ranges: a previous-frame record outside them is solved like a unit without one,
    also under the longest search, and every unit's search still ends."""
    x = K.make_inputs(K.CASES[3])
    x.refine, x.max_one = 1, 0
    first = int(np.flatnonzero(x.prev["restoration_type"] == 1)[0])
    x.prev[first]["hfilter"][1], x.prev[first]["hfilter"][5], x.prev[first]["hfilter"][3] = 100, 100, x.prev[first]["hfilter"][3] - 2 * (100 - int(x.prev[first]["hfilter"][1]))
    assert not K.prev_usable(x.case.win, x.prev[first]) and any(K.prev_usable(x.case.win, r) for r in x.prev)
    want = K.drive(x, K.OrcLeaves(x, orc))
    assert want["cover"][:, K.COVER.index("prev")].sum() >= 1 and want["cover"][first, K.COVER.index("prev")] == 0
    u = Uploaded(hip, x)
    u.run(hip)
    got = u.pick.download()
    assert K.same(got, want, OUT) == [], (got["units"], want["units"])


def test_rejections_launch_nothing(hip):
    x = K.make_inputs(K.CASES[0])
    u = Uploaded(hip, x)
    before = u.pick.download()
    ws_before = u.pick.workspace.download(np.uint8, (u.pick.workspace.nbytes,))
    good = dict(zip(K.ARGS, [None, None, u.M.ptr, u.H.ptr, u.pick.units.ptr, u.pick.result.ptr, u.pick.lr_units.ptr, u.pick.workspace.ptr]))
    for label, change, limits, null, count, short in K.rejections(x):
        prm, units = K.params(x), K.wiener_units(x, u.dgd0, u.src.ptr)
        for k, v in change.items():
            setattr(prm, k, v)
        for k, v in limits.items():
            setattr(units[0], k, v)
        a = dict(good, prm=C.addressof(prm), units=C.addressof(units))
        if null:
            a[null] = None
        rc = hip.svt_hip_wiener_pick_plane(a["prm"], a["units"], u.n if count is None else count, a["d_M"], a["d_H"], None, a["d_unit_records"],
                                           a["d_result"], a["d_lr_units"], a["d_workspace"], u.pick.workspace.nbytes - short, None)
        assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER, label
        assert b"svt_hip_wiener_pick_plane" in hip.svt_hip_last_error(), label
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert K.same(u.pick.download(), before, OUT) == []
    assert np.array_equal(u.pick.workspace.download(np.uint8, (u.pick.workspace.nbytes,)), ws_before)
    u.run(hip)                          # and the same buffers serve a good call afterwards
    assert K.same(u.pick.download(), K.golden(x.case), OUT) == []
