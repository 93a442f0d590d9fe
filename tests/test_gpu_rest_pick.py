"""GPU parity: svt_hip_rest_pick_plane (the restoration decision of a plane with the self-guided filter on the device) against the
fixture of the reference's own leaves and against the same driver over the oracle's leaves, bit-exact, the doubles by their bit
patterns; and the chain statistics -> Wiener pick -> restoration pick -> frame filter with no host step in between."""
import ctypes as C

import numpy as np
import pytest

import lr_cases as R
import rest_pick_cases as K
from lf_cases import V
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
OUT = ("units", "result", "lr_units")
IDS = [c.name for c in K.CASES]
LAUNCHES = 4


class Uploaded:
    """The planes of one case in device memory, the Wiener unit records of the fixture (where the case has any) and the pick's buffers."""

    def __init__(self, hip, x, records=True):
        c = x.case
        self.x, self.prm, self.n = x, K.params(x), len(x.limits)
        self.dgd, self.src = device.DeviceBuffer(hip, x.dgd.nbytes), device.DeviceBuffer(hip, x.src.nbytes)
        self.dgd.upload(x.dgd), self.src.upload(x.src)
        self.dgd0 = self.dgd.ptr + (K.B * x.dgd.shape[1] + K.B) * x.dgd.itemsize          # sample (0, 0) of the plane
        self.units = K.wiener_units(x, self.dgd0, self.src.ptr)
        self.wrecs = None
        if c.win:
            self.wrecs = device.DeviceBuffer(hip, self.n * C.sizeof(abi.WienerPickUnit))
            if records:
                self.wrecs.upload(np.ascontiguousarray(K.golden(c)["wiener"]))
        self.pick = device.DeviceRestPick(hip, self.n, c.w, c.h, K.n_ep(c))
        device.check(hip, hip.svt_hip_stream_sync(None), "sync")

    def run(self, hip, stream=None):
        rc = self.pick.run(self.prm, self.units, self.wrecs.ptr if self.wrecs else None, stream)
        assert rc == LAUNCHES, (rc, hip.svt_hip_last_error())

    def inputs(self):
        return (self.dgd.download(self.x.dgd.dtype, self.x.dgd.shape), self.src.download(self.x.src.dtype, self.x.src.shape),
                self.wrecs.download(abi.WIENER_PICK_UNIT_DTYPE, (self.n,)) if self.wrecs else None)


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The driver over the oracle's leaves, computed once for all tests of the module."""
    return {c.name: K.drive_orc(K.make_inputs(c), orc) for c in K.CASES}


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_case_equals_fixture_and_oracle(hip, oracle_results, case):
    x = K.make_inputs(case)
    u = Uploaded(hip, x)
    u.run(hip)
    got = u.pick.download()
    gold = K.golden(case)
    assert K.same(got, gold, OUT) == [], (got["result"], gold["result"], got["units"], gold["units"])
    assert K.same(got, oracle_results[case.name], OUT) == []
    dgd, src, wrecs = u.inputs()
    assert np.array_equal(dgd, x.dgd) and np.array_equal(src, x.src), "the planes were modified"
    assert wrecs is None or wrecs.tobytes() == gold["wiener"].tobytes(), "the Wiener records were modified"
    u.run(hip)      # a second call on the same workspace and outputs starts from its own clean state
    assert K.same(u.pick.download(), gold, OUT) == []


def test_two_streams_do_not_disturb_each_other(hip):
    cases = [K.CASES[0], K.CASES[6], K.CASES[3], K.CASES[11]]      # different planes, bit depths, ep ranges and search lengths
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


@pytest.mark.parametrize("case", [K.CASES[0], K.CASES[6], K.CASES[14], K.CASES[2]], ids=lambda c: c.name)
def test_stats_picks_filter_chain_stays_on_the_device(hip, orc, case):
    """svt_hip_wiener_stats -> svt_hip_wiener_pick_plane -> svt_hip_rest_pick_plane -> svt_hip_restoration_filter_frame with d_lr_units,
    enqueued back to back on one stream with nothing downloaded in between (without a window: the last two alone); the restored plane
    is the oracle's frame filter run with the fixture's units."""
    x = K.make_inputs(case)
    gold = K.golden(case)
    hu, vu, dst_stride = R.units_in(case.w, case.unit), R.units_in(case.h, case.unit), case.w + R.DST_EXTRA
    assert hu * vu == len(x.limits)

    def plane(src, dst, units):
        return abi.LrPlane(src, dst, x.dgd.shape[1], dst_stride, case.w, case.h, x.ss, x.ss, case.is16, case.bd, case.unit, hu, vu, units, 0, 0, 0, 1)
    want = np.zeros((case.h + 2, dst_stride), x.dgd.dtype)
    units = np.ascontiguousarray(gold["lr_units"])
    arr = (abi.LrPlane * 1)(plane(K.W.G.at(x.dgd), want.ctypes.data, units.ctypes.data))
    orc.orc_restoration_filter_frame(arr, C.c_uint32(1))
    u = Uploaded(hip, x, records=False)
    n = u.n
    d_dst = device.DeviceBuffer(hip, want.nbytes)
    d_dst.fill(0)
    if case.win:
        M, H, wpick = device.DeviceBuffer(hip, n * 49 * 8), device.DeviceBuffer(hip, n * 49 * 49 * 8), device.DeviceWienerPick(hip, n)
        x.case, keep = x.wcase, x.case
        wprm = K.W.params(x)
        x.case = keep
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    s = C.c_void_p()
    device.check(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
    try:
        if case.win:
            device.check(hip, hip.svt_hip_wiener_stats(u.units, n, case.win, case.is16, case.bd, V(M.ptr), V(H.ptr), s), "svt_hip_wiener_stats")
            device.check(hip, wpick.run(wprm, u.units, M.ptr, H.ptr, None, s), "svt_hip_wiener_pick_plane")
            u.wrecs = wpick.units
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
    assert any(not np.array_equal(got[vs:ve, hs:he], inner[vs:ve, hs:he]) for hs, he, vs, ve in x.limits), "nothing was restored"
    for (hs, he, vs, ve), lr in zip(x.limits, gold["lr_units"]):      # RESTORE_NONE units come out as copies
        if lr["restoration_type"] == 0:
            assert np.array_equal(got[vs:ve, hs:he], inner[vs:ve, hs:he]), (hs, vs)


def test_rejections_launch_nothing(hip):
    x = K.make_inputs(K.CASES[0])
    u = Uploaded(hip, x)
    before = u.pick.download()
    ws_before = u.pick.workspace.download(np.uint8, (u.pick.workspace.nbytes,))
    good = dict(zip(K.ARGS[2:], [u.pick.units.ptr, u.pick.result.ptr, u.pick.lr_units.ptr, u.pick.workspace.ptr]), dgd=u.dgd0, src=u.src.ptr)
    for rej in K.rejections(x):
        rc = K.call_rejection(hip, x, rej, good, u.n, u.wrecs.ptr, u.pick.workspace.nbytes)
        assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER, rej[0]
        assert b"svt_hip_rest_pick_plane" in hip.svt_hip_last_error(), rej[0]
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert K.same(u.pick.download(), before, OUT) == []
    assert np.array_equal(u.pick.workspace.download(np.uint8, (u.pick.workspace.nbytes,)), ws_before)
    u.run(hip)                          # and the same buffers serve a good call afterwards
    assert K.same(u.pick.download(), K.golden(x.case), OUT) == []
