"""GPU parity: svt_hip_cdef_pick_strengths (finish_cdef_search on the device) against the fixture of the reference's own
svt_search_one_dual and against the same driver over the oracle's leaf, bit-exact; and the search -> pick -> apply chain with no
host step in between."""
import ctypes as C

import numpy as np
import pytest

import cdef_pick_cases as K
import lf_cases as L
from lf_cases import P, V
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
OUT = ("result", "fb_gi", "fb_strength")
IDS = [c.name for c in K.CASES]


class Uploaded:
    """The tables and the skip map of one case in device memory."""

    def __init__(self, hip, x):
        self.x, self.prm = x, K.params(x)
        self.mse, self.filt = device.DeviceBuffer(hip, x.mse.nbytes), device.DeviceBuffer(hip, x.filt.nbytes)
        self.mse.upload(x.mse), self.filt.upload(x.filt)
        self.pick = device.DeviceCdefPick(hip, x.n_fb, x.case.n)

    def run(self, hip, stream=None):
        device.check(hip, self.pick.run(self.prm, self.mse.ptr, self.filt.ptr, stream), "svt_hip_cdef_pick_strengths")


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The driver over the oracle's leaf, computed once for all tests of the module."""
    search = K.orc_search(orc)
    return {c.name: K.drive(K.make_inputs(c), search) for c in K.CASES}


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_case_equals_fixture_and_oracle(hip, oracle_results, case):
    x = K.make_inputs(case)
    u = Uploaded(hip, x)
    u.run(hip)
    got = u.pick.download()
    assert K.same(got, K.golden(case), OUT) == [], (got["result"], K.golden(case)["result"])
    assert K.same(got, oracle_results[case.name], OUT) == []
    assert np.array_equal(u.mse.download(np.uint64, x.mse.shape), x.mse), "d_mse was modified"
    u.run(hip)      # a second call on the same workspace and outputs starts from its own clean state
    assert K.same(u.pick.download(), K.golden(case), OUT) == []


def test_two_streams_do_not_disturb_each_other(hip):
    cases = [K.CASES[12], K.CASES[19], K.CASES[5], K.CASES[15]]      # different grids, list lengths and step times
    streams, ups = [], [Uploaded(hip, K.make_inputs(c)) for c in cases]
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


def test_rejections_launch_nothing(hip):
    x = K.make_inputs(K.CASES[3])
    u = Uploaded(hip, x)
    before = u.pick.download()
    ws_before = u.pick.workspace.download(np.uint8, (u.pick.workspace.nbytes,))
    args = ("prm", u.mse.ptr, u.filt.ptr, u.pick.result.ptr, u.pick.fb_gi.ptr, u.pick.fb_strength.ptr, u.pick.workspace.ptr)
    for label, change, null, short in K.rejections(x):
        prm = K.rejected_params(x, change)
        a = [C.addressof(prm)] + list(args[1:])
        if null:
            a[K.ARGS.index(null)] = None
        rc = hip.svt_hip_cdef_pick_strengths(*a, u.pick.workspace.nbytes - short, None)
        assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER, label
        assert b"svt_hip_cdef_pick_strengths" in hip.svt_hip_last_error(), label
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert K.same(u.pick.download(), before, OUT) == []
    assert np.array_equal(u.pick.workspace.download(np.uint8, (u.pick.workspace.nbytes,)), ws_before)
    u.run(hip)                          # and the same buffers serve a good call afterwards
    assert K.same(u.pick.download(), K.golden(x.case), OUT) == []


@pytest.mark.parametrize("bd,is16", [(8, 0), (10, 1)])
def test_search_pick_apply_chain_stays_on_the_device(hip, orc, bd, is16):
    """svt_hip_cdef_search_plane x3 -> svt_hip_cdef_pick_strengths -> svt_hip_cdef_apply_frame, enqueued back to back on one stream
    with no host step between them, on a 200x136 4:2:0 picture (4 x 3 filter blocks) with skipped 8x8 blocks; the output planes
    are the oracle's apply with the strengths the Python driver picks from the oracle's search tables."""
    rng = np.random.default_rng(40 + bd)
    lw8, lh8, cols, rows, cs, sub = 200, 136, 4, 3, bd - 8, 1
    w8, h8, n_fb = lw8 // 8, lh8 // 8, cols * rows
    dt = np.uint16 if is16 else np.uint8
    filt = (rng.random((h8, w8)) < 0.7).astype(np.uint8)
    filt[0:8, 8:16] = 0                                    # one filter block takes no part at all
    strengths = [0, 5, 18, 35, 63, 12, 1, 2]
    strengths_uv = [0, 4, -1, 34, 63, -1, 1, 3]
    n, damping = len(strengths), 3 + int(rng.integers(0, 3))
    prm_y, prm_uv = L.search_params(strengths, damping, cs, sub), L.search_params([-1 if u == -1 else s for s, u in zip(strengths, strengths_uv)], damping, cs, sub)
    planes = []
    for pli in range(3):
        w, h = lw8 >> (pli > 0), lh8 >> (pli > 0)
        recon = L.smooth_plane(rng, w + 11, h, bd).astype(dt)
        source = np.clip(recon.astype(np.int32) + rng.integers(-6, 7, size=recon.shape), 0, (1 << bd) - 1).astype(dt)
        planes.append((recon, source, w, h, int(pli > 0)))
    # the oracle's tables, the driver's decision, the oracle's apply
    mse_o, ldir, lvar = np.zeros((3, n_fb, n), np.uint64), np.zeros((n_fb, 64), np.uint8), np.zeros((n_fb, 64), np.int32)
    for pli, (recon, source, w, h, dec) in enumerate(planes):
        pl = abi.CdefPlane(recon.ctypes.data, source.ctypes.data, recon.shape[1], recon.shape[1], w, h, is16, dec, dec, pli)
        orc.orc_cdef_search_plane(C.byref(pl), P(filt), C.byref(prm_uv if pli else prm_y), P(mse_o[pli]), P(ldir), P(lvar))
    x = K.Inputs()
    x.case = K.Case("chain", cols, rows, n, 0, "picture", "most", 1, 62, 40 << cs, 0)
    x.n_fb, x.w8, x.h8, x.mse, x.filt, x.strengths, x.strengths_uv = n_fb, w8, h8, mse_o, filt, strengths, strengths_uv
    want = K.drive(x, K.orc_search(orc))
    expected = []
    for pli, (recon, source, w, h, dec) in enumerate(planes):
        out = np.zeros_like(recon)
        pl = abi.CdefPlane(recon.ctypes.data, out.ctypes.data, recon.shape[1], recon.shape[1], w, h, is16, dec, dec, pli)
        fbs = np.ascontiguousarray(want["fb_strength"][int(pli > 0)])
        orc.orc_cdef_apply_plane(C.byref(pl), P(filt), P(fbs), damping, cs, P(ldir), P(lvar))
        expected.append(out)
    # the device: uploads first, then five calls and no host step until the final synchronise
    d_filt, d_mse = device.DeviceBuffer(hip, filt.nbytes), device.DeviceBuffer(hip, mse_o.nbytes)
    d_dir, d_var = device.DeviceBuffer(hip, n_fb * 64), device.DeviceBuffer(hip, n_fb * 64 * 4)
    d_filt.upload(filt), d_mse.fill(0), d_dir.fill(0), d_var.fill(0)
    bufs = []
    for recon, source, w, h, dec in planes:
        b = [device.DeviceBuffer(hip, recon.nbytes) for _ in range(3)]
        b[0].upload(recon), b[1].upload(source), b[2].fill(0)
        bufs.append(b)
    pick = device.DeviceCdefPick(hip, n_fb, n)
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    arr = (abi.CdefPlane * 3)()
    for pli, (recon, source, w, h, dec) in enumerate(planes):
        pl = abi.CdefPlane(bufs[pli][0].ptr, bufs[pli][1].ptr, recon.shape[1], recon.shape[1], w, h, is16, dec, dec, pli)
        device.check(hip, hip.svt_hip_cdef_search_plane(C.byref(pl), d_filt.ptr, C.byref(prm_uv if pli else prm_y), d_mse.ptr + pli * n_fb * n * 8,
                                                        d_dir.ptr, d_var.ptr, None), "cdef_search")
        arr[pli] = abi.CdefPlane(bufs[pli][0].ptr, bufs[pli][2].ptr, recon.shape[1], recon.shape[1], w, h, is16, dec, dec, pli)
    device.check(hip, pick.run(K.params(x), d_mse.ptr, d_filt.ptr, None), "cdef_pick")
    st = (C.c_void_p * 3)(pick.fb_strength.ptr, pick.fb_strength.ptr + n_fb, pick.fb_strength.ptr + n_fb)
    device.check(hip, hip.svt_hip_cdef_apply_frame(arr, 3, d_filt.ptr, st, damping, cs, d_dir.ptr, d_var.ptr, None), "cdef_apply_frame")
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert np.array_equal(d_mse.download(np.uint64, mse_o.shape), mse_o)
    got = pick.download()
    assert K.same(got, want, OUT) == [], (got["result"], want["result"])
    off = np.flatnonzero((want["fb_strength"] == 0).all(axis=0))
    assert 0 < len(off) and (want["fb_gi"] != 0xFF).sum() == n_fb - 1
    for pli, (recon, source, w, h, dec) in enumerate(planes):
        out = bufs[pli][2].download(dt, recon.shape)
        assert np.array_equal(out[:, :w], expected[pli][:, :w]), pli
        for fb in off:                  # both strengths 0: the block comes out as a copy
            r0, c0, side = fb // cols * (64 >> dec), fb % cols * (64 >> dec), 64 >> dec
            assert np.array_equal(out[r0:r0 + side, c0:min(c0 + side, w)], recon[r0:r0 + side, c0:min(c0 + side, w)]), (pli, fb)
