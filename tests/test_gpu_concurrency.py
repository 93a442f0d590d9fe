"""GPU: the concurrency contract of include/svt_hip.h — every function thread-safe and re-entrant, every Tier B entry point
asynchronous on the caller's stream — against the oracle, the reference's golden data and the committed fixtures, bit-exact.

Every expected result is computed serially in the main thread before any GPU call or thread starts; a test never only compares
two GPU runs with each other.  The library's state shared between calls is what is under test: the per-thread staging ring of
host descriptor arrays (4 slots), the per-thread Tier A scratch, the pool of 8 streams behind stream = NULL, the grow-only
buffers of the Wiener statistics and of the grouped transform path, and caller-owned workspaces reused across jobs."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import conv_cases as K
import intra_cases as I
import leaf_cases as LC
import lf_cases as L
import lr_cases as R
import me_cases
import sgr_cases as G
import test_lf_oracle as TL
import tf_picture_cases as tpc
import tpl_cases as TP
import tx_cases as T
from arena import GUARD
from lf_cases import BS, HB, VB
from svtav1_hip import abi, device, frames
from test_gpu_lf import deblock_inputs
from test_gpu_txfm import hip_inverse
from test_leaves_oracle import orc_residual, orc_sse

pytestmark = pytest.mark.gpu
V = C.c_void_p
HERE = os.path.dirname(os.path.abspath(__file__))
N_THREADS = 24   # more than the pool of 8 streams behind stream = NULL


def P(a):
    return V(a.ctypes.data)


def enc16(addr):
    return V(addr >> 1)      # CONVERT_TO_BYTEPTR, as the reference's callers pass uint16 buffers


@pytest.fixture(scope="module")
def gold_intra():
    return np.load(I.GOLD)


def new_stream(hip):
    s = V()
    device.check(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
    return s.value


def sync(hip, *streams):
    for s in streams:
        device.check(hip, hip.svt_hip_stream_sync(V(s)), "svt_hip_stream_sync")


def destroy(hip, *streams):
    for s in streams:
        device.check(hip, hip.svt_hip_stream_destroy(V(s)), "svt_hip_stream_destroy")


def settle(hip):
    """Set-up fills device buffers on the calling thread's pool stream; a call on another stream must not overtake them."""
    sync(hip, None)


# ------------------------------------------------------------------------------------------------ Tier B cases
# Each case computes its expectation in __init__; issue(stream) makes the call without waiting and returns the host descriptor
# array it passed (dead the moment the call returns) or None; check() compares once the caller has synchronised the stream.
class WienerCase:
    def __init__(self, hip, orc, w, h, bd, is16, win, unit, seed):
        self.hip, self.win, self.args = hip, win, (win, is16, bd)
        rng = np.random.default_rng(seed)
        dat, src = G.sgr_plane(rng, w, h, bd, is16, 0)
        self.d_dat, self.d_src = device.DeviceBuffer(hip, dat.nbytes), device.DeviceBuffer(hip, src.nbytes)
        self.d_dat.upload(dat), self.d_src.upload(src)
        off = (G.B * dat.shape[1] + G.B) * dat.itemsize
        self.limits = [(x, min(x + unit, w), y, min(y + unit, h)) for y in range(0, h, unit) for x in range(0, w, unit)]
        n = len(self.limits)
        self.units = [abi.WienerUnit(self.d_dat.ptr + off, self.d_src.ptr + off, dat.shape[1], src.shape[1], *lim) for lim in self.limits]
        self.want_M, self.want_H = np.zeros((n, 49), np.int64), np.zeros((n, 49 * 49), np.int64)
        for i, (hs, he, vs, ve) in enumerate(self.limits):
            orc.orc_wiener_compute_stats(win, V(G.at(dat)), V(G.at(src)), hs, he, vs, ve, dat.shape[1], src.shape[1], P(self.want_M[i]),
                                         P(self.want_H[i]), is16, bd)
        self.dM, self.dH = device.DeviceBuffer(hip, n * 49 * 8), device.DeviceBuffer(hip, n * 49 * 49 * 8)
        self.dM.fill(0x5A), self.dH.fill(0x5A)
        settle(hip)

    def issue(self, stream):
        win, is16, bd = self.args
        arr = (abi.WienerUnit * len(self.units))(*self.units)
        device.check(self.hip, self.hip.svt_hip_wiener_stats(arr, len(self.units), win, is16, bd, V(self.dM.ptr), V(self.dH.ptr), V(stream)),
                     "svt_hip_wiener_stats")
        return arr

    def check(self, what=""):
        n, w2 = len(self.limits), self.win * self.win
        M, H = self.dM.download(np.int64, (n, 49)), self.dH.download(np.int64, (n, 49 * 49))
        bad_M = int((M[:, :w2] != self.want_M[:, :w2]).sum())
        bad_H = int((H.reshape(n, 49, 49)[:, :w2, :w2] != self.want_H.reshape(n, 49, 49)[:, :w2, :w2]).sum())
        assert bad_M == 0 and bad_H == 0, f"{what}: wiener_stats: {bad_M} M and {bad_H} H entries differ from the oracle ({n} units)"


class MeCase:
    def __init__(self, hip, orc, kind, w, h, key, seed):
        self.hip = hip
        cur, l0, l1 = 2, [1, 0], [3, 4]
        pyrs = me_cases.build_pyramids(orc, me_cases.make_clip(kind, w, h, 5, seed=seed))
        prm = me_cases.scenario_params(key, cur, l0, l1)
        self.want = me_cases.run_cpu(orc.orc_me_frame_range, prm, pyrs, cur, l0, l1, w, h)
        self.dpyr = [device.DevicePyramid(hip, p) for p in pyrs]
        self.out = device.DeviceMeOut(hip, prm, frames.b64_count(w, h))
        self.job = me_cases.host_job(prm, self.dpyr, cur, l0, l1, self.out.desc())
        settle(hip)

    def issue(self, stream):
        arr = (abi.MeFrameJob * 1)(self.job)
        device.check(self.hip, self.hip.svt_hip_me_frames(arr, C.c_uint32(1), V(stream)), "svt_hip_me_frames")
        return arr

    def check(self, what=""):
        me_cases.assert_same(self.want, self.out.download(), f"{what}: me_frames")


class AnalysisCase:
    def __init__(self, hip, orc, sizes, l1, fp, seed):
        self.hip, self.l1, self.fp, self.keep, self.jobs = hip, l1, fp, [], []
        for i, (w, h) in enumerate(sizes):
            clip = me_cases.make_clip("pan", w, h, 1, seed=seed + i)
            hp = frames.HostPyramid(clip[0])
            d = hp.desc()
            orc.orc_pyramid_frame(C.byref(d.full), C.byref(d.quarter), C.byref(d.sixteenth), l1)
            nb = frames.b64_count(w, h)
            v1, m1 = np.zeros((nb, 85), np.uint16), np.zeros((nb, 85), np.uint64)
            orc.orc_variance_frame(C.byref(d.full), v1.ctypes.data_as(V), m1.ctypes.data_as(V), fp)
            dp = device.DevicePyramid(hip, frames.HostPyramid(clip[0]))
            dv, dm = device.DeviceBuffer(hip, v1.nbytes), device.DeviceBuffer(hip, m1.nbytes)
            self.jobs.append(abi.AnalysisJob(dp.desc(), dv.ptr, dm.ptr))
            self.keep.append((hp, v1, m1, dp, dv, dm))
        settle(hip)

    def issue(self, stream):
        arr = (abi.AnalysisJob * len(self.jobs))(*self.jobs)
        device.check(self.hip, self.hip.svt_hip_analysis_frames(arr, len(self.jobs), self.l1, self.fp, V(stream)), "svt_hip_analysis_frames")
        return arr

    def check(self, what=""):
        for i, (hp, v1, m1, dp, dv, dm) in enumerate(self.keep):
            if self.l1:
                assert np.array_equal(dp.quarter.download(), hp.quarter.buf), (what, "quarter", i)
            assert np.array_equal(dp.sixteenth.download(), hp.sixteenth.buf), (what, "sixteenth", i)
            assert np.array_equal(dv.download(np.uint16, v1.shape), v1), (what, "variance", i)
            assert np.array_equal(dm.download(np.uint64, m1.shape), m1), (what, "mean", i)


class IntraCase:
    """Expected results: the golden fixture recorded from the reference's own functions."""

    def __init__(self, hip, gold, case):
        self.hip, self.gold, self.case = hip, gold, case
        plane = I.case_plane(case, I.ALL_CASES.index(case))
        self.buf = device.DeviceBuffer(hip, plane.buf.nbytes)
        self.buf.upload(plane.buf)
        self.out = device.DeviceIntraOut(hip, plane.width, plane.height, all_modes=case in I.CASES)
        self.job = abi.IntraSearchJob()
        self.job.src, self.job.ctrls = plane.desc(self.buf.ptr), I.case_ctrls(case)
        self.out.fill_job(self.job)
        settle(hip)

    def issue(self, stream):
        arr = (abi.IntraSearchJob * 1)(self.job)
        device.check(self.hip, self.hip.svt_hip_intra_search_frames(arr, C.c_uint32(1), V(stream)), "svt_hip_intra_search_frames")
        return arr

    def check(self, what=""):
        got = self.out.download()
        if "pred" in got:   # predictions of unsearched modes and blocks stay at the 0xA5 fill; the oracle leaves them at 0
            end, searched = self.case[4], got["best_mode"] != I.NOT_SEARCHED
            assert (got["pred"][searched][:, end + 1:] == GUARD).all() and (got["pred"][~searched] == GUARD).all(), (what, self.case[0])
            got["pred"][~searched] = 0
            got["pred"][:, :, end + 1:] = 0
        I.check_against_golden(self.gold, self.case[0], got)


def tf_case(name):
    return next(c for c in tpc.CASES if c[0] == name)


class TfCase:
    def __init__(self, hip, orc, case, decay=None, ws=None):
        self.hip, self.case = hip, case
        name, kind, w, h, n_refs, bd, key, ctl = case
        if decay is None:
            decay = tuple(int(x) for x in np.load(tpc.GOLD)[f"{name}_decay"])
        pics = tpc.case_window(orc, case)
        ostates, self.otot = tpc.run_oracle(orc, pics, case, decay)
        self.want, self.want_states = pics[0].arrays(), tpc.states_to_array(ostates)
        self.dev = tpc.DevWindow(hip, tpc.case_window(orc, case))
        self.job = tpc.make_job(self.dev.pics, w, h, bd, key, ctl, decay, self.dev.ptrs)
        need = hip.svt_hip_tf_workspace_bytes(w, h, n_refs)
        self.ws = ws if ws is not None else device.tf_workspace(hip, self.job)
        assert self.ws.nbytes >= need
        self.tot = device.DeviceBuffer(hip, 8)
        self.tot.fill(0)
        settle(hip)

    def issue(self, stream):
        device.tf_filter_picture(self.hip, self.job, self.ws, self.tot, stream, sync=False)

    def check(self, what=""):
        name = self.case[0]
        states, tot = device.tf_read_back(self.hip, self.job, self.ws, self.tot)
        bad = np.argwhere((states != self.want_states).any(axis=1))
        assert len(bad) == 0, (what, name, "refinement state of (ref, b64) entries", bad[:8].ravel().tolist())
        assert tot == self.otot, (what, name, "tot")
        got = self.dev.centre_arrays()
        for k, v in self.want.items():
            assert np.array_equal(got[k], v), (what, name, k, int((got[k] != v).sum()))


class TplCase:
    def __init__(self, hip, orc, case):
        self.hip, self.case = hip, case
        TP.load_quant(np.load(TP.GOLD))
        a, b = TP.TplScene(orc, case), TP.TplScene(orc, case)
        if case[5]["src_data_ready"]:
            TP.prime_second_pass(orc, a), TP.prime_second_pass(orc, b)
        assert orc.orc_tpl_dispenser_frame(C.byref(b.job())) == 0
        self.want, self.scene = b.results(), a
        self.dm = device.DeviceMap(hip)
        self.job = a.job(self.dm)
        self.ws = device.tpl_workspace(hip, self.job)
        self.ws.fill(0xCD)
        settle(hip)

    def issue(self, stream):
        device.tpl_dispenser_frame(self.hip, self.job, self.ws, stream, sync=False)

    def check(self, what=""):
        assert device.tpl_status(self.hip, self.job, self.ws) == 0, (what, self.case[0], "a dependency wait ran into its bound")
        got = {"recon": self.dm.download(self.scene.out.buf), "stats": self.dm.download(self.scene.stats).view(np.uint8),
               "src_stats": self.dm.download(self.scene.src_stats).view(np.uint8)}
        for k, v in self.want.items():
            assert np.array_equal(got[k], v), (what, self.case[0], k, int((got[k] != v).sum()))


class TxfmCase:
    def __init__(self, hip, orc, w, h, n_tb, seed):
        self.hip, self.w, self.h, self.n = hip, w, h, n_tb
        self.arena, self.descs, self.expect = T.fused_batch(orc, np.random.default_rng(seed), w, h, n_tb)
        self.darena = device.DeviceBuffer(hip, self.arena.nbytes + 256)
        self.darena.upload(self.arena)
        self.ddesc = device.DeviceBuffer(hip, C.sizeof(self.descs))
        self.ddesc.upload(np.frombuffer(self.descs, dtype=np.uint8))
        self.dres = device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_tb)
        settle(hip)

    def issue(self, stream):
        device.check(self.hip, self.hip.svt_hip_txfm_quant_batch(V(self.darena.ptr), V(self.ddesc.ptr), V(self.dres.ptr), C.c_uint32(self.n),
                                                                 C.c_uint32(self.w), C.c_uint32(self.h), V(stream)), "svt_hip_txfm_quant_batch")

    def check(self, what=""):
        T.check_fused_batch(self.w, self.h, self.descs, self.expect, self.darena.download(np.uint8, (self.arena.nbytes,)),
                            self.dres.download(np.uint8, (self.n, abi.TXFM_RESULT_BYTES)), what)


class DeblockCase:
    def __init__(self, hip, orc, variant):
        self.hip = hip
        planes, w, h, flat, mi_stride, mi_rows, mi_cols, hdr, bd, is16, lvl, ps, pe = deblock_inputs(variant)
        self.want = [p.copy() for p in planes]
        f = L.lf_frame(self.want, w, h, flat.ctypes.data, mi_stride, mi_rows, mi_cols, hdr, bd, is16, ps, pe, lvl)
        orc.orc_loop_filter_frame(C.byref(f), 64)
        self.planes, self.flat, self.lvl = planes, flat, lvl
        self.bufs = [device.DeviceBuffer(hip, p.nbytes) for p in planes]
        for b, p in zip(self.bufs, planes):
            b.upload(p)
        self.d_mi = device.DeviceBuffer(hip, flat.nbytes)
        self.d_mi.upload(flat.view(np.uint8))
        dev_planes = [(b.ptr + (L.PAD * p.shape[1] + L.PAD) * p.itemsize, p.shape[1]) for b, p in zip(self.bufs, planes)]
        self.frame = L.lf_frame(dev_planes, w, h, self.d_mi.ptr, mi_stride, mi_rows, mi_cols, hdr, bd, is16, ps, pe, lvl)
        settle(hip)

    def issue(self, stream):
        device.check(self.hip, self.hip.svt_hip_loop_filter_frame(C.byref(self.frame), V(stream)), "svt_hip_loop_filter_frame")

    def check(self, what=""):
        for i, (b, p, want) in enumerate(zip(self.bufs, self.planes, self.want)):
            got = b.download(p.dtype, p.shape)
            assert np.array_equal(got, want), (what, "deblock plane", i, int((got != want).sum()))


class LrCase:
    def __init__(self, hip, orc, name):
        self.hip, self.case = hip, R.make_case(name)
        arr, outs = R.lr_planes(self.case)
        orc.orc_restoration_filter_frame(arr, C.c_uint32(len(self.case)))
        self.want = [o[:c["h"], :c["w"]].copy() for o, c in zip(outs, self.case)]
        self.keep, ptrs, self.dsts = [], {}, []
        for c in self.case:
            for k in ("src", "above", "below", "units"):
                b = device.DeviceBuffer(hip, c[k].nbytes)
                b.upload(c[k])
                self.keep.append(b)
                ptrs[id(c[k])] = b.ptr
            d = device.DeviceBuffer(hip, (c["h"] + 2) * (c["w"] + R.DST_EXTRA) * c["src"].itemsize)
            d.fill(0)
            self.dsts.append(d)
        self.arr, _ = R.lr_planes(self.case, ptr_of=lambda a: ptrs[id(a)], dsts=[d.ptr for d in self.dsts])
        settle(hip)

    def issue(self, stream):
        device.check(self.hip, self.hip.svt_hip_restoration_filter_frame(self.arr, C.c_uint32(len(self.case)), V(stream)),
                     "svt_hip_restoration_filter_frame")

    def check(self, what=""):
        for p, (d, c, want) in enumerate(zip(self.dsts, self.case, self.want)):
            got = d.download(c["src"].dtype, (c["h"] + 2, c["w"] + R.DST_EXTRA))[:c["h"], :c["w"]]
            assert np.array_equal(got, want), (what, "restoration plane", p, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------ 1a: two streams, one thread
TWO_STREAM_FAMILIES = {
    # A: every 256 x 256 unit of a 4K 10-bit luma plane, 7x7 window; B: an 8-bit plane with other content, 5x5 window
    "wiener_stats": (lambda h, o, g: WienerCase(h, o, 3840, 2160, 10, 1, 7, 256, 4000),
                     lambda h, o, g: WienerCase(h, o, 520, 300, 8, 0, 5, 128, 4001)),
    "me_frames": (lambda h, o, g: MeCase(h, o, "blocks", 1280, 720, "m8_720p_tl2", 71),
                  lambda h, o, g: MeCase(h, o, "pan", 320, 200, "m4_360p_tl2", 72)),
    "analysis_frames": (lambda h, o, g: AnalysisCase(h, o, [(1920, 1080)], 1, 0, 73),
                        lambda h, o, g: AnalysisCase(h, o, [(328, 200), (200, 136)], 0, 1, 74)),
    "intra_search_frames": (lambda h, o, g: IntraCase(h, g, I.BIG_CASES[1]), lambda h, o, g: IntraCase(h, g, I.CASES[0])),
    "tf_filter_picture": (lambda h, o, g: TfCase(h, o, tf_case("blocks_lvl1_8bit")), lambda h, o, g: TfCase(h, o, tf_case("pan_lvl6_10bit"))),
    "tpl_dispenser_frame": (lambda h, o, g: TplCase(h, o, TP.CASES[1]), lambda h, o, g: TplCase(h, o, TP.CASES[0])),
    "txfm_quant_batch": (lambda h, o, g: TxfmCase(h, o, 16, 16, 1024, 75), lambda h, o, g: TxfmCase(h, o, 8, 8, 300, 76)),
    "loop_filter_frame": (lambda h, o, g: DeblockCase(h, o, 6), lambda h, o, g: DeblockCase(h, o, 0)),
    "restoration_filter_frame": (lambda h, o, g: LrCase(h, o, "b_10bit"), lambda h, o, g: LrCase(h, o, "a_8bit")),
}


@pytest.mark.parametrize("family", list(TWO_STREAM_FAMILIES))
def test_two_streams_one_thread(hip, orc, gold_intra, family):
    """A long call A on s1, right behind it a different call B on s2, no synchronisation in between; both match."""
    make_a, make_b = TWO_STREAM_FAMILIES[family]
    a, b = make_a(hip, orc, gold_intra), make_b(hip, orc, gold_intra)
    s1, s2 = new_stream(hip), new_stream(hip)
    try:
        keep = [a.issue(s1), b.issue(s2)]
        sync(hip, s1, s2)
        del keep
        a.check(f"{family} A on s1")
        b.check(f"{family} B on s2")
    finally:
        destroy(hip, s1, s2)


# ------------------------------------------------------------------------------------------------ 1b: more calls than staging slots
def test_more_calls_in_flight_than_staging_slots(hip, orc, gold_intra):
    """6 calls each of me_frames, intra_search_frames and wiener_stats from one thread, each on its own stream, no synchronisation,
    every host descriptor array overwritten with 0xFF right after its call: 18 calls through a ring of 4 staging slots."""
    keys = ["m8_360p_tl2", "m4_360p_tl2", "m12_360p_tl2", "m8_360p_tl0", "m6_360p_tl2", "m10_360p_tl2"]
    cases = []
    for i, key in enumerate(keys):
        cases.append(MeCase(hip, orc, ("pan", "blocks", "noise")[i % 3], 320, 200, key, 80 + i))
        cases.append(IntraCase(hip, gold_intra, I.CASES[i]))
        cases.append(WienerCase(hip, orc, 200 + 24 * i, 136, (8, 10)[i % 2], i % 2, (7, 5)[i % 2], 64, 90 + i))
    streams = [new_stream(hip) for _ in cases]
    try:
        for c, s in zip(cases, streams):
            arr = c.issue(s)
            C.memset(arr, 0xFF, C.sizeof(arr))          # the caller's array is dead the moment the call returns
        sync(hip, *streams)
        for k, c in enumerate(cases):
            c.check(f"call {k}")
    finally:
        destroy(hip, *streams)


def test_wiener_buffer_grows_with_work_in_flight(hip, orc):
    """A fresh thread's buffer of raw moments starts empty: 2 units on s1 size it for 4, then, with nothing synchronised, 15 units
    on s2 make it grow while the first call may still be using it."""
    seed = 4100
    a, b = WienerCase(hip, orc, 128, 64, 8, 0, 7, 64, seed), WienerCase(hip, orc, 264, 136, 10, 1, 5, 64, seed + 1)
    assert (len(a.units), len(b.units)) == (2, 15)
    s1, s2 = new_stream(hip), new_stream(hip)

    def worker(t, fail):
        keep = [a.issue(s1), b.issue(s2)]
        sync(hip, s1, s2)
        del keep
        a.check("2 units on s1")
        b.check("15 units on s2, grown buffer")
    try:
        failures = run_threads(1, worker)
    finally:
        destroy(hip, s1, s2)
    assert not failures[0], failures[0]


# ------------------------------------------------------------------------------------------------ 1c: many host threads, Tier A
def same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def tier_a_items(hip, orc, t):
    """Seeded work of thread t: [(name, call returning the HIP result, the oracle's result)]; every item owns its inputs."""
    rng = np.random.default_rng(7000 + t)
    items = []
    # svt_sad_loop_kernel on SadTest-style cases
    sad_cases = list(me_cases.iter_sad_loop_cases())
    for prm, src, refw in sad_cases[t * 7 % len(sad_cases)::97][:3]:
        items.append(("sad_loop", lambda p=prm, s=src, r=refw: me_cases.call_sad_loop(hip.svt_sad_loop_kernel_hip, p, s, r),
                      me_cases.call_sad_loop(orc.orc_sad_loop_kernel, prm, src, refw)))
    # svt_nxm_sad_kernel and the ext 8x8 / 16x16 SADs
    stride = 89
    src, refw = rng.integers(0, 256, size=(64, stride), dtype=np.uint8), rng.integers(0, 256, size=(64, stride), dtype=np.uint8)
    for h, w in ((64, 64), (16, 8), (7, 5)):
        items.append(("nxm_sad", lambda h=h, w=w, s=src, r=refw: hip.svt_nxm_sad_kernel_hip(P(s), stride, P(r), stride, h, w),
                      orc.orc_nxm_sad(P(src), stride, P(refw), stride, h, w)))

    def ext16(fn, s=src, r=refw, sub=t % 2):
        u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        b8, b16 = np.full(4, 5000, np.uint32), np.full(1, 20000, np.uint32)
        m8, m16, s16, s8 = np.zeros(4, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(4, np.uint32)
        fn(C.cast(s.ctypes.data, u8p), C.c_uint32(stride), C.cast(r.ctypes.data + 3, u8p), C.c_uint32(stride), b8.ctypes.data_as(u32p),
           b16.ctypes.data_as(u32p), m8.ctypes.data_as(u32p), m16.ctypes.data_as(u32p), C.c_uint32(7), s16.ctypes.data_as(u32p),
           s8.ctypes.data_as(u32p), C.c_uint8(sub))
        return b8, b16, m8, m16, s16, s8
    items.append(("ext_sad", lambda: ext16(hip.svt_ext_sad_calculation_8x8_16x16_hip), ext16(orc.orc_ext_sad_calculation_8x8_16x16)))
    # forward and inverse transforms of several sizes
    for w, h in ((4, 4), (8, 8), (16, 16), (32, 32), (16, 8), (64, 64))[t % 3::3][:2] + ((8, 16),):
        tt = [x for x in range(16) if orc.orc_txfm_valid(w, h, x)][t % 4 if max(w, h) < 32 else 0]
        bd = (8, 10)[t % 2]
        res = T.residual(rng, w, h, bd, t % 3)
        want = np.zeros(w * h, np.int32)
        orc.orc_fwd_txfm2d(P(res), P(want), C.c_uint32(w + 3), w, h, tt, bd, 0)

        def fwd(w=w, h=h, res=res, tt=tt, bd=bd):
            o = np.full(w * h, 5, np.int32)
            getattr(hip, f"svt_av1_fwd_txfm2d_{w}x{h}_hip")(P(res), P(o), C.c_uint32(w + 3), tt, C.c_uint8(bd))
            return o
        items.append((f"fwd_txfm {w}x{h}", fwd, want))
        co = T.coeffs_for_inverse(rng, orc, w, h, tt, bd, t % 3)
        pred = rng.integers(0, 1 << bd, size=(h, w + 5)).astype(np.uint16)
        rw = np.zeros((h, w + 7), np.uint16)
        orc.orc_inv_txfm2d_add(P(co), P(pred), w + 5, P(rw), w + 7, w, h, tt, bd)

        def inv(w=w, h=h, co=co, pred=pred, tt=tt, bd=bd):
            r = np.zeros((h, w + 7), np.uint16)
            hip_inverse(hip, w, h, co, pred, w + 5, r, w + 7, tt, bd)
            return r
        items.append((f"inv_txfm {w}x{h}", inv, rw))
    # the quantisers
    for trial in range(t, 4 * N_THREADS, N_THREADS):
        c = T.quant_case(rng, trial)
        if c["qm"] is not None:
            continue
        tq, n = c["t"], c["n"]

        def quant(fn, rnd, qnt, *tail, c=c, tq=tq, n=n):
            qc, dq, eob = np.full(n, 7, np.int32), np.full(n, 7, np.int32), C.c_uint16(9999)
            fn(P(c["coeff"]), C.c_ssize_t(n), P(tq["zbin"]), P(rnd), P(qnt), P(tq["qshift"]), P(qc), P(dq), P(tq["dequant"]), C.byref(eob),
               P(c["scan"]), P(c["iscan"]), *tail)
            return qc, dq, eob.value
        items.append(("quantize_b", lambda c=c, tq=tq, quant=quant: quant(hip.svt_aom_quantize_b_hip, tq["round"], tq["quant"], None, None,
                                                                         C.c_int32(c["ls"])), tuple(T.orc_quant(orc, 1, c))))
        items.append(("highbd_quantize_fp", lambda c=c, tq=tq, quant=quant: quant(hip.svt_av1_highbd_quantize_fp_hip, tq["round_fp"],
                                                                                 tq["quant_fp"], C.c_int16(c["ls"])), tuple(T.orc_quant(orc, 4, c))))
    # CDEF: direction search and the block filter
    bd = (8, 10)[t % 2]
    img = rng.integers(0, 1 << bd, size=(16, 24)).astype(np.uint16)
    v1 = C.c_int32(-1)
    d1 = orc.orc_cdef_find_dir(P(img), 24, C.byref(v1), bd - 8)

    def find_dir(img=img, bd=bd):
        v = C.c_int32(-1)
        return hip.svt_aom_cdef_find_dir_hip(P(img), 24, C.byref(v), bd - 8), v.value
    items.append(("cdef_find_dir", find_dir, (d1, v1.value)))
    tile = L.cdef_tile(rng, bd, edge=t % 16)
    bsize, cs = t % 4, bd - 8
    bw, bh = 4 << (bsize in (2, 3)), 4 << (bsize in (1, 3))
    off = (VB + 3 * bh) * BS + HB + 5 * bw
    pri, sec = int(rng.integers(0, 16)) << cs, int(rng.choice([0, 1, 2, 4])) << cs
    dd, damp = int(rng.integers(0, 8)), int(rng.integers(3, 7)) + cs
    want = np.full((8, 16), 0xAAAA, np.uint16)
    orc.orc_cdef_filter_block(None, P(want), 16, V(tile.ctypes.data + 2 * off), pri, sec, dd, damp, damp, bsize, cs, C.c_uint8(1))

    def cdef(tile=tile, off=off, pri=pri, sec=sec, dd=dd, damp=damp, bsize=bsize, cs=cs):
        o = np.full((8, 16), 0xAAAA, np.uint16)
        hip.svt_cdef_filter_block_hip(None, P(o), 16, V(tile.ctypes.data + 2 * off), pri, sec, dd, damp, damp, bsize, cs, C.c_uint8(1))
        return o
    items.append(("cdef_filter_block", cdef, want))
    # deblocking: one 8-tap vertical edge
    a = np.ascontiguousarray(TL.lpf_block(rng, 8, t)).astype(np.uint8)
    level, sharp = int(rng.integers(1, 64)), int(rng.integers(0, 8))
    lim, mblim, hev = C.c_int(), C.c_int(), C.c_int()
    orc.orc_lf_thresholds(level, sharp, C.byref(lim), C.byref(mblim), C.byref(hev))
    th = [np.full(16, v.value, np.uint8) for v in (mblim, lim, hev)]
    want = a.copy()
    orc.orc_lpf(V(want.ctypes.data + 4 * 16 + 8), 16, mblim.value, lim.value, hev.value, 8, 0, 8, 1)

    def lpf(a=a, th=th):
        b = a.copy()
        hip.svt_aom_lpf_vertical_8_hip(V(b.ctypes.data + 4 * 16 + 8), 16, P(th[0]), P(th[1]), P(th[2]))
        return b
    items.append(("lpf_vertical_8", lpf, want))
    # Wiener statistics and the Wiener filter
    win, (w, h) = (7, 5)[t % 2], ((64, 48), (100, 37), (33, 64))[t % 3]
    dat, src = G.sgr_plane(rng, w + 8, h + 8, 8, 0, t % 3)
    M1, H1 = np.zeros(49, np.int64), np.zeros(49 * 49, np.int64)
    orc.orc_wiener_compute_stats(win, V(G.at(dat)), V(G.at(src)), 3, 3 + w, 2, 2 + h, dat.shape[1], src.shape[1], P(M1), P(H1), 0, 8)

    def stats(win=win, dat=dat, src=src, w=w, h=h):
        M, H = np.zeros(49, np.int64), np.zeros(49 * 49, np.int64)
        hip.svt_av1_compute_stats_hip(win, V(G.at(dat)), V(G.at(src)), 3, 3 + w, 2, 2 + h, dat.shape[1], src.shape[1], P(M), P(H))
        return M[:win * win], H[:win ** 4]
    items.append(("compute_stats", stats, (M1[:win * win], H1[:win ** 4])))
    dat16, _ = G.sgr_plane(rng, 40, 17, 10, 1, 0)
    fx, kx = G.wiener_filter(rng)
    fy, ky = G.wiener_filter(rng)
    r0, r1 = G.wiener_rounds(10)
    want = np.zeros((17, 43), np.uint16)
    orc.orc_wiener_convolve_add_src(V(G.at(dat16)), dat16.shape[1], P(want), 43, P(fx), P(fy), 40, 17, r0, r1, 10, 1)

    def wconv(d=dat16, fx=fx, fy=fy, keep=(kx, ky)):
        o = np.zeros((17, 43), np.uint16)
        cp = abi.ConvolveParams(round_0=r0, round_1=r1)
        hip.svt_av1_highbd_wiener_convolve_add_src_hip(enc16(G.at(d)), C.c_ssize_t(d.shape[1]), enc16(o.ctypes.data), C.c_ssize_t(43), P(fx),
                                                       P(fy), 40, 17, C.byref(cp), 10)
        return o
    items.append(("wiener_convolve_add_src", wconv, want))
    # single-reference 2-D convolve (sr)
    cw, ch = K.SIZES[t % len(K.SIZES)]
    tab = K.kernel_table(list(K.TABLES)[t % 3])[0]
    sx, sy = int(rng.integers(0, 16)), int(rng.integers(0, 16))
    plane, at = K.ref_plane(rng, cw, ch, 8, 0, t % 3)
    cr0, cr1 = K.conv_rounds(8)
    want = np.zeros((ch, cw + 3), plane.dtype)
    orc.orc_convolve_sr(V(at), plane.shape[1], P(want), cw + 3, cw, ch, V(tab[sx].ctypes.data), 8, V(tab[sy].ctypes.data), 8, cr0, cr1, 8, 0)

    def conv(plane=plane, at=at, tab=tab, sx=sx, sy=sy, cw=cw, ch=ch):
        o = np.zeros((ch, cw + 3), plane.dtype)
        fp = abi.InterpFilterParams(tab.ctypes.data, 8, 16, t % 3)
        cp = abi.ConvolveParams(round_0=cr0, round_1=cr1)
        hip.svt_av1_convolve_2d_sr_hip(V(at), plane.shape[1], P(o), cw + 3, cw, ch, C.byref(fp), C.byref(fp), sx, sy, C.byref(cp))
        return o
    items.append(("convolve_2d_sr", conv, want))
    # residual and SSE
    rcases = list(LC.residual_cases())
    h, w, rs, a, b, hbd = rcases[t % len(rcases)]

    def residual(h=h, w=w, rs=rs, a=a, b=b, hbd=hbd):
        out = np.full((h, rs), -9, np.int16)
        (hip.svt_residual_kernel16bit_hip if hbd else hip.svt_residual_kernel8bit_hip)(P(a), C.c_uint32(a.shape[1]), P(b), C.c_uint32(b.shape[1]),
                                                                                      P(out), C.c_uint32(rs), C.c_uint32(w), C.c_uint32(h))
        return out
    items.append(("residual", residual, orc_residual(orc, h, w, rs, a, b, hbd)))
    scases = list(LC.sse_cases())
    h, w, o0, o1, a, b, hbd = scases[t % len(scases)]

    def sse(h=h, w=w, o0=o0, o1=o1, a=a, b=b, hbd=hbd):
        fn = hip.svt_full_distortion_kernel16_bits_hip if hbd else hip.svt_spatial_full_distortion_kernel_hip
        return fn(P(a), C.c_uint32(o0), C.c_uint32(a.shape[1]), P(b), C.c_int32(o1), C.c_uint32(b.shape[1]), C.c_uint32(w), C.c_uint32(h))
    items.append(("sse", sse, orc_sse(orc, h, w, o0, o1, a, b, hbd)))
    return items


def run_threads(n, target):
    """n threads released together; failures collected per thread (asserted by the caller in the main thread)."""
    failures, start = [[] for _ in range(n)], threading.Barrier(n)

    def body(t):
        try:
            start.wait(timeout=60)
            target(t, failures[t])
        except Exception as e:  # noqa: BLE001
            failures[t].append(f"thread {t}: {type(e).__name__}: {e}")
    threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=240)
    assert not any(th.is_alive() for th in threads), "a worker thread did not finish"
    return failures


def test_many_threads_tier_a(hip, orc):
    """24 host threads (the 8 pooled streams are shared) call a mix of Tier A leaves at once, each on its own seeded inputs."""
    assert hip.svt_hip_debug_tier_a_broken(0) == 0
    work = [tier_a_items(hip, orc, t) for t in range(N_THREADS)]
    kinds = {name.split()[0] for items in work for name, _, _ in items}
    assert kinds >= {"sad_loop", "nxm_sad", "ext_sad", "fwd_txfm", "inv_txfm", "quantize_b", "highbd_quantize_fp", "cdef_find_dir",
                     "cdef_filter_block", "lpf_vertical_8", "compute_stats", "wiener_convolve_add_src", "convolve_2d_sr", "residual", "sse"}

    def worker(t, fail):
        for rep in range(3):
            for name, call, want in work[t]:
                if not same(call(), want):
                    fail.append(f"thread {t} round {rep}: {name} differs from the oracle")
    failures = run_threads(N_THREADS, worker)
    bad = [f for fs in failures for f in fs]
    assert not bad, bad[:10]
    assert hip.svt_hip_debug_tier_a_broken(0) == 0


# ------------------------------------------------------------------------------------------------ 1d: many host threads, Tier B
def test_many_threads_tier_b(hip, orc, gold_intra):
    """24 host threads each run intra_search_frames, me_frames and wiener_stats on their own inputs, half of them on the shared pool
    (stream = NULL), half on a stream of their own.  One more thread makes a refused call: its message stays its own."""
    keys = ["m8_360p_tl2", "m4_360p_tl2", "m12_360p_tl2", "m6_360p_tl2"]
    work = []
    for t in range(N_THREADS):
        work.append((IntraCase(hip, gold_intra, I.CASES[t % len(I.CASES)]),
                     MeCase(hip, orc, ("pan", "blocks", "noise")[t % 3], 200, 136, keys[t % 4], 300 + t),
                     WienerCase(hip, orc, 136 + 8 * t, 72, (8, 10)[t % 2], t % 2, (7, 5)[t % 2], 64, 400 + t)))
    own = [new_stream(hip) if t % 2 else None for t in range(N_THREADS)]
    marker = b"ctrls out of range"
    refused, refusal = threading.Event(), []

    def refuse():
        job = abi.IntraSearchJob()
        job.ctrls.intra_mode_end = abi.INTRA_MODES      # one past the last mode
        rc = hip.svt_hip_intra_search_frames((abi.IntraSearchJob * 1)(job), C.c_uint32(1), None)
        refusal.append((rc, hip.svt_hip_last_error()))
        refused.set()

    def worker(t, fail):
        for c in work[t]:
            c.issue(own[t])
        sync(hip, own[t])
        for c in work[t]:
            c.check(f"thread {t}")
        if not refused.wait(timeout=60):
            fail.append("the refusing thread did not run")
        msg = hip.svt_hip_last_error()
        if marker in msg:
            fail.append(f"thread {t} sees another thread's error: {msg!r}")
    refuser = threading.Thread(target=refuse, daemon=True)
    try:
        refuser.start()
        failures = run_threads(N_THREADS, worker)
        refuser.join(timeout=60)
    finally:
        destroy(hip, *[s for s in own if s])
    assert refusal and refusal[0][0] == abi.SVT_HIP_ERR_BAD_PARAMETER and marker in refusal[0][1], refusal
    bad = [f for fs in failures for f in fs]
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------ 1e: one workspace, many jobs
def test_tf_workspace_reuse(hip, orc):
    """One workspace sized for the largest job: a larger picture with 4 references, then a smaller one with 2, then 8x8 prediction.
    Each job must match the oracle, whatever an earlier job left in the workspace."""
    big = ("pan_4refs_8bit", "pan", 256, 192, 4, 8, "m8_360p_tl0", tpc.LVL6)
    cases = [(big, (2247286, 6156426, 6156426)), (tf_case("pan_lvl6_8bit"), None), (tf_case("blocks_lvl1_8x8_8bit"), None),
             (tf_case("pan_lvl6_10bit"), None)]
    ws = device.DeviceBuffer(hip, max(hip.svt_hip_tf_workspace_bytes(c[2], c[3], c[4]) for c, _ in cases))
    for case, decay in cases:
        tc = TfCase(hip, orc, case, decay, ws=ws)
        tc.issue(None)
        sync(hip, None)
        tc.check(f"shared workspace, {case[0]}")


def test_sgr_search_work_reuse(hip, orc):
    """svt_hip_sgr_search_unit: one d_work buffer across units of different size and ep range."""
    units = [(328, 200, 8, 0, 64, (0, 16, 1, 1)), (96, 80, 10, 1, 64, (10, 16, 1, 0)), (200, 120, 8, 1, 32, (0, 8, 3, 1)),
             (56, 40, 8, 0, 32, (14, 16, 1, 1)), (256, 256, 10, 1, 64, (0, 16, 4, 1))]
    work = device.DeviceBuffer(hip, max(hip.svt_hip_sgr_search_work_bytes(w, h, (s1 - s0 + inc - 1) // inc)
                                        for w, h, _, _, _, (s0, s1, inc, _) in units))
    orc.orc_sgr_search_unit.restype = C.c_int64
    for k, (w, h, bd, is16, pu, (s0, s1, inc, refine)) in enumerate(units):
        rng = np.random.default_rng(500 + k)
        dat, src = G.sgr_plane(rng, w, h, bd, is16, k % 3)
        want = np.zeros(3, np.int32)
        e1 = orc.orc_sgr_search_unit(V(G.at(dat)), w, h, dat.shape[1], V(G.at(src)), src.shape[1], is16, bd, pu, pu, s0, s1, inc, refine, P(want))
        d_dat, d_src = device.DeviceBuffer(hip, dat.nbytes), device.DeviceBuffer(hip, src.nbytes)
        d_dat.upload(dat), d_src.upload(src)
        off = (G.B * dat.shape[1] + G.B) * dat.itemsize
        unit = abi.SgrUnit(d_dat.ptr + off, d_src.ptr + off, dat.shape[1], src.shape[1], w, h, is16, bd, pu, pu)
        got, e2 = np.zeros(3, np.int32), C.c_int64(0)
        device.check(hip, hip.svt_hip_sgr_search_unit(C.byref(unit), s0, s1, inc, refine, V(work.ptr), P(got), C.byref(e2), None), "sgr_search")
        assert np.array_equal(got, want) and e2.value == e1, (k, got, want, e2.value, e1)


# ------------------------------------------------------------------------------------------------ 1f: the grouped transform path
def test_grouped_transform_two_streams():
    """SVTAV1_HIP_GROUP_TX is read once per process: a child process runs fused batches of >= 2048 blocks with mixed tx_type
    (4x4, 8x8, 4x8, 16x16) on two streams and compares them with the oracle (tests/grouped_txfm_child.py)."""
    env = dict(os.environ, SVTAV1_HIP_GROUP_TX="1", SVTAV1_HIP_TEST_HOOKS="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "grouped_txfm_child.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, f"child exit status {r.returncode}\nstdout:\n{r.stdout[-3000:]}\nstderr:\n{r.stderr[-6000:]}"
    assert r.stdout.count("bit-exact") == 4, r.stdout
