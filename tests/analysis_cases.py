"""Plumbing shared by the tests of svt_hip_analysis_frames (tests/test_gpu_analysis_fused.py): oracle references, device
jobs whose decimated planes and outputs start as 0xA5, whole-buffer comparison.  Run as a script it is the child process
of the switch test: it runs SWITCH_BATCH in the environment it was given and saves every buffer to the .npz named on its
command line."""
import ctypes as C
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import me_cases  # noqa: E402
import pyorc  # noqa: E402
from arena import GUARD as FILL  # noqa: E402  (a byte nobody writes keeps it on both sides; zeros would hide it)
from svtav1_hip import abi, device, frames  # noqa: E402

SWITCH_BATCH = [("noise", 64, 64, 41), ("pan", 206, 142, 42), ("noise", 648, 360, 43)]


def luma_of(kind, w, h, seed):
    return me_cases.make_clip(kind, w, h, 1, seed=seed)[0]


def prefilled_pyramid(luma, quarter_size=None):
    """HostPyramid of the reference's sizes (or another quarter size) with both decimated planes set to FILL."""
    hp = frames.HostPyramid(luma)
    if quarter_size is not None:
        hp.quarter = frames.HostPlane(quarter_size[0], quarter_size[1], frames.QUARTER_PAD)
    hp.quarter.buf[...] = FILL
    hp.sixteenth.buf[...] = FILL
    return hp


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, seed, l1, fp):
    """What the oracle leaves for one picture: {quarter, sixteenth, variance, mean}, read-only and computed once.
    With l1 == 0 the quarter plane is the untouched FILL."""
    orc = pyorc.oracle()
    hp = prefilled_pyramid(luma_of(kind, w, h, seed))
    d = hp.desc()
    orc.orc_pyramid_frame(C.byref(d.full), C.byref(d.quarter), C.byref(d.sixteenth), l1)
    nb = frames.b64_count(w, h)
    v, m = np.zeros((nb, 85), np.uint16), np.zeros((nb, 85), np.uint64)
    orc.orc_variance_frame(C.byref(d.full), v.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), fp)
    out = {"quarter": hp.quarter.buf, "sixteenth": hp.sixteenth.buf, "variance": v, "mean": m}
    for a in out.values():
        a.flags.writeable = False
    return out


class DeviceJob:
    """One picture on the device: full plane uploaded, decimated planes and outputs FILL."""

    def __init__(self, hip, kind, w, h, seed, with_mean=True, quarter_size=None):
        self.hp = prefilled_pyramid(luma_of(kind, w, h, seed), quarter_size)
        self.dp = device.DevicePyramid(hip, self.hp)
        self.nb = frames.b64_count(w, h)
        self.dv = device.DeviceBuffer(hip, self.nb * 85 * 2)
        self.dm = device.DeviceBuffer(hip, self.nb * 85 * 8) if with_mean else None
        self.refill()

    def refill(self):
        self.dp.quarter.buf.upload(self.hp.quarter.buf)
        self.dp.sixteenth.buf.upload(self.hp.sixteenth.buf)
        for b in (self.dv, self.dm):
            if b is not None:
                b.fill(FILL)
        device.check(self.dv.lib, self.dv.lib.svt_hip_stream_sync(None), "svt_hip_stream_sync")

    def job(self):
        return abi.AnalysisJob(self.dp.desc(), self.dv.ptr, self.dm.ptr if self.dm else None)

    def results(self):
        r = {"quarter": self.dp.quarter.download(), "sixteenth": self.dp.sixteenth.download(),
             "variance": self.dv.download(np.uint16, (self.nb, 85))}
        if self.dm is not None:
            r["mean"] = self.dm.download(np.uint64, (self.nb, 85))
        return r


def run(hip, jobs, l1, fp):
    arr = (abi.AnalysisJob * len(jobs))(*jobs)
    device.check(hip, hip.svt_hip_analysis_frames(arr, len(jobs), l1, fp, None), "svt_hip_analysis_frames")
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")


def assert_equal(got, want, what):
    """Whole buffers, padding included; names the first byte that differs."""
    for k, g in got.items():
        w = want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            i = tuple(bad[0])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} of {g.size} entries, first at {i}: got {g[i]}, want {w[i]}")


def switch_batch_results(hip, l1, fp):
    djobs = [DeviceJob(hip, *c) for c in SWITCH_BATCH]
    run(hip, [d.job() for d in djobs], l1, fp)
    return {f"{i}_{l1}{fp}_{k}": v for i, d in enumerate(djobs) for k, v in d.results().items()}


if __name__ == "__main__":
    lib = abi.load()
    assert lib.svt_hip_init(0) == 0, lib.svt_hip_last_error().decode()
    res = {}
    for l1_, fp_ in ((1, 0), (0, 1)):
        res.update(switch_batch_results(lib, l1_, fp_))
    np.savez(sys.argv[1], **res)
    print("saved", len(res), "arrays")
