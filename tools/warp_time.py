#!/usr/bin/env python3
"""Time the global-motion error of a 1920x1080 picture pair on both sides (one measurement, no threshold):
  GPU: svt_hip_warp_error_batch with N = 1 and N = 8 candidates (HIP events around the library's launches, pictures resident,
       warm-up, median of the repeats); the 8-byte read-back that svt_hip_gm_refine pays per step (host clock around a
       synchronised copy on an idle stream); one launch + read-back as the driver does it; one whole svt_hip_gm_refine.
  CPU: svt_av1_warp_error of the reference (oracle/_ref) on one core, with the C and with the AVX2 svt_av1_warp_affine.
The GPU error of every timed candidate is checked against the reference's.  Writes profiles/r06_warp_error_1080p.json; without a
device the GPU half is recorded as null.
    python tools/warp_time.py [repeats]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import pyorc  # noqa: E402
import warp_cases as W  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

WIDTH, HEIGHT = 1920, 1080
TRUE = [5 * W.ONE + 21000, -3 * W.ONE + 40000, W.ONE + 300, -450, 350, W.ONE - 200]
MODELS = [TRUE] + [[TRUE[0] + 4096 * k, TRUE[1] - 2048 * k, TRUE[2] + 16 * k, TRUE[3] - 8 * k, TRUE[4] + 8 * k, TRUE[5] - 16 * k] for k in range(1, 8)]


def cpu_leg(ref, pair, repeats=5):
    """{variant: median ms} of svt_av1_warp_error over the whole picture, no early exit, on this one core."""
    orc = W.RefError(ref)
    slot = C.c_void_p.in_dll(ref, "svt_av1_warp_affine")
    out, errors = {}, {}
    for variant in ("c", "avx2"):
        slot.value = C.cast(getattr(ref, f"svt_av1_warp_affine_{variant}"), C.c_void_p).value
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            errors[variant] = orc.error(TRUE, W.AFFINE, *pair, 0, W.INT64_MAX)
            ms.append((time.perf_counter() - t0) * 1e3)
        out[f"warp_affine_{variant}_ms"] = round(statistics.median(ms), 3)
    slot.value = C.cast(ref.svt_av1_warp_affine_c, C.c_void_p).value
    assert errors["c"] == errors["avx2"]
    out["error"] = errors["c"]
    return out


def host_clock(repeats, step):
    for _ in range(3):
        step()
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        step()
        us.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    assert repeats >= 20
    pair = W.picture_pair(99, WIDTH, HEIGHT, TRUE)
    res = {"width": WIDTH, "height": HEIGHT, "repeats": repeats, "error_blocks": -(-WIDTH // 32) * -(-HEIGHT // 32)}
    ref = pyorc.ref() if pyorc.have_ref() else None
    res["cpu_reference_one_core"] = cpu_leg(ref, pair) if ref else None   # before anything touches the GPU
    lib = timing.open_library()
    if lib is None:   # no device: the CPU half alone is still a record
        res["gpu"] = None
        return timing.write_profile("r06_warp_error_1080p.json", res)
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    bufs, ptrs = [], {}
    for b in pair:
        d = device.DeviceBuffer(lib, b.a.nbytes)
        d.upload(b.a)
        bufs.append(d)
        ptrs[id(b)] = d.ptr
    d_filter = device.DeviceBuffer(lib, abi.WARP_FILTER_BYTES)
    d_filter.upload(np.load(W.GOLD)["warped_filter"])
    res["gpu"] = {}
    for chess in (0, 1):
        for n in (1, 8):
            job = W.error_job(*pair, chess, d_filter.ptr, ptrs)
            ws = device.warp_error_workspace(lib, job, n)
            cand = np.zeros(n, np.dtype(abi.WARP_CANDIDATE_DTYPE))
            for c, m in zip(cand, MODELS):
                c["mat"], (c["alpha"], c["beta"], c["gamma"], c["delta"]), c["best_error"] = m, W.lib_shear(m)[1], W.INT64_MAX
            got = device.warp_error_batch(lib, job, cand)
            assert (got["status"] == 0).all()
            if ref:
                want = [W.RefError(ref).error(m, W.AFFINE, *pair, chess, W.INT64_MAX) for m in MODELS[:n]]
                assert got["error"].tolist() == want, (got["error"].tolist(), want)
            d_cand, d_res = device.DeviceBuffer(lib, cand.nbytes), device.DeviceBuffer(lib, 16 * n)
            d_cand.upload(cand)
            launch = lambda: device.check(lib, lib.svt_hip_warp_error_batch(C.byref(job), d_cand.ptr, d_res.ptr, n, sp), "warp_error")  # noqa: E731
            res["gpu"][f"warp_error_batch_n{n}_chess{chess}"] = {**timing.summary(timing.events(torch, stream, repeats, launch)), "errors": got["error"].tolist()}
            if n == 1 and chess == 0:
                host8 = np.zeros(1, np.int64)

                def read_back():
                    device.check(lib, lib.svt_hip_download(host8.ctypes.data_as(C.c_void_p), d_res.ptr, 8, sp), "download")
                    device.check(lib, lib.svt_hip_stream_sync(sp), "sync")

                torch.cuda.synchronize()
                res["gpu"]["read_back_8_bytes_idle_stream"] = host_clock(200, read_back)
                res["gpu"]["launch_n1_plus_read_back"] = host_clock(100, lambda: (launch(), read_back()))
                start = [TRUE[0] + 30000, TRUE[1] - 25000, TRUE[2] + 260, TRUE[3] - 180, TRUE[4] + 100, TRUE[5] - 140, 0, 0]
                t0 = time.perf_counter()
                mat, wt, err = device.gm_refine(lib, job, start, W.AFFINE, 5, W.INT64_MAX, stream.cuda_stream)
                res["gpu"]["gm_refine_affine_5_refinements"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 2), "error": err, "wmmat": mat[:6]}
            del ws
    timing.write_profile("r06_warp_error_1080p.json", res)


if __name__ == "__main__":
    main()
