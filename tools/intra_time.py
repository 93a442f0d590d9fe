#!/usr/bin/env python3
"""Time svt_hip_intra_search_frames on one whole picture (default 3840x2160, the "edges" test picture of tests/intra_cases.py):
ms per picture for SAD and SATD over all 13 modes, one picture per call and 16 pictures per call.  Needs the GPU.
    python tools/intra_time.py [width height] [iterations]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import intra_cases as I  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402


def main():
    w, h = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    lib = abi.load()
    rc = lib.svt_hip_init(0)
    assert rc == 0, lib.svt_hip_last_error().decode()
    plane = I.Plane(I.picture("edges", w, h, 1), 1)
    buf = device.DeviceBuffer(lib, plane.buf.nbytes)
    buf.upload(plane.buf)
    out = device.DeviceIntraOut(lib, w, h)
    res = {"width": w, "height": h, "iterations": iters}
    for name, use_sad in (("sad", 1), ("satd", 0)):
        job = out.fill_job(abi.IntraSearchJob())
        job.src, job.ctrls = plane.desc(buf.ptr), abi.IntraCtrls(abi.PAETH_PRED, use_sad, abi.DEFAULT_SHAPE, 0, w, h)
        for batch in (1, 16):
            jobs = [job] * batch  # the same picture and outputs: the launch does the work of `batch` pictures
            arr = (abi.IntraSearchJob * batch)(*jobs)
            for _ in range(3):
                device.check(lib, lib.svt_hip_intra_search_frames(arr, batch, None), "warm-up")
            device.check(lib, lib.svt_hip_stream_sync(None), "sync")
            t0 = time.perf_counter()
            for _ in range(iters):
                device.check(lib, lib.svt_hip_intra_search_frames(arr, batch, None), "intra search")
            device.check(lib, lib.svt_hip_stream_sync(None), "sync")
            res[f"{name}_ms_per_picture_batch{batch}"] = round((time.perf_counter() - t0) * 1e3 / (iters * batch), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
