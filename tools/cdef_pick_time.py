#!/usr/bin/env python3
"""Time one CDEF strength decision of a 4K picture (60 x 34 = 2040 filter blocks, all taking part) with 16 and with 64 searched
strengths, on both sides (one measurement, no threshold):
  device: svt_hip_cdef_pick_strengths, tables resident, HIP events around the whole launch chain, warm-up, median of the repeats;
  host:   what the encoder glue does for the same decision without it: the download of the three tables (host clock around a
          synchronised copy) plus the finish_cdef_search driver of tests/cdef_pick_cases.py over the reference's svt_search_one_dual
          (oracle/_ref) on one core, the C function and the one the reference's dispatch pointer selects; the time spent inside
          the 75 leaf calls is given apart from the driver's own Python.
The device result is checked against the host's.  Prints one JSON line and writes it to profiles/cdef_pick_4k.json (or --out);
without a device the device half is null, without oracle/_ref the host half.
    python tools/cdef_pick_time.py [--repeats 20] [--out FILE]"""
import argparse
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
import cdef_pick_cases as K  # noqa: E402
import leaf_cases  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import device  # noqa: E402

COLS, ROWS = 60, 34
STEPS = 5 << 3                      # the widest signalling width: 8 greedy + 32 refinement steps; the others run beside it
LAUNCHES = 1 + 2 * STEPS + 1        # prepare, (accumulate, select) per step, finish (csrc/loopfilter_cdef_pick.hip)


def case(n):
    return K.Case(f"time_n{n}", COLS, ROWS, n, 24, "plain", "all", 1, 62, 1 << 32, 100 + n)


def host_leg(ref, x, repeats):
    """Median ms of the driver over each reference leaf, and of the part of it spent inside the leaf."""
    V = C.c_void_p
    proto = C.CFUNCTYPE(C.c_uint64, V, V, C.c_int, V, C.c_int, C.c_int, C.c_int)
    leaves = {"dispatch": proto(V.in_dll(ref, "svt_search_one_dual").value), "c": proto(C.cast(ref.svt_search_one_dual_c, V).value)}
    out, results = {}, {}
    for name, fn in leaves.items():
        total, inside = [], []
        for _ in range(repeats):
            spent = [0.0]

            def timed(*a):
                t0 = time.perf_counter()
                r = fn(*a)
                spent[0] += time.perf_counter() - t0
                return r

            t0 = time.perf_counter()
            results[name] = K.drive(x, lambda c: leaf_cases.run_dual(timed, c))
            total.append((time.perf_counter() - t0) * 1e3), inside.append(spent[0] * 1e3)
        out[f"driver_{name}_ms"], out[f"leaf_calls_{name}_ms"] = round(statistics.median(total), 3), round(statistics.median(inside), 3)
    assert K.same(results["c"], results["dispatch"]) == []
    return out, results["c"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdef_pick_4k.json"))
    args = ap.parse_args()
    assert args.repeats >= 20
    res = {"filter_blocks": COLS * ROWS, "repeats": args.repeats, "launches_per_pick": LAUNCHES, "serial_steps": STEPS}
    ref = pyorc.ref() if pyorc.have_ref() else None
    lib = timing.open_library()
    if lib is not None:
        import torch
        stream = torch.cuda.Stream()
        sp = C.c_void_p(stream.cuda_stream)
    for n in (16, 64):
        x = K.make_inputs(case(n))
        r = res[f"n_strengths_{n}"] = {"bytes_no_longer_transferred": {"tables_down": int(x.mse.nbytes), "strengths_up": 2 * x.n_fb},
                                       "host": None, "device": None}
        want = None
        if ref:
            r["host"], want = host_leg(ref, x, 3)
        if lib is None:
            continue
        d_mse, d_filt = device.DeviceBuffer(lib, x.mse.nbytes), device.DeviceBuffer(lib, x.filt.nbytes)
        d_mse.upload(x.mse), d_filt.upload(x.filt)
        pick, prm = device.DeviceCdefPick(lib, x.n_fb, n), K.params(x)
        launch = lambda: device.check(lib, pick.run(prm, d_mse.ptr, d_filt.ptr, sp), "svt_hip_cdef_pick_strengths")  # noqa: E731
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        if want is not None:
            assert K.same(pick.download(), want, ("result", "fb_gi", "fb_strength")) == []
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.repeats)]
        enqueue = []
        for a, b in evs:
            a.record(stream)
            t0 = time.perf_counter()
            launch()
            enqueue.append((time.perf_counter() - t0) * 1e3)
            b.record(stream)
            torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in evs]
        r["device"] = {**timing.summary(ms), "per_launch_us": round(statistics.median(ms) * 1e3 / LAUNCHES, 2), "host_enqueue_median_ms": round(statistics.median(enqueue), 4),
                       "workspace_bytes": pick.workspace.nbytes}
        host = np.empty_like(x.mse)
        down = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            device.check(lib, lib.svt_hip_download(host.ctypes.data_as(C.c_void_p), d_mse.ptr, host.nbytes, sp), "download")
            device.check(lib, lib.svt_hip_stream_sync(sp), "sync")
            down.append((time.perf_counter() - t0) * 1e3)
        r["tables_download_ms"] = round(statistics.median(down), 4)
    timing.write_profile(os.path.abspath(args.out), res)


if __name__ == "__main__":
    main()
