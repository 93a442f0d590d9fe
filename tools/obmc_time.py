#!/usr/bin/env python3
"""Time OBMC motion refinement (one measurement, no threshold): svt_hip_obmc_target_batch and svt_hip_obmc_search_batch on batches of 4096
descriptors per size class (8 x 8, 16 x 16, 32 x 32, 64 x 64, 128 x 128), under fpel_search_range 8 without diagonals and 16 with them, both
stages on, 8 taps, two iterations per step, entropy costs.  A batch repeats DISTINCT generated blocks of tests/obmc_cases.py (each with its own
samples, neighbours and wsrc / mask arrays).  Device time of each entry point alone between two HIP events, everything resident, warm-up,
median / minimum / maximum of the repeats; the search also at batches of 1 and 64 for the launch overhead.  Every record is checked
against the restatement.  Every size class runs in a process of its own under a time limit, and nothing more is started once one has failed.

    python tools/obmc_time.py --host     # where the reference tree is: per-block time of the reference's calc_target_weighted_pred and
                                         # single_motion_search on one host core, through tests/obmc_pin_driver.c; no device
    python tools/obmc_time.py            # on the device; keeps the "host" section the file already has
Both write profiles/obmc_search_mi355x.json (or --out) and print it as one JSON line."""
import argparse
import ctypes as C
import json
import os
import platform
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import obmc_cases as O  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

SIZES = (8, 16, 32, 64, 128)
CONFIGS = {"r8": dict(fp_range=8, diag=0), "r16_diag": dict(fp_range=16, diag=1)}
BATCH, DISTINCT, STEP_SECONDS = 4096, 32, 400


def cases(size, config):
    """DISTINCT blocks of size x size: smooth content a few samples and a fraction away from the start, 8-sample neighbours on both sides"""
    out = []
    for k in range(DISTINCT):
        start = (8 * (k % 3 - 1), 8 * ((k // 3) % 3 - 1))
        true = (start[0] + (k * 13) % 71 - 35, start[1] + (k * 29 + 5) % 71 - 35)
        n4 = size // 4
        out.append(O.Case("time", size, size, mi_row=32, mi_col=32, mi_rows=128, mi_cols=128, up=1, left=1, above_tiles=((2, 1),) * (n4 // 2), above_from=32,
                          left_tiles=((2, 1),) * (n4 // 2), left_from=32, start=start, ref_mv=(start[0] + k % 7 - 3, start[1] + (k // 7) % 5 - 2), true_mv=true,
                          full=1, frac=1, qindex=100, full_lambda=5000, approx=0, hp=1, taps=3, stop=0, iters=2, kind="smooth", noise=2, seed=7000 + k,
                          **CONFIGS[config]))
    return out


def host(repeats):
    import pyorc
    res = {"what": "least nanoseconds of one call on one core, contexts made beforehand, mean over the distinct blocks", "cpu": cpu_name(), "repeats": repeats}
    with tempfile.TemporaryDirectory() as tmp:
        pin = O.Pin(pyorc.ref(), tmp)
        pin.lib.pin_time.argtypes = [C.c_void_p] * 15 + [C.c_int, C.c_void_p]
        for size in SIZES:
            for config in CONFIGS:
                ns = np.zeros((DISTINCT, 2))
                for k, c in enumerate(cases(size, config)):
                    r = O.Restated(c)
                    src, above, left, ref = (np.ascontiguousarray(p) for p in (r.src, r.above, r.left, r.ref))
                    a_size, a_inter = O.edge_arrays(c.above_tiles, c.above_from, c.mi_cols)
                    l_size, l_inter = O.edge_arrays(c.left_tiles, c.left_from, c.mi_rows)
                    t = O.PinTarget(c.w, c.h, c.mi_row, c.mi_col, c.mi_rows, c.mi_cols, c.up, c.left, c.w, c.w, c.w)
                    a = O.PinSearch(c.w, c.h, ref.shape[1], c.start[0], c.start[1], c.ref_mv[0], c.ref_mv[1], c.mi_row, c.mi_col, c.mi_rows, c.mi_cols, 1, 1,
                                    c.fp_range, c.diag, c.qindex, c.full_lambda, c.approx, c.hp, c.taps, c.stop, c.iters)
                    wsrc, mask, one = np.zeros((c.h, c.w), np.int32), np.zeros((c.h, c.w), np.int32), np.zeros(2)
                    pin.lib.pin_time(C.addressof(t), C.addressof(a), src.ctypes.data, above.ctypes.data, left.ctypes.data, a_size.ctypes.data, a_inter.ctypes.data,
                                     l_size.ctypes.data, l_inter.ctypes.data, wsrc.ctypes.data, mask.ctypes.data, ref.ctypes.data + O.BORDER * ref.shape[1] + O.BORDER,
                                     pin.mvj.ctypes.data, pin.mvrow.ctypes.data - 4 * O.MV_LOW, pin.mvcol.ctypes.data - 4 * O.MV_LOW, repeats, one.ctypes.data)
                    assert (wsrc == r.wsrc).all() and (mask == r.mask).all()
                    ns[k] = one
                res[f"{size}x{size}_{config}"] = {"target_us_per_block": round(float(ns[:, 0].mean()) / 1e3, 3), "search_us_per_block": round(float(ns[:, 1].mean()) / 1e3, 3)}
    return res


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            return next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        return platform.processor()


def child(size, repeats):
    import torch
    lib = timing.open_library()
    if lib is None:
        print(json.dumps(None))
        return
    res = {}
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    for config in CONFIGS:
        cs = cases(size, config)
        restated = [O.Restated(c) for c in cs]
        ar = O.Arena(cs, restated=restated)
        buf = device.DeviceBuffer(lib, ar.host.nbytes)
        buf.upload(ar.host)
        job = ar.job(buf.ptr)
        pick = np.arange(BATCH) % DISTINCT
        t_desc, s_desc = ar.target_descs(buf.ptr)[pick], ar.search_descs(buf.ptr)[pick]
        d_t, d_s = device.upload_descriptors(lib, t_desc), device.upload_descriptors(lib, s_desc)
        d_status, d_out = device.DeviceBuffer(lib, 4 * BATCH), device.DeviceBuffer(lib, C.sizeof(abi.ObmcSearchResult) * BATCH)
        target = lambda: device.check(lib, lib.svt_hip_obmc_target_batch(C.c_void_p(d_t.ptr), C.c_void_p(d_status.ptr), BATCH, sp), "target")  # noqa: E731
        entry = {"blocks": BATCH, "distinct_blocks": DISTINCT}
        ms = timing.events(torch, stream, repeats, target)
        entry["target"] = {**timing.summary(ms), "us_per_block": round(float(np.median(ms)) * 1e3 / BATCH, 4)}
        assert not d_status.download(np.uint32, (BATCH,)).any()
        for n in (1, 64, BATCH):
            search = lambda: device.check(lib, lib.svt_hip_obmc_search_batch(C.byref(job), C.c_void_p(d_s.ptr), C.c_void_p(d_out.ptr), n, sp), "search")  # noqa: E731
            ms = timing.events(torch, stream, repeats, search)
            entry["search" if n == BATCH else f"search_batch_{n}"] = {**timing.summary(ms), "us_per_block": round(float(np.median(ms)) * 1e3 / n, 4)}
        out = d_out.download(np.dtype(abi.OBMC_SEARCH_RESULT_DTYPE), (BATCH,))
        for k in range(BATCH):
            assert out[k]["status"] == abi.OBMC_OK and O.result_tuple(out[k]) == restated[pick[k]].record(), (k, cs[pick[k]])
        entry["checked_against_restatement"] = BATCH
        entry["mean_fullpel_rounds"] = round(float(out["fullpel_rounds"].mean()), 2)
        res[config] = entry
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obmc_search_mi355x.json"))
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--child", type=int, metavar="SIZE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats)
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    if args.host:
        res["host"] = host(args.repeats)
    else:
        res["device"] = dev = {"repeats": args.repeats, "what": "device time of each entry point alone (HIP events), everything resident; a batch repeats "
                               f"{DISTINCT} distinct blocks"}
        for size in SIZES:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--child", str(size)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:   # nothing more is started on the device after a failure
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"obmc_time.py: {size} x {size} ended with status {r.returncode}")
            for config, entry in json.loads(r.stdout.strip().splitlines()[-1]).items():
                dev[f"{size}x{size}_{config}"] = entry
    timing.write_profile(os.path.abspath(args.out), res)


if __name__ == "__main__":
    main()
