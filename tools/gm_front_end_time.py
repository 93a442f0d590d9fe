#!/usr/bin/env python3
"""Time the global-motion front end on the device (a measurement, no threshold) beside the reference's own two functions on the CPU of
the same machine:
  detect   svt_hip_gm_detect_corners, one call over a plane and its 1/4 and 1/16 planes (2 x 2 means), for 3840 x 2160 and 1920 x 1080:
           cells of 8 x 8 random levels under +-8 noise, so that corners sit where cells meet
  match    svt_hip_gm_match_corners, 4096 frame corners against 4096 reference corners of a 1920 x 1080 noise picture and its copy shifted
           by (3, 2) under +-6 noise, at match_sz 7 and 13, for two corner sets:
             spread   random positions over the whole picture, the usual case: few candidates within the radius of 120
             packed   a 64 x 64 grid of adjacent positions: every pair within the radius, 16.7 M correlations
The device results are compared with the reference's before anything is timed.  HIP events after warm-up, median of the repeats.
reference_cpu: svt_av1_fast_corner_detect and svt_av1_determine_correspondence of oracle/_ref/libsvtref.so on the same inputs, single
thread, one run each (the packed case takes seconds), with the C table and, where the intrinsics table of ref_set_simd offers
svt_av1_compute_cross_correlation, with that table too.  Each half is measured where it can be and merged into the record that is
already at the output path.  Writes profiles/gm_front_end.json, or the path given as second argument.
    python tools/gm_front_end_time.py [repeats] [output]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import gm_cases as K  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "gm_front_end.json")
DETECT_SIZES = ((3840, 2160), (1920, 1080))
MATCH_W, MATCH_H, MATCH_SIZES, N = 1920, 1080, (7, 13), abi.GM_MAX_CORNERS


def pyramid(w, h, seed):
    """[full, 1/4, 1/16] planes, (h, w) uint8 each"""
    rng = np.random.RandomState(seed)
    cells = rng.randint(0, 256, (-(-h // 8), -(-w // 8)))
    full = np.clip(np.kron(cells, np.ones((8, 8), np.int64))[:h, :w] + rng.randint(-8, 9, (h, w)), 0, 255).astype(np.uint8)
    out = [full]
    for _ in range(2):
        a = out[-1].astype(np.uint32)
        a = a[:a.shape[0] // 2 * 2, :a.shape[1] // 2 * 2]
        out.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return out


def match_inputs():
    """(frame, reference, {set: (frame corners, reference corners)}), the corners as [N, 2] int32 in raster order"""
    rng = np.random.RandomState(77)
    canvas = rng.randint(0, 256, (MATCH_H + 8, MATCH_W + 8))
    frm = canvas[4:4 + MATCH_H, 4:4 + MATCH_W].astype(np.uint8)
    ref = np.clip(canvas[2:2 + MATCH_H, 1:1 + MATCH_W] + rng.randint(-6, 7, (MATCH_H, MATCH_W)), 0, 255).astype(np.uint8)
    flat = np.sort(rng.choice((MATCH_W - 40) * (MATCH_H - 40), N, replace=False))
    spread = np.stack([flat % (MATCH_W - 40) + 16, flat // (MATCH_W - 40) + 16], axis=1).astype(np.int32)
    gy, gx = np.divmod(np.arange(N), 64)
    packed = np.stack([gx + 900, gy + 500], axis=1).astype(np.int32)
    return frm, ref, {"spread": (spread, spread + np.array([3, 2], np.int32)), "packed": (packed, packed + np.array([3, 2], np.int32))}


def corner_record(xy):
    rec = np.zeros(1, abi.GM_CORNERS_DTYPE)
    rec["count"], rec["found"] = len(xy), len(xy)
    rec["xy"][0, :2 * len(xy)] = xy.reshape(-1)
    return rec


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, round((time.perf_counter() - t0) * 1e3, 3)


def correlation_tables(ref):
    """{label: level of ref_set_simd}: the C table, and the intrinsics table where it has a row for svt_av1_compute_cross_correlation"""
    tables, fn, i = {"c": 0}, C.c_char_p(), 0
    ref.ref_simd_row.restype = C.c_char_p
    while True:
        name = ref.ref_simd_row(i, C.byref(fn), None, None)
        if name is None:
            return tables
        if name == b"svt_av1_compute_cross_correlation":
            tables[fn.value.decode()] = 1
        i += 1


def reference_cpu():
    """(milliseconds of the reference's functions on this machine's CPU, the correspondences of the C table per case), or (None, {})
    without oracle/_ref/libsvtref.so"""
    import pyorc
    if not pyorc.have_ref():
        return None, {}
    ref, kept = pyorc.ref(), {}
    out = {"note": "single thread, one run each, on the CPU of the machine that ran this tool", "detect": {}, "match": {}}
    for w, h in DETECT_SIZES:
        row = {}
        for p in pyramid(w, h, w):
            (_, found, _), ms = clock(lambda: K.ref_detect(ref, p, p.shape[1]))      # two calls: with and without the cap
            row[f"{p.shape[1]}x{p.shape[0]}"] = {"found": found, "ms_two_calls": ms}
        out["detect"][f"{w}x{h}"] = row
        print("reference detect", w, h, row, flush=True)
    frm, rbuf, sets = match_inputs()
    for table, level in correlation_tables(ref).items():
        ref.ref_set_simd(level)
        for name, (fxy, rxy) in sets.items():
            for sz in MATCH_SIZES:
                pts, ms = clock(lambda: K.ref_correspond(ref, frm, fxy, rbuf, rxy, MATCH_W, MATCH_H, sz))
                out["match"][f"{name}_sz{sz}_{table}"] = {"correspondences": len(pts), "ms": ms}
                kept.setdefault((name, sz), pts)
                print("reference match", name, sz, table, len(pts), ms, flush=True)
    ref.ref_set_simd(0)
    return out, kept


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    target = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else PROFILE     # read and written at the same place
    try:
        with open(target) as f:
            res = json.load(f)
    except OSError:
        res = {}
    res.update({"repeats": repeats, "match_picture": [MATCH_W, MATCH_H], "corners": N})
    cpu, want_pts = reference_cpu()
    if cpu is not None:
        res["reference_cpu"] = cpu
    res.setdefault("reference_cpu", None)
    lib = timing.open_library()
    if lib is None:
        res.setdefault("gpu", None)
        return timing.write_profile(target, res)
    import pyorc
    import torch
    ref = pyorc.ref() if pyorc.have_ref() else None
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    gpu = {"detect": {}, "match": {}}

    def up(arr):
        d = device.DeviceBuffer(lib, arr.nbytes)
        d.upload(arr)
        return d
    for w, h in DETECT_SIZES:
        planes = pyramid(w, h, w)
        d_planes = [up(p) for p in planes]
        arr = (abi.GmPlane * 3)(*[abi.GmPlane(d.ptr, p.shape[1], p.shape[0], p.shape[1], 0) for d, p in zip(d_planes, planes)])
        ws_bytes = sum(lib.svt_hip_gm_corners_workspace_bytes(p.shape[1], p.shape[0], 1) for p in planes)
        d_ws, d_out = device.DeviceBuffer(lib, ws_bytes), device.DeviceBuffer(lib, 3 * C.sizeof(abi.GmCorners))

        def detect():
            device.check(lib, lib.svt_hip_gm_detect_corners(arr, 3, d_out.ptr, d_ws.ptr, ws_bytes, sp), "svt_hip_gm_detect_corners")
        detect()
        torch.cuda.synchronize()
        recs = d_out.download(abi.GM_CORNERS_DTYPE, (3,))
        if ref is not None:
            for rec, p in zip(recs, planes):
                count, found, xy = K.ref_detect(ref, p, p.shape[1])
                assert (int(rec["count"]), int(rec["found"])) == (count, found) and np.array_equal(rec["xy"][:2 * count].reshape(-1, 2), xy)
        entry = timing.summary(timing.events(torch, stream, repeats, detect))
        entry.update(found=[int(r["found"]) for r in recs], checked_against_reference=ref is not None, workspace_bytes=int(ws_bytes))
        gpu["detect"][f"{w}x{h}_and_quarter_and_sixteenth"] = entry
        print("detect", w, h, entry, flush=True)
    frm, rbuf, sets = match_inputs()
    d_frm, d_ref, d_out = up(frm), up(rbuf), device.DeviceBuffer(lib, C.sizeof(abi.GmMatches))
    for name, (fxy, rxy) in sets.items():
        d_fc, d_rc = up(corner_record(fxy)), up(corner_record(rxy))
        for sz in MATCH_SIZES:
            jobs = (abi.GmMatchJob * 1)(abi.GmMatchJob(abi.GmPlane(d_frm.ptr, MATCH_W, MATCH_H, MATCH_W, 0), abi.GmPlane(d_ref.ptr, MATCH_W, MATCH_H, MATCH_W, 0),
                                                       d_fc.ptr, d_rc.ptr, 4, 4, sz))

            def match():
                device.check(lib, lib.svt_hip_gm_match_corners(jobs, 1, d_out.ptr, sp), "svt_hip_gm_match_corners")
            match()
            torch.cuda.synchronize()
            rec = d_out.download(abi.GM_MATCHES_DTYPE, (1,))[0]
            checked = (name, sz) in want_pts
            if checked:
                want = want_pts[name, sz]
                assert int(rec["count"]) == len(want) and np.array_equal(rec["pts"][:4 * len(want)].reshape(-1, 4), want), (name, sz)
            entry = timing.summary(timing.events(torch, stream, repeats, match))
            entry.update(correspondences=int(rec["count"]), checked_against_reference=checked)
            gpu["match"][f"{name}_sz{sz}"] = entry
            print("match", name, sz, entry, flush=True)
    res["gpu"] = gpu
    timing.write_profile(target, res)


if __name__ == "__main__":
    main()
