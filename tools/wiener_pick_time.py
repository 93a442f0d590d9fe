#!/usr/bin/env python3
"""Time the Wiener decision of one 4K 10-bit luma plane (3840 x 2160, restoration units of 256: 15 x 8 = 120 units) on the device at
the controls of wn_filter_lvl 1, 2 and 5, next to the pieces of the same hand-over that the host path needs and that can be timed
from Python (one measurement, no threshold):
  pick            svt_hip_wiener_pick_plane, statistics resident, HIP events around the whole launch chain, warm-up, median of the repeats;
  moments_down    the download of M and H of all units (host clock around a synchronised copy);
  filter_frame    one svt_hip_restoration_filter_frame of the plane: one trial filter per unit (the host path runs one per trial
                  of the finer search, each a round trip, and reads an SSE back);
  units_up        the upload of the SvtHipLrUnit array.
The host's integer solver is not timed here.  Prints one JSON line and writes it to profiles/wiener_pick_4k.json (or --out).
    python tools/wiener_pick_time.py [--repeats 20] [--out FILE]"""
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

import lr_cases as R  # noqa: E402
import wiener_pick_cases as K  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

W, H, UNIT, BD = 3840, 2160, 256, 10
WIN_OF_LEVEL = {1: 7, 2: 7, 5: 5}        # filter_tap_lvl 1 / 1 / 2 (enc_mode_config.c:1335-1374)


def trial_launches(win, refine, max_one):
    """The trials svt_hip_wiener_pick_plane enqueues up front (trial_bound, csrc/loopfilter_wiener_pick.hip)."""
    per_tap = lambda p: 2 if max_one else 2 + (15, 31, 63)[p] // 4 + 2 + 2      # noqa: E731
    return 1 + (2 * sum(per_tap(p) for p in range((7 - win) >> 1, 3)) if refine else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiener_pick_4k.json"))
    args = ap.parse_args()
    lib = timing.open_library()
    assert lib is not None, "no device"
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    res = {"plane": [W, H], "bit_depth": BD, "unit_size": UNIT, "repeats": args.repeats}
    for lvl, win in WIN_OF_LEVEL.items():
        x = K.make_inputs(K.Case(f"time_l{lvl}", W, H, UNIT, BD, 1, win, lvl, 4000, (200, 1000), "bnbhb", 40 + lvl))
        n = len(x.limits)
        d_dgd, d_src = device.DeviceBuffer(lib, x.dgd.nbytes), device.DeviceBuffer(lib, x.src.nbytes)
        d_dgd.upload(x.dgd), d_src.upload(x.src)
        dgd0 = d_dgd.ptr + (K.B * x.dgd.shape[1] + K.B) * 2
        units, prm = K.wiener_units(x, dgd0, d_src.ptr), K.params(x)
        d_M, d_H = device.DeviceBuffer(lib, n * 49 * 8), device.DeviceBuffer(lib, n * 49 * 49 * 8)
        device.check(lib, lib.svt_hip_wiener_stats(units, n, win, 1, BD, C.c_void_p(d_M.ptr), C.c_void_p(d_H.ptr), sp), "svt_hip_wiener_stats")
        pick = device.DeviceWienerPick(lib, n)
        ms = timing.events(torch, stream, args.repeats, lambda: device.check(lib, pick.run(prm, units, d_M.ptr, d_H.ptr, None, sp), "svt_hip_wiener_pick_plane"))
        got = pick.download()
        trials = got["units"]["trials"]
        r = res[f"wn_filter_lvl_{lvl}"] = {"wiener_win": win, "units": n, "launches_per_pick": 2 + trial_launches(win, x.refine, x.max_one),
                                          "pick": timing.summary(ms),
                                          "trials_per_unit": {"mean": round(float(trials.mean()), 2), "max": int(trials.max()), "sum": int(trials.sum())},
                                          "units_wiener": int(got["result"]["n_wiener"]), "frame_restoration_type": int(got["result"]["frame_restoration_type"])}
        # the parent's pieces of the same hand-over
        host = np.empty(n * (49 + 49 * 49), np.int64)
        down = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            device.check(lib, lib.svt_hip_download(host.ctypes.data, d_M.ptr, n * 49 * 8, sp), "download")
            device.check(lib, lib.svt_hip_download(host.ctypes.data + n * 49 * 8, d_H.ptr, n * 49 * 49 * 8, sp), "download")
            device.check(lib, lib.svt_hip_stream_sync(sp), "sync")
            down.append((time.perf_counter() - t0) * 1e3)
        hu, vu = R.units_in(W, UNIT), R.units_in(H, UNIT)
        assert hu * vu == n
        d_dst = device.DeviceBuffer(lib, (H + 2) * (W + R.DST_EXTRA) * 2)
        lr = got["lr_units"].copy()
        lr["restoration_type"], lr["hfilter"], lr["vfilter"] = 1, got["units"]["hfilter"], got["units"]["vfilter"]     # a trial filters every unit
        d_lr = device.DeviceBuffer(lib, lr.nbytes)
        up = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            device.check(lib, lib.svt_hip_upload(d_lr.ptr, lr.ctypes.data, lr.nbytes, sp), "upload")
            device.check(lib, lib.svt_hip_stream_sync(sp), "sync")
            up.append((time.perf_counter() - t0) * 1e3)
        arr = (abi.LrPlane * 1)(abi.LrPlane(dgd0, d_dst.ptr, x.dgd.shape[1], W + R.DST_EXTRA, W, H, 0, 0, 1, BD, UNIT, hu, vu, d_lr.ptr, 0, 0, 0, 1))
        fms = timing.events(torch, stream, args.repeats, lambda: device.check(lib, lib.svt_hip_restoration_filter_frame(arr, C.c_uint32(1), sp), "filter_frame"))
        pieces = {"moments_down_ms": round(statistics.median(down), 4), "moments_bytes": int(host.nbytes), "filter_frame": timing.summary(fms),
                  "units_up_ms": round(statistics.median(up), 4), "units_bytes": int(lr.nbytes)}
        r["parent_pieces"] = pieces
        pm, fm = r["pick"]["median_ms"], pieces["filter_frame"]["median_ms"]
        serial = pieces["moments_down_ms"] + int(trials.max()) * fm + pieces["units_up_ms"]      # one frame-wide trial per step of the longest search
        r["ratio"] = {"pick_over_moments_down": round(pm / pieces["moments_down_ms"], 2), "pick_over_one_filter_frame": round(pm / fm, 2),
                      "pick_over_units_up": round(pm / pieces["units_up_ms"], 2),
                      "parent_pieces_with_max_trials_ms": round(serial, 4), "pick_over_parent_pieces": round(pm / serial, 3)}
        r["copied_back_bytes"] = C.sizeof(abi.WienerPickResult) + n * C.sizeof(abi.WienerPickUnit)
    timing.write_profile(os.path.abspath(args.out), res)


if __name__ == "__main__":
    main()
