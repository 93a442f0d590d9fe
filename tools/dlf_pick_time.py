#!/usr/bin/env python3
"""Time one deblocking level search of a 4K 10-bit 4:2:0 picture, all three planes searched, on both sides (one measurement, no
threshold):
  new:    svt_hip_dlf_pick_levels, HIP events around the whole chain of max_rounds x {plan, trial} + plan, warm-up, median of repeats;
  parent: the SAME trials (the measured entries of the device record's ss_err) with every trial issued as the encoder glue's
          svt_hip_bind_dlf_try issues it: svt_hip_copy of the plane (and its synchronise), svt_hip_loop_filter_frame of that
          plane, svt_hip_plane_sse, the 8-byte download and a synchronise, timed on the host clock: the time includes the round trips.
Every error of the parent leg is checked against the device record.  The new chain is timed a second time with max_rounds = the rounds
the search needs, which gives the cost of an empty round.  Prints one JSON line and writes it to profiles/dlf_pick_4k.json (or --out)
with the medians, the parent's run-to-run spread (max - min of its repeats), the trial counts and the number of empty rounds.
    python tools/dlf_pick_time.py [--repeats 20] [--rounds N] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import dlf_pick_cases as K  # noqa: E402
from benchlib import lf_inputs as LB  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

W, H, BD = 3840, 2160, 10
START = (16, 8, 8)


def picture(rng, torch, dev, inp):
    """Source = smooth content with a little noise; reconstruction = source + one step per 8x8 block (the partition of
    benchlib.lf_inputs has its edges on that grid).  Written into the planes lf_inputs.build allocated."""
    for pl in range(3):
        w, h = (W >> (pl > 0)) + 2 * LB.PAD, (H >> (pl > 0)) + 2 * LB.PAD
        yy, xx = np.mgrid[0:h, 0:w]
        src = (1 << BD) * (0.5 + 0.25 * np.sin(xx / 23.0) * np.cos(yy / 31.0)) + rng.integers(-4, 5, size=(h, w))
        rec = src + 4 * rng.integers(-7, 8, size=(h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w]
        for t, img in ((inp["srcs"][pl], src), (inp["planes"][pl], rec)):
            t.copy_(torch.from_numpy(np.clip(np.rint(img), 0, (1 << BD) - 1).astype(np.uint16).view(np.int16)).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=abi.DLF_PICK_DEFAULT_ROUNDS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dlf_pick_4k.json"))
    args = ap.parse_args()
    lib = timing.open_library()
    if lib is None:
        sys.exit("dlf_pick_time.py: no device")
    import torch
    dev, rng = torch.device("cuda:0"), np.random.default_rng(5)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    inp = LB.build(lib, dev, rng, W, H, BD, torch)
    picture(rng, torch, dev, inp)
    torch.cuda.synchronize()
    strides = [(W >> (p > 0)) + 2 * LB.PAD for p in range(3)]
    prm = abi.DlfPickParams()
    C.memmove(C.addressof(prm.frame), C.addressof(inp["lf_frame"]), C.sizeof(abi.LfFrame))
    for p in range(3):
        prm.src[p], prm.src_stride[p] = inp["ptr"](inp["srcs"][p], W >> (p > 0)), strides[p]
        prm.sse_width[p], prm.sse_height[p], prm.start_level[p] = W >> (p > 0), H >> (p > 0), START[p]
    prm.plane_mask, prm.max_rounds = 7, args.rounds
    pick = device.DeviceDlfPick(lib, W, H, 1)
    launch = lambda: device.check(lib, pick.run(prm, sp), "svt_hip_dlf_pick_levels")  # noqa: E731
    ms = timing.events(torch, stream, args.repeats, launch)
    rec = pick.download(sp)
    assert int(rec["finished"]) == 7, rec
    needed = int(rec["rounds"].max())          # the same search with no empty round: the difference is what the empty ones cost
    prm.max_rounds = needed
    ms_needed = timing.events(torch, stream, args.repeats, launch)
    assert pick.download(sp).tobytes() == rec.tobytes()
    prm.max_rounds = args.rounds

    # ---- the parent's chain: one trial = copy + frame filter of one plane + SSE + 8-byte download, the loop on the host
    work = [torch.empty_like(t) for t in inp["planes"]]
    d_sum, h_sum = device.DeviceBuffer(lib, 8), np.zeros(1, np.uint64)
    x = K.Inputs()      # what level_table reads: no segment features
    x.case = K.Case("time_4k", W, H, BD, 1, 64, 0, 0, 0, 0, 0, 0, 7, START, "aligned", 0)
    x.seg_enabled, x.seg_data = np.zeros((8, 4), np.uint8), np.zeros((8, 4), np.int16)

    def trial(p, level):
        f = abi.LfFrame()
        C.memmove(C.addressof(f), C.addressof(inp["lf_frame"]), C.sizeof(f))
        levels = [level, level, 0, 0] if p == 0 else [0, 0, level if p == 1 else 0, level if p == 2 else 0]
        f.plane[p] = inp["ptr"](work[p], W >> (p > 0))
        f.filter_level[0], f.filter_level[1], f.filter_level_u, f.filter_level_v = levels
        f.plane_start, f.plane_end = p, p + 1
        C.memmove(f.lvl, K.level_table(x, levels).ctypes.data, 768)
        device.check(lib, lib.svt_hip_copy(work[p].data_ptr(), inp["planes"][p].data_ptr(), work[p].numel() * 2, sp), "svt_hip_copy")
        device.check(lib, lib.svt_hip_stream_sync(sp), "svt_hip_stream_sync")
        device.check(lib, lib.svt_hip_loop_filter_frame(C.byref(f), sp), "svt_hip_loop_filter_frame")
        device.check(lib, lib.svt_hip_plane_sse(prm.src[p], strides[p], f.plane[p], strides[p], W >> (p > 0), H >> (p > 0), 1, d_sum.ptr, sp),
                     "svt_hip_plane_sse")
        device.check(lib, lib.svt_hip_download(h_sum.ctypes.data, d_sum.ptr, 8, sp), "svt_hip_download")
        device.check(lib, lib.svt_hip_stream_sync(sp), "svt_hip_stream_sync")
        return int(h_sum[0])

    # the trials the search made are the measured entries of the record; each one, issued the parent's way, gives the record's error
    sequence = [(p, level) for p in range(3) for level in range(64) if rec["ss_err"][p][level] >= 0]
    for p, level in sequence:
        assert trial(p, level) == int(rec["ss_err"][p][level]), (p, level)
    parent = []
    for _ in range(3 + args.repeats):
        t0 = time.perf_counter()
        for p, level in sequence:
            trial(p, level)
        parent.append((time.perf_counter() - t0) * 1e3)
    parent = parent[3:]
    res = {"picture": f"{W}x{H} {BD}-bit 4:2:0, all planes searched, start levels {list(START)}", "repeats": args.repeats,
           "levels": [int(v) for v in rec["level"]], "rounds": [int(v) for v in rec["rounds"]], "trials": [int(v) for v in rec["trials"]],
           "max_rounds": args.rounds, "empty_rounds": args.rounds - int(rec["rounds"].max()), "launches": 2 * args.rounds + 1,
           "new_chain": timing.summary(ms),
           "new_chain_without_empty_rounds": {**timing.summary(ms_needed), "max_rounds": needed},
           "empty_round_us": round((statistics.median(ms) - statistics.median(ms_needed)) * 1e3 / max(1, args.rounds - needed), 2),
           "parent_chain": {**timing.summary(parent), "spread_ms": round(max(parent) - min(parent), 4), "trials_issued": len(sequence),
                            "host_round_trips": 2 * len(sequence)},
           "new_minus_parent_median_ms": round(statistics.median(ms) - statistics.median(parent), 4)}
    timing.write_profile(os.path.abspath(args.out), res)


if __name__ == "__main__":
    main()
