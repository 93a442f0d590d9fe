#!/usr/bin/env python3
"""Time the sub-pel motion search of a 4K picture's blocks against one reference (one measurement, no threshold): the descriptors
a 3840 x 2160 picture gives for 16 x 16 blocks (32400) and for 64 x 64 blocks (1980), under the controls of md_subpel level 1 (_tree,
8 taps, two iterations per step, 1/8 pel) and of level 8 (_pruned, quarter-pel, skip_diag_refinement 4, with its variance, error and
deviation exits).  Device time of svt_hip_subpel_search_batch alone between two HIP events, pictures, tables and descriptors resident,
warm-up, median / minimum / maximum of the repeats.  A sample of the records is checked against the restatement of
tests/subpel_cases.py.  Every configuration runs in a process of its own under a time limit, and nothing more is started once one
has failed.  Prints one JSON line and writes it to profiles/subpel_4k.json (or --out).
    python tools/subpel_time.py [--repeats 20] [--out FILE]"""
import argparse
import collections
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import subpel_cases as S  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

WIDTH, HEIGHT, PAD = 3840, 2160, 32
LEVELS = {   # md_subpel_me_controls (enc_mode_config.c)
    1: dict(method=S.TREE, taps=abi.SUBPEL_USE_8_TAPS, iters=2, forced_stop=0, pred_var_th=0, abs_th_mult=0, round_dev_th=S.INT_MAX, skip_diag=0, bias_fp=0),
    8: dict(method=S.PRUNED, taps=abi.SUBPEL_USE_4_TAPS, iters=1, forced_stop=1, pred_var_th=100, abs_th_mult=2, round_dev_th=-25, skip_diag=4, bias_fp=1)}
STEP_SECONDS = 240


def picture():
    """(src, ref) with PAD samples of border: smooth content plus noise; every block of src is ref moved by half a sample, to the right in
    even block columns of 16 and down in odd ones, so that sub-pel positions win"""
    rs = np.random.RandomState(2160)
    H, W = HEIGHT + 2 * PAD, WIDTH + 2 * PAD
    coarse = rs.randint(16, 240, (H // 8 + 5, W // 8 + 5)).astype(np.int64)
    smooth = np.kron(coarse, np.ones((8, 8), np.int64))
    for axis in (0, 1, 0, 1):   # two box filters of 8 each way: close to the interpolation of a coarse grid
        c = np.cumsum(smooth, axis=axis)
        smooth = (c.take(range(8, c.shape[axis]), axis) - c.take(range(0, c.shape[axis] - 8), axis) + 4) >> 3
    ref = smooth[:H + 1, :W + 1] + rs.randint(-3, 4, (H + 1, W + 1))
    right = (ref[:H, :W] + ref[:H, 1:W + 1] + 1) >> 1
    down = (ref[:H, :W] + ref[1:H + 1, :W] + 1) >> 1
    odd = ((np.arange(W) - PAD) // 16) % 2 == 1
    src = np.where(odd[None, :], down, right) + rs.randint(-2, 3, (H, W))
    return np.clip(src, 0, 255).astype(np.uint8), np.clip(ref[:H, :W], 0, 255).astype(np.uint8)


def case_at(size, level, k):
    kw = dict(group="time", w=size, h=size, cost_type=S.ENTROPY, epb=900, early_exit_th=0, early_exit=0, allow_hp=1, qp=32, mvp_th=0, hp_mv_th=0, mvp_dist=0,
              mvp=(0, 0), start=(8 * (k % 3 - 1), 8 * ((k // 3) % 3 - 1)), ref_mv=(k % 7 - 3, (k // 7) % 9 - 4), true_mv=(0, 0), limits=None, kind="time",
              noise=0, seed=0)
    kw.update(LEVELS[level])
    return S.Case(**kw)


def child(size, level, repeats):
    import torch
    lib = timing.open_library()
    if lib is None:
        print(json.dumps(None))
        return
    src, ref = picture()
    stride = src.shape[1]
    _, row, col = mvtab = S.mv_cost_tables()
    d_src, d_ref = device.DeviceBuffer(lib, src.nbytes), device.DeviceBuffer(lib, ref.nbytes)
    d_row, d_col = device.DeviceBuffer(lib, row.nbytes), device.DeviceBuffer(lib, col.nbytes)
    d_src.upload(src), d_ref.upload(ref), d_row.upload(row), d_col.upload(col)
    job = abi.SubpelJob()
    job.mvjcost[:] = [int(v) for v in mvtab[0]]
    job.mvcost[0], job.mvcost[1] = d_row.ptr - 4 * S.MV_LOW, d_col.ptr - 4 * S.MV_LOW
    blocks = [(y, x) for y in range(0, HEIGHT - size + 1, size) for x in range(0, WIDTH - size + 1, size)]
    cases = [case_at(size, level, k) for k in range(len(blocks))]
    descs = np.zeros(len(blocks), abi.SUBPEL_DESC_DTYPE)
    for k, ((y, x), c) in enumerate(zip(blocks, cases)):
        at = (y + PAD) * stride + x + PAD
        lim = S.mv_limits(S.LimitCase(y // 4, x // 4, size // 4, size // 4, HEIGHT // 4, WIDTH // 4, c.ref_mv[0], c.ref_mv[1]))
        descs[k] = S.fill_desc(c, d_src.ptr + at, d_ref.ptr + at, stride, stride, lim)
    d_desc = device.upload_descriptors(lib, descs)
    d_out = device.DeviceBuffer(lib, C.sizeof(abi.SubpelResult) * len(blocks))
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    launch = lambda: device.check(lib, lib.svt_hip_subpel_search_batch(C.byref(job), C.c_void_p(d_desc.ptr), C.c_void_p(d_out.ptr), len(blocks), sp),  # noqa: E731
                                  "svt_hip_subpel_search_batch")
    ms = timing.events(torch, stream, repeats, launch)
    out = d_out.download(np.dtype(abi.SUBPEL_RESULT_DTYPE), (len(blocks),))
    assert not out["status"].any()
    # a sample against the restatement, on the picture's own samples around the block
    B = S.BORDER
    assert PAD >= B
    sample = list(range(len(blocks)))[::max(1, len(blocks) // 48)][:48]
    for k in sample:
        y, x = blocks[k][0] + PAD, blocks[k][1] + PAD
        crop = lambda p: p[y - B:y + size + B, x - B:x + size + B]  # noqa: E731
        c = cases[k]._replace(limits=tuple(int(descs[k][f]) for f in ("col_min", "col_max", "row_min", "row_max")))
        assert S.result_tuple(out[k]) == S.Search(c, crop(src), crop(ref)).record(), (k, c)
    exits = collections.Counter(int(e) for e in out["exit"])
    moved = int(((out["best_mv"]["row"] != descs["start_mv"]["row"]) | (out["best_mv"]["col"] != descs["start_mv"]["col"])).sum())
    print(json.dumps({**timing.summary(ms), "blocks": len(blocks), "us_per_block": round(float(np.median(ms)) * 1e3 / len(blocks), 4),
                      "checked_against_restatement": len(sample), "exits": {str(k): exits[k] for k in sorted(exits)}, "blocks_that_left_the_start": moved}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subpel_4k.json"))
    ap.add_argument("--child", nargs=2, type=int, metavar=("SIZE", "LEVEL"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.repeats)
    res = {"picture": [WIDTH, HEIGHT], "repeats": args.repeats, "what": "device time of svt_hip_subpel_search_batch alone (HIP events), everything resident",
           "exit_codes": "SVT_HIP_SUBPEL_EXIT_*: 1 early flag, 2 variance, 3 error threshold, 4 no round, 5 round deviation, 6 ran to the end"}
    for size in (16, 64):
        for level in (1, 8):
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--child", str(size), str(level)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:   # nothing more is started on the device after a failure
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"subpel_time.py: {size} x {size} at level {level} ended with status {r.returncode}")
            res[f"{size}x{size}_level{level}"] = json.loads(r.stdout.strip().splitlines()[-1])
    timing.write_profile(os.path.abspath(args.out), res)


if __name__ == "__main__":
    main()
