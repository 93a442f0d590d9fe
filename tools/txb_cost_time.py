#!/usr/bin/env python3
"""Time svt_hip_txb_cost_batch on a 4K picture's worth of transform-type search (one measurement, no threshold): every 4 x 4, 8 x 8,
16 x 16 and 32 x 32 luma block of a 3840 x 2160 picture x 16 candidate transform types, one descriptor and one quantised block each,
rate and RD cost written per descriptor.  The candidates cycle through the scans of tests/golden/txb_cost.npz (one type per class the
size allows); eob is uniform in 0 .. n / 4 with small magnitudes below it, the table set alternates per block.  Both placements of
the launch's two coefficient-cost tables through svt_hip_txb_cost_batch_placed: read through the cache (0) and staged into LDS once
per workgroup (1).  HIP events around the launch after warm-up, median of the repeats.  Writes profiles/txb_cost_4k.json, beside
the wave-launch bound that profiles/intra_predict_4k.json measured; without a device the GPU half is recorded as null.
    python tools/txb_cost_time.py [repeats]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import txb_cost_cases as T  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

WIDTH, HEIGHT, CANDIDATES = 3840, 2160, 16
SIZES = (4, 8, 16, 32)


def workload(gold, size, rng):
    """(arena image, descriptor record array): blocks in raster order, the 16 candidates of a block adjacent."""
    n = size * size
    nd = (WIDTH // size) * (HEIGHT // size) * CANDIDATES
    types = T.size_types(size, size)
    iscans = [gold.iscan(size, size, t) for t in types]
    iscan_bytes = (n * 2 + 255) // 256 * 256
    qoff = iscan_bytes * len(types)
    arena = np.zeros(qoff + nd * n * 4, np.uint8)
    for k, a in enumerate(iscans):
        arena[k * iscan_bytes:k * iscan_bytes + n * 2] = a.view(np.uint8)
    which = np.arange(nd) % len(types)
    eob = rng.integers(0, n // 4 + 1, nd)
    in_scan = rng.integers(-3, 4, (nd, n), dtype=np.int8).astype(np.int32) * (np.arange(n)[None, :] < eob[:, None])
    last = np.maximum(eob - 1, 0)
    in_scan[np.arange(nd), last] = np.where(eob > 0, np.where(in_scan[np.arange(nd), last] == 0, 1, in_scan[np.arange(nd), last]), 0)
    q = arena[qoff:].view(np.int32).reshape(nd, n)
    for k, a in enumerate(iscans):   # raster[pos] = in_scan[iscan[pos]]
        sel = which == k
        q[sel] = in_scan[sel][:, a.astype(np.int64)]
    d = np.zeros(nd, np.dtype(abi.TXB_COST_DESC_DTYPE))
    d["qcoeff_off"] = qoff + np.arange(nd, dtype=np.uint64) * (n * 4)
    d["iscan_off"] = which * iscan_bytes
    d["table"], d["lambda"], d["eob"], d["tx_type"] = (np.arange(nd) // CANDIDATES) % len(gold.tables), 15000, eob, np.array(types)[which]
    d["txb_skip_ctx"], d["dc_sign_ctx"], d["pred_mode"], d["filter_intra_mode"], d["fast_coeff_est_level"] = 1, 1, T.NEARESTMV, T.FILTER_INTRA_NONE, 1
    return arena, d


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    res = {"width": WIDTH, "height": HEIGHT, "candidates_per_block": CANDIDATES, "repeats": repeats,
           "placement": "tables_in_lds 0: the two SvtHipCoeffCost tables of the launch read through the cache; 1: staged into LDS once per workgroup"}
    try:
        with open(os.path.join(ROOT, "profiles", "intra_predict_4k.json")) as f:
            intra = json.load(f)["gpu"]
        res["intra_predict_descriptors_per_us"] = {k: v["waves_per_workgroup_4"]["descriptors_per_us"] for k, v in intra.items()}
    except (OSError, KeyError, TypeError):
        res["intra_predict_descriptors_per_us"] = None
    lib = timing.open_library()
    if lib is None:
        res["gpu"] = None
        return timing.write_profile("txb_cost_4k.json", res)
    import torch
    gold = T.Golden()
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    rng = np.random.default_rng(5)
    d_tab = device.DeviceBuffer(lib, gold.tables.nbytes)
    d_tab.upload(gold.tables)
    res["gpu"] = {}
    for size in SIZES:
        arena, descs = workload(gold, size, rng)
        nd = len(descs)
        d_arena, d_out, d_dist = device.DeviceBuffer(lib, arena.nbytes), device.DeviceBuffer(lib, 16 * nd), device.DeviceBuffer(lib, 16 * nd)
        d_arena.upload(arena)
        d_dist.fill(1)
        d_desc = device.upload_descriptors(lib, descs)
        entry = {"descriptors": nd, "qcoeff_bytes": int(nd * size * size * 4), "descriptor_bytes": int(descs.nbytes), "mean_eob": round(float(descs["eob"].mean()), 2)}
        for lds in (0, 1):
            launch = lambda: device.check(lib, lib.svt_hip_txb_cost_batch_placed(C.c_void_p(d_arena.ptr), C.c_void_p(d_desc.ptr), C.c_void_p(d_tab.ptr),  # noqa: E731
                                                                                 len(gold.tables), None, C.c_void_p(d_dist.ptr), C.c_void_p(d_out.ptr), nd, size, size,
                                                                                 lds, sp), "svt_hip_txb_cost_batch_placed")
            t = timing.summary(timing.events(torch, stream, repeats, launch))
            t["descriptors_per_us"] = round(nd / (t["median_ms"] * 1e3), 1)
            entry[f"tables_in_lds_{lds}"] = t
        res["gpu"][f"{size}x{size}_16types"] = entry
        del d_desc, d_dist, d_out, d_arena, arena, descs
    timing.write_profile("txb_cost_4k.json", res)


if __name__ == "__main__":
    main()
