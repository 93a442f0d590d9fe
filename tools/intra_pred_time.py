#!/usr/bin/env python3
"""Time svt_hip_intra_predict_batch on a 4K picture's worth of mode-decision work (one measurement, no threshold), edges read
straight from the picture, one dst per descriptor:
  8x8_13modes_8bit     every 8 x 8 luma block x the 13 modes
  4x4_13modes_8bit     every 4 x 4 block x the 13 modes
  32x32_61variants_10bit   every 32 x 32 block x the 61 mode variants (5 non-directional + 8 directional x 7 deltas)
Each with 4, 2 and 1 descriptors (wavefronts) per workgroup through svt_hip_intra_predict_batch_packed: 4 is what
svt_hip_intra_predict_batch uses, 1 is plain wave-per-descriptor.  HIP events around the launch after warm-up, median of the repeats.
Algorithmic bytes = samples written (d * w * h) + edge samples read; the 64-byte descriptors are listed apart.  Writes
profiles/intra_predict_4k.json; without a device the GPU half is recorded as null.
    python tools/intra_pred_time.py [repeats]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import intra_pred_cases as P  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

WIDTH, HEIGHT = 3840, 2160
ROOF_TBPS = (5.6, 6.5)   # practical HBM roof of DESIGN section 10
WORKLOADS = [("8x8_13modes_8bit", 8, [(m, 0) for m in range(abi.INTRA_MODES)], 8, 0),
             ("4x4_13modes_8bit", 4, [(m, 0) for m in range(abi.INTRA_MODES)], 8, 0),
             ("32x32_61variants_10bit", 32, P.MODE_VARIANTS, 10, 1)]


def descriptors(size, variants, bd, is16, plane_ptr, stride, dst_ptr):
    """(record array, algorithmic bytes): one descriptor per (block, variant), blocks in raster order, variants adjacent."""
    px = 2 if is16 else 1
    cols, rows, nv = WIDTH // size, HEIGHT // size, len(variants)
    by, bx, v = np.meshgrid(np.arange(rows), np.arange(cols), np.arange(nv), indexing="ij")
    x, y = (bx * size).reshape(-1), (by * size).reshape(-1)
    d = np.zeros(x.size, P.DESC_DTYPE)
    d["above"] = plane_ptr + ((y - 1) * stride + x) * px
    d["left"] = plane_ptr + (y * stride + x - 1) * px
    d["dst"] = dst_ptr + np.arange(x.size, dtype=np.uint64) * (size * size * px)
    d["left_stride"], d["dst_stride"], d["w"], d["h"] = stride, size, size, size
    d["mode"], d["angle_delta"] = np.array([m for m, _ in variants])[v.reshape(-1)], np.array([a for _, a in variants])[v.reshape(-1)]
    d["filter_intra_mode"], d["is_16bit"], d["bit_depth"] = abi.FILTER_INTRA_NONE, is16, bd
    d["n_top_px"], d["n_left_px"] = np.where(y > 0, size, 0), np.where(x > 0, size, 0)
    d["n_topright_px"] = np.where((y > 0) & (x + 2 * size <= WIDTH), size, 0)
    d["n_bottomleft_px"] = np.where((x > 0) & (y + 2 * size <= HEIGHT), size, 0)
    d["above"][y == 0], d["left"][x == 0] = 0, 0
    edges = d["n_top_px"].astype(np.int64) + d["n_topright_px"] + d["n_left_px"] + d["n_bottomleft_px"] + 1
    return d, int(x.size * size * size * px + edges.sum() * px)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    res = {"width": WIDTH, "height": HEIGHT, "repeats": repeats, "roof_TBps": list(ROOF_TBPS),
           "packing": "waves_per_workgroup descriptors share one workgroup, one wavefront each; 4 is svt_hip_intra_predict_batch, 1 is wave-per-descriptor"}
    lib = timing.open_library()
    if lib is None:
        res["gpu"] = None
        return timing.write_profile("intra_predict_4k.json", res)
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    stride = WIDTH + 64
    rng = np.random.default_rng(3)
    res["gpu"] = {}
    for name, size, variants, bd, is16 in WORKLOADS:
        plane = rng.integers(0, 1 << bd, (HEIGHT + 2, stride)).astype(P.sample_type(is16))
        d_plane = device.DeviceBuffer(lib, plane.nbytes)
        d_plane.upload(plane)
        px = 2 if is16 else 1
        n = (WIDTH // size) * (HEIGHT // size) * len(variants)
        d_dst = device.DeviceBuffer(lib, n * size * size * px)
        descs, algo_bytes = descriptors(size, variants, bd, is16, d_plane.ptr + (stride + 32) * px, stride, d_dst.ptr)
        d_desc = device.upload_descriptors(lib, descs)
        entry = {"descriptors": n, "algorithmic_bytes": algo_bytes, "descriptor_bytes": int(descs.nbytes)}
        for waves in (4, 2, 1):
            launch = lambda: device.check(lib, lib.svt_hip_intra_predict_batch_packed(C.c_void_p(d_desc.ptr), n, waves, sp), "intra_predict")  # noqa: E731
            t = timing.summary(timing.events(torch, stream, repeats, launch))
            t["fraction_of_roof"] = [round(algo_bytes / (t["median_ms"] * 1e-3) / (r * 1e12), 4) for r in ROOF_TBPS]
            t["descriptors_per_us"] = round(n / (t["median_ms"] * 1e3), 1)
            entry[f"waves_per_workgroup_{waves}"] = t
        res["gpu"][name] = entry
        del d_desc, d_dst, d_plane
    timing.write_profile("intra_predict_4k.json", res)


if __name__ == "__main__":
    main()
