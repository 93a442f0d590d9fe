#!/usr/bin/env python3
"""Time the luma palette search and the screen-content decision on the device (a measurement, no threshold) beside the reference's own
search_palette_luma on the CPU:
  search    svt_hip_palette_search_batch, one call per block size over EVERY 8 x 8, 16 x 16, 32 x 32 and 64 x 64 block of a synthetic
            1920 x 1080 text-like picture (a light page, dark glyph strokes, two in-between levels at stroke edges and a few shaded
            panels), 8 bit, dominant_color_step 1, max_itr 50; the blocks of the last row are short (1080 is no multiple of 16).  The
            events span the whole call: the upload of the descriptor array, the kernel.
  classify  svt_hip_sc_classify on the same picture
reference_cpu: search_palette_luma over the same blocks through tests/palette_pin_driver.c (objects fabricated once per size; only the
time inside search_palette_luma counts), single thread, on whatever CPU runs this tool -- its name is recorded.  The rate terms that the
device call also computes (svt_av1_cost_color_map ...) are NOT in the reference's figure.  The device's candidates (their number,
sizes and colours per block) are compared with the reference's before anything is timed, through a digest that the record keeps.
Each half is measured where it can be and merged into the record that is already at the output path.  Writes
profiles/palette_search.json, or the path given as second argument.
    python tools/palette_time.py [repeats] [output]"""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import palette_cases as K  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "palette_search.json")
W, H, SIZES = 1920, 1080, (8, 16, 32, 64)


def picture():
    """(H, W) uint8: text-like"""
    rng = np.random.RandomState(2024)
    img = np.full((H, W), 238, np.int64)
    for y0 in range(0, H, 270):                 # shaded panels
        img[y0 + 200:y0 + 260, 100:1500] = 205
    ink = np.zeros((H, W), bool)
    for line in range(12, H - 12, 18):          # lines of glyph-like strokes, 10 pixels high
        x = 40
        while x < W - 40:
            gw = rng.randint(4, 9)
            for _ in range(rng.randint(1, 4)):
                if rng.rand() < 0.5:
                    ink[line:line + 10, x + rng.randint(0, gw)] = True
                else:
                    ink[line + rng.randint(0, 10), x:x + gw] = True
            x += gw + (2 if rng.rand() < 0.85 else 8)
    img[ink] = 25
    edge = np.zeros((H, W), bool)
    edge[:, 1:] |= ink[:, :-1]
    edge[:, :-1] |= ink[:, 1:]
    edge &= ~ink
    img[edge & (rng.rand(H, W) < 0.5)] = 150
    img[edge & (img == 238) & (rng.rand(H, W) < 0.5)] = 200
    return img.astype(np.uint8)


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def blocks(size):
    """[(x, y, rows, cols)] of every size x size block, in raster order"""
    return [(x, y, min(size, H - y), min(size, W - x)) for y in range(0, H, size) for x in range(0, W, size)]


def checksum(recs):
    """What pin_palette_picture sums per block, from the device's records"""
    sizes, cols = recs["cand"]["palette_size"].astype(np.int64), recs["cand"]["palette_colors"].astype(np.int64)
    weight = (31 * np.arange(K.MAX_CANDS)[:, None] + np.arange(K.MAX_SIZE)[None, :] + 1)[None]
    return ((sizes.sum(axis=1) + (cols * weight).sum(axis=(1, 2))) & 0xFFFFFFFF).astype(np.uint32)


def digest(n_cands, check):
    """Of the candidates of all blocks of one size: the device half, run elsewhere, compares its own with it"""
    return hashlib.sha256(n_cands.astype("<i4").tobytes() + check.astype("<u4").tobytes()).hexdigest()


def reference_cpu(img):
    """The record, or None without oracle/_ref/libsvtref.so or without the reference tree that the pin driver is compiled against"""
    import pyorc
    from support import build_pin, have_reference_tree
    if not pyorc.have_ref() or not have_reference_tree():
        return None
    out = {"cpu": cpu_name(), "note": "single thread, one pass, time inside search_palette_luma only", "search": {}}
    with tempfile.TemporaryDirectory() as tmp:
        pin = build_pin(tmp, K.DRIVER)
        pin.pin_palette_picture.restype = C.c_double
        for size in SIZES:
            n = len(blocks(size))
            n_cands, check = np.zeros(n, np.int32), np.zeros(n, np.uint32)
            sec = pin.pin_palette_picture(img.ctypes.data_as(C.c_void_p), W, H, W, size, size, 1, n_cands.ctypes.data_as(C.c_void_p), check.ctypes.data_as(C.c_void_p))
            out["search"][f"{size}x{size}"] = {"blocks": n, "candidates": int(n_cands.sum()), "ms": round(sec * 1e3, 3), "digest": digest(n_cands, check)}
            print("reference", size, out["search"][f"{size}x{size}"], flush=True)
    out["search"]["all_sizes_ms"] = round(sum(v["ms"] for v in out["search"].values()), 3)
    return out


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    target = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else PROFILE     # read and written at the same place
    try:
        with open(target) as f:
            res = json.load(f)
    except OSError:
        res = {}
    res.update({"repeats": repeats, "picture": [W, H], "bit_depth": 8, "dominant_color_step": 1, "max_itr": 50})
    img = picture()
    cpu = reference_cpu(img)
    if cpu is not None:
        res["reference_cpu"] = cpu
    res.setdefault("reference_cpu", None)
    want = {size: res["reference_cpu"]["search"][f"{size}x{size}"]["digest"] for size in SIZES} if res["reference_cpu"] else {}
    lib = timing.open_library()
    if lib is None:
        res.setdefault("gpu", None)
        return timing.write_profile(target, res)
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    gpu = {"search": {}}

    def up(arr):
        d = device.DeviceBuffer(lib, arr.nbytes)
        d.upload(arr)
        return d
    ysize, ycolor = K.golden_rates()
    d_img, d_rates = up(img), up(np.frombuffer(K.rates_struct(ysize, ycolor), np.uint8))
    ctrls = abi.PaletteCtrls(d_rates.ptr, 1, 8, 50)
    for size in SIZES:
        blks = blocks(size)
        d_rec, d_maps = device.DeviceBuffer(lib, len(blks) * K.RECORD_BYTES), device.DeviceBuffer(lib, len(blks) * K.MAX_CANDS * size * size)
        descs = np.zeros(len(blks), abi.record_dtype(abi.PaletteDesc))
        descs["src"], descs["stride"], descs["width"], descs["height"] = d_img.ptr, W, size, size
        descs["org_x"], descs["org_y"], descs["rows"], descs["cols"] = (np.array([b[i] for b in blks]) for i in range(4))
        descs["record"] = np.uint64(d_rec.ptr) + np.arange(len(blks), dtype=np.uint64) * np.uint64(K.RECORD_BYTES)
        descs["maps"] = np.uint64(d_maps.ptr) + np.arange(len(blks), dtype=np.uint64) * np.uint64(K.MAX_CANDS * size * size)

        def search():
            device.check(lib, lib.svt_hip_palette_search_batch(C.byref(ctrls), descs.ctypes.data_as(C.c_void_p), len(blks), sp), "svt_hip_palette_search_batch")
        search()
        torch.cuda.synchronize()
        recs = d_rec.download(abi.PALETTE_RECORD_DTYPE, (len(blks),))
        if size in want:
            assert digest(recs["n_cands"], checksum(recs)) == want[size], size
        entry = timing.summary(timing.events(torch, stream, repeats, search))
        entry.update(blocks=len(blks), candidates=int(recs["n_cands"].sum()), searched_blocks=int(((recs["colors"] > 1) & (recs["colors"] <= 64)).sum()),
                     checked_against_reference=size in want)
        gpu["search"][f"{size}x{size}"] = entry
        print("search", size, entry, flush=True)
    gpu["search"]["all_sizes_median_ms"] = round(sum(v["median_ms"] for v in gpu["search"].values()), 4)
    d_out = device.DeviceBuffer(lib, C.sizeof(abi.ScClass))

    def classify():
        device.check(lib, lib.svt_hip_sc_classify(d_img.ptr, W, H, W, d_out.ptr, sp), "svt_hip_sc_classify")
    classify()
    torch.cuda.synchronize()
    rec = d_out.download(abi.SC_CLASS_DTYPE, (1,))[0]
    c1, c2, nblk, cls = K.sc_classify(img, W, H)
    assert (int(rec["counts_1"]), int(rec["counts_2"]), int(rec["blocks"]), list(rec["sc_class"])) == (c1, c2, nblk, cls)
    entry = timing.summary(timing.events(torch, stream, repeats, classify))
    entry.update(counts_1=c1, counts_2=c2, blocks=nblk, sc_class=cls)
    gpu["classify"] = entry
    print("classify", entry, flush=True)
    res["gpu"] = gpu
    if res["reference_cpu"]:
        res["reference_ms_over_gpu_ms"] = round(res["reference_cpu"]["search"]["all_sizes_ms"] / gpu["search"]["all_sizes_median_ms"], 1)
    timing.write_profile(target, res)


if __name__ == "__main__":
    main()
