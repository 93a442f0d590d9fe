#!/usr/bin/env python3
"""Time svt_hip_blend_batch and svt_hip_compound_mask_search_batch on whole 4K pictures (HIP events around the library's
launches, inputs resident before the timed region, warm-up, median of the repeats):
  (a) the masked-compound (wedge) blend of every 16x16 luma block and its two 8x8 chroma blocks of a 10-bit picture in one call;
  (b) the mask search over every 16x16 and over every 32x32 block of an 8-bit picture.
Beside each median: its algorithmic bytes / time, and the reference's C functions (oracle/_ref) on the same inputs on 16 host
processes (the per-call cost of ctypes is measured and reported apart).  Writes profiles/r05_inter_blend_4k.json.  Needs the GPU.
    python tools/blend_time.py [repeats]"""
import ctypes as C
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import blend_cases as B  # noqa: E402
import conv_cases as K  # noqa: E402
import pyorc  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

W, H, WORKERS = 3840, 2160, 16


def blend_inputs():
    """ConvBufType planes of two compound-1 predictions (Y, U, V) of a 10-bit picture and a wedge (index, sign) per 16x16 block."""
    rng = np.random.default_rng(31)
    planes = [[B.conv_buf_block(rng, w, h, 10, False) for _ in range(2)] for w, h in ((W, H), (W // 2, H // 2), (W // 2, H // 2))]
    return planes, rng.integers(0, 32, (H // 16, W // 16))


def search_inputs():
    rng = np.random.default_rng(32)
    yy, xx = np.mgrid[0:H, 0:W]
    src = 128 + 70 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + rng.integers(-5, 6, (H, W))
    preds = [src + np.where(np.sin(xx / (9.0 + 2 * j) + yy / 13.0) > 0.2, rng.integers(-90, 91, (H, W)), rng.integers(-3, 4, (H, W))) for j in range(2)]
    return [np.clip(np.rint(v), 0, 255).astype(np.uint8) for v in [src] + preds]


# ---- the reference on host processes (forked before the GPU is touched) -------------------------------------------------------
def _cpu_blend(rows):
    ref, gold = pyorc.ref(), np.load(B.GOLD)
    planes, wedge = blend_inputs()
    masks = np.ascontiguousarray(gold["wedge_16x16"])
    fn = B.RefBlend(ref).d16_hb
    r0, r1 = K.conv_rounds_compound(10)
    cp = abi.ConvolveParams(round_0=r0, round_1=r1, is_compound=1)
    cpp = C.addressof(cp)
    dst = [np.zeros(p[0].shape, np.uint16) for p in planes]
    ptr = [(d.ctypes.data, p[0].ctypes.data, p[1].ctypes.data, p[0].shape[1]) for d, p in zip(dst, planes)]
    mptr = [[masks.ctypes.data + 256 * int(v) for v in row] for row in wedge]
    t0 = time.perf_counter()
    for by in rows:
        for bx in range(W // 16):
            m = mptr[by][bx]
            for (d, a, b, s), size, sub in zip(ptr, (16, 8, 8), (0, 1, 1)):
                o = (by * size * s + bx * size) * 2
                fn(d + o, s, a + o, s, b + o, s, m, 16, size, size, sub, sub, cpp, 10)
    return time.perf_counter() - t0, 3 * len(rows) * (W // 16)


def _cpu_search(args):
    """The calls of blend_cases.RefSearch.run on preallocated buffers: nothing but the reference's functions inside the timed loop.
    The predictions are tiled beforehand: the reference keeps pred0 / pred1 of a block contiguous."""
    size, rows = args
    gold = np.load(B.GOLD)
    o = B.RefSearch(pyorc.ref(), gold)
    src, p0, p1 = search_inputs()
    N, nbx = size * size, W // size
    masks = np.ascontiguousarray(gold[f"wedge_{size}x{size}"])
    mp0 = [masks.ctypes.data + 2 * i * N for i in range(abi.WEDGE_TYPES)]
    tiles = [[np.ascontiguousarray(p[by * size:(by + 1) * size].reshape(size, nbx, size).swapaxes(0, 1)) for by in rows] for p in (p0, p1)]
    keep = [np.zeros(N, np.int16) for _ in range(4)] + [np.zeros(N, np.uint8)]   # the pointers below stay valid while these live
    res0, res1, d10, ds, seg = (a.ctypes.data for a in keep)
    sp = src.ctypes.data
    sse_sum = 0
    t0 = time.perf_counter()
    for k, by in enumerate(rows):
        a0, a1 = tiles[0][k].ctypes.data, tiles[1][k].ctypes.data
        for bx in range(nbx):
            s, a, b = sp + by * size * W + bx * size, a0 + bx * N, a1 + bx * N
            o.sad8(a, size, b, size, size, size)
            o.sub8(size, size, res1, size, s, W, b, size)
            o.sub8(size, size, d10, size, b, size, a, size)
            o.sub8(size, size, res0, size, s, W, a, size)
            limit = (o.sumsq(res0, N) - o.sumsq(res1, N)) * 32
            o.delta(ds, res0, res1, N)
            for m in mp0:
                sse_sum += o.sse(res1, d10, m + N * o.sign(ds, m, N, limit), N)
            for t in (0, 1):
                o.dw8(seg, t, a, size, b, size, size, size)
                sse_sum += o.sse(res1, d10, seg, N)
    return time.perf_counter() - t0, 43 * len(rows) * nbx   # 43 reference calls per block


def _cpu_call_overhead(n):
    """Seconds per ctypes call: a reference function of the search on one sample."""
    sse = B.RefSearch(pyorc.ref(), {}).sse
    keep = (np.zeros(1, np.int16), np.zeros(1, np.uint8))
    r, m = keep[0].ctypes.data, keep[1].ctypes.data
    t0 = time.perf_counter()
    for _ in range(n):
        sse(r, r, m, 1)
    return (time.perf_counter() - t0) / n


def cpu_legs():
    """{leg: ms} of the reference over the whole picture on WORKERS processes (wall = the slowest worker)."""
    if not pyorc.have_ref():
        return None
    out = {"workers": WORKERS, "ctypes_us_per_call": round(_cpu_call_overhead(200000) * 1e6, 3)}
    with mp.get_context("fork").Pool(WORKERS) as pool:
        for leg, fn, jobs in (("blend_4k10", _cpu_blend, [list(range(k, H // 16, WORKERS)) for k in range(WORKERS)]),
                              ("search_16x16_4k8", _cpu_search, [(16, list(range(k, H // 16, WORKERS))) for k in range(WORKERS)]),
                              ("search_32x32_4k8", _cpu_search, [(32, list(range(k, H // 32, WORKERS))) for k in range(WORKERS)])):
            res = pool.map_async(fn, jobs).get(timeout=600)   # a worker that died must not hang the tool
            wall, calls = max(t for t, _ in res), max(n for _, n in res)
            out[leg] = {"ms": round(wall * 1e3, 2), "ms_without_ctypes_call_cost": round(max(0.0, wall - calls * out["ctypes_us_per_call"] * 1e-6) * 1e3, 2)}
    return out


# ---- the GPU ------------------------------------------------------------------------------------------------------------------
def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    assert repeats >= 20
    cpu = cpu_legs()   # before anything touches the GPU: the workers are forked
    lib = timing.open_library()
    assert lib is not None, abi.load().svt_hip_last_error().decode()
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    gold = np.load(B.GOLD)
    res = {"width": W, "height": H, "repeats": repeats, "hbm_roof_TBps": [5.6, 6.5], "cpu_reference": cpu, "legs": {}}

    def up(a):
        d = device.DeviceBuffer(lib, a.nbytes)
        d.upload(a)
        return d

    def leg(name, ms, n, nbytes, extra=None):
        res["legs"][name] = {"descriptors": n, **timing.summary(ms), "algorithmic_bytes": nbytes,
                             "TBps": round(nbytes / (statistics.median(ms) * 1e-3) / 1e12, 3), **(extra or {})}

    # (a) blend
    planes, wedge = blend_inputs()
    d_planes = [[up(p) for p in pl] for pl in planes]
    d_dst = [device.DeviceBuffer(lib, pl[0].nbytes) for pl in planes]
    d_masks = up(gold["wedge_16x16"])
    r0, r1 = K.conv_rounds_compound(10)
    descs = []
    for by in range(H // 16):
        for bx in range(W // 16):
            m = d_masks.ptr + int(wedge[by, bx]) * 256
            for p, (size, sub) in enumerate(((16, 0), (8, 1), (8, 1))):
                s = planes[p][0].shape[1]
                o = (by * size * s + bx * size) * 2
                descs.append(abi.BlendDesc(d_planes[p][0].ptr + o, d_planes[p][1].ptr + o, d_dst[p].ptr + o, m, s, s, s, 16, size, size,
                                           abi.BLEND_D16, sub, sub, 0, r0, r1, 10, 1, 0))
    d_desc = device.upload_descriptors(lib, descs)
    n_luma, n_chroma = W * H, 2 * (W // 2) * (H // 2)
    leg("blend_4k10", timing.events(torch, stream, repeats, lambda: device.check(lib, lib.svt_hip_blend_batch(d_desc.ptr, len(descs), sp), "blend")),
        len(descs), n_luma * (4 + 1 + 2) + n_chroma * (4 + 4 + 2),
        {"bytes_note": "luma 4 N in + N mask + 2 N out, chroma 4 n in + 4 n mask + 2 n out; the masks come from an 8 KiB table"})
    got = d_dst[0].download(np.uint16, planes[0][0].shape)
    del d_planes, d_desc, descs

    # (b) search
    pics = search_inputs()
    d_pics = [up(p) for p in pics]
    for size in (16, 32):
        d_wm = up(gold[f"wedge_{size}x{size}"])
        descs = [abi.MaskSearchDesc(*(d.ptr + y * W + x for d in d_pics), d_wm.ptr, W, W, W, size, size, 8, 0)
                 for y in range(0, H - size + 1, size) for x in range(0, W - size + 1, size)]
        d_desc = device.upload_descriptors(lib, descs)
        d_res = device.DeviceBuffer(lib, C.sizeof(abi.MaskSearchResult) * len(descs))
        n = len(descs) * size * size
        leg(f"search_{size}x{size}_4k8",
            timing.events(torch, stream, repeats, lambda: device.check(lib, lib.svt_hip_compound_mask_search_batch(d_desc.ptr, d_res.ptr, len(descs), sp), "search")),
            len(descs), 3 * n + C.sizeof(abi.MaskSearchResult) * len(descs),
            {"bytes_note": "3 N samples in + one 168-byte record out per block; the 32 N mask bytes per block come from one table per size "
                           f"({32 * size * size} bytes, cache-resident)", "mask_bytes_read": 32 * n})
    timing.write_profile("r05_inter_blend_4k.json", res)
    assert got.any()


if __name__ == "__main__":
    main()
