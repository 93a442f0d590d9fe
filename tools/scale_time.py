#!/usr/bin/env python3
"""Time reference scaling on the device (a measurement, no threshold) beside the reference's own C functions on one core of the CPU of
the machine that ran this tool:
  resize    svt_hip_resize_planes, the three planes of a 3840 x 2160 10-bit 4:2:0 picture in one call, at denominators 9 and 16
            (reference: svt_av1_highbd_resize_plane_c per plane)
  superres  svt_hip_superres_upscale_planes, the three planes of a picture of 1920 x 2160 up to 3840 x 2160 (denominator 16), 10 bit, one
            tile column (reference: svt_av1_upscale_normative_rows per plane, through tests/scale_pin_driver.c)
  predict   svt_hip_convolve_scale_batch, 4096 blocks of 16 x 16 and 1024 blocks of 64 x 64 at step 2048 on both axes from one 10-bit plane,
            regular filters, single reference (reference: svt_av1_highbd_convolve_2d_scale_c per block, the ctypes calls included)
Noise pictures.  The device results are compared with the numpy restatement of tests/scale_cases.py, which tests/golden/scale.npz pins to
the reference, before anything is timed.  HIP events after warm-up, median of the repeats.  Each half is measured where it can be (the
super-res reference needs the reference tree for the pin driver) and merged into the record that is already at the output path.
Writes profiles/scale.json, or the path given as second argument.
    python tools/scale_time.py [repeats] [output]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import conv_cases  # noqa: E402
import scale_cases as K  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "scale.json")
W, H, BD = 3840, 2160, 10
RESIZE_DENOMS = (9, 16)
BLOCKS = ((16, 4096), (64, 1024))      # block size, blocks per batch
STEP, PLANE_W, PLANE_H = 2048, 3840, 2160


def resize_cases(denom):
    out = []
    for name, ss in (("y", 0), ("u", 1), ("v", 1)):
        sw, sh = W >> ss, H >> ss
        out.append(K.ResizeCase(f"time_d{denom}_{name}", sw, sh, K.scaled_size(W, denom) >> ss, K.scaled_size(H, denom) >> ss, BD, 1, "noise", sw, sw))
    return out


def superres_cases():
    out = []
    for name, ss in (("y", 0), ("u", 1), ("v", 1)):
        mi_cols = 2 * ((W // 2 + 7) >> 3)
        out.append(K.SuperresCase(f"time_sr_{name}", W, 16, ss, (0, mi_cols), BD, 1, H >> ss, ((mi_cols * 4) >> ss) + 2 * K.SR_MARGIN, W >> ss))
    return out


def block_positions(size, count):
    """Top-left corners of `count` blocks of one size whose taps stay inside the plane, spread over it"""
    span = 2 * size + 8
    rng = np.random.RandomState(size)
    return np.stack([rng.randint(8, PLANE_W - span, count), rng.randint(8, PLANE_H - span, count)], axis=1)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, round((time.perf_counter() - t0) * 1e3, 3)


def predict_plane():
    return K.make_samples(11, PLANE_H, PLANE_W, BD, 1, "noise")


def reference_predict(ref, plane, size, at):
    tab = K.sc_table(K.TABLES8[0], 8)
    fp = conv_cases.InterpFilterParams(tab.ctypes.data, 8, 16, 0)
    r0, r1 = conv_cases.conv_rounds(BD)
    cp = abi.ConvolveParams()
    cp.round_0, cp.round_1 = r0, r1
    dst = np.zeros((len(at), size, size), np.uint16)
    for i, (x, y) in enumerate(at):
        ref.svt_av1_highbd_convolve_2d_scale_c(C.c_void_p(plane.ctypes.data + (int(y) * PLANE_W + int(x)) * 2), PLANE_W, C.c_void_p(dst[i].ctypes.data), size,
                                               size, size, C.byref(fp), C.byref(fp), 37, STEP, 29, STEP, C.byref(cp), BD)
    return dst


def reference_cpu():
    """Milliseconds of the reference's functions, single thread, one run each; None without oracle/_ref/libsvtref.so"""
    import pyorc
    import support
    if not pyorc.have_ref():
        return None
    ref = pyorc.ref()
    out = {"note": "single thread, one run each, on the CPU of the machine that ran this tool", "resize": {}, "predict": {}}
    for denom in RESIZE_DENOMS:
        planes = [(c, K.resize_source(c)) for c in resize_cases(denom)]
        _, ms = clock(lambda: [K.reference_resize(ref, c, src) for c, src in planes])
        out["resize"][f"denominator_{denom}"] = {"ms_three_planes": ms}
        print("reference resize", denom, ms, flush=True)
    plane = predict_plane()
    for size, count in BLOCKS:
        at = block_positions(size, count)
        _, ms = clock(lambda: reference_predict(ref, plane, size, at))
        out["predict"][f"{size}x{size}_x{count}"] = {"ms": ms}
        print("reference predict", size, count, ms, flush=True)
    if support.have_reference_tree():
        with tempfile.TemporaryDirectory() as tmp:
            pin = K.build_pin(tmp)
            planes = [(c, K.superres_source(c)) for c in superres_cases()]
            _, ms = clock(lambda: [K.reference_superres(pin, c, src) for c, src in planes])      # with its copy of the source for the restore check
        out["superres"] = {"ms_three_planes": ms}
        print("reference superres", ms, flush=True)
    return out


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    target = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else PROFILE     # read and written at the same place
    try:
        with open(target) as f:
            res = json.load(f)
    except OSError:
        res = {}
    res.update({"repeats": repeats, "picture": [W, H, BD], "step": STEP})
    cpu = reference_cpu() if "--no-reference" not in sys.argv else None
    if cpu is not None:
        kept = res.get("reference_cpu") or {}
        res["reference_cpu"] = {**kept, **cpu}      # a half measured elsewhere (super-res needs the reference tree) stays
    res.setdefault("reference_cpu", None)
    lib = timing.open_library()
    if lib is None:
        res.setdefault("gpu", None)
        return timing.write_profile(target, res)
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    gpu, keep = {"resize": {}, "predict": {}}, []

    def up(arr):
        d = device.DeviceBuffer(lib, arr.nbytes)
        d.upload(arr)
        keep.append(d)
        return d

    def timed(call, name):
        def launch():
            device.check(lib, call(), name)
        launch()
        torch.cuda.synchronize()
        return lambda: timing.summary(timing.events(torch, stream, repeats, launch))

    for denom in RESIZE_DENOMS:
        cases = resize_cases(denom)
        srcs = [up(K.resize_source(c)) for c in cases]
        dsts = [device.DeviceBuffer(lib, c.dw * c.dh * 2) for c in cases]
        jobs = (abi.ResizePlane * 3)(*[abi.ResizePlane(s.ptr, d.ptr, c.sstride, c.dw, c.sw, c.sh, c.dw, c.dh, 1, BD) for s, d, c in zip(srcs, dsts, cases)])
        ws_bytes = lib.svt_hip_resize_workspace_bytes(jobs, 3)
        ws = device.DeviceBuffer(lib, max(ws_bytes, 256))
        measure = timed(lambda: lib.svt_hip_resize_planes(jobs, 3, ws.ptr, ws_bytes, sp), "svt_hip_resize_planes")
        for d, c in zip(dsts, cases):
            assert np.array_equal(d.download(np.uint16, (c.dh, c.dw)), K.restate_resize(c)), c.name
        entry = measure()
        entry.update(checked_against_restatement=True, workspace_bytes=int(ws_bytes), planes=[[c.sw, c.sh, c.dw, c.dh] for c in cases])
        gpu["resize"][f"denominator_{denom}"] = entry
        print("resize", denom, entry, flush=True)
    cases = superres_cases()
    srcs = [up(K.superres_source(c)) for c in cases]
    dsts = [device.DeviceBuffer(lib, c.rows * c.dstride * 2) for c in cases]
    jobs = (abi.SuperresPlane * 3)()
    for j, s, d, c in zip(jobs, srcs, dsts, cases):
        j.src, j.dst, j.src_stride, j.dst_stride, j.rows = s.ptr + K.SR_MARGIN * 2, d.ptr, c.sstride, c.dstride, c.rows
        j.frame_width, j.superres_upscaled_width, j.superres_denominator, j.sub_x = K.sr_frame_width(c), c.up_width, c.denom, c.sub_x
        j.is_16bit, j.bit_depth, j.tile_cols = 1, BD, 1
        j.tile_col_start_mi[0], j.tile_col_start_mi[1] = c.starts
    measure = timed(lambda: lib.svt_hip_superres_upscale_planes(jobs, 3, sp), "svt_hip_superres_upscale_planes")
    for d, c in zip(dsts, cases):
        assert np.array_equal(d.download(np.uint16, (c.rows, c.dstride)), K.restate_superres(c)), c.name
    gpu["superres"] = dict(measure(), checked_against_restatement=True, planes=[[K.sr_widths(c)[0], K.sr_widths(c)[1], c.rows] for c in cases])
    print("superres", gpu["superres"], flush=True)
    plane = predict_plane()
    d_plane, d_tab = up(plane), up(K.sc_table(K.TABLES8[0], 8))
    r0, r1 = conv_cases.conv_rounds(BD)
    for size, count in BLOCKS:
        at = block_positions(size, count)
        d_dst = device.DeviceBuffer(lib, count * size * size * 2)
        descs = np.zeros(count, abi.CONVOLVE_SCALE_DESC_DTYPE)
        descs["src"] = d_plane.ptr + (at[:, 1].astype(np.uint64) * PLANE_W + at[:, 0].astype(np.uint64)) * 2
        descs["dst"] = d_dst.ptr + np.arange(count, dtype=np.uint64) * (size * size * 2)
        descs["src_stride"], descs["dst_stride"], descs["w"], descs["h"] = PLANE_W, size, size, size
        descs["filter_x"] = descs["filter_y"] = d_tab.ptr
        descs["subpel_x_qn"], descs["x_step_qn"], descs["subpel_y_qn"], descs["y_step_qn"] = 37, STEP, 29, STEP
        descs["taps_x"] = descs["taps_y"] = 8
        descs["round_0"], descs["round_1"], descs["bit_depth"], descs["is_16bit"] = r0, r1, BD, 1
        d_desc = up(descs)
        measure = timed(lambda: lib.svt_hip_convolve_scale_batch(d_desc.ptr, count, sp), "svt_hip_convolve_scale_batch")
        got = d_dst.download(np.uint16, (count, size, size))
        for i in range(0, count, max(1, count // 64)):          # every 64th block against the restatement
            c = K.ScaleCase("t", size, size, STEP, STEP, 37, 29, K.TABLES8[0], K.TABLES8[0], (8, 8), 0, BD, 8, 8, 0)
            x, y = at[i]
            window = plane[y - K.SC_MARGIN:y - K.SC_MARGIN + K.sc_extent(c)[0], x - K.SC_MARGIN:x - K.SC_MARGIN + K.sc_extent(c)[1]]
            assert np.array_equal(got[i], K.restate_scaled(c, src=window)), (size, i)
        gpu["predict"][f"{size}x{size}_x{count}"] = dict(measure(), checked_against_restatement=True)
        print("predict", size, count, gpu["predict"][f"{size}x{size}_x{count}"], flush=True)
    res["gpu"] = gpu
    timing.write_profile(target, res)


if __name__ == "__main__":
    main()
