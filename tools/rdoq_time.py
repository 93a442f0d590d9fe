#!/usr/bin/env python3
"""Time svt_hip_rdoq_batch on a 4K picture's worth of transform-type search (a measurement, no threshold): every luma block of a
3840 x 2160 picture x 4 candidate transform types, for each of the 14 transform sizes without a 64-point side (those run the same
kernels on their retained 32-wide blocks).  The residuals are random walks of three amplitudes, the quantiser tables those of base
qindex 40 (tests/golden/rdoq.npz), so the blocks cover eob 0 up to dense; the mix is recorded with the times.  Per size:
  stage    svt_hip_rdoq_batch_mapped with every mapping the size has: 0 a lane group per block, update_coeff_simple by its walking lane
           in scan order; 1 a lane group per block, one anti-diagonal per round; 2 one lane per block (up to 128 retained coefficients).
           The mappings ALTERNATE within each repeat, each launch behind an untimed svt_hip_txfm_quant_batch that restores the arrays
           it updates in place; "fastest" names the smallest median and says whether its range is clear of the next one's;
  chain    quant (FWD + QUANT_FP + SATD) -> [rdoq] -> quant (INV only) -> distortion -> txb_cost on one stream, with and without the stage;
  reference_cpu   svt_aom_quantize_inv_quantize (first quantiser included) through tests/rdoq_pin_driver.c on a sample of the square
           sizes' blocks, single thread: a CPU-only number from whatever machine built the reference tree, not from the GPU machine.
HIP events after warm-up, median of the repeats.  Each half is measured where it can be (a device / the reference tree) and merged
into the record that is already at the output path.  Writes profiles/rdoq_4k.json, or the path given as second argument.
    python tools/rdoq_time.py [repeats] [output]"""
import collections
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

import rdoq_cases as R  # noqa: E402
import tx_cases  # noqa: E402
import txb_cost_cases as T  # noqa: E402
from benchlib import timing  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

WIDTH, HEIGHT, CANDIDATES = 3840, 2160, 4
SIZES = ((4, 4), (8, 8), (16, 16), (32, 32), (4, 8), (8, 4), (4, 16), (16, 4), (8, 16), (16, 8), (8, 32), (32, 8), (16, 32), (32, 16))
CPU_SIZES = SIZES[:4]
MAPPINGS = {0: "group_scan_order", 1: "group_rounds", 2: "lane_per_block"}
SIGMAS = (1.5, 5.0, 16.0)
CPU_SAMPLE = 3000
PROFILE = os.path.join(ROOT, "profiles", "rdoq_4k.json")


def case_of(w, h, tx_type, k):
    return R.Case("time", w, h, tx_type, plane=0, is_inter=k % 2, bd=8, table=0, qm=0, lam=20000, skip_ctx=k % 13, dc_sign_ctx=k % 3, perform=1, fast=0,
                  sharp=0, eob_th=85, eob_fast_th=30, satd_factor=255, early_exit_th=0, sq_size=16, fp_q=1, eob=0, dc="", recipe="", pic_bd=8)


def residuals(w, h, rng, nd):
    """A two-dimensional random walk per block (energy falls with frequency, as a prediction residual's does), scaled to one of SIGMAS"""
    sigma = np.array(SIGMAS, np.float32)[np.arange(nd) % len(SIGMAS)]
    walk = np.cumsum(np.cumsum(rng.standard_normal((nd, h, w), dtype=np.float32), axis=1), axis=2) / np.float32(np.sqrt(w * h))
    return np.clip(np.rint(walk * sigma[:, None, None]), -255, 255).astype(np.int16).reshape(nd, w * h)


def workload(gold, w, h, rng):
    """(arena image, forward descriptors, INV-only descriptors, RDOQ descriptors, rate descriptors)"""
    n = w * h
    nd = (WIDTH // w) * (HEIGHT // h) * CANDIDATES
    types = T.size_types(w, h)
    qt = R.quant_dict(gold.quant[0][0])
    iscan_bytes = (n * 2 + 255) // 256 * 256
    per = 16 * n                              # residual 2n, coeff / qcoeff / dqcoeff 4n each, pred n, recon n
    base = iscan_bytes * len(types)
    arena = np.zeros(base + nd * per, np.uint8)
    for k, t in enumerate(types):
        arena[k * iscan_bytes:k * iscan_bytes + n * 2] = gold.iscan(w, h, t).view(np.uint8)
    blk = arena[base:].reshape(nd, per)
    blk[:, :2 * n] = residuals(w, h, rng, nd).view(np.uint8)
    blk[:, 14 * n:15 * n] = 128
    which = np.arange(nd) % len(types)
    off = base + np.arange(nd, dtype=np.uint64) * per
    fwd = np.zeros(nd, abi.TXFM_DESC_DTYPE)
    fwd["residual_off"], fwd["coeff_off"], fwd["qcoeff_off"], fwd["dqcoeff_off"] = off, off + 2 * n, off + 6 * n, off + 10 * n
    fwd["pred_off"], fwd["recon_off"], fwd["iscan_off"], fwd["qm_off"], fwd["iqm_off"] = off + 14 * n, off + 15 * n, which * iscan_bytes, abi.NO_OFFSET, abi.NO_OFFSET
    fwd["residual_stride"] = fwd["pred_stride"] = fwd["recon_stride"] = w
    for f, src in (("zbin", "zbin"), ("round", "round_fp"), ("quant", "quant_fp"), ("quant_shift", "qshift"), ("dequant", "dequant")):
        fwd[f] = qt[src][:2]
    fwd["tx_type"], fwd["bit_depth"], fwd["quant_mode"], fwd["log_scale"] = np.array(types)[which], 8, abi.QUANT_FP, T.tx_scale(w, h)
    fwd["flags"] = abi.TX_FWD | abi.TX_SATD
    inv = fwd.copy()
    inv["quant_mode"], inv["flags"] = abi.QUANT_NONE, abi.TX_INV
    rd = np.zeros(nd, abi.RDOQ_DESC_DTYPE)
    c = case_of(w, h, 0, 0)
    rd["table"], rd["lambda"], rd["eob_th"], rd["eob_fast_th"], rd["satd_factor"], rd["dequant_shift"], rd["flags"] = 0, c.lam, c.eob_th, c.eob_fast_th, 255, 3, abi.RDOQ_PERFORM
    for f, src in (("zbin", "zbin"), ("round", "round"), ("quant", "quant"), ("quant_shift", "qshift")):
        rd[f] = qt[src][:2]
    rd["is_inter"], rd["txb_skip_ctx"], rd["dc_sign_ctx"] = np.arange(nd) % 2, np.arange(nd) % 13, np.arange(nd) % 3
    cost = np.zeros(nd, abi.TXB_COST_DESC_DTYPE)
    cost["qcoeff_off"], cost["iscan_off"], cost["lambda"], cost["tx_type"] = fwd["qcoeff_off"], fwd["iscan_off"], c.lam, fwd["tx_type"]
    cost["txb_skip_ctx"], cost["dc_sign_ctx"], cost["pred_mode"], cost["filter_intra_mode"], cost["fast_coeff_est_level"] = rd["txb_skip_ctx"], rd["dc_sign_ctx"], T.NEARESTMV, T.FILTER_INTRA_NONE, 1
    return arena, fwd, inv, rd, cost


def reference_cpu(gold):
    """Seconds per block of the reference's own function on the first CPU_SAMPLE blocks of each size's workload, or None"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from support import have_reference_tree
    import pyorc
    if not (have_reference_tree() and pyorc.have_ref()):
        return None
    orc, out = pyorc.oracle(), {}
    with tempfile.TemporaryDirectory() as tmp:
        pin = R.Pin(pyorc.ref(), tmp)
        for w, h in CPU_SIZES:
            n, types = w * h, T.size_types(w, h)
            res = residuals(w, h, np.random.default_rng(5 + w * 100 + h), CPU_SAMPLE)   # the first blocks of workload(): the generator fills row by row
            coeffs = []
            for k, r in enumerate(res):
                co = np.zeros(n, np.int32)
                orc.orc_fwd_txfm2d(tx_cases.P(np.ascontiguousarray(r)), tx_cases.P(co), C.c_uint32(w), w, h, types[k % len(types)], 8, 0)
                coeffs.append(co)
            cases = [case_of(w, h, types[k % len(types)], k) for k in range(len(res))]
            pin.run_many(cases[:50], coeffs[:50])
            t0 = time.perf_counter()
            eobs = pin.run_many(cases, coeffs)[2]
            dt = time.perf_counter() - t0
            out[f"{w}x{h}"] = {"blocks": len(res), "us_per_block": round(dt / len(res) * 1e6, 2), "mean_eob": round(float(np.mean(eobs)), 2),
                                     "includes": "the first FP quantiser; one call into C for all blocks"}
    out["note"] = "CPU-only, single thread, measured on the machine that built the reference tree: not the GPU machine's host"
    return out


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    target = sys.argv[2] if len(sys.argv) > 2 else PROFILE
    try:
        with open(target) as f:
            res = json.load(f)
    except OSError:
        res = {}
    res.update({"width": WIDTH, "height": HEIGHT, "candidates_per_block": CANDIDATES, "repeats": repeats, "residual_sigmas": list(SIGMAS),
                "mapping": "stage_<name>: svt_hip_rdoq_batch_mapped with mapping " + ", ".join(f"{k} = {v}" for k, v in MAPPINGS.items()) +
                           "; alternating within each repeat"})
    gold = R.Golden()
    cpu = reference_cpu(gold)
    if cpu is not None:
        res["reference_cpu"] = cpu
    res.setdefault("reference_cpu", None)
    lib = timing.open_library()
    if lib is None:
        res.setdefault("gpu", None)
        return timing.write_profile(target, res)
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    V = C.c_void_p
    d_tab = device.DeviceBuffer(lib, gold.tables.nbytes)
    d_tab.upload(gold.tables)
    nt = len(gold.tables)
    res["gpu"] = {}
    for w, h in SIZES:
        arena, fwd, inv, rd, cost = workload(gold, w, h, np.random.default_rng(5 + w * 100 + h))
        nd = len(fwd)
        d_arena = device.DeviceBuffer(lib, arena.nbytes)
        d_arena.upload(arena)
        d_fwd, d_inv, d_rd, d_cost = (device.upload_descriptors(lib, x) for x in (fwd, inv, rd, cost))
        d_res, d_res_inv, d_out = device.DeviceBuffer(lib, 16 * nd), device.DeviceBuffer(lib, 16 * nd), device.DeviceBuffer(lib, 4 * nd)
        d_dist, d_bits = device.DeviceBuffer(lib, 16 * nd), device.DeviceBuffer(lib, 16 * nd)

        def quant():
            device.check(lib, lib.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_res.ptr), nd, w, h, sp), "svt_hip_txfm_quant_batch")

        def rdoq(mapping):
            device.check(lib, lib.svt_hip_rdoq_batch_mapped(V(d_arena.ptr), V(d_fwd.ptr), V(d_rd.ptr), V(d_tab.ptr), nt, V(d_res.ptr), V(d_out.ptr), nd, w, h,
                                                            mapping, sp), "svt_hip_rdoq_batch_mapped")

        def shipped():
            device.check(lib, lib.svt_hip_rdoq_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_rd.ptr), V(d_tab.ptr), nt, V(d_res.ptr), V(d_out.ptr), nd, w, h, sp),
                         "svt_hip_rdoq_batch")

        def tail():
            device.check(lib, lib.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_inv.ptr), V(d_res_inv.ptr), nd, w, h, sp), "svt_hip_txfm_quant_batch (INV)")
            device.check(lib, lib.svt_hip_txfm_distortion_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_dist.ptr), nd, w, h, sp), "svt_hip_txfm_distortion_batch")
            device.check(lib, lib.svt_hip_txb_cost_batch(V(d_arena.ptr), V(d_cost.ptr), V(d_tab.ptr), nt, V(d_res.ptr), V(d_dist.ptr), V(d_bits.ptr), nd, w, h, sp),
                         "svt_hip_txb_cost_batch")

        def timed(before, whats):
            """median of each of `whats` alone, taking turns within every repeat, `before` enqueued (untimed) ahead of every launch"""
            for _ in range(3):
                for what in whats:
                    before(), what()
            torch.cuda.synchronize()
            evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in whats] for _ in range(repeats)]
            for row in evs:
                for (a, b), what in zip(row, whats):
                    before()
                    a.record(stream)
                    what()
                    b.record(stream)
            torch.cuda.synchronize()
            return [timing.summary([row[k][0].elapsed_time(row[k][1]) for row in evs]) for k in range(len(whats))]

        entry = {"blocks": nd, "arena_bytes": int(arena.nbytes)}
        quant()
        torch.cuda.synchronize()
        eob_in = d_res.download(np.dtype(abi.TXFM_RESULT_DTYPE), (nd,))["eob"].astype(np.int64)
        mappings = [m for m in MAPPINGS if m < 2 or w * h <= 128]
        outs = []
        for m in mappings:   # the mappings agree before any is timed
            quant(), rdoq(m)
            torch.cuda.synchronize()
            outs.append(d_out.download(np.dtype(abi.RDOQ_RESULT_DTYPE), (nd,)))
            assert outs[-1].tobytes() == outs[0].tobytes(), "the mappings disagree"
        times = timed(quant, [lambda m=m: rdoq(m) for m in mappings])
        for m, t in zip(mappings, times):
            t["blocks_per_us"] = round(nd / (t["median_ms"] * 1e3), 2)
            entry["stage_" + MAPPINGS[m]] = t
        order = sorted(range(len(mappings)), key=lambda k: times[k]["median_ms"])
        entry["fastest"] = {"mapping": MAPPINGS[mappings[order[0]]], "ahead_of_next_by": round(times[order[1]]["median_ms"] / times[order[0]]["median_ms"] - 1, 4),
                            "ranges_apart": times[order[0]]["max_ms"] < times[order[1]]["min_ms"]}
        ways = collections.Counter((outs[0]["path"] & abi.RDOQ_PATH_MASK).tolist())
        entry["mean_eob_in"], entry["mean_eob_out"] = round(float(eob_in.mean()), 2), round(float(outs[0]["eob"].mean()), 2)
        entry["paths"] = {name: ways.get(getattr(abi, "RDOQ_PATH_" + name), 0) for name in ("EOB_ZERO", "REQUANT_EOB", "EARLY_EXIT", "TRELLIS")}
        entry["chain_without_stage"], entry["chain_with_stage"] = timed(lambda: None, [lambda: (quant(), tail()), lambda: (quant(), shipped(), tail())])
        res["gpu"][f"{w}x{h}_{CANDIDATES}types"] = entry
        del d_arena, d_fwd, d_inv, d_rd, d_cost, d_res, d_res_inv, d_out, d_dist, d_bits, arena
    timing.write_profile(target, res)


if __name__ == "__main__":
    main()
