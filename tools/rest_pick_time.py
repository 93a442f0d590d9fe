#!/usr/bin/env python3
"""Time the restoration decision of one 4K 10-bit plane with the self-guided filter (no Wiener records: what the three paths share),
three ways, in one session (one measurement, no threshold):
  a  svt_hip_rest_pick_plane: HIP events around the whole launch chain, warm-up, median of the repeats;
  b  the only device path before it: per unit svt_hip_sgr_search_unit (which reads its winner back) and svt_hip_sgr_apply_unit, then
     one download of the restored plane, the SSEs and the decision on the host (host clock, median of --host-repeats);
  c  the oracle's C functions on one CPU core: orc_sgr_search_unit, orc_apply_selfguided_restoration in stripes, SSE, decision
     (host clock, once).
Configurations: luma 3840 x 2160 (units of 256: 120) at the ep settings of sg_filter_lvl 1 (0..16, refine) and 3 (0..16 step 8,
refine), and the 4:2:0 chroma plane 1920 x 1080 (units of 128) at 4..5 without refinement.  The decisions of a, b and c are compared
where they must agree (b applies from the unit's top-left instead of in stripes, so its SSE may differ; its search may not).
Prints one JSON line and writes it to profiles/rest_pick_4k.json (or --out).
    python tools/rest_pick_time.py [--repeats 10] [--host-repeats 3] [--out FILE] [--skip-cpu]"""
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

import rest_pick_cases as K  # noqa: E402
from benchlib import timing  # noqa: E402
from lf_cases import P, V  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

BD = 10
CONFIGS = {"luma_lvl1": (3840, 2160, 256, 0, K.EP_ALL), "luma_lvl3": (3840, 2160, 256, 0, K.EP_STEP8), "chroma_4_5": (1920, 1080, 128, 1, K.EP_4_5)}


def sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def finish(case, x, sse_none, sse_sgr, ep, xqd):
    """The host's share of b and c: the finish visitors and the plane decision -> (plane type, units of type SGRPROJ)"""
    n = len(x.limits)
    best, _, _, _, _, plane_type, _, _ = K.decide(case, [[sse_none[i], K.INT64_MAX, sse_sgr[i]] for i in range(n)], [None] * n, [0] * n, ep, xqd)
    return plane_type, sum(b[1] == K.SGRPROJ for b in best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rest_pick_4k.json"))
    args = ap.parse_args()
    lib = timing.open_library()
    assert lib is not None, "no device"
    import pyorc
    import torch
    orc = pyorc.oracle()
    orc.orc_sgr_search_unit.restype = C.c_int64
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    res = {"bit_depth": BD, "repeats": args.repeats, "host_repeats": args.host_repeats, "wiener_records": False}
    for name, (w, h, unit, ss, ep_range) in CONFIGS.items():
        case = K.Case("time_" + name, w, h, unit, BD, 1, ss, 0, ep_range, 4000, (0, 0), (200, 1000), (0, 0, 0), "bnmhl", 40)
        x = K.make_inputs(case)
        n, pu, n_ep = len(x.limits), 64 >> ss, K.n_ep(case)
        d_dgd, d_src = device.DeviceBuffer(lib, x.dgd.nbytes), device.DeviceBuffer(lib, x.src.nbytes)
        d_dgd.upload(x.dgd), d_src.upload(x.src)
        ds = x.dgd.shape[1]
        dgd0 = d_dgd.ptr + (K.B * ds + K.B) * 2
        units, prm = K.wiener_units(x, dgd0, d_src.ptr), K.params(x)
        # a
        pick = device.DeviceRestPick(lib, n, w, h, n_ep)

        def run_a():
            rc = pick.run(prm, units, None, sp)
            assert rc > 0, lib.svt_hip_last_error()
            return rc
        launches = run_a()
        ms = timing.events(torch, stream, args.repeats, run_a)
        got = pick.download(sp)
        r = res[name] = {"plane": [w, h], "unit_size": unit, "units": n, "ep": list(ep_range), "a_rest_pick_plane": dict(timing.summary(ms), launches=launches),
                         "workspace_bytes": int(pick.workspace.nbytes), "frame_restoration_type": int(got["result"]["frame_restoration_type"]),
                         "trials_of_winner": {"mean": round(float(got["units"]["trials"].mean()), 2), "max": int(got["units"]["trials"].max())}}
        # b
        d_dst = device.DeviceBuffer(lib, h * w * 2)
        work = device.DeviceBuffer(lib, max(lib.svt_hip_sgr_search_work_bytes(he - hs, ve - vs, n_ep) for hs, he, vs, ve in x.limits))
        restored = np.zeros((h, w), np.uint16)
        inner = x.dgd[K.B:-K.B, K.B:-K.B]

        def run_b():
            eps, xqds = [], []
            for hs, he, vs, ve in x.limits:
                u = abi.SgrUnit(dgd0 + (vs * ds + hs) * 2, d_src.ptr + (vs * w + hs) * 2, ds, w, he - hs, ve - vs, 1, BD, pu, pu)
                out = np.zeros(3, np.int32)
                device.check(lib, lib.svt_hip_sgr_search_unit(C.byref(u), *ep_range, V(work.ptr), P(out), None, sp), "svt_hip_sgr_search_unit")
                xqd = out[1:].copy()
                device.check(lib, lib.svt_hip_sgr_apply_unit(C.byref(u), int(out[0]), P(xqd), V(d_dst.ptr + (vs * w + hs) * 2), w, sp), "svt_hip_sgr_apply_unit")
                eps.append(int(out[0])), xqds.append([int(out[1]), int(out[2])])
            device.check(lib, lib.svt_hip_download(restored.ctypes.data, d_dst.ptr, restored.nbytes, sp), "download")
            device.check(lib, lib.svt_hip_stream_sync(sp), "sync")
            s_none = [sse(inner[vs:ve, hs:he], x.src[vs:ve, hs:he]) for hs, he, vs, ve in x.limits]
            s_sgr = [sse(restored[vs:ve, hs:he], x.src[vs:ve, hs:he]) for hs, he, vs, ve in x.limits]
            return eps, xqds, finish(case, x, s_none, s_sgr, eps, xqds)
        run_b()
        tb = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            eps_b, xqd_b, dec_b = run_b()
            tb.append((time.perf_counter() - t0) * 1e3)
        assert eps_b == got["units"]["ep"].tolist() and xqd_b == got["units"]["xqd"].tolist(), "a and b disagree on a search"
        r["b_per_unit_search_apply_host_decision"] = {"median_ms": round(statistics.median(tb), 3), "min_ms": round(min(tb), 3), "max_ms": round(max(tb), 3),
                                                      "launches": n * (n_ep + 3), "host_round_trips": n + 1}
        r["a_faster_than_b_by"] = round(statistics.median(tb) / r["a_rest_pick_plane"]["median_ms"], 1)
        # c
        if not args.skip_cpu:
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
            lv = K.OrcLeaves(x, orc)
            t0 = time.perf_counter()
            eps, xqds, s_none, s_sgr = [], [], [], []
            for limits in x.limits:
                hs, he, vs, ve = limits
                out = np.zeros(3, np.int32)
                orc.orc_sgr_search_unit(V(K._addr(x.dgd, K.B + vs, K.B + hs)), he - hs, ve - vs, ds, V(K._addr(x.src, vs, hs)), w, 1, BD, pu, pu, *ep_range, P(out))
                eps.append(int(out[0])), xqds.append([int(out[1]), int(out[2])])
                s_none.append(sse(inner[vs:ve, hs:he], x.src[vs:ve, hs:he]))
                s_sgr.append(K.trial_sse(x, lv, limits, eps[-1], xqds[-1]))
            dec_c = finish(case, x, s_none, s_sgr, eps, xqds)
            r["c_oracle_one_core_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert eps == got["units"]["ep"].tolist() and s_sgr == got["units"]["sse"][:, 2].tolist(), "a and c disagree"
            assert dec_c[0] == r["frame_restoration_type"]
            r["a_faster_than_c_by"] = round(r["c_oracle_one_core_ms"] / r["a_rest_pick_plane"]["median_ms"], 1)
    timing.write_profile(os.path.abspath(args.out), res)


if __name__ == "__main__":
    main()
