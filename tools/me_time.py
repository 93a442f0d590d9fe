#!/usr/bin/env python3
"""Tuning aid: milliseconds per me_b64_kernel launch of the headline workload (16 x 4K x 5 references) for the library named by
SVTAV1_HIP_LIB (default: the in-tree build), and a sha256 over what the last launch computed (bench.me_workload_outputs); builds
are compared by running this once per build, alternating, in one session.  --params KEY: another parameter set of
tests/golden/me_params.json (m6_4k_tl2: prepared references, staged windows; m4_4k_tl2: the unprepared staged loop)."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mod-by-patman_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", metavar="KEY", default="m8_4k_tl2")
    args = ap.parse_args()
    import torch
    import bench
    from svtav1_hip import abi
    lib = abi.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    assert lib.svt_hip_init(0) == 0
    mw = bench.MeWorkload(lib, dev, 3840, 2160, 16, args.params, (-1, -2, -3), (1, 2), seed=7)
    stream = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(stream.cuda_stream)
    mw.analysis(sp)
    ms = [round(bench.timed_launches(stream, 5, 2, lambda: mw.me(sp)), 4) for _ in range(4)]
    torch.cuda.synchronize()
    digest = hashlib.sha256()
    for name, a in sorted(bench.me_workload_outputs(mw).items()):
        digest.update(name.encode() + a.tobytes())
    print(os.environ.get("SVTAV1_HIP_LIB", "libsvtav1_hip.so"), args.params, ms, "sha256", digest.hexdigest(), flush=True)


if __name__ == "__main__":
    main()
