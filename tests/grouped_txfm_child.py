"""Child process of tests/test_gpu_concurrency.py::test_grouped_transform_two_streams (run with SVTAV1_HIP_GROUP_TX=1, which the
library reads once per process): fused transform batches of at least GROUP_MIN_BLOCKS blocks with mixed tx_type, so that the
descriptors are grouped by type first, for 4x4, 8x8, 4x8 and 16x16, issued back to back on two streams without synchronisation.
The calls share the thread's grow-only index buffer, which an event guards against the other stream.  Every coefficient, eob and
reconstruction is compared with the oracle.  Exit status 0 when everything matches."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "svt-av1-mod-by-patman_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pyorc  # noqa: E402
import tx_cases as T  # noqa: E402
from svtav1_hip import abi, device  # noqa: E402

V = C.c_void_p
# largest batch first: the index buffer grows once (a synchronising free), every later call reuses it behind the event
BATCHES = [(4, 4, 2560), (8, 8, 2304), (4, 8, 2048), (16, 16, 2048)]


def main():
    assert os.environ.get("SVTAV1_HIP_GROUP_TX"), "run with SVTAV1_HIP_GROUP_TX=1"
    orc = pyorc.oracle()
    hip = abi.load()
    device.check(hip, hip.svt_hip_init(0), "svt_hip_init")
    rng = np.random.default_rng(2048)
    jobs = []
    for w, h, n_tb in BATCHES:
        arena, descs, expect = T.fused_batch(orc, rng, w, h, n_tb)
        assert len({d.tx_type for d in descs}) > 1
        darena = device.DeviceBuffer(hip, arena.nbytes + 256)
        darena.upload(arena)
        ddesc = device.DeviceBuffer(hip, C.sizeof(descs))
        ddesc.upload(np.frombuffer(descs, dtype=np.uint8))
        dres = device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_tb)
        jobs.append((w, h, n_tb, arena, descs, expect, darena, ddesc, dres))
    streams = [V(), V()]
    for s in streams:
        device.check(hip, hip.svt_hip_stream_create(C.byref(s)), "svt_hip_stream_create")
    for k, (w, h, n_tb, arena, descs, expect, darena, ddesc, dres) in enumerate(jobs):
        device.check(hip, hip.svt_hip_txfm_quant_batch(V(darena.ptr), V(ddesc.ptr), V(dres.ptr), C.c_uint32(n_tb), C.c_uint32(w),
                                                       C.c_uint32(h), streams[k % 2]), f"svt_hip_txfm_quant_batch {w}x{h}")
    for s in streams:
        device.check(hip, hip.svt_hip_stream_sync(s), "svt_hip_stream_sync")
    for w, h, n_tb, arena, descs, expect, darena, ddesc, dres in jobs:
        out = darena.download(np.uint8, (arena.nbytes,))
        res_raw = dres.download(np.uint8, (n_tb, abi.TXFM_RESULT_BYTES))
        T.check_fused_batch(w, h, descs, expect, out, res_raw, f"grouped {w}x{h}")
        print(f"grouped {w}x{h}: {n_tb} blocks bit-exact", flush=True)
    for s in streams:
        device.check(hip, hip.svt_hip_stream_destroy(s), "svt_hip_stream_destroy")
    return 0


if __name__ == "__main__":
    sys.exit(main())
