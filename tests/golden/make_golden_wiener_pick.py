#!/usr/bin/env python3
"""Golden results for svt_hip_wiener_pick_plane: the driver of tests/wiener_pick_cases.py over the REAL reference's statistics,
separable filter and SSE, taken through the reference's own dispatch pointers (oracle/_ref).  Planes are seeded
(tests/wiener_pick_cases.py); only results are stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pyorc  # noqa: E402
import wiener_pick_cases as K  # noqa: E402

ref = pyorc.ref()
store = {}
for case in K.CASES:
    x = K.make_inputs(case)
    out = K.drive(x, K.RefLeaves(x, ref))
    for f in K.FIELDS:
        store[f"{case.name}_{f}"] = out[f]
path = os.path.join(HERE, "wiener_pick.npz")
np.savez_compressed(path, **store)
print("wiener_pick.npz:", len(store), "arrays", os.path.getsize(path), "bytes")
