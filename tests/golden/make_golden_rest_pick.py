#!/usr/bin/env python3
"""Golden results for svt_hip_rest_pick_plane: the driver of tests/rest_pick_cases.py over the REAL reference's self-guided filter,
svt_get_proj_subspace, projection error, svt_apply_selfguided_restoration and SSE, taken through the reference's own dispatch pointers
(oracle/_ref), the Wiener unit records from wiener_pick_cases.drive over the reference's leaves.  Planes are seeded
(tests/rest_pick_cases.py); only results are stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pyorc  # noqa: E402
import rest_pick_cases as K  # noqa: E402

ref = pyorc.ref()
store = {}
for case in K.CASES:
    x = K.make_inputs(case)
    wrecs = K.wiener_records(x, K.wiener_leaves(x, ref, "ref"))
    out = K.drive(x, K.RefLeaves(x, ref), wrecs)
    for f in K.FIELDS:
        store[f"{case.name}_{f}"] = out[f]
    if wrecs is not None:
        store[f"{case.name}_wiener"] = wrecs
path = os.path.join(HERE, "rest_pick.npz")
np.savez_compressed(path, **store)
print("rest_pick.npz:", len(store), "arrays", os.path.getsize(path), "bytes")
