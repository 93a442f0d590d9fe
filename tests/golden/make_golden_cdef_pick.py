#!/usr/bin/env python3
"""Golden results for svt_hip_cdef_pick_strengths: the finish_cdef_search driver of tests/cdef_pick_cases.py over the REAL
reference svt_search_one_dual, taken through the reference's own dispatch pointer (oracle/_ref) as make_golden_leaves.py takes
it.  Inputs are seeded (tests/cdef_pick_cases.py); only results are stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pyorc  # noqa: E402
import cdef_pick_cases as K  # noqa: E402

search = K.ref_search(pyorc.ref())
store = {}
for case in K.CASES:
    out = K.drive(K.make_inputs(case), search)
    for f in K.FIELDS:
        store[f"{case.name}_{f}"] = out[f]
path = os.path.join(HERE, "cdef_pick.npz")
np.savez_compressed(path, **store)
print("cdef_pick.npz:", len(store), "arrays", os.path.getsize(path), "bytes")
