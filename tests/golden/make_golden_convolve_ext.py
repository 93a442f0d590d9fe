#!/usr/bin/env python3
"""Golden vectors for the interpolation cases the first fixtures (convolve.npz, convolve_jnt.npz) leave out, produced by the REAL
reference functions (oracle/_ref RTCD pointers svt_av1_(highbd_)convolve_*_sr and svt_av1_(highbd_)jnt_convolve_*): every kernel
table in x and in y with another table in the other direction, blocks of width 2, an InterpFilterParams of 4 taps, 8 / 10 / 12 bit,
adversarial planes; per case the single-reference prediction, the conv buffer of a first compound prediction and the pixels of both
compound averages.

    python tests/golden/make_golden_convolve_ext.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pyorc  # noqa: E402
import conv_cases as K  # noqa: E402
import lf_cases as L  # noqa: E402
import test_convolve_oracle as T  # noqa: E402
from lf_cases import V  # noqa: E402

R8, SHARP, BIL, SM8, R4, SM4 = list(K.TABLES)
CASES = [  # w, h, mode, x table, y table, x phase, y phase, taps, plane kind, bit depth
    K.ExtCase(8, 8, 0, R8, SHARP, 3, 11, (8, 8), K.KIND_UNIFORM, 8),
    K.ExtCase(16, 8, 0, SHARP, SM8, 7, 8, (8, 8), K.KIND_UNIFORM, 10),
    K.ExtCase(8, 16, 0, SM8, BIL, 9, 5, (8, 8), K.KIND_UNIFORM, 12),
    K.ExtCase(16, 16, 0, BIL, R4, 13, 2, (8, 8), K.KIND_SMOOTH, 8),
    K.ExtCase(4, 8, 0, R4, SM4, 6, 10, (8, 8), K.KIND_BINARY, 10),
    K.ExtCase(8, 4, 0, SM4, R8, 1, 15, (8, 8), K.KIND_UNIFORM, 12),
    K.ExtCase(2, 8, 0, R4, SHARP, 8, 4, (8, 8), K.KIND_UNIFORM, 8),
    K.ExtCase(2, 2, 1, SM4, SM4, 5, 0, (8, 8), K.KIND_UNIFORM, 10),
    K.ExtCase(2, 4, 2, SM4, R4, 0, 14, (8, 8), K.KIND_BINARY, 12),
    K.ExtCase(12, 6, 0, R4, SM4, 12, 7, (4, 4), K.KIND_UNIFORM, 12),
    K.ExtCase(6, 10, 2, BIL, R8, 0, 9, (8, 6), K.KIND_SMOOTH, 8),
    K.ExtCase(10, 6, 1, BIL, BIL, 11, 0, (2, 2), K.KIND_UNIFORM, 10),
    K.ExtCase(16, 16, 3, R8, SHARP, 0, 0, (8, 8), K.KIND_UNIFORM, 12),
    K.ExtCase(8, 8, 0, SHARP, R8, 8, 8, (8, 8), K.KIND_ADV, 12),
    K.ExtCase(8, 8, 0, SHARP, R4, 4, 12, (8, 8), K.KIND_ADV_INV, 8),
    K.ExtCase(8, 8, 2, R8, SHARP, 5, 7, (8, 8), K.KIND_ADV, 10),
]

ref = pyorc.ref()
sig8 = (V, C.c_int32, V, C.c_int32, C.c_int32, C.c_int32, V, V, C.c_int32, C.c_int32, V)
store, names = {}, list(K.TABLES)
rng = np.random.default_rng(2718)
for i, c in enumerate(CASES):
    sig = sig8 + ((C.c_int32,) if c.is16 else ())
    hb = "highbd_" if c.is16 else ""
    sr = [L.rtcd(ref, f"svt_av1_{hb}convolve_{m}_sr", None, *sig) for m in K.MODES]
    jnt = [L.rtcd(ref, f"svt_av1_{hb}jnt_convolve_{m}", None, *sig) for m in K.MODES]
    (p0, a0), (p1, a1) = K.ext_plane(rng, c), K.ext_plane(rng, c, second=True)
    fwd, bck = K.DIST_WEIGHTS[i % 8]       # never (8, 8): the weighted average must differ from the plain one
    store[f"c{i}_meta"] = np.array([c.w, c.h, c.mode, names.index(c.tx), names.index(c.ty), c.sx, c.sy, c.taps[0], c.taps[1], c.kind, c.bd,
                                    fwd, bck], np.int32)
    store[f"c{i}_p0"], store[f"c{i}_p1"] = p0, p1
    store[f"c{i}_sr"] = T.ext_run_fn_sr(sr, c, p0, a0, T.ConvolveParams, K.InterpFilterParams)[:, :c.w].copy()
    for key, avg in (("avg", 2), ("wtd", 3)):
        first, out = T.ext_run_fn_jnt(jnt, c, p0, a0, p1, a1, avg, fwd, bck, T.ConvolveParams, K.InterpFilterParams)
        store[f"c{i}_first"], store[f"c{i}_{key}"] = first[:, :c.w].copy(), out[:, :c.w].copy()
store["n"] = np.array(len(CASES))
np.savez_compressed(os.path.join(HERE, "convolve_ext.npz"), **store)
print("convolve_ext.npz:", len(CASES), "cases", os.path.getsize(os.path.join(HERE, "convolve_ext.npz")), "bytes")
