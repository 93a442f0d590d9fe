#!/usr/bin/env python3
"""Writes tests/golden/scale.npz from the reference's own functions only (oracle/_ref/libsvtref.so and tests/scale_pin_driver.c; needs the
reference tree): per case of tests/scale_cases.py what svt_av1_resize_plane_c, svt_av1_upscale_normative_rows and
svt_av1_convolve_2d_scale_c (or their highbd twins) gave for the case's generated input, and for a chain
svt_av1_jnt_convolve_2d_c behind it, as the array or, above scale_cases.ARRAY_MAX_BYTES, as the SHA-256 of its bytes; and the reference's five filter banks and two half filters, which the numpy
restatement reads.  Inputs are not stored: the case lists and the seeded makers of scale_cases.py regenerate them."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import pyorc  # noqa: E402
import scale_cases as K  # noqa: E402

ref, store = pyorc.ref(), {}
with tempfile.TemporaryDirectory() as tmp:
    pin = K.build_pin(tmp)
    store["banks"], store["half"] = K.reference_banks(pin)
    for c in K.SUPERRES:
        K.record(store, "superres/" + c.name, K.reference_superres(pin, c))
for c in K.RESIZE:
    K.record(store, "resize/" + c.name, K.reference_resize(ref, c))
for c in K.SCALED:
    K.record(store, "scaled/" + c.name, K.reference_scaled(ref, c))
for ch in K.CHAINS:
    K.record(store, "scaled/" + ch.first.name, K.reference_scaled(ref, ch.first))
    K.record(store, "chain/" + ch.name, K.reference_chain(ref, ch))
path = os.path.join(HERE, "scale.npz")
np.savez_compressed(path, **store)
print("scale.npz:", len(store), "arrays,", sum(k.startswith("sha/") for k in store), "of them digests,", os.path.getsize(path), "bytes")
assert os.path.getsize(path) <= K.GOLD_MAX_BYTES
