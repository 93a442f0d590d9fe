#!/usr/bin/env python3
"""Writes tests/golden/ifs.npz: the reference's five filter banks and, per case of tests/ifs_cases.py, what the reference's own functions
(driven by tests/ifs_pin_driver.c in the loop order of interpolation_filter_search) leave: the nine (sse, rd) pairs, the winner record
(index, packed filters, switchable rate) and the CRC-32 of the winner's prediction.  Results only: the inputs are regenerated from seeds.
Needs oracle/_ref/libsvtref.so."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import ifs_cases as I  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as d:
        pin = I.Pin(d)
        got = [pin.search(c) for c in I.CASES]
        banks = pin.banks()
    np.savez_compressed(I.GOLDEN, banks=banks, sse=np.array([g[0] for g in got], np.uint64), rd=np.array([g[1] for g in got], np.uint64),
                        rec=np.array([g[2] for g in got], np.int64), crc=np.array([g[3] for g in got], np.uint32))
    print(len(got), "cases ->", I.GOLDEN, os.path.getsize(I.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
