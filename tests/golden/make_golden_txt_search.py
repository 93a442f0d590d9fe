"""TEST INFRASTRUCTURE — writes tests/golden/txt_search.npz from the reference (oracle/_ref/libsvtref.so + tests/txt_search_pin_driver.c): per
case of txt_search_cases.SEARCH_CASES what the reference's static tx_type_search leaves: transform_type, y_coeff_bits,
y_full_distortion[DIST_SSD][2], eob.y, y_has_coeff and 64-bit digests of the quant / rec_coeff / recon blocks in cand_bf (recon only where
the search measures spatial SSE: elsewhere the reference runs no inverse transform).  Inputs are not stored: every case is a seed and
parameters in txt_search_cases.py.  The winner's index, cul_level, the cost and the two candidate masks are the restatement's (the
reference has no such outputs); they are stored only once everything the reference does return equals the restatement's.
    python tests/golden/make_golden_txt_search.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import pyorc  # noqa: E402
import rdoq_cases as R  # noqa: E402
import txt_search_cases as X  # noqa: E402


def main():
    gold, orc = R.Golden(), pyorc.oracle()
    rows = [None] * len(X.SEARCH_CASES)
    with tempfile.TemporaryDirectory() as tmp:
        pin = X.Pin(pyorc.ref(), tmp)
        for w, h in X.SEARCH_SIZES:
            s = X.Search(gold, orc, w, h)
            for bi, i in enumerate(s.case_index):
                got = pin.run(s, bi)
                assert got == X.Pin.restated(s, bi), (i, X.SEARCH_CASES[i], got, X.Pin.restated(s, bi))
                extra = s.summary(bi)
                rows[i] = got + tuple(extra[X.FIXTURE_FIELDS.index(f)] for f in X.RESTATED_FIELDS)
    dtypes = dict(tx_type=np.uint8, cand=np.uint8, eob=np.uint16, cul_level=np.uint8, quant_mask=np.uint16, cost_mask=np.uint16, has_coeff=np.uint8)
    np.savez_compressed(X.GOLD, seed=np.array([c.seed for c in X.SEARCH_CASES], np.uint32),
                        **{f: np.array(col, dtypes.get(f, np.uint64)) for f, col in zip(X.REFERENCE_FIELDS + X.RESTATED_FIELDS, zip(*rows))})
    print(len(rows), "cases ->", X.GOLD, os.path.getsize(X.GOLD), "bytes")


if __name__ == "__main__":
    main()
