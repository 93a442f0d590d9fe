"""TEST INFRASTRUCTURE — writes tests/golden/rdoq.npz from the reference (oracle/_ref/libsvtref.so + tests/rdoq_pin_driver.c): the
quantiser tables of svt_av1_build_quantizer at the bit depths and base qindex classes the cases use, the quantisation matrices of
svt_av1_qm_init for the (plane, size) pairs that use them, and per case what svt_aom_quantize_inv_quantize leaves: eob, cul_level, the
number of coefficients the stage changed and a 64-bit digest of qcoeff and of dqcoeff.  `path` is the restatement's (the reference has
no such output); it is stored only once the restatement's arrays equal the reference's.  Rate tables and scans are those of
tests/golden/txb_cost.npz.
    python tests/golden/make_golden_rdoq.py"""
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
import txb_cost_cases as T  # noqa: E402


class Seed:
    """What Block needs of a Golden before the fixture exists"""

    def __init__(self, pin):
        self.txb = T.Golden()
        self.tables, self.quant, self.qms = self.txb.tables, pin.quant_tables(), {}
        for c in R.CASES:
            key = (c.plane, T.TX_INDEX[(c.w, c.h)])
            if c.qm and key not in self.qms:
                self.qms[key] = pin.qm(c.plane, c.w, c.h)
    iscan, qt, qm = R.Golden.iscan, R.Golden.qt, R.Golden.qm


def main():
    orc = pyorc.oracle()
    with tempfile.TemporaryDirectory() as tmp:
        pin = R.Pin(pyorc.ref(), tmp)
        seed = Seed(pin)
        rows = []
        for i, c in enumerate(R.CASES):
            b = R.Block(seed, orc, i)
            q, dq, eob, cul = pin.run(c, b.coeff)
            assert np.array_equal(q, b.q) and np.array_equal(dq, b.dq) and (eob, cul) == (b.eob, b.cul), (i, c)
            rows.append((eob, cul, b.path, b.changed, R.digest(q), R.digest(dq)))
    keys = sorted(seed.qms)
    offsets = np.cumsum([0] + [len(seed.qms[k][0]) for k in keys])
    cols = list(zip(*rows))
    np.savez_compressed(R.GOLD, quant=seed.quant, qm=np.concatenate([seed.qms[k][0] for k in keys]), iqm=np.concatenate([seed.qms[k][1] for k in keys]),
                        qm_index=np.array([(p, s, o, len(seed.qms[(p, s)][0])) for (p, s), o in zip(keys, offsets)], np.int32),
                        eob=np.array(cols[0], np.uint16), cul_level=np.array(cols[1], np.uint8), path=np.array(cols[2], np.uint8),
                        changed=np.array(cols[3], np.uint32), q_digest=np.array(cols[4], np.uint64), dq_digest=np.array(cols[5], np.uint64))
    print(len(R.CASES), "cases ->", R.GOLD, os.path.getsize(R.GOLD), "bytes")


if __name__ == "__main__":
    main()
