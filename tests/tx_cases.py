"""Shared case generators for the transform / quantiser parity tests (test infrastructure)."""
import ctypes as C

import numpy as np

SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64),
         (64, 32), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
V = C.c_void_p


def P(a):
    return V(a.ctypes.data)


def residual(rng, w, h, bd, trial, pad=3):
    """Recipe of test/FwdTxfm2dAsmTest.cc: values in +-(2^bd - 1), plus the all-max / alternating extremes."""
    lim = (1 << bd) - 1
    if trial == 0:
        return rng.integers(-lim, lim + 1, size=(h, w + pad)).astype(np.int16)
    if trial == 1:
        return np.full((h, w + pad), lim, np.int16)
    return ((rng.integers(0, 2, size=(h, w + pad)) * 2 - 1) * lim).astype(np.int16)


def coeffs_for_inverse(rng, orc, w, h, tt, bd, trial):
    iw, ih = min(w, 32), min(h, 32)
    if trial == 0:  # a real forward transform output
        res = residual(rng, w, h, bd, 0)
        co = np.zeros(w * h, np.int32)
        orc.orc_fwd_txfm2d(P(res), P(co), C.c_uint32(w + 3), w, h, tt, bd, 0)
        return co.reshape(h, w)[:ih, :iw].copy().reshape(-1)
    if trial == 1:
        return rng.integers(-(1 << (bd + 7)), 1 << (bd + 7), size=iw * ih).astype(np.int32)
    co = rng.integers(-(1 << (bd + 9)), 1 << (bd + 9), size=iw * ih).astype(np.int32)  # out of range: clamps
    co[rng.integers(0, iw * ih, size=iw * ih // 2)] = 0
    return co


def quant_tables(rng, bd):
    """Quantiser tables with the structure of svt_av1_build_quantizer (md_config_process.c:83-144)."""
    q = int(rng.integers(4, 1337 if bd == 8 else 5347))
    dequant = np.array([q, min(32767, int(q * 1.3) + 1)] + [0] * 6, np.int16)

    def inv(d):
        l = int(d).bit_length() - 1
        m = 1 + (1 << (16 + l)) // int(d)
        return np.int16(m - (1 << 16)), np.int16(1 << (16 - l))
    quant, qshift = np.zeros(8, np.int16), np.zeros(8, np.int16)
    for i in range(2):
        quant[i], qshift[i] = inv(dequant[i])
    t = dict(dequant=dequant, quant=quant, qshift=qshift,
             zbin=np.array([(int(d) * 84 + 64) >> 7 for d in dequant[:2]] + [0] * 6, np.int16),
             round=np.array([(int(d) * 48) >> 7 for d in dequant[:2]] + [0] * 6, np.int16),
             round_fp=np.array([(int(d) * 64) >> 7 for d in dequant[:2]] + [0] * 6, np.int16),
             quant_fp=np.array([min(32767, (1 << 16) // int(d)) for d in dequant[:2]] + [0] * 6, np.int16))
    return t


def quant_case(rng, trial):
    n = int(rng.choice([16, 64, 256, 1024]))
    ls = int(rng.integers(0, 3))
    bd = int(rng.choice([8, 10]))
    mag = int(rng.choice([50, 2000, 1 << (bd + 7), 1 << 20]))
    coeff = rng.integers(-mag, mag + 1, size=n).astype(np.int32)
    coeff[rng.random(n) < 0.5] = 0
    scan = rng.permutation(n).astype(np.int16) if trial % 3 else np.arange(n, dtype=np.int16)
    iscan = np.empty(n, np.int16)
    iscan[scan] = np.arange(n)
    use_qm = trial % 4 == 1
    qm = rng.integers(16, 64, size=n).astype(np.uint8) if use_qm else None
    iqm = rng.integers(16, 64, size=n).astype(np.uint8) if use_qm else None
    return dict(n=n, ls=ls, bd=bd, coeff=coeff, scan=scan, iscan=iscan, qm=qm, iqm=iqm, t=quant_tables(rng, bd))


def orc_quant(orc, mode, c):
    """mode: 1 quantize_b, 2 highbd_quantize_b, 3 quantize_fp, 4 highbd_quantize_fp -> (qcoeff, dqcoeff, eob)"""
    n, t = c["n"], c["t"]
    qc, dq, eob = np.full(n, 7, np.int32), np.full(n, 7, np.int32), C.c_uint16(9999)
    qm = P(c["qm"]) if c["qm"] is not None else None
    iqm = P(c["iqm"]) if c["iqm"] is not None else None
    if mode in (1, 2):
        fn = orc.orc_quantize_b if mode == 1 else orc.orc_highbd_quantize_b
        fn(P(c["coeff"]), C.c_ssize_t(n), P(t["zbin"]), P(t["round"]), P(t["quant"]), P(t["qshift"]), P(qc), P(dq),
           P(t["dequant"]), C.byref(eob), P(c["scan"]), qm, iqm, c["ls"])
    else:
        fn = orc.orc_quantize_fp if mode == 3 else orc.orc_highbd_quantize_fp
        fn(P(c["coeff"]), C.c_ssize_t(n), P(t["round_fp"]), P(t["quant_fp"]), P(qc), P(dq), P(t["dequant"]), C.byref(eob),
           P(c["scan"]), qm, iqm, c["ls"])
    return qc, dq, eob.value


class Arena:
    """Host image of a device arena: arrays placed at 256-byte aligned offsets with 256 bytes of slack between them."""

    def __init__(self):
        self.chunks, self.size = [], 0

    def add(self, arr=None, nbytes=None):
        off = self.size
        nbytes = arr.nbytes if arr is not None else nbytes
        self.chunks.append((off, None if arr is None else np.ascontiguousarray(arr).view(np.uint8).reshape(-1)))
        self.size += (nbytes + 255) // 256 * 256 + 256
        return off

    def build(self):
        buf = np.zeros(self.size, np.uint8)
        for off, a in self.chunks:
            if a is not None:
                buf[off:off + a.size] = a
        return buf


def fused_batch(orc, rng, w, h, n_tb):
    """n_tb blocks of w x h for svt_hip_txfm_quant_batch (residual -> fwd -> quantise -> inverse -> recon) with every valid tx_type
    in turn, 8- / 10-bit, both pixel widths and all four quantisers, and what the oracle pipeline makes of each.
    -> (arena image, descriptor array, expectations); check_fused_batch compares a device result with them."""
    from svtav1_hip import abi
    iw, ih = min(w, 32), min(h, 32)
    n = iw * ih
    ls = 2 if max(w, h) == 64 and (w * h) > 1024 else (1 if w * h > 256 and max(w, h) >= 32 and min(w, h) >= 16 else 0)
    types = [tt for tt in range(16) if orc.orc_txfm_valid(w, h, tt)]
    scan = rng.permutation(n).astype(np.int16)
    iscan = np.empty(n, np.int16)
    iscan[scan] = np.arange(n)
    ab = Arena()
    iscan_off = ab.add(iscan)
    descs, expect = (abi.TxfmDesc * n_tb)(), []
    for i in range(n_tb):
        bd = 8 if i % 3 == 0 else 10
        pix16 = bd == 10 or i % 2 == 0
        tt, mode = types[(i * 7) % len(types)], 1 + (i % 4)
        tq = quant_tables(rng, bd)
        res = (residual(rng, w, h, bd, 0, pad=5) // (1 + (i % 5))).astype(np.int16)
        pred16 = rng.integers(0, 1 << bd, size=(h, w + 2)).astype(np.uint16)
        d = descs[i]
        d.residual_off, d.residual_stride = ab.add(res), w + 5
        d.coeff_off = ab.add(nbytes=n * 4) if i % 2 else abi.NO_OFFSET
        d.qcoeff_off, d.dqcoeff_off = ab.add(nbytes=n * 4), ab.add(nbytes=n * 4)
        d.pred_off = ab.add(pred16 if pix16 else pred16.astype(np.uint8))
        d.recon_off = ab.add(nbytes=h * (w + 4) * (2 if pix16 else 1))
        d.pred_stride, d.recon_stride = w + 2, w + 4
        d.iscan_off, d.qm_off, d.iqm_off = iscan_off, abi.NO_OFFSET, abi.NO_OFFSET
        rnd, qnt = (tq["round"], tq["quant"]) if mode <= 2 else (tq["round_fp"], tq["quant_fp"])
        for k in range(2):
            d.zbin[k], d.round[k], d.quant[k] = int(tq["zbin"][k]), int(rnd[k]), int(qnt[k])
            d.quant_shift[k], d.dequant[k] = int(tq["qshift"][k]), int(tq["dequant"][k])
        d.tx_type, d.shape, d.bit_depth, d.quant_mode, d.log_scale = tt, 0, bd, mode, ls
        d.flags = abi.TX_FWD | abi.TX_INV | (abi.TX_PIXEL16 if pix16 else 0)
        co = np.zeros(w * h, np.int32)
        orc.orc_fwd_txfm2d(P(res), P(co), C.c_uint32(w + 5), w, h, tt, bd, 0)
        co = co[:n].copy()
        qc, dq, eob = orc_quant(orc, mode, dict(n=n, ls=ls, coeff=co, scan=scan, iscan=iscan, qm=None, iqm=None, t=tq))
        rec = np.zeros((h, w + 4), np.uint16)
        orc.orc_inv_txfm2d_add(P(dq), P(pred16), w + 2, P(rec), w + 4, w, h, tt, bd)
        expect.append((co, qc, dq, eob, rec if pix16 else rec.astype(np.uint8), pix16))
    return ab.build(), descs, expect


def check_fused_batch(w, h, descs, expect, out, res_raw, what=""):
    """out: the arena after the call; res_raw: (n_tb, 16) bytes of SvtHipTxfmResult"""
    from svtav1_hip import abi
    n = min(w, 32) * min(h, 32)
    for i, (co, qc, dq, eob, rec, pix16) in enumerate(expect):
        d = descs[i]

        def g(off, cnt, dt):
            return out[off:off + cnt * np.dtype(dt).itemsize].view(dt)
        if d.coeff_off != abi.NO_OFFSET:
            assert np.array_equal(g(d.coeff_off, n, np.int32), co), (what, "coeff", i, d.tx_type)
        assert np.array_equal(g(d.qcoeff_off, n, np.int32), qc), (what, "qcoeff", i, d.tx_type)
        assert np.array_equal(g(d.dqcoeff_off, n, np.int32), dq), (what, "dqcoeff", i, d.tx_type)
        assert int(res_raw[i, 8:10].view(np.uint16)[0]) == eob, (what, "eob", i, d.tx_type)
        got = g(d.recon_off, h * (w + 4), np.uint16 if pix16 else np.uint8).reshape(h, w + 4)
        assert np.array_equal(got[:, :w], rec[:, :w]), (what, "recon", i, d.tx_type)
