"""Shared case generators for the transform / quantiser parity tests (test infrastructure)."""
import ctypes as C

import numpy as np

from arena import PATTERN, Arena

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


def quant_tables(rng, bd, q=None):
    """Quantiser tables with the structure of svt_av1_build_quantizer (md_config_process.c:83-144)."""
    q = int(rng.integers(4, 1337 if bd == 8 else 5347)) if q is None else q
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
    iscan_off = ab.add("iscan", iscan)
    descs, expect = (abi.TxfmDesc * n_tb)(), []
    for i in range(n_tb):
        bd = 8 if i % 3 == 0 else 10
        pix16 = bd == 10 or i % 2 == 0
        tt, mode = types[(i * 7) % len(types)], 1 + (i % 4)
        tq = quant_tables(rng, bd)
        res = (residual(rng, w, h, bd, 0, pad=5) // (1 + (i % 5))).astype(np.int16)
        pred16 = rng.integers(0, 1 << bd, size=(h, w + 2)).astype(np.uint16)
        d = descs[i]
        d.residual_off, d.residual_stride = ab.add(f"residual {i}", res), w + 5
        d.coeff_off = ab.add(f"coeff {i}", nbytes=n * 4) if i % 2 else abi.NO_OFFSET
        d.qcoeff_off, d.dqcoeff_off = ab.add(f"qcoeff {i}", nbytes=n * 4), ab.add(f"dqcoeff {i}", nbytes=n * 4)
        d.pred_off = ab.add(f"pred {i}", pred16 if pix16 else pred16.astype(np.uint8))
        d.recon_off = ab.add(f"recon {i}", nbytes=h * (w + 4) * (2 if pix16 else 1))
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


# ---- inputs with a known composition per wavefront for the fused kernel (tests/test_gpu_txfm_paths.py) ----
def wave_blocks(w, h):
    """Consecutive descriptors of one launch that share a wavefront: NT of Geo<W, H> in csrc/txfm_block.hpp."""
    return max(1, 64 // max(w, h))


def own_log_scale(w, h):
    return 2 if max(w, h) == 64 and (w * h) > 1024 else (1 if w * h > 256 and max(w, h) >= 32 and min(w, h) >= 16 else 0)


def declared_outputs(d, w, h):
    """(offset, bytes) of everything descriptor d allows the fused kernel to write."""
    from svtav1_hip import abi
    n, px = min(w, 32) * min(h, 32), 2 if d.flags & abi.TX_PIXEL16 else 1
    out = []
    if d.flags & abi.TX_FWD and d.coeff_off != abi.NO_OFFSET:
        out.append((d.coeff_off, (w * h if d.flags & abi.TX_FULLCOEFF else n) * 4))
    if d.quant_mode != abi.QUANT_NONE:
        out += [(off, n * 4) for off in (d.qcoeff_off, d.dqcoeff_off) if off != abi.NO_OFFSET]
    if d.flags & abi.TX_INV:
        out += [(d.recon_off + r * d.recon_stride * px, w * px) for r in range(h)]
    return out


def _fused_block(ab, orc, rng, w, h, d, i, scan, iscan, iscan_off, res, bd, pix16, tt, shape, mode, ls, flags, qm=None, iqm=None,
                 skew=0, want_coeff=True, want_q=True, want_dq=True, dq_mode=0, crop=False, tq=None):
    """Place block i in the arena, fill descriptor d and return what the oracle pipeline makes of it.  Without TX_FWD the
    oracle's coefficients are the input at coeff_off (quantiser on) or their dq_mode quantisation is at dqcoeff_off."""
    from svtav1_hip import abi
    iw, ih = min(w, 32), min(h, 32)
    n = iw * ih
    fwd, inv, quant = bool(flags & abi.TX_FWD), bool(flags & abi.TX_INV), mode != abi.QUANT_NONE
    tq = tq or quant_tables(rng, bd)
    pred16 = rng.integers(0, 1 << bd, size=(h, w + 2)).astype(np.uint16)
    full = np.zeros(w * h, np.int32)
    orc.orc_fwd_txfm2d(P(res), P(full), C.c_uint32(res.shape[1]), w, h, tt, bd, shape)
    co, energy = full.copy(), 0
    if max(w, h) == 64:
        orc.orc_handle_transform64.restype = C.c_uint64
        energy = orc.orc_handle_transform64(P(co), w, h)
    co = co[:n].copy()
    orc.orc_satd.restype = C.c_int
    case = dict(n=n, ls=ls, coeff=co, scan=scan, iscan=iscan, qm=qm, iqm=iqm, t=tq)
    qc, dq, eob = orc_quant(orc, mode or dq_mode, case) if (mode or dq_mode) else (None, None, 0)
    name = lambda s: f"{s} of block {i}"
    d.residual_off, d.residual_stride = (ab.add(name("residual"), res) if fwd else abi.NO_OFFSET), res.shape[1]
    if fwd:
        nco = w * h if flags & abi.TX_FULLCOEFF else n
        d.coeff_off = ab.add(name("coeff"), nbytes=nco * 4, skew=skew) if want_coeff else abi.NO_OFFSET
    else:
        d.coeff_off = ab.add(name("coeff (input)"), co, skew=skew) if quant else abi.NO_OFFSET
    d.qcoeff_off = ab.add(name("qcoeff"), nbytes=n * 4, skew=skew) if quant and want_q else abi.NO_OFFSET
    if quant:
        d.dqcoeff_off = ab.add(name("dqcoeff"), nbytes=n * 4, skew=skew) if want_dq else abi.NO_OFFSET
    else:
        d.dqcoeff_off = ab.add(name("dqcoeff (input)"), dq, skew=skew) if inv and not fwd else abi.NO_OFFSET
    d.pred_off = d.recon_off = abi.NO_OFFSET
    if inv:
        d.pred_off = ab.add(name("pred"), pred16 if pix16 else pred16.astype(np.uint8))
        d.recon_off = ab.add(name("recon"), nbytes=h * (w + 4) * (2 if pix16 else 1))
    d.pred_stride, d.recon_stride = w + 2, w + 4
    d.iscan_off = iscan_off
    d.qm_off = ab.add(name("qm"), qm) if qm is not None else abi.NO_OFFSET
    d.iqm_off = ab.add(name("iqm"), iqm) if iqm is not None else abi.NO_OFFSET
    rnd, qnt = (tq["round"], tq["quant"]) if mode <= 2 else (tq["round_fp"], tq["quant_fp"])
    for k in range(2):
        d.zbin[k], d.round[k], d.quant[k] = int(tq["zbin"][k]), int(rnd[k]), int(qnt[k])
        d.quant_shift[k], d.dequant[k] = int(tq["qshift"][k]), int(tq["dequant"][k])
    d.tx_type, d.shape, d.bit_depth, d.quant_mode, d.log_scale = tt, shape, bd, mode, ls
    d.flags = flags | (abi.TX_PIXEL16 if pix16 else 0)
    if crop:      # a block cut by the picture edge: the caller's cropped_tx_width / cropped_tx_height
        d.dist_w, d.dist_h = max(1, iw - 3), max(1, ih // 2)
    rec = None
    if inv:
        rec = np.zeros((h, w + 4), np.uint16)
        orc.orc_inv_txfm2d_add(P(dq), P(pred16), w + 2, P(rec), w + 4, w, h, tt, bd)
        rec = rec if pix16 else rec.astype(np.uint8)
    return dict(case=case, full=full, co=co, qc=qc, dq=dq, eob=eob if quant else 0, energy=energy if fwd else 0,
                satd=orc.orc_satd(P(co), n) if fwd and flags & abi.TX_SATD else 0, rec=rec)


def check_fused_blocks(orc, w, h, descs, blocks, out, res_raw, dist=None, what=""):
    """Every output a descriptor declares, and its SvtHipTxfmResult, against the oracle's; dist: svt_hip_txfm_distortion_batch's."""
    from svtav1_hip import abi
    iw, ih = min(w, 32), min(h, 32)
    n = iw * ih
    for i, b in enumerate(blocks):
        d = descs[i]
        tag = (what, i, b.get("kind"), d.tx_type, d.quant_mode, d.bit_depth, d.flags)

        def g(off, cnt, dt):
            return out[off:off + cnt * np.dtype(dt).itemsize].view(dt)
        fwd, quant, pix16 = d.flags & abi.TX_FWD, d.quant_mode != abi.QUANT_NONE, d.flags & abi.TX_PIXEL16
        if fwd and d.coeff_off != abi.NO_OFFSET:
            if d.flags & abi.TX_FULLCOEFF:
                assert np.array_equal(g(d.coeff_off, w * h, np.int32), b["full"]), ("full coeff",) + tag
            else:
                assert np.array_equal(g(d.coeff_off, n, np.int32), b["co"]), ("coeff",) + tag
        if quant and d.qcoeff_off != abi.NO_OFFSET:
            assert np.array_equal(g(d.qcoeff_off, n, np.int32), b["qc"]), ("qcoeff",) + tag
        if quant and d.dqcoeff_off != abi.NO_OFFSET:
            assert np.array_equal(g(d.dqcoeff_off, n, np.int32), b["dq"]), ("dqcoeff",) + tag
        r = abi.TxfmResult.from_buffer_copy(res_raw[i].tobytes())
        assert r.eob == b["eob"], ("eob", r.eob, b["eob"]) + tag
        assert r.three_quad_energy == b["energy"], ("three_quad_energy",) + tag
        assert r.satd == b["satd"], ("satd", r.satd, b["satd"]) + tag
        if d.flags & abi.TX_INV:
            got = g(d.recon_off, h * (w + 4), np.uint16 if pix16 else np.uint8).reshape(h, w + 4)
            assert np.array_equal(got[:, :w], b["rec"][:, :w]), ("recon",) + tag
        if dist is not None:
            want = np.zeros(2, np.uint64)
            if d.coeff_off != abi.NO_OFFSET and d.dqcoeff_off != abi.NO_OFFSET and not d.flags & abi.TX_FULLCOEFF:
                orc.orc_full_distortion32(P(b["co"]), iw, P(b["dq"]), iw, P(want), d.dist_w or iw, d.dist_h or ih)
            assert np.array_equal(dist[i], want), ("distortion",) + tag


def path_plan(nt):
    """The waves of one round of path_cases, each a list of nt (kind, quant_mode): kind 'small' (every coefficient within
    int16), 'large1' / 'large2' (the all-max / alternating-sign residual), 'qm+iqm', 'qm', 'iqm' (what matrices it carries),
    'edge' (small, but |DC| + round is past int16: the saturation of QUANT_B / QUANT_FP inside a short form), 'over' (a DC in
    32768..65535 on which the 32-bit products of the short form would overflow: the threshold of the path choice itself)."""
    waves = [[("small", mode)] * nt for _ in range(2) for mode in (1, 2, 3, 4)]
    waves[4][nt - 1], waves[6][0] = ("edge", 1), ("edge", 3)
    for k in range(2):                      # among quantize_b neighbours: without the threshold the wave would run quant_small<true>
        waves.append([("small", (2, 1)[k])] * nt)
        waves[-1][(nt // 2, 0)[k]] = ("over", 2)
    for k, (trial, slot) in enumerate((tr, s) for tr in (1, 2) for s in (0, nt // 2, nt - 1)):
        mode = (1, 3, 2, 4, 3, 1)[k]       # the neighbours share its quantiser: only the coefficient forces the wave
        waves.append([("small", mode)] * nt)
        waves[-1][slot] = (f"large{trial}", mode)
    for k in range(2):                      # one carrier of both matrices among small blocks of one quantiser
        waves.append([("small", (2, 3)[k])] * nt)
        waves[-1][(0, nt - 1)[k]] = ("qm+iqm", (1, 4)[k])
    for k in range(2):                      # every block carries both
        waves.append([("qm+iqm", 1 + (s + k) % 4) for s in range(nt)])
    for kind in ("qm", "iqm"):              # one matrix only: on every block, then on one block
        waves.append([(kind, 1 + (s + (kind == "iqm")) % 4) for s in range(nt)])
        waves.append([("small", 4 if kind == "qm" else 1)] * nt)
        waves[-1][nt // 2] = (kind, 2 if kind == "qm" else 3)
    if nt > 1:                              # both families, all small (a wave of one block cannot mix)
        waves += [[("small", (1, 3, 2, 4)[s % 4]) for s in range(nt)], [("small", (4, 2, 3, 1)[s % 4]) for s in range(nt)]]
    return waves


def path_cases(orc, rng, w, h):
    """Blocks of w x h for svt_hip_txfm_quant_batch in runs of wave_blocks(w, h) descriptors, so that whole wavefronts have a
    known composition (path_plan), and one trailing block in a wave of its own where waves hold several.  Bit depths 8 / 10 /
    12, both pixel widths, every valid tx_type, the three shapes, the size's own log_scale and (a minority) the other two, a
    third of the blocks with their coefficient arrays 4 / 8 / 12 bytes past a 16-byte boundary.
    -> dict(arena, regions, descs, blocks): blocks[i] is what the oracle pipeline makes of descriptor i (_fused_block)."""
    from svtav1_hip import abi
    nt, iw, ih, L = wave_blocks(w, h), min(w, 32), min(h, 32), max(w, h)
    n, ls0 = iw * ih, own_log_scale(w, h)
    types = [tt for tt in range(16) if orc.orc_txfm_valid(w, h, tt)]
    scan = rng.permutation(n).astype(np.int16)
    iscan = np.empty(n, np.int16)
    iscan[scan] = np.arange(n)
    kinds = [km for _ in range(1 if L <= 8 else (2 if L == 16 else 3)) for wave in path_plan(nt) for km in wave]
    if nt > 1:
        kinds.append(("small", 2))
    ab = Arena(fill=PATTERN)
    iscan_off = ab.add("iscan", iscan)
    descs, blocks = (abi.TxfmDesc * len(kinds))(), []

    def coeff_max(res, tt, bd, shape):
        co = np.zeros(w * h, np.int32)
        orc.orc_fwd_txfm2d(P(res), P(co), C.c_uint32(w + 5), w, h, tt, bd, shape)
        if max(w, h) == 64:
            orc.orc_handle_transform64(P(co), w, h)
        return int(np.abs(co[:n].astype(np.int64)).max())
    n_mat = 0
    for i, (kind, mode) in enumerate(kinds):
        bd, tq = (8, 10, 12)[i % 3], None
        tt, shape = types[(i + (i // nt if nt > 1 else 0)) % len(types)], (0, 0, 1, 2)[(i // 3) % 4]
        ls = ls0 if i % 7 not in (3, 5) else (ls0 + (1 if i % 7 == 3 else 2)) % 3
        qm = iqm = None
        if kind.startswith("large"):
            # 10 bits and the first type from here on that carries the residual past int16; 12 bits where none does (the
            # largest 4x4 coefficient of 10-bit samples is 32 * 1023 = 32736, and the random signs reach less at 8 points)
            order, shape = types[types.index(tt):] + types[:types.index(tt)], 0
            for bd in (10, 12):
                res = residual(rng, w, h, bd, int(kind[5]), pad=5)
                over = [t for t in order if coeff_max(res, t, bd, 0) > 32767]
                if over:
                    tt = over[0]
                    break
        elif kind in ("edge", "over"):
            # a flat residual, DCT_DCT: only the DC is set, to the largest value below the bound that the sample range reaches
            tt, shape, ls, top = 0, 0, ls0, 32767 if kind == "edge" else 65535
            for bd in (10, 12):
                flat = lambda v: np.full((h, w + 5), v, np.int16)
                v = next(v for v in range((1 << bd) - 1, 0, -1) if coeff_max(flat(v), tt, bd, 0) <= top)
                res = flat(v)
                if coeff_max(flat(v + 1), tt, bd, 0) > top:
                    break
            if kind == "over":   # dequant 4095: quant = -32759, the largest magnitude the tables take
                tq = quant_tables(rng, bd, q=4095)
            else:                # tables whose rounding term carries this DC past int16: the 8-bit form then differs from the highbd one
                co = np.zeros(w * h, np.int32)
                orc.orc_fwd_txfm2d(P(res), P(co), C.c_uint32(w + 5), w, h, tt, bd, 0)
                if max(w, h) == 64:
                    orc.orc_handle_transform64(P(co), w, h)
                for _ in range(200):
                    tq = quant_tables(rng, bd)
                    c = dict(n=n, ls=ls, coeff=co[:n].copy(), scan=scan, iscan=iscan, qm=None, iqm=None, t=tq)
                    if not np.array_equal(orc_quant(orc, mode, c)[0], orc_quant(orc, mode + 1, c)[0]):
                        break
        else:
            res = (residual(rng, w, h, bd, 0, pad=5) // (1 + (i % 5))).astype(np.int16)
            if kind == "small":
                while coeff_max(res, tt, bd, shape) > 32767:
                    res = (res // 2).astype(np.int16)
            else:                        # 16..63 as in quant_case; every fourth carrier the whole range of a QmVal
                lo, hi = (1, 256) if n_mat % 4 == 3 else (16, 64)
                n_mat += 1
                qm = rng.integers(lo, hi, size=n).astype(np.uint8) if kind in ("qm+iqm", "qm") else None
                iqm = rng.integers(lo, hi, size=n).astype(np.uint8) if kind in ("qm+iqm", "iqm") else None
        b = _fused_block(ab, orc, rng, w, h, descs[i], i, scan, iscan, iscan_off, res, bd, bd != 8 or i % 2 == 0, tt, shape, mode, ls,
                         abi.TX_FWD | abi.TX_INV | (abi.TX_SATD if i % 2 else 0), qm, iqm,
                         skew=(4, 8, 12)[(i // 3) % 3] if i % 3 == 1 else 0, want_coeff=i % 4 != 3, crop=i % 6 == 1, tq=tq)
        b["kind"] = kind
        blocks.append(b)
    return dict(arena=ab.build(), regions=ab.regions, descs=descs, blocks=blocks)


def path_census(w, h, descs, coeffs):
    """Which quantiser each wavefront of a svt_hip_txfm_quant_batch launch runs, and why, from the descriptors and the
    retained coefficients coeffs[i] the quantiser of block i sees.  This MIRRORS the kernel (csrc/txfm.hip txfm_kernel,
    csrc/txfm_block.hpp txfm_block / load_qp) and must follow it if the mapping changes: a wave holds the wave_blocks(w, h)
    consecutive descriptors i // NT; a row of a block is plain when the block has no matrix, its tables fit 16 bits, its
    log_scale is 0..2 and the row's largest |coefficient| is at most 32767; a wave of plain rows of quantize_b blocks only
    runs quant_small<true>, of fp blocks only quant_small<false>, any other wave quant_one.
    -> one dict per wave: path, modes (of its blocks) and why (what keeps it from a short form: 'large', 'qm+iqm', 'qm',
    'iqm' for a block that is not plain, 'mixed' for both families among the plain ones)."""
    from svtav1_hip import abi
    nt, iw, ih = wave_blocks(w, h), min(w, 32), min(h, 32)
    waves = []
    for w0 in range(0, len(descs), nt):
        paths, why, modes = [], set(), []
        for i in range(w0, min(w0 + nt, len(descs))):
            d = descs[i]
            ls, has_qm, has_iqm = d.log_scale, d.qm_off != abi.NO_OFFSET, d.iqm_off != abi.NO_OFFSET
            rpot = lambda v: (v + ((1 << ls) >> 1)) >> ls
            tables = all(rpot(d.zbin[k]) >= 0 and rpot(d.round[k]) >= 0 and d.quant_shift[k] >= 0 and d.dequant[k] >= 0 for k in range(2))
            simple = tables and not has_qm and not has_iqm and 0 <= ls <= 2
            rows = np.abs(np.asarray(coeffs[i], np.int64).reshape(ih, iw)).max(axis=1)
            for rowmax in rows:
                paths.append((1 if d.quant_mode in (abi.QUANT_B, abi.QUANT_B_HBD) else 2) if simple and rowmax <= 32767 else 0)
            if has_qm or has_iqm:
                why.add("qm+iqm" if has_qm and has_iqm else ("qm" if has_qm else "iqm"))
            elif rows.max() > 32767:
                why.add("large")
            modes.append(d.quant_mode)
        if set(paths) >= {1, 2}:
            why.add("mixed")
        path = "quant_small<true>" if set(paths) == {1} else ("quant_small<false>" if set(paths) == {2} else "quant_one")
        waves.append(dict(path=path, why=frozenset(why), modes=tuple(modes)))
    return waves


CENSUS_CLASSES = ("small QUANT_B", "small QUANT_B_HBD", "small QUANT_FP", "small QUANT_FP_HBD", "large", "qm+iqm", "qm", "iqm", "mixed")


def census_classes(waves):
    """Waves per class of CENSUS_CLASSES: a short-form wave of one quantiser, or a quant_one wave with exactly one cause."""
    count = dict.fromkeys(CENSUS_CLASSES, 0)
    for wv in waves:
        if wv["path"] != "quant_one":
            if len(set(wv["modes"])) == 1:
                count[CENSUS_CLASSES[wv["modes"][0] - 1]] += 1
        elif len(wv["why"]) == 1:
            count[next(iter(wv["why"]))] += 1
    return count


def saturation_census(orc, w, h, blocks, descs):
    """Blocks on whose coefficients the 8-bit form of their quantiser family and the highbd form differ (the int16 saturation
    of QUANT_B / QUANT_FP is what tells them apart), counted by (path of the block's wave, family 'b' / 'fp'); and under
    'overflow' the QUANT_B_HBD blocks in a quant_one wave with no coefficient past 65535 and one past 32767 for which
    (|c| + round) * quant leaves 32 bits, as it must not in the short form."""
    nt, iw = wave_blocks(w, h), min(w, 32)
    waves = path_census(w, h, descs, [b["co"] for b in blocks])
    hits = {}
    for i, (b, d) in enumerate(zip(blocks, descs)):
        if not d.quant_mode:
            continue
        fam, path = (d.quant_mode - 1) // 2, waves[i // nt]["path"]
        a, c = orc_quant(orc, 1 + 2 * fam, b["case"]), orc_quant(orc, 2 + 2 * fam, b["case"])
        if not (np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and a[2] == c[2]):
            hits[path, "b" if fam == 0 else "fp"] = hits.get((path, "b" if fam == 0 else "fp"), 0) + 1
        mag, ls = np.abs(b["co"].astype(np.int64)), d.log_scale
        if d.quant_mode == 2 and path == "quant_one" and waves[i // nt]["why"] == {"large"} and mag.max() <= 65535:
            ac = (np.arange(mag.size) != 0).astype(int)
            rnd, qnt = np.array([(d.round[k] + ((1 << ls) >> 1)) >> ls for k in range(2)])[ac], np.array([abs(d.quant[k]) for k in range(2)])[ac]
            if np.any((mag > 32767) & ((mag + rnd) * qnt >= 1 << 31)):
                hits["overflow"] = hits.get("overflow", 0) + 1
    return hits


FLAG_COMBOS = ("fwd", "fwd full", "inv", "quant inv", "quant", "no qcoeff", "no dqcoeff", "all")


def flag_cases(orc, rng, w, h):
    """Blocks of w x h for svt_hip_txfm_quant_batch that take the FLAG_COMBOS in turn, shifted by one per wave so that every
    wave of several blocks mixes them, the last wave partly filled:
      fwd         TX_FWD | TX_SATD, no quantiser: packed coefficients out
      fwd full    the same with TX_FULLCOEFF: the whole [h][w] array, for 64-point sizes before energy / repack
      inv         TX_INV alone: the inverse of what is at dqcoeff_off
      quant inv   a quantiser and TX_INV without TX_FWD: coeff_off is the input
      quant       the same without TX_INV
      no qcoeff   TX_FWD | TX_INV | TX_SATD and a quantiser, qcoeff_off = NO_OFFSET
      no dqcoeff  the same with dqcoeff_off = NO_OFFSET instead
      all         TX_FWD | TX_INV | TX_SATD and a quantiser, every output
    -> as path_cases."""
    from svtav1_hip import abi
    nt, iw, ih = wave_blocks(w, h), min(w, 32), min(h, 32)
    n, ls = iw * ih, own_log_scale(w, h)
    types = [tt for tt in range(16) if orc.orc_txfm_valid(w, h, tt)]
    scan = rng.permutation(n).astype(np.int16)
    iscan = np.empty(n, np.int16)
    iscan[scan] = np.arange(n)
    n_tb = max(24, 4 * nt) + (nt > 1)
    ab = Arena(fill=PATTERN)
    iscan_off = ab.add("iscan", iscan)
    descs, blocks = (abi.TxfmDesc * n_tb)(), []
    F, I, S = abi.TX_FWD, abi.TX_INV, abi.TX_SATD
    for i in range(n_tb):
        combo = FLAG_COMBOS[(i + (i // nt if nt > 1 else 0)) % len(FLAG_COMBOS)]
        bd = (8, 10, 12)[i % 3]
        mode, mat = 1 + (i // 2) % 4, i % 5 == 2
        res = (residual(rng, w, h, bd, 0, pad=5) // (1 + (i % 4))).astype(np.int16)
        kw = dict(want_coeff=i % 4 != 3)
        if combo in ("fwd", "fwd full"):
            flags, mode, mat = F | S | (abi.TX_FULLCOEFF if combo == "fwd full" else 0), abi.QUANT_NONE, False
            kw = {}
        elif combo == "inv":
            flags, kw, mode = I, dict(dq_mode=mode), abi.QUANT_NONE
        elif combo in ("quant inv", "quant"):
            flags = I if combo == "quant inv" else 0
        else:
            flags = F | I | S
            kw.update(want_q=combo != "no qcoeff", want_dq=combo != "no dqcoeff")
        qm = rng.integers(16, 64, size=n).astype(np.uint8) if mat else None
        iqm = rng.integers(16, 64, size=n).astype(np.uint8) if mat else None
        b = _fused_block(ab, orc, rng, w, h, descs[i], i, scan, iscan, iscan_off, res, bd, bd != 8 or i % 2 == 0,
                         types[(i + (i // nt if nt > 1 else 0)) % len(types)], (0, 0, 1, 2)[(i // 3) % 4], mode, ls, flags, qm, iqm,
                         skew=(4, 8, 12)[(i // 3) % 3] if i % 3 == 1 else 0, **kw)
        b["kind"] = combo
        blocks.append(b)
    return dict(arena=ab.build(), regions=ab.regions, descs=descs, blocks=blocks)


def quantize_batch_cases(orc, rng, n, n_tb=64):
    """n_tb blocks of n coefficients for svt_hip_quantize_batch: the four quantisers in turn, the magnitudes of quant_case
    (1 << 20 among them), log_scale 0..2, a permuted scan, matrices on a third of the blocks.
    -> dict(arena, regions, descs, expect): expect[i] = (qcoeff, dqcoeff, eob) of the oracle."""
    from svtav1_hip import abi
    ab = Arena(fill=PATTERN)
    descs, expect = (abi.TxfmDesc * n_tb)(), []
    for i in range(n_tb):
        bd, mode = int(rng.choice([8, 10])), 1 + i % 4
        mag = (50, 2000, 1 << (bd + 7), 1 << 20)[(i // 4) % 4]
        coeff = rng.integers(-mag, mag + 1, size=n).astype(np.int32)
        coeff[rng.random(n) < 0.5] = 0
        scan = rng.permutation(n).astype(np.int16)
        iscan = np.empty(n, np.int16)
        iscan[scan] = np.arange(n)
        qm = rng.integers(16, 64, size=n).astype(np.uint8) if i % 3 == 1 else None
        iqm = rng.integers(16, 64, size=n).astype(np.uint8) if i % 3 == 1 else None
        c = dict(n=n, ls=int(rng.integers(0, 3)), bd=bd, coeff=coeff, scan=scan, iscan=iscan, qm=qm, iqm=iqm, t=quant_tables(rng, bd))
        d, t = descs[i], c["t"]
        d.coeff_off, d.iscan_off = ab.add(f"coeff of block {i}", coeff), ab.add(f"iscan of block {i}", iscan)
        d.qcoeff_off, d.dqcoeff_off = ab.add(f"qcoeff of block {i}", nbytes=n * 4), ab.add(f"dqcoeff of block {i}", nbytes=n * 4)
        d.qm_off = ab.add(f"qm of block {i}", qm) if qm is not None else abi.NO_OFFSET
        d.iqm_off = ab.add(f"iqm of block {i}", iqm) if iqm is not None else abi.NO_OFFSET
        d.residual_off = d.pred_off = d.recon_off = abi.NO_OFFSET
        rnd, qnt = (t["round"], t["quant"]) if mode <= 2 else (t["round_fp"], t["quant_fp"])
        for k in range(2):
            d.zbin[k], d.round[k], d.quant[k] = int(t["zbin"][k]), int(rnd[k]), int(qnt[k])
            d.quant_shift[k], d.dequant[k] = int(t["qshift"][k]), int(t["dequant"][k])
        d.quant_mode, d.log_scale = mode, c["ls"]
        expect.append(orc_quant(orc, mode, c))
    return dict(arena=ab.build(), regions=ab.regions, descs=descs, expect=expect)


def assert_path_census(orc, w, h, batch):
    """The design of path_cases' inputs, a condition on them and no measurement: at least two waves in every class of
    CENSUS_CLASSES (a wave of one block cannot mix the families: none there), the int16 saturation of QUANT_B and of QUANT_FP
    in play on a block that uses that family, and the spread of the other inputs.  -> waves per class."""
    from svtav1_hip import abi
    descs, blocks, nt = batch["descs"], batch["blocks"], wave_blocks(w, h)
    count = census_classes(path_census(w, h, descs, [b["co"] for b in blocks]))
    for cls in CENSUS_CLASSES:
        if cls == "mixed" and nt == 1:
            assert count[cls] == 0, (w, h, count)
        else:
            assert count[cls] >= 2, (w, h, cls, count)
    hits = saturation_census(orc, w, h, blocks, descs)
    for key in (("quant_small<true>", "b"), ("quant_small<false>", "fp"), ("quant_one", "b"), ("quant_one", "fp"), "overflow"):
        assert hits.get(key, 0) >= 1, (w, h, key, hits)
    skewed = [d.qcoeff_off % 16 for d in descs]
    assert {0, 4, 8, 12} == set(skewed) and {d.dqcoeff_off % 16 for d in descs} == {0, 4, 8, 12}, (w, h)
    assert {d.coeff_off % 16 for d in descs if d.coeff_off != abi.NO_OFFSET} == {0, 4, 8, 12}, (w, h)
    assert 3 * sum(s != 0 for s in skewed) >= len(descs) - 2, (w, h)
    assert all(not (skewed[i] and skewed[i + 1]) for i in range(len(descs) - 1)), (w, h)   # the neighbours stay aligned
    assert {d.tx_type for d in descs} == {tt for tt in range(16) if orc.orc_txfm_valid(w, h, tt)}, (w, h)
    assert {(d.bit_depth, bool(d.flags & abi.TX_PIXEL16)) for d in descs} == {(8, False), (8, True), (10, True), (12, True)}, (w, h)
    assert {d.log_scale for d in descs} == {0, 1, 2} and {d.shape for d in descs} == {0, 1, 2}, (w, h)
    assert 2 * sum(d.log_scale == own_log_scale(w, h) for d in descs) > len(descs), (w, h)
    return count
