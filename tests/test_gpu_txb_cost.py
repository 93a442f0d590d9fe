"""GPU: svt_hip_txb_cost_batch against the golden bits of the reference's svt_av1_cost_coeffs_txb (tests/golden/txb_cost.npz) and, chained
behind the transform batch, against the restatement fed with the oracle's quantiser output.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import tx_cases
import txb_cost_cases as T
from arena import GUARD, PATTERN, Arena, check_containment
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
V = C.c_void_p


@pytest.fixture(scope="module")
def gold():
    return T.Golden()


def run(hip, gold, w, h, order=None, with_distortion=True, tables_in_lds=None):
    idx, arena, descs, dist, regions = T.batch(gold, w, h, order)
    d_arena, d_dist = device.DeviceBuffer(hip, arena.nbytes), device.DeviceBuffer(hip, dist.nbytes)
    d_arena.upload(arena)
    d_dist.upload(dist)
    out, guard = device.txb_cost_batch(hip, d_arena.ptr, descs, gold.tables, w, h, d_distortion=d_dist.ptr if with_distortion else None,
                                       tables_in_lds=tables_in_lds)
    assert (guard == GUARD).all(), "bytes around d_out were written"
    check_containment(arena, d_arena.download(np.uint8, (arena.nbytes,)), regions, [], "svt_hip_txb_cost_batch")
    return idx, out


@pytest.mark.parametrize("w, h", tx_cases.SIZES, ids=lambda v: str(v))
def test_txb_cost_matches_reference(hip, gold, w, h):
    """Every case of the size in one launch, with both placements of the coefficient tables: bits as the reference returns them,
    rd_cost as RDCOST gives it on the host."""
    for tables_in_lds in (None, 0, 1):
        idx, out = run(hip, gold, w, h, tables_in_lds=tables_in_lds)
        want_bits = gold.bits[idx]
        bad = np.nonzero(out["bits"] != want_bits)[0]
        assert bad.size == 0, (tables_in_lds, [(T.CASES[idx[k]], int(out["bits"][k]), int(want_bits[k])) for k in bad[:4]])
        want_rd = np.array([T.expected_rd(i, b) for i, b in zip(idx, want_bits)], np.uint64)
        bad = np.nonzero(out["rd_cost"] != want_rd)[0]
        assert bad.size == 0, (tables_in_lds, [(T.CASES[idx[k]], int(out["rd_cost"][k]), int(want_rd[k])) for k in bad[:4]])


@pytest.mark.parametrize("w, h", [(4, 4), (8, 4), (8, 8), (16, 16), (32, 32), (64, 16)], ids=lambda v: str(v))
def test_reversed_order_and_no_distortion(hip, gold, w, h):
    """The same descriptors in reversed order give the same bits (no block depends on its place in the wave or workgroup); without
    d_distortion rd_cost is 0."""
    idx, out = run(hip, gold, w, h, order=lambda n: range(n - 1, -1, -1), with_distortion=False)
    assert np.array_equal(out["bits"], gold.bits[idx]) and not out["rd_cost"].any()


@pytest.mark.parametrize("w, h", [(4, 4), (16, 8), (64, 64)], ids=lambda v: str(v))
def test_chain_behind_the_transform_batch(hip, orc, gold, w, h):
    """svt_hip_txfm_quant_batch -> svt_hip_txfm_distortion_batch -> svt_hip_txb_cost_batch on one stream; eob, three_quad_energy and the
    distortion are handed over on the device.  Equal to the restatement on the oracle's quantiser output and to RDCOST on the host."""
    rng = np.random.default_rng(w * 100 + h)
    iw, ih = T.retained(w, h)
    n, n_tb = iw * ih, 7
    ls = 2 if max(w, h) == 64 and (w * h) > 1024 else (1 if w * h > 256 and max(w, h) >= 32 and min(w, h) >= 16 else 0)
    types = T.size_types(w, h)
    ab = Arena(fill=PATTERN)
    iscan_off = {t: ab.add(f"iscan {t}", gold.iscan(w, h, t)) for t in types}
    descs, cost_descs, want = (abi.TxfmDesc * n_tb)(), np.zeros(n_tb, np.dtype(abi.TXB_COST_DESC_DTYPE)), []
    for i in range(n_tb):
        bd, tt, mode = (8, 10)[i % 2], types[i % len(types)], (abi.QUANT_B, abi.QUANT_FP, abi.QUANT_B_HBD)[i % 3]
        tq = tx_cases.quant_tables(rng, bd)
        res = (tx_cases.residual(rng, w, h, bd, 0, pad=5) // (1, 3, 40, 400)[i % 4]).astype(np.int16)
        if i == 5:
            res[:] = 0                                  # eob 0
        iscan = gold.iscan(w, h, tt)
        d = descs[i]
        d.residual_off, d.residual_stride = ab.add(f"residual {i}", res), w + 5
        d.coeff_off, d.qcoeff_off, d.dqcoeff_off = ab.add(f"coeff {i}", nbytes=n * 4), ab.add(f"qcoeff {i}", nbytes=n * 4), ab.add(f"dqcoeff {i}", nbytes=n * 4)
        d.pred_off = d.recon_off = d.qm_off = d.iqm_off = abi.NO_OFFSET
        d.iscan_off = iscan_off[tt]
        rnd, qnt = (tq["round"], tq["quant"]) if mode != abi.QUANT_FP else (tq["round_fp"], tq["quant_fp"])
        for k in range(2):
            d.zbin[k], d.round[k], d.quant[k] = int(tq["zbin"][k]), int(rnd[k]), int(qnt[k])
            d.quant_shift[k], d.dequant[k] = int(tq["qshift"][k]), int(tq["dequant"][k])
        d.tx_type, d.shape, d.bit_depth, d.quant_mode, d.log_scale, d.flags = tt, 0, bd, mode, ls, abi.TX_FWD
        c = T.Case("chain", w, h, tt, 0, 0xFFFF, (0, 5, 12)[i % 3], i % 3, 0 if tt == T.DCT_DCT and i % 2 == 0 else T.NEARESTMV, T.FILTER_INTRA_NONE,
                   0, 1 + i % 3, i % 2, 0, 0, i % 2, 1000 + 77777 * i, "", 0, 0)
        k = cost_descs[i]
        k["qcoeff_off"], k["iscan_off"], k["table"], k["lambda"], k["eob"] = d.qcoeff_off, d.iscan_off, c.table, c.lam, c.eob
        k["tx_type"], k["plane_type"], k["txb_skip_ctx"], k["dc_sign_ctx"], k["pred_mode"] = tt, 0, c.skip_ctx, c.dc_sign_ctx, c.pred_mode
        k["filter_intra_mode"], k["fast_coeff_est_level"], k["subres_step"] = c.fim, c.fast, c.step
        # the oracle's pipeline
        co = np.zeros(w * h, np.int32)
        orc.orc_fwd_txfm2d(tx_cases.P(res), tx_cases.P(co), C.c_uint32(w + 5), w, h, tt, bd, 0)
        energy = 0
        if max(w, h) == 64:
            orc.orc_handle_transform64.restype = C.c_uint64
            energy = orc.orc_handle_transform64(tx_cases.P(co), w, h)
        co = co[:n].copy()
        qc, dq, eob = tx_cases.orc_quant(orc, {abi.QUANT_B: 1, abi.QUANT_B_HBD: 2, abi.QUANT_FP: 3}[mode],
                                         dict(n=n, ls=ls, coeff=co, scan=T.scan_of(iscan).astype(np.int16), iscan=iscan, qm=None, iqm=None, t=tq))
        dist = int(((co.astype(np.int64) - dq) ** 2).sum())
        bits = T.restate_bits(gold.tables[c.table], c, qc, iscan, eob=eob)
        want.append((eob, bits, T.rd_cost(w, h, c.lam, bits, c.step, dist, energy)))
    assert {e for e, _, _ in want} >= {0} and max(e for e, _, _ in want) > 1
    arena = ab.build()
    d_arena, d_desc = device.DeviceBuffer(hip, arena.nbytes + 256), device.upload_descriptors(hip, list(descs))
    d_arena.upload(arena)
    d_res, d_dist = device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_tb), device.DeviceBuffer(hip, 16 * n_tb)
    device.check(hip, hip.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_desc.ptr), V(d_res.ptr), n_tb, w, h, None), "svt_hip_txfm_quant_batch")
    device.check(hip, hip.svt_hip_txfm_distortion_batch(V(d_arena.ptr), V(d_desc.ptr), V(d_dist.ptr), n_tb, w, h, None), "svt_hip_txfm_distortion_batch")
    before = d_arena.download(np.uint8, (arena.nbytes,))
    out, guard = device.txb_cost_batch(hip, d_arena.ptr, cost_descs, gold.tables, w, h, d_txfm_result=d_res.ptr, d_distortion=d_dist.ptr)
    assert (guard == GUARD).all()
    assert [(int(b), int(r)) for b, r in zip(out["bits"], out["rd_cost"])] == [(b, r) for _, b, r in want], want
    check_containment(before, d_arena.download(np.uint8, (arena.nbytes,)), ab.regions, [], "svt_hip_txb_cost_batch behind the transform")
