"""GPU: svt_hip_rdoq_batch against the Python restatement of the reference's RDOQ stage (tests/rdoq_cases.py) and the golden digests of
svt_aom_quantize_inv_quantize (tests/golden/rdoq.npz), and chained between the transform batch and the distortion and rate batches
against the oracle's transform and quantiser fed through the restatement.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import rdoq_cases as R
import tx_cases
import txb_cost_cases as T
from arena import GUARD, PATTERN, Arena, check_containment, rows
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
V = C.c_void_p


def mappings(w, h):
    """svt_hip_rdoq_batch's own choice and every work split svt_hip_rdoq_batch_mapped has for the size (one lane per block up to 128
    retained coefficients)"""
    return (None, 0, 1, 2) if min(w, 32) * min(h, 32) <= 128 else (None, 0, 1)


@pytest.fixture(scope="module")
def gold():
    return R.Golden()


@pytest.fixture(scope="module")
def blocks(gold, orc):
    """Every case with its restated result, made once"""
    return [R.Block(gold, orc, i) for i in range(len(R.CASES))]


def launch(hip, gold, arena, tdescs, descs, results, w, h, mapping=None):
    """-> (arena after the call, SvtHipRdoqResult records, SvtHipTxfmResult records after the call)"""
    d_arena, d_tdesc = device.DeviceBuffer(hip, arena.nbytes), device.upload_descriptors(hip, tdescs)
    d_res = device.upload_descriptors(hip, results)
    d_arena.upload(arena)
    out, guard = device.rdoq_batch(hip, d_arena.ptr, d_tdesc.ptr, descs, gold.tables, d_res.ptr, w, h, mapping=mapping)
    assert (guard == GUARD).all(), "bytes around d_out were written"
    return d_arena.download(np.uint8, (arena.nbytes,)), out, d_res.download(np.dtype(abi.TXFM_RESULT_DTYPE), (len(results),))


def i32(buf, off, n):
    return buf[int(off):int(off) + 4 * n].view(np.int32)


def check(gold, blocks, idx, arena, regions, tdescs, results, got_arena, out, got_results):
    declared = []
    for k, i in enumerate(idx):
        b, d, n = blocks[i], tdescs[k], len(blocks[i].q)
        q, dq = i32(got_arena, d["qcoeff_off"], n), i32(got_arena, d["dqcoeff_off"], n)
        assert np.array_equal(q, b.q), ("qcoeff", i, b.c, np.nonzero(q != b.q)[0][:8])
        assert np.array_equal(dq, b.dq), ("dqcoeff", i, b.c, np.nonzero(dq != b.dq)[0][:8])
        assert (R.digest(q), R.digest(dq)) == (gold.q_digest[i], gold.dq_digest[i]), ("digest", i, b.c)
        assert (int(out["eob"][k]), int(out["cul_level"][k]), int(out["path"][k])) == (b.eob, b.cul, b.path), ("result", i, b.c, out[k])
        assert (b.eob, b.cul, b.path) == (gold.eob[i], gold.cul_level[i], gold.path[i])
        declared += [(int(d["qcoeff_off"]), 4 * n), (int(d["dqcoeff_off"]), 4 * n)]
    check_containment(arena, got_arena, regions, declared, "svt_hip_rdoq_batch")
    want_results = results.copy()
    want_results["eob"] = [blocks[i].eob for i in idx]     # an unflagged block keeps the eob it came with: the restatement's too
    assert got_results.tobytes() == want_results.tobytes(), "d_txfm_result: only eob may change"


@pytest.mark.parametrize("w, h", tx_cases.SIZES, ids=lambda v: str(v))
def test_rdoq_matches_reference(hip, gold, blocks, w, h):
    """Every case of the size in one launch, with every work split the size has: both arrays, eob, cul_level and path as the
    restatement (pinned to the reference) has them, the digests of the fixture, eob handed on in d_txfm_result, nothing else written."""
    idx, arena, tdescs, descs, results, regions = R.batch(blocks, w, h)
    assert len(idx) >= 40
    for mapping in mappings(w, h):
        check(gold, blocks, idx, arena, regions, tdescs, results, *launch(hip, gold, arena, tdescs, descs, results, w, h, mapping))


@pytest.mark.parametrize("w, h", [(4, 4), (8, 4), (8, 8), (16, 16), (32, 32), (64, 16)], ids=lambda v: str(v))
def test_reversed_order(hip, gold, blocks, w, h):
    """The same descriptors in reversed order give the same results: no block depends on its place in the wave or the batch."""
    idx, arena, tdescs, descs, results, regions = R.batch(blocks, w, h, order=lambda n: range(n - 1, -1, -1))
    for mapping in mappings(w, h)[1:]:
        check(gold, blocks, idx, arena, regions, tdescs, results, *launch(hip, gold, arena, tdescs, descs, results, w, h, mapping))


@pytest.mark.parametrize("w, h, mapping", [(4, 4, 0), (4, 4, 1), (4, 4, 2), (8, 8, 0), (8, 8, 1)], ids=lambda v: str(v))
def test_more_blocks_than_one_pass_of_the_grid(hip, gold, blocks, w, h, mapping):
    """The grid is capped at 16 workgroups per compute unit and a workgroup takes 64 / min(n, 64) blocks per step (64 with one lane per
    block), so a launch this long makes every workgroup come round again and reuse its LDS (levels, scan, nz_ci, the staged tables)
    for blocks of other table sets and paths.  The case list of the size is repeated; the copies' coefficient arrays lie packed behind
    the arena of the first."""
    n, compute_units = w * h, 320                            # an MI355X has 256; the margin keeps the test meaningful on a larger part
    per_pass = compute_units * 16 * (64 if mapping == 2 else 64 // min(n, 64))
    idx, arena, tdescs, descs, results, regions = R.batch(blocks, w, h)
    repeat = per_pass // len(idx) + 2
    nb = len(idx) * repeat
    packed = np.tile(np.stack([np.stack([blocks[i].coeff, blocks[i].q0, blocks[i].dq0]) for i in idx]), (repeat, 1, 1))   # [nb][3][n]
    big = np.concatenate([arena, packed.reshape(-1).view(np.uint8)])
    tdescs, descs, results = np.tile(tdescs, repeat), np.tile(descs, repeat), np.tile(results, repeat)
    at = arena.nbytes + np.arange(nb, dtype=np.uint64) * np.uint64(12 * n)
    tdescs["coeff_off"], tdescs["qcoeff_off"], tdescs["dqcoeff_off"] = at, at + np.uint64(4 * n), at + np.uint64(8 * n)
    got, out, got_results = launch(hip, gold, big, tdescs, descs, results, w, h, mapping)
    want = np.tile(np.stack([np.stack([blocks[i].coeff, blocks[i].q, blocks[i].dq]) for i in idx]), (repeat, 1, 1))
    check_containment(arena, got[:arena.nbytes], regions, [], "svt_hip_rdoq_batch_mapped")
    bad = np.nonzero((got[arena.nbytes:].view(np.int32).reshape(nb, 3, n) != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, (bad[:8], [blocks[idx[k % len(idx)]].c for k in bad[:2]])
    for field, attr in (("eob", "eob"), ("cul_level", "cul"), ("path", "path")):
        assert np.array_equal(out[field], np.tile([getattr(blocks[i], attr) for i in idx], repeat)), field
    results["eob"] = out["eob"]
    assert got_results.tobytes() == results.tobytes()


@pytest.mark.parametrize("w, h", [(4, 4), (8, 16), (32, 32)], ids=lambda v: str(v))
def test_out_of_range_fields_are_clamped(hip, gold, blocks, w, h):
    """include/svt_hip_txfm.h: a table index beyond n_tables, contexts beyond their tables and an eob above the retained count are
    clamped, iscan values are reduced modulo the retained count.  Each is given where the clamped value is the case's own, so the
    results are the restatement's."""
    idx, arena, tdescs, descs, results, regions = R.batch(blocks, w, h)
    n = min(w, 32) * min(h, 32)
    cs = [blocks[i].c for i in idx]
    hit = dict(table=0, skip=0, sign=0, eob=0)
    for k, (i, c) in enumerate(zip(idx, cs)):
        if c.table == len(gold.tables) - 1 and k % 2:
            descs["table"][k], hit["table"] = 7 + k, hit["table"] + 1
        if c.skip_ctx == 12:
            descs["txb_skip_ctx"][k], hit["skip"] = 13 + k % 200, hit["skip"] + 1
        if c.dc_sign_ctx == 2 and k % 3:
            descs["dc_sign_ctx"][k], hit["sign"] = 3 + k % 250, hit["sign"] + 1
        if blocks[i].eob0 == n and c.perform:
            results["eob"][k], hit["eob"] = n + 1 + k, hit["eob"] + 1
    assert min(hit.values()) >= 3, hit
    for off in {int(d["iscan_off"]) for d in tdescs}:      # iscan + a multiple of n that keeps it a positive int16
        arena[off:off + 2 * n].view(np.int16)[:] += np.int16((16384 // n) * n)
    for mapping in mappings(w, h):
        check(gold, blocks, idx, arena, regions, tdescs, results, *launch(hip, gold, arena, tdescs, descs, results, w, h, mapping))


@pytest.mark.parametrize("w, h", [(4, 8), (16, 16), (32, 64)], ids=lambda v: str(v))
def test_unflagged_blocks_are_left_alone(hip, gold, blocks, w, h):
    """Without SVT_HIP_RDOQ_PERFORM a block keeps its arrays and its eob in d_txfm_result whatever else its descriptor says; it gets
    cul_level, and an eob above the retained count is clamped in d_out only."""
    idx, arena, tdescs, descs, results, regions = R.batch(blocks, w, h)
    descs["flags"] &= ~np.uint8(abi.RDOQ_PERFORM)
    n = min(w, 32) * min(h, 32)
    results["eob"][::5] = n + 7
    got_arena, out, got_results = launch(hip, gold, arena, tdescs, descs, results, w, h)
    check_containment(arena, got_arena, regions, [], "svt_hip_rdoq_batch")
    assert got_results.tobytes() == results.tobytes()
    for k, i in enumerate(idx):
        b = blocks[i]
        eob = min(int(results["eob"][k]), n)
        want = (eob, R.cul_level(b.q0.tolist(), T.scan_of(b.iscan).tolist(), eob), abi.RDOQ_PATH_NOT_FLAGGED)
        assert (int(out["eob"][k]), int(out["cul_level"][k]), int(out["path"][k])) == want, (i, b.c)


@pytest.mark.parametrize("w, h", [(4, 4), (16, 8), (32, 32)], ids=lambda v: str(v))
def test_zero_at_the_last_position_is_refused(hip, gold, blocks, w, h):
    """The reference asserts qcoeff[scan[eob - 1]] != 0 at the start of the trellis.  A block that breaks it keeps arrays and eob,
    gets cul_level and PATH_TRELLIS | PATH_BAD_EOB (include/svt_hip_txfm.h); its neighbours in the launch are not disturbed."""
    idx, arena, tdescs, descs, results, regions = R.batch(blocks, w, h)
    broken = []
    for k, i in enumerate(idx):
        b = blocks[i]
        plain = b.path == abi.RDOQ_PATH_TRELLIS and not b.c.fast and b.c.eob_fast_th == 255 and b.eob0 >= 2
        if plain and len(broken) < 12 and k % 2:
            last = T.scan_of(b.iscan)[b.eob0 - 1]
            i32(arena, tdescs[k]["qcoeff_off"], len(b.q))[last] = 0
            broken.append(k)
    assert len(broken) >= 5
    got_arena, out, got_results = launch(hip, gold, arena, tdescs, descs, results, w, h, mapping=(2, 1, 0)[(w > 4) + (w > 16)])
    for k, i in enumerate(idx):
        b, d, n = blocks[i], tdescs[k], len(blocks[i].q)
        if k in broken:
            q = i32(arena, d["qcoeff_off"], n)
            assert np.array_equal(i32(got_arena, d["qcoeff_off"], n), q) and np.array_equal(i32(got_arena, d["dqcoeff_off"], n), b.dq0), (i, b.c)
            want = (b.eob0, R.cul_level(q.tolist(), T.scan_of(b.iscan).tolist(), b.eob0), abi.RDOQ_PATH_TRELLIS | abi.RDOQ_PATH_BAD_EOB)
            assert (int(out["eob"][k]), int(out["cul_level"][k]), int(out["path"][k])) == want, (i, b.c, out[k])
            assert int(got_results["eob"][k]) == b.eob0
        else:
            assert np.array_equal(i32(got_arena, d["qcoeff_off"], n), b.q) and np.array_equal(i32(got_arena, d["dqcoeff_off"], n), b.dq), (i, b.c)
            assert (int(out["eob"][k]), int(out["cul_level"][k]), int(out["path"][k])) == (b.eob, b.cul, b.path), (i, b.c)
    check_containment(arena, got_arena, regions, [(int(d[f]), 4 * len(blocks[i].q)) for d, i in zip(tdescs, idx) for f in ("qcoeff_off", "dqcoeff_off")],
                      "svt_hip_rdoq_batch_mapped")


@pytest.mark.parametrize("w, h", [(4, 4), (16, 8), (16, 64), (64, 64)], ids=lambda v: str(v))
def test_chain_of_five_launches(hip, orc, gold, w, h):
    """svt_hip_txfm_quant_batch (FWD + QUANT_FP[_HBD] + SATD) -> svt_hip_rdoq_batch -> svt_hip_txfm_quant_batch (INV only, its own result
    array) -> svt_hip_txfm_distortion_batch -> svt_hip_txb_cost_batch on one stream.  Equal to the oracle's forward transform and FP
    quantiser fed through the restatement, then the oracle's inverse, the distortion on the host, restate_bits and rd_cost."""
    rng = np.random.default_rng(w * 1000 + h)
    iw, ih = T.retained(w, h)
    n, n_tb, ls = iw * ih, 9, T.tx_scale(w, h)
    types = T.size_types(w, h)
    ab = Arena(fill=PATTERN)
    iscan_off = {t: ab.add(f"iscan {t}", gold.iscan(w, h, t)) for t in types}
    fwd, inv = np.zeros(n_tb, abi.TXFM_DESC_DTYPE), np.zeros(n_tb, abi.TXFM_DESC_DTYPE)
    rdescs, cdescs = np.zeros(n_tb, abi.RDOQ_DESC_DTYPE), np.zeros(n_tb, abi.TXB_COST_DESC_DTYPE)
    want = []
    for i in range(n_tb):
        bd, tt = R.BIT_DEPTHS[i % 2], types[i % len(types)]
        c = R.Case("chain", w, h, tt, plane=i % 2, is_inter=(i // 2) % 2, bd=bd, table=i % 2, qm=0, lam=R.LAMBDAS[1 + i % 5], skip_ctx=(0, 5, 12)[i % 3],
                   dc_sign_ctx=i % 3, perform=int(i != 7), fast=int(i == 3), sharp=0, eob_th=(255, 85)[i == 6], eob_fast_th=(255, 30)[i == 4], satd_factor=255,
                   early_exit_th=0, sq_size=16, fp_q=1, eob=0, dc="", recipe="", pic_bd=bd)
        qt = gold.qt(c)
        iscan = gold.iscan(w, h, tt)
        pix16 = bd > 8
        res = (tx_cases.residual(rng, w, h, bd, 0, pad=5) // (1, 3, 9, 40, 150)[i % 5]).astype(np.int16)
        if i == 5:
            res[:] = 0                                  # eob 0
        pred16 = rng.integers(0, 1 << bd, size=(h, w + 2)).astype(np.uint16)
        d = fwd[i]
        d["residual_off"], d["residual_stride"] = ab.add(f"residual {i}", res), w + 5
        d["coeff_off"], d["qcoeff_off"], d["dqcoeff_off"] = ab.add(f"coeff {i}", nbytes=n * 4), ab.add(f"qcoeff {i}", nbytes=n * 4), ab.add(f"dqcoeff {i}", nbytes=n * 4)
        d["pred_off"] = ab.add(f"pred {i}", pred16 if pix16 else pred16.astype(np.uint8))
        d["recon_off"] = ab.add(f"recon {i}", nbytes=h * (w + 4) * (2 if pix16 else 1))
        d["pred_stride"], d["recon_stride"] = w + 2, w + 4
        d["iscan_off"], d["qm_off"], d["iqm_off"] = iscan_off[tt], abi.NO_OFFSET, abi.NO_OFFSET
        d["zbin"], d["round"], d["quant"], d["quant_shift"], d["dequant"] = qt["zbin"][:2], qt["round_fp"][:2], qt["quant_fp"][:2], qt["qshift"][:2], qt["dequant"][:2]
        mode = abi.QUANT_FP_HBD if pix16 else abi.QUANT_FP
        d["tx_type"], d["bit_depth"], d["quant_mode"], d["log_scale"] = tt, bd, mode, ls
        d["flags"] = abi.TX_FWD | abi.TX_SATD | (abi.TX_PIXEL16 if pix16 else 0)
        inv[i] = d
        inv[i]["quant_mode"], inv[i]["flags"] = abi.QUANT_NONE, abi.TX_INV | (abi.TX_PIXEL16 if pix16 else 0)
        r = rdescs[i]
        r["table"], r["lambda"], r["early_exit_limit"] = c.table, c.lam, R.early_exit_limit(c)
        r["zbin"], r["round"], r["quant"], r["quant_shift"] = qt["zbin"][:2], qt["round"][:2], qt["quant"][:2], qt["qshift"][:2]
        r["plane_type"], r["txb_skip_ctx"], r["dc_sign_ctx"], r["is_inter"] = c.plane, c.skip_ctx, c.dc_sign_ctx, c.is_inter
        r["eob_th"], r["eob_fast_th"], r["satd_factor"], r["dequant_shift"] = c.eob_th, c.eob_fast_th, c.satd_factor, R.dequant_shift(c)
        r["flags"] = abi.RDOQ_PERFORM * c.perform | abi.RDOQ_FAST_MODE * c.fast
        tc = T.Case("chain", w, h, tt, c.plane, 0xFFFF, c.skip_ctx, c.dc_sign_ctx, T.NEARESTMV if c.is_inter else 0, T.FILTER_INTRA_NONE, 0, 1 + i % 3, i % 2, 0, 0,
                    c.table, c.lam, "", 0, 0)
        k = cdescs[i]
        k["qcoeff_off"], k["iscan_off"], k["table"], k["lambda"], k["eob"] = d["qcoeff_off"], d["iscan_off"], tc.table, tc.lam, tc.eob
        k["tx_type"], k["plane_type"], k["txb_skip_ctx"], k["dc_sign_ctx"], k["pred_mode"] = tt, tc.plane, tc.skip_ctx, tc.dc_sign_ctx, tc.pred_mode
        k["filter_intra_mode"], k["fast_coeff_est_level"], k["subres_step"] = tc.fim, tc.fast, tc.step
        # the oracle's pipeline
        co = np.zeros(w * h, np.int32)
        orc.orc_fwd_txfm2d(tx_cases.P(res), tx_cases.P(co), C.c_uint32(w + 5), w, h, tt, bd, 0)
        energy = 0
        if max(w, h) == 64:
            orc.orc_handle_transform64.restype = C.c_uint64
            energy = orc.orc_handle_transform64(tx_cases.P(co), w, h)
        co = co[:n].copy()
        q0, dq0, eob0 = R.quant(orc, mode, c, co, iscan, qt, None, None)
        satd = int(np.abs(co.astype(np.int64)).sum())
        q, dq, eob, cul, path = R.restate(c, gold.tables[c.table], co, mode, q0, dq0, eob0, satd, iscan, qt, None, None,
                                          lambda: R.quant(orc, abi.QUANT_B_HBD if pix16 else abi.QUANT_B, c, co, iscan, qt, None, None))
        rec = np.zeros((h, w + 4), np.uint16)
        orc.orc_inv_txfm2d_add(tx_cases.P(dq), tx_cases.P(pred16), w + 2, tx_cases.P(rec), w + 4, w, h, tt, bd)
        dist = int(((co.astype(np.int64) - dq) ** 2).sum())
        bits = T.restate_bits(gold.tables[tc.table], tc, q, iscan, eob=eob)
        want.append(dict(q=q, dq=dq, eob=eob, cul=cul, path=path, rec=rec if pix16 else rec.astype(np.uint8), bits=bits,
                         rd=T.rd_cost(w, h, tc.lam, bits, tc.step, dist, energy), changed=not np.array_equal(q, q0), satd=satd, energy=energy))
    ways = {x["path"] & abi.RDOQ_PATH_MASK for x in want}
    assert ways >= {abi.RDOQ_PATH_NOT_FLAGGED, abi.RDOQ_PATH_EOB_ZERO, abi.RDOQ_PATH_TRELLIS} and any(x["changed"] for x in want)
    arena = ab.build()
    d_arena, d_fwd, d_inv = device.DeviceBuffer(hip, arena.nbytes + 256), device.upload_descriptors(hip, fwd), device.upload_descriptors(hip, inv)
    d_arena.upload(arena)
    d_res, d_res_inv, d_dist = (device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_tb), device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_tb),
                                device.DeviceBuffer(hip, 16 * n_tb))
    device.check(hip, hip.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_res.ptr), n_tb, w, h, None), "svt_hip_txfm_quant_batch")
    out, guard = device.rdoq_batch(hip, d_arena.ptr, d_fwd.ptr, rdescs, gold.tables, d_res.ptr, w, h)
    assert (guard == GUARD).all()
    device.check(hip, hip.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_inv.ptr), V(d_res_inv.ptr), n_tb, w, h, None), "svt_hip_txfm_quant_batch (INV)")
    device.check(hip, hip.svt_hip_txfm_distortion_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_dist.ptr), n_tb, w, h, None), "svt_hip_txfm_distortion_batch")
    cost, guard = device.txb_cost_batch(hip, d_arena.ptr, cdescs, gold.tables, w, h, d_txfm_result=d_res.ptr, d_distortion=d_dist.ptr)
    assert (guard == GUARD).all()
    got = d_arena.download(np.uint8, (arena.nbytes,))
    res = d_res.download(np.dtype(abi.TXFM_RESULT_DTYPE), (n_tb,))
    for i, x in enumerate(want):
        d = fwd[i]
        assert np.array_equal(i32(got, d["qcoeff_off"], n), x["q"]) and np.array_equal(i32(got, d["dqcoeff_off"], n), x["dq"]), i
        assert (int(out["eob"][i]), int(out["cul_level"][i]), int(out["path"][i])) == (x["eob"], x["cul"], x["path"]), (i, out[i])
        assert (int(res["eob"][i]), int(res["satd"][i]), int(res["three_quad_energy"][i])) == (x["eob"], x["satd"], x["energy"]), i
        pix = np.uint16 if d["flags"] & abi.TX_PIXEL16 else np.uint8
        rec = got[int(d["recon_off"]):int(d["recon_off"]) + h * (w + 4) * np.dtype(pix).itemsize].view(pix).reshape(h, w + 4)
        assert np.array_equal(rec[:, :w], x["rec"][:, :w]), ("recon", i)
    assert [(int(b), int(r)) for b, r in zip(cost["bits"], cost["rd_cost"])] == [(x["bits"], x["rd"]) for x in want]
    declared = [(int(d[f]), 4 * n) for d in fwd for f in ("coeff_off", "qcoeff_off", "dqcoeff_off")]
    for d in fwd:
        px = 2 if d["flags"] & abi.TX_PIXEL16 else 1
        declared += rows(int(d["recon_off"]), (w + 4) * px, w * px, h)
    check_containment(arena, got, ab.regions, declared, "the chain of five launches")
