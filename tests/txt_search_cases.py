"""TEST INFRASTRUCTURE — cases, Python restatement and arena / descriptor builders for the transform-type search of a transform block
(svt_hip_txt_select_batch, svt_hip_txfm_spatial_distortion_batch and svt_hip_txt_search_batch, include/svt_hip_txfm.h).

The search is tx_type_search (product_coding_loop.c:4458-4940).  Its per-candidate stages are restated elsewhere and composed here: the
oracle's forward transform, quantisers and inverse (tx_cases), the RDOQ stage (rdoq_cases.restate) and the coefficient rate
(txb_cost_cases.restate_bits); what this file restates is the loop's decision (decide) and the spatial distortion.  Two kinds of cases:
  SEARCH_CASES   whole searches from seeded pixels, one list per transform size,
  synthetic()    select-only blocks over made-up per-candidate records with small value ranges, so that ties and every exit are common."""
import collections
import ctypes as C
import os

import numpy as np

import rdoq_cases as R
import tx_cases
import txb_cost_cases as T
from arena import PATTERN, Arena, rows
from svtav1_hip import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "txt_search.npz")
M64 = (1 << 64) - 1
DCT_DCT = 0
# tx_type_group / tx_type_group_sc (definitions.h:1007-1034) as lists of TxType
TX_TYPE_GROUP = ((0,), (10, 11), (3,), (1, 2), (6, 9), (4, 5, 7, 8, 12, 13, 14, 15))
TX_TYPE_GROUP_SC = ((0, 9), (10, 11), (3,), (1, 2), (6,), (4, 5, 7, 8, 12, 13, 14, 15))
EXITS = ("rate", "satd", "early_cost", "group")   # the four data-dependent exits of the loop
SEARCH_SIZES = ((4, 4), (4, 16), (16, 4), (8, 8), (16, 16), (16, 8), (32, 32), (64, 64))


def rdcost(lam, rate, dist):
    """RDCOST (rd_cost.h:37) as the uint64_t the loop compares"""
    return (((rate * lam + 256) >> 9) + dist * 128) & M64


def i32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def candidate_order(w, h, is_inter, reduced, sc, n_groups):
    """The transform types tx_type_search visits, in its order: the first n_groups rows of tx_type_group[_sc] without the types
    av1_ext_tx_used refuses -> (types, group_start mask: bit k set where candidate k is the first its group visits)."""
    used = T.EXT_TX_USED[T.ext_tx_set_type(w, h, is_inter, reduced)]
    types, mask = [], 0
    for group in (TX_TYPE_GROUP_SC if sc else TX_TYPE_GROUP)[:n_groups]:
        kept = [t for t in group if t == DCT_DCT or t in used]
        if kept:
            mask |= 1 << len(types)
            types += kept
    return types, mask


RateKey = collections.namedtuple("RateKey", "w h tx_type pred_mode fim reduced")


def form_distortion(w, h, raw, energy, step, spatial):
    """One entry of the distortion pair as the loop uses it (:4717-4749): the spatial figure as it is, the transform-domain one with the
    64-point energy added and the scale shift applied"""
    if spatial:
        return int(raw)
    shift = (1 - T.tx_scale(w, h)) * 2
    d = (int(raw) + int(energy)) & M64
    return ((((d << -shift) if shift < 0 else (d >> shift)) << step)) & M64


def decide(tables, w, h, b, cdescs, results, rdoq, dist, cost, disable=()):
    """The loop of tx_type_search (:4581-4812) for the block b (one record of abi.TXT_DESC_DTYPE) over the per-candidate record arrays
    cdescs (abi.TXB_COST_DESC_DTYPE), results (abi.TXFM_RESULT_DTYPE), rdoq (abi.RDOQ_RESULT_DTYPE or None), dist (uint64 [n][2]) and cost
    (abi.TXB_COST_DTYPE), in Python integers.  disable: exits of EXITS that are taken out (what the case conditions are counted with).
    -> the fields of SvtHipTxtResult, and `tie` (two compared candidates share the winning cost), `rate_before_dct` (the rate-cost test ran
    while dct_dct_cost was still ~0)."""
    n_total = len(cdescs)
    first = int(b["first_cand"])
    n = 0 if first >= n_total else min(int(b["n_cand"]), abi.TXT_MAX_CAND, n_total - first)
    lam, flags = int(b["full_lambda"]), int(b["flags"])
    satd_th, rate_th = int(b["satd_early_exit_th"]), int(b["txt_rate_cost_th"])
    coeff_th, dist_th = int(b["early_exit_coeff_th"]), int(b["early_exit_dist_th"])
    spatial = bool(flags & abi.TXT_SPATIAL_SSE)
    best_cost = dct_cost = M64
    best_satd, best_non_coeff = (1 << 31) - 1, 64 * 64
    r = dict(tx_type=DCT_DCT, cand=abi.TXT_NO_CAND, eob=0, cul_level=0, bits=0, distortion=(0, 0), quant_mask=0, cost_mask=0, tie=False,
             rate_before_dct=False)
    cost_th = rdcost(lam, 1, (int(b["tx_pixels"]) * dist_th) & 0xFFFFFFFF) if dist_th else 0
    compared = []
    for k in range(n):
        i = first + k
        cd = cdescs[i]
        tx_type = int(cd["tx_type"]) & 15
        if (int(b["group_start"]) >> k) & 1:
            best_non_coeff = 64 * 64
        if tx_type != DCT_DCT and rate_th:
            t = tables[min(int(cd["table"]), len(tables) - 1)]
            rate = T.tx_type_rate(t, RateKey(w, h, tx_type, int(cd["pred_mode"]), int(cd["filter_intra_mode"]), int(cd["reduced_tx_set"])))
            r["rate_before_dct"] |= dct_cost == M64
            if "rate" not in disable and (rdcost(lam, rate, 0) * 1000) & M64 > (dct_cost * rate_th) & M64:
                continue
        res = results[i]
        if satd_th:
            satd = i32(int(res["satd"]))
            if satd < best_satd:
                best_satd = satd
            elif "satd" not in disable and i32((satd - best_satd) * 100) > i32(best_satd * satd_th):
                continue
        r["quant_mask"] |= 1 << k
        eob = int(res["eob"])
        if eob == 0 and tx_type != DCT_DCT:
            continue
        step = min(int(cd["subres_step"]), 2)
        dr, dp = (form_distortion(w, h, dist[i][j], res["three_quad_energy"], step, spatial) for j in (0, 1))
        if "early_cost" not in disable and rdcost(lam, 0, dr) > best_cost:
            continue
        r["cost_mask"] |= 1 << k
        bits = int(cost[i]["bits"])
        c = rdcost(lam, bits, dr)
        compared.append(c)
        if c < best_cost:
            best_cost, best_non_coeff = c, eob
            r.update(tx_type=tx_type, cand=k, eob=eob, bits=bits, distortion=(dr, dp), cul_level=int(rdoq[i]["cul_level"]) if rdoq is not None else 0)
            if tx_type == DCT_DCT:
                dct_cost = c
        if flags & abi.TXT_EARLY_EXIT and "group" not in disable and (best_non_coeff < coeff_th or best_cost < cost_th):
            break
    r["cost"] = best_cost
    r["tie"] = compared.count(best_cost) >= 2
    return r


RESULT_FIELDS = ("tx_type", "cand", "eob", "cul_level", "bits", "cost", "quant_mask", "cost_mask")


def same_record(got, want):
    """A downloaded SvtHipTxtResult record against decide()'s"""
    return all(int(got[f]) == want[f] for f in RESULT_FIELDS) and tuple(int(v) for v in got["distortion"]) == tuple(want["distortion"]) and \
        not np.asarray(got["pad_"]).any()


# ------------------------------------------------------------------------------------------------ select only: synthetic records
Synthetic = collections.namedtuple("Synthetic", "w h descs cdescs results rdoq dist cost")


def synthetic(gold, seed, n_blocks, counts, w=4, h=4, n_extra=3):
    """n_blocks blocks of w x h whose candidate counts take `counts` in turn, with ragged first_cand (a few unused records between
    blocks, n_extra behind the last) and per-candidate records drawn from small ranges: few distinct bits, distortions, eobs and SATDs,
    so that equal costs and every exit are common.  Every fourth block lists a type other than DCT_DCT first."""
    rng = np.random.default_rng(seed)
    descs = np.zeros(n_blocks, abi.TXT_DESC_DTYPE)
    firsts, at = [], 0
    for k in range(n_blocks):
        at += int(rng.integers(0, 3))
        firsts.append(at)
        at += counts[k % len(counts)]
    n_cand = at + n_extra
    cdescs, results = np.zeros(n_cand, abi.TXB_COST_DESC_DTYPE), np.zeros(n_cand, abi.TXFM_RESULT_DTYPE)
    rdoq, cost = np.zeros(n_cand, abi.RDOQ_RESULT_DTYPE), np.zeros(n_cand, abi.TXB_COST_DTYPE)
    dist = np.zeros((n_cand, 2), np.uint64)
    cdescs["tx_type"] = rng.integers(0, 16, n_cand)
    cdescs["table"] = rng.integers(0, len(gold.tables) + 1, n_cand)          # one beyond the sets: clamped
    cdescs["filter_intra_mode"] = T.FILTER_INTRA_NONE
    results["eob"] = rng.choice((0, 1, 1, 2, 3, 5), n_cand)
    results["satd"] = rng.choice((40, 44, 48, 60, 90), n_cand)
    if max(w, h) == 64:
        results["three_quad_energy"] = rng.choice((0, 16, 64), n_cand)
    rdoq["cul_level"], rdoq["eob"] = rng.integers(0, 256, n_cand), results["eob"]
    cost["bits"], cost["rd_cost"] = rng.choice((512, 1024, 1536, 2048), n_cand), 0x5A5A
    dist[:] = rng.choice((0, 64, 128, 192, 256), (n_cand, 2))
    for k in range(n_blocks):
        b, n = descs[k], counts[k % len(counts)]
        b["first_cand"], b["n_cand"] = firsts[k], n
        if k % 4 != 3:
            cdescs["tx_type"][firsts[k]] = DCT_DCT
        elif cdescs["tx_type"][firsts[k]] == DCT_DCT:
            cdescs["tx_type"][firsts[k]] = 9
        cdescs["pred_mode"][firsts[k]:firsts[k] + n] = T.NEARESTMV if k % 2 else int(rng.integers(0, 13))
        b["group_start"] = 1 | int(rng.integers(0, 1 << 16))
        b["full_lambda"] = int(rng.choice((300, 1000, 4000)))
        b["satd_early_exit_th"] = int(rng.choice((0, 5, 20, 60)))
        b["txt_rate_cost_th"] = int(rng.choice((0, 100, 250, 600)))
        b["early_exit_coeff_th"], b["early_exit_dist_th"] = int(rng.choice((0, 1, 2, 4))), int(rng.choice((0, 1, 3, 5)))
        b["tx_pixels"] = w * h
        b["flags"] = int(rng.integers(0, 4))
        b["src_off"] = b["dst_qcoeff_off"] = b["dst_dqcoeff_off"] = b["dst_recon_off"] = abi.NO_OFFSET
    return Synthetic(w, h, descs, cdescs, results, rdoq, dist, cost)


def synthetic_expected(gold, s, disable=()):
    return [decide(gold.tables, s.w, s.h, b, s.cdescs, s.results, s.rdoq, s.dist, s.cost, disable) for b in s.descs]


def synthetic_sets(gold):
    """The select-only inputs of the CPU conditions and the GPU tests: candidate counts 1, 2 and 16 and a ragged mix; 1, 63 and 65 blocks"""
    return [synthetic(gold, 11, 1, (1,)), synthetic(gold, 12, 1, (16,)), synthetic(gold, 13, 63, (2,)), synthetic(gold, 14, 65, (16,)),
            synthetic(gold, 15, 65, (1, 5, 16, 2, 3, 9, 4)), synthetic(gold, 16, 63, (7, 1, 12, 2), w=8, h=8),
            synthetic(gold, 17, 65, (3, 16, 6), w=64, h=16), synthetic(gold, 18, 65, (4, 8, 11)), synthetic(gold, 19, 63, (16, 13), w=16, h=16)]


# ------------------------------------------------------------------------------------------------ the whole search
SearchCase = collections.namedtuple("SearchCase", "w h bd is_inter spatial rdoq sc n_groups table lam div satd_th rate_th coeff_th dist_th early crop "
                                                  "own_dst seed")
LAMBDAS = (900, 20000, 500000)


def _search_cases():
    out = []
    per_size = {(4, 4): 16, (8, 8): 12, (4, 16): 8, (16, 4): 8, (16, 8): 8, (16, 16): 8, (32, 32): 6, (64, 64): 4}
    for w, h in SEARCH_SIZES:
        for k in range(per_size[(w, h)]):
            i = len(out)
            out.append(SearchCase(w, h, bd=R.BIT_DEPTHS[k % 2], is_inter=(k // 2) % 2, spatial=(k // 4) % 2 if k >= 4 else k % 2, rdoq=int(k % 3 != 2),
                                  sc=int(k % 5 == 3), n_groups=(6, 6, 4, 2, 5, 1)[k % 6], table=(k // 3) % 2, lam=LAMBDAS[i % 3], div=(3, 9, 40, 150)[k % 4],
                                  satd_th=(0, 5, 30, 12)[(k // 2) % 4], rate_th=(0, 60, 250)[k % 3], coeff_th=(0, 2, 8)[(k // 2) % 3],
                                  dist_th=(0, 40, 400)[(k // 3) % 3], early=int(k % 4 != 1), crop=int(k % 4 == 2), own_dst=int(k % 2), seed=7000 + i))
    return out


SEARCH_CASES = _search_cases()


def digest_pixels(a):
    return R.digest(np.ascontiguousarray(a).astype(np.int32))


def iscan_of(gold, w, h, tx_type):
    """The scan of a transform type is its class's (tests/test_rdoq_abi.py::test_neighbours_follow_in_every_scan_of_the_reference); the
    fixture holds one type per class"""
    for t in T.size_types(w, h):
        if T.tx_class(t) == T.tx_class(tx_type):
            return gold.iscan(w, h, t)
    raise KeyError((w, h, tx_type))


class Search:
    """The SEARCH_CASES of one size as one svt_hip_txt_search_batch launch, and what the oracle's stages and the restated decision make
    of every block.  order: a permutation of the blocks."""

    def __init__(self, gold, orc, w, h, order=None):
        self.w, self.h = w, h
        self.case_index = [i for i, c in enumerate(SEARCH_CASES) if (c.w, c.h) == (w, h)]
        if order is not None:
            self.case_index = [self.case_index[k] for k in order(len(self.case_index))]
        cases = self.cases = [SEARCH_CASES[i] for i in self.case_index]
        iw, ih = T.retained(w, h)
        n, ls = iw * ih, T.tx_scale(w, h)
        self.n = n
        plan = [candidate_order(w, h, c.is_inter, 0, c.sc, c.n_groups) for c in cases]
        n_cand = sum(len(p[0]) for p in plan)
        ab = Arena(fill=PATTERN)
        shared = {}
        self.tdescs, self.rdescs = np.zeros(n_cand, abi.TXFM_DESC_DTYPE), np.zeros(n_cand, abi.RDOQ_DESC_DTYPE)
        self.cdescs, self.descs = np.zeros(n_cand, abi.TXB_COST_DESC_DTYPE), np.zeros(len(cases), abi.TXT_DESC_DTYPE)
        results, rdoq = np.zeros(n_cand, abi.TXFM_RESULT_DTYPE), np.zeros(n_cand, abi.RDOQ_RESULT_DTYPE)
        dist, cost = np.zeros((n_cand, 2), np.uint64), np.zeros(n_cand, abi.TXB_COST_DTYPE)
        self.cand, self.written, self.inputs = [], [], []          # per candidate what the chain leaves; (offset, bytes) the call may write
        at = 0
        for bi, (c, (types, mask)) in enumerate(zip(cases, plan)):
            rng, ci = np.random.default_rng(c.seed), self.case_index[bi]      # what varies from case to case goes by ci, not by the place in the batch
            pix16 = c.bd > 8
            pix = np.uint16 if pix16 else np.uint8
            ps, ss, rs, res_stride = w + 3, w + 7, w + 5, w + 1            # odd strides
            pred = rng.integers(0, 1 << c.bd, size=(h, ps))
            src = np.clip(pred[:, :w] + rng.integers(-(1 << c.bd), 1 << c.bd, size=(h, w)) // c.div, 0, (1 << c.bd) - 1)
            src = np.concatenate([src, rng.integers(0, 1 << c.bd, size=(h, ss - w))], axis=1)
            res = np.zeros((h, res_stride), np.int16)
            res[:, :w] = src[:, :w] - pred[:, :w]
            skew = pix().itemsize * (1 + ci % 3)                          # pixel planes off their 256-byte boundaries
            pred_off = ab.add(f"pred of block {bi}", pred.astype(pix), skew=skew)
            src_off = ab.add(f"src of block {bi}", src.astype(pix), skew=skew)
            res_off = ab.add(f"residual of block {bi}", res)
            pred_mode = T.NEARESTMV if c.is_inter else (0, 1, 9)[ci % 3]
            cw, ch = (max(1, w - 1 - ci % 3), max(1, h - 2)) if c.crop else (w, h)
            self.inputs.append(dict(res=res, pred=pred.astype(pix), src=src.astype(pix), strides=(res_stride, ps, ss, rs), crop=(cw, ch), pred_mode=pred_mode))
            rc = R.Case("txt", w, h, 0, plane=0, is_inter=c.is_inter, bd=c.bd, table=c.table, qm=0, lam=c.lam, skip_ctx=0, dc_sign_ctx=0, perform=c.rdoq,
                        fast=0, sharp=0, eob_th=255, eob_fast_th=255, satd_factor=255, early_exit_th=0, sq_size=16, fp_q=1, eob=0, dc="", recipe="",
                        pic_bd=c.bd)
            qt = gold.qt(rc)
            fp = bool(c.rdoq)
            mode = (abi.QUANT_FP_HBD if pix16 else abi.QUANT_FP) if fp else (abi.QUANT_B_HBD if pix16 else abi.QUANT_B)
            b = self.descs[bi]
            b["first_cand"], b["n_cand"], b["group_start"] = at, len(types), mask
            b["src_off"], b["src_stride"], b["crop_w"], b["crop_h"] = src_off, ss, cw if c.crop else 0, ch if c.crop else 0
            b["full_lambda"], b["satd_early_exit_th"], b["txt_rate_cost_th"] = c.lam, c.satd_th, c.rate_th
            b["early_exit_coeff_th"], b["early_exit_dist_th"], b["tx_pixels"] = c.coeff_th, c.dist_th, w * h
            b["flags"] = abi.TXT_EARLY_EXIT * c.early | abi.TXT_SPATIAL_SSE * c.spatial
            for k, tt in enumerate(types):
                i = at + k
                iscan = iscan_of(gold, w, h, tt)
                key = ("iscan", T.tx_class(tt))
                if key not in shared:
                    shared[key] = ab.add(f"iscan of class {key[1]}", iscan)
                d = self.tdescs[i]
                d["residual_off"], d["residual_stride"] = res_off, res_stride
                d["coeff_off"], d["qcoeff_off"], d["dqcoeff_off"] = (ab.add(f"{f} of candidate {i}", nbytes=n * 4) for f in ("coeff", "qcoeff", "dqcoeff"))
                d["pred_off"], d["pred_stride"], d["recon_off"], d["recon_stride"] = pred_off, ps, ab.add(f"recon of candidate {i}", nbytes=h * rs * pix().itemsize), rs
                d["iscan_off"], d["qm_off"], d["iqm_off"] = shared[key], abi.NO_OFFSET, abi.NO_OFFSET
                d["zbin"], d["round"], d["quant"] = qt["zbin"][:2], qt["round_fp" if fp else "round"][:2], qt["quant_fp" if fp else "quant"][:2]
                d["quant_shift"], d["dequant"] = qt["qshift"][:2], qt["dequant"][:2]
                d["tx_type"], d["bit_depth"], d["quant_mode"], d["log_scale"] = tt, c.bd, mode, ls
                d["flags"] = abi.TX_FWD | abi.TX_SATD | (abi.TX_PIXEL16 if pix16 else 0)
                self.written += [(int(d["coeff_off"]), n * 4), (int(d["qcoeff_off"]), n * 4), (int(d["dqcoeff_off"]), n * 4)]
                self.written += rows(int(d["recon_off"]), rs * pix().itemsize, w * pix().itemsize, h)
                r = self.rdescs[i]
                cc = rc._replace(tx_type=tt)
                r["table"], r["lambda"], r["early_exit_limit"] = c.table, c.lam, R.early_exit_limit(cc)
                r["zbin"], r["round"], r["quant"], r["quant_shift"] = qt["zbin"][:2], qt["round"][:2], qt["quant"][:2], qt["qshift"][:2]
                r["is_inter"], r["eob_th"], r["eob_fast_th"], r["satd_factor"], r["dequant_shift"] = c.is_inter, 255, 255, 255, R.dequant_shift(cc)
                r["flags"] = abi.RDOQ_PERFORM * c.rdoq
                tc = T.Case("txt", w, h, tt, 0, 0xFFFF, 0, 0, pred_mode, T.FILTER_INTRA_NONE, 0, 1, 0, 0, 0, c.table, c.lam,
                            "", 0, 0)
                kd = self.cdescs[i]
                kd["qcoeff_off"], kd["iscan_off"], kd["table"], kd["lambda"], kd["eob"] = d["qcoeff_off"], d["iscan_off"], tc.table, tc.lam, tc.eob
                kd["tx_type"], kd["pred_mode"], kd["filter_intra_mode"], kd["fast_coeff_est_level"] = tt, tc.pred_mode, tc.fim, tc.fast
                # the oracle's stages
                co = np.zeros(w * h, np.int32)
                orc.orc_fwd_txfm2d(tx_cases.P(res), tx_cases.P(co), C.c_uint32(res_stride), w, h, tt, c.bd, 0)
                energy = 0
                if max(w, h) == 64:
                    orc.orc_handle_transform64.restype = C.c_uint64
                    energy = orc.orc_handle_transform64(tx_cases.P(co), w, h)
                co = co[:n].copy()
                q0, dq0, eob0 = R.quant(orc, mode, cc, co, iscan, qt, None, None)
                satd = int(np.abs(co.astype(np.int64)).sum())
                q, dq, eob, cul, _ = R.restate(cc, gold.tables[c.table], co, mode, q0, dq0, eob0, satd, iscan, qt, None, None,
                                               lambda: R.quant(orc, abi.QUANT_B_HBD if pix16 else abi.QUANT_B, cc, co, iscan, qt, None, None))
                rec, pred16, dq = np.zeros((h, rs), np.uint16), pred.astype(np.uint16), np.ascontiguousarray(dq, np.int32)
                orc.orc_inv_txfm2d_add(tx_cases.P(dq), tx_cases.P(pred16), ps, tx_cases.P(rec), rs, w, h, tt, c.bd)
                rec = rec[:, :w].astype(np.int64)
                if c.spatial:
                    s = src[:ch, :cw].astype(np.int64)
                    dist[i] = (int(((s - rec[:ch, :cw]) ** 2).sum()) << 4, int(((s - pred[:ch, :cw]) ** 2).sum()) << 4)
                else:
                    dist[i] = (int(((co.astype(np.int64) - dq) ** 2).sum()), int((co.astype(np.int64) ** 2).sum()))
                results[i]["three_quad_energy"], results[i]["eob"], results[i]["satd"] = energy, eob, satd
                rdoq[i]["eob"], rdoq[i]["cul_level"] = eob, cul
                cost[i]["bits"] = T.restate_bits(gold.tables[tc.table], tc, q, iscan, eob=eob)
                self.cand.append(dict(q=q, dq=dq, rec=rec.astype(pix)))
            # the winner's destinations: the DCT_DCT candidate's own arrays (the reference's cand_bf), or arrays of their own
            dct = at + types.index(DCT_DCT)
            if c.own_dst:
                b["dst_qcoeff_off"], b["dst_dqcoeff_off"] = ab.add(f"dst qcoeff of block {bi}", nbytes=n * 4), ab.add(f"dst dqcoeff of block {bi}", nbytes=n * 4)
                b["dst_recon_off"], b["dst_recon_stride"] = ab.add(f"dst recon of block {bi}", nbytes=h * (w + 9) * pix().itemsize), w + 9
            else:
                b["dst_qcoeff_off"], b["dst_dqcoeff_off"] = self.tdescs[dct]["qcoeff_off"], self.tdescs[dct]["dqcoeff_off"]
                b["dst_recon_off"], b["dst_recon_stride"] = self.tdescs[dct]["recon_off"], rs
            self.written += [(int(b["dst_qcoeff_off"]), n * 4), (int(b["dst_dqcoeff_off"]), n * 4)]
            self.written += rows(int(b["dst_recon_off"]), int(b["dst_recon_stride"]) * pix().itemsize, w * pix().itemsize, h)
            at += len(types)
        self.arena, self.regions = ab.build(), ab.regions
        self.records = (results, rdoq, dist, cost)
        self.want = [decide(gold.tables, w, h, b, self.cdescs, results, rdoq, dist, cost) for b in self.descs]

    def decide(self, gold, disable=()):
        return [decide(gold.tables, self.w, self.h, b, self.cdescs, *self.records, disable) for b in self.descs]

    def winner(self, bi):
        """(qcoeff, dqcoeff, recon [h][w]) the reference leaves in cand_bf for block bi, or None where no candidate reached the comparison"""
        k = self.want[bi]["cand"]
        return None if k == abi.TXT_NO_CAND else self.cand[int(self.descs[bi]["first_cand"]) + k]

    def summary(self, bi):
        """What the fixture stores of block bi: the record and the digests of the arrays the search leaves in cand_bf (the reference runs the
        inverse transform only where the distortion is spatial: no reconstruction digest elsewhere)"""
        want, win = self.want[bi], self.winner(bi)
        dig = (0, 0, 0) if win is None else (R.digest(win["q"]), R.digest(win["dq"]), digest_pixels(win["rec"]) if self.cases[bi].spatial else 0)
        return (want["tx_type"], want["cand"], want["eob"], want["cul_level"], want["bits"], want["distortion"][0], want["distortion"][1], want["cost"],
                want["quant_mask"], want["cost_mask"]) + dig


REFERENCE_FIELDS = ("tx_type", "bits", "dist_residual", "dist_prediction", "eob", "has_coeff", "q_digest", "dq_digest", "recon_digest")   # Pin.run's tuple
RESTATED_FIELDS = ("cand", "cul_level", "cost", "quant_mask", "cost_mask")                                                            # the restatement's own
FIXTURE_FIELDS = ("tx_type", "cand", "eob", "cul_level", "bits", "dist_residual", "dist_prediction", "cost", "quant_mask", "cost_mask", "q_digest",
                  "dq_digest", "recon_digest")


# ------------------------------------------------------------------------------------------------ the reference, where it was built
class PinArgs(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("bit_depth", "qindex", "tx_size", "w", "h", "is_inter", "pred_mode", "spatial_sse", "rdoq_level", "sc_class1",
                                         "n_groups")] + [("lam", C.c_uint32)] + \
               [(f, C.c_int32) for f in ("satd_th", "rate_th", "coeff_th", "dist_th", "crop_w", "crop_h", "residual_stride", "pred_stride", "src_stride",
                                         "recon_stride")]


class Pin:
    """tests/txt_search_pin_driver.c built into `directory` against oracle/_ref/libsvtref.so (ref: the loaded pyorc.ref(), whose ref_init
    has set the RTCD pointers the transforms, quantisers and distortion kernels go through)."""

    def __init__(self, ref, directory):
        from support import build_pin
        self.ref, self.lib = ref, build_pin(directory, os.path.join(HERE, "txt_search_pin_driver.c"))
        self.lib.pin_tables_new.restype, self.lib.pin_tables_new.argtypes = C.c_void_p, [C.c_int32]
        self.lib.pin_tx_type_search.restype, self.lib.pin_tx_type_search.argtypes = None, [C.c_void_p] * 9
        self.handles = [self.lib.pin_tables_new(q) for q in T.QINDEX]

    def candidate_order(self, w, h, is_inter, reduced, sc, n_groups):
        types, mask = np.zeros(64, np.uint8), C.c_uint32(0)
        n = self.lib.pin_candidate_order(T.TX_INDEX[(w, h)], int(is_inter), int(reduced), int(sc), int(n_groups), C.c_void_p(types.ctypes.data), C.byref(mask))
        return [int(t) for t in types[:n]], mask.value

    def run(self, S, bi):
        """The reference's tx_type_search on block bi of the Search S -> (transform_type, y_coeff_bits, distortion residual, prediction, eob.y,
        y_has_coeff, digests of the quant, rec_coeff and recon blocks it leaves in cand_bf; recon only where the search measures spatial SSE)"""
        c, x = S.cases[bi], S.inputs[bi]
        res_stride, ps, ss, rs = x["strides"]
        # without the early exit flag the restatement never leaves early; the reference has no such switch, thresholds of 0 do the same
        a = PinArgs(c.bd, T.QINDEX[c.table], T.TX_INDEX[(c.w, c.h)], c.w, c.h, c.is_inter, x["pred_mode"], c.spatial, c.rdoq, c.sc, c.n_groups, c.lam,
                    c.satd_th, c.rate_th, c.coeff_th if c.early else 0, c.dist_th if c.early else 0, x["crop"][0], x["crop"][1], res_stride, ps, ss, rs)
        res, pred, src = (np.ascontiguousarray(x[k]).copy() for k in ("res", "pred", "src"))
        quant, rec_coeff = np.full(c.w * c.h, 7, np.int32), np.full(c.w * c.h, 7, np.int32)
        recon, out = np.zeros((c.h, rs), pred.dtype), np.zeros(6, np.uint64)
        self.lib.pin_tx_type_search(C.c_void_p(self.handles[c.table]), C.byref(a), *(C.c_void_p(v.ctypes.data) for v in (res, pred, src, quant, rec_coeff, recon, out)))
        assert np.array_equal(res, x["res"]) and np.array_equal(pred, x["pred"]) and np.array_equal(src, x["src"])
        assert not quant[S.n:].any() and not rec_coeff[S.n:].any()
        return tuple(int(v) for v in out) + (R.digest(quant[:S.n]), R.digest(rec_coeff[:S.n]), digest_pixels(recon[:, :c.w]) if c.spatial else 0)

    @staticmethod
    def restated(S, bi):
        """The same tuple from the restatement"""
        want, win = S.want[bi], S.winner(bi)
        return (want["tx_type"], want["bits"], want["distortion"][0], want["distortion"][1], want["eob"], int(want["eob"] > 0)) + S.summary(bi)[-3:]
