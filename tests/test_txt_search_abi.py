"""CPU: the restatement of the transform-type search (tests/txt_search_cases.py) equals the fixture tests/golden/txt_search.npz, the case
lists make every exit of the loop matter, the mirrors match the header, and the entry points refuse bad arguments without a device."""
import collections
import ctypes as C

import numpy as np
import pytest

import rdoq_cases as R
import txt_search_cases as X
from support import assert_not_rtcd_leaf, fresh_process, have_reference_tree, header_values
from svtav1_hip import abi

NAMES = ["svt_hip_txfm_spatial_distortion_batch", "svt_hip_txt_select_batch", "svt_hip_txt_select_batch_mapped", "svt_hip_txt_search_batch",
         "svt_hip_txt_search_scratch_bytes"]


@pytest.fixture(scope="module")
def gold():
    return R.Golden()


@pytest.fixture(scope="module")
def searches(gold, orc):
    return {s: X.Search(gold, orc, *s) for s in X.SEARCH_SIZES}


@pytest.fixture(scope="module")
def decided(gold, searches):
    """Every case of both lists as (record with every exit in place, {exit: record with that exit taken out})"""
    out = []
    for s in X.synthetic_sets(gold):
        without = {e: X.synthetic_expected(gold, s, (e,)) for e in X.EXITS}
        out += [(r, {e: without[e][k] for e in X.EXITS}) for k, r in enumerate(X.synthetic_expected(gold, s))]
    for S in searches.values():
        without = {e: S.decide(gold, (e,)) for e in X.EXITS}
        out += [(r, {e: without[e][k] for e in X.EXITS}) for k, r in enumerate(S.want)]
    return out


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    return X.Pin(ref, tmp_path_factory.mktemp("txt_search_pin"))


def test_golden_matches_reference(pin, searches):
    """Every case's transform_type, y_coeff_bits, y_full_distortion[DIST_SSD][2], eob.y, y_has_coeff and the digests of the quant / rec_coeff /
    recon blocks in cand_bf, recomputed by the reference's own tx_type_search now.
    Two limits: cul_level is not pinned here (with update_skip_ctx_dc_sign_ctx off the reference's search returns 0 for it; the value rests
    on the RDOQ pin of tests/test_rdoq_abi.py), and the recon digest is compared only where the distortion is spatial, because only there
    does the reference's search run the inverse transform."""
    z = np.load(X.GOLD)
    for S in searches.values():
        for bi, i in enumerate(S.case_index):
            assert pin.run(S, bi) == tuple(int(z[f][i]) for f in X.REFERENCE_FIELDS), (i, X.SEARCH_CASES[i])


def test_restatement_is_what_the_reference_does(pin, searches):
    """The restatement (the oracle's transforms and quantisers, the restated RDOQ stage and rate, and decide()) against the real function on
    every case; and the candidate order against tx_type_group[_sc] and av1_ext_tx_used for every size, prediction kind, tx set and group count.
    The same two limits as above: cul_level is outside the compared tuple (the RDOQ pin holds it), and the recon digest counts only in the
    cases that measure spatial SSE."""
    for S in searches.values():
        for bi in range(len(S.cases)):
            assert pin.run(S, bi) == X.Pin.restated(S, bi), (S.cases[bi],)
    for w, h in R.T.SIZES:
        for is_inter in (0, 1):
            for reduced in (0, 1):
                for sc in (0, 1):
                    for n_groups in range(1, 7):
                        assert pin.candidate_order(w, h, is_inter, reduced, sc, n_groups) == X.candidate_order(w, h, is_inter, reduced, sc, n_groups)


def test_restatement_matches_golden(searches):
    """What every GPU test compares with is what the fixture holds: record and digests of every whole-search case."""
    z = np.load(X.GOLD)
    assert len(z["seed"]) == len(X.SEARCH_CASES) and [int(v) for v in z["seed"]] == [c.seed for c in X.SEARCH_CASES]
    seen = 0
    for S in searches.values():
        for bi, i in enumerate(S.case_index):
            assert tuple(int(z[f][i]) for f in X.FIXTURE_FIELDS) == S.summary(bi), (i, X.SEARCH_CASES[i])
            assert tuple(int(z[f][i]) for f in X.REFERENCE_FIELDS) == X.Pin.restated(S, bi), (i, X.SEARCH_CASES[i])
            seen += 1
    assert seen == len(X.SEARCH_CASES)


@pytest.mark.parametrize("exit_", ["rate", "satd", "group"])
def test_exit_decides_the_winner(decided, exit_):
    """The rate-cost threshold, the SATD early exit and the coefficient-count / cost group exit: at least 20 cases each whose restated
    winner is another one with that exit taken out."""
    assert sum(r["cand"] != without[exit_]["cand"] for r, without in decided) >= 20


def test_early_cost_skip_never_decides_the_winner(decided):
    """The early_cost skip (:4751-4755) is the one exit that cannot change the winner: a candidate it skips has
    cost = RDCOST(lambda, bits, dist) >= RDCOST(lambda, 0, dist) > best_cost, so it would lose the strict comparison; and the group
    exit behind the comparison sees the state of its last evaluation, or one with best_tx_non_coeff reset, which exits no sooner.
    That holds for every early_exit_coeff_th up to 64 * 64, the value a group reset gives best_tx_non_coeff (no preset sets more), so no
    case list within it can make the winner differ.  What it does change is which candidates reach the rate estimation: at least 20 cases
    whose cost mask differs with the skip taken out, and in every case the same winner, bits, distortions and cost."""
    assert sum(r["cost_mask"] != without["early_cost"]["cost_mask"] for r, without in decided) >= 20
    for r, without in decided:
        other = without["early_cost"]
        assert all(r[f] == other[f] for f in ("tx_type", "cand", "eob", "bits", "distortion", "cost", "quant_mask")), (r, other)


def test_ties_and_the_wrapped_rate_test(decided):
    """At least 20 cases in which two compared candidates share the winning cost (the earlier one wins by the strict <), and at least 5 in
    which the rate-cost test runs while dct_dct_cost is still ~0 (a candidate list whose first entry is not DCT_DCT)."""
    assert sum(r["tie"] for r, _ in decided) >= 20
    assert sum(r["rate_before_dct"] for r, _ in decided) >= 5
    assert sum(r["cand"] == abi.TXT_NO_CAND for r, _ in decided) >= 1


def test_tie_keeps_the_earlier_candidate(gold):
    s = X.synthetic(gold, 99, 1, (3,))
    s.cdescs["tx_type"][s.descs["first_cand"][0]:][:3] = (0, 3, 9)
    s.results["eob"][:], s.cost["bits"][:], s.dist[:] = 2, 1024, 128
    s.descs["satd_early_exit_th"], s.descs["txt_rate_cost_th"], s.descs["flags"] = 0, 0, 0
    r = X.synthetic_expected(gold, s)[0]
    assert (r["cand"], r["tx_type"], r["tie"], r["cost_mask"]) == (0, 0, True, 7)


def test_search_cases_cover_what_they_must(searches):
    cs = X.SEARCH_CASES
    assert {(c.w, c.h) for c in cs} == {(4, 4), (4, 16), (16, 4), (8, 8), (16, 16), (16, 8), (32, 32), (64, 64)}
    for w, h in X.SEARCH_SIZES:
        of = [c for c in cs if (c.w, c.h) == (w, h)]
        assert {c.bd for c in of} == {8, 10} and {c.is_inter for c in of} == {0, 1} and {c.spatial for c in of} == {0, 1}, (w, h)
        assert {c.rdoq for c in of} == {0, 1} and {c.own_dst for c in of} == {0, 1}, (w, h)
    assert any(c.sc for c in cs) and any(c.crop for c in cs)
    assert all(int(n) == 1 for n in searches[(64, 64)].descs["n_cand"])                     # one type in the set
    assert max(int(n) for S in searches.values() for n in S.descs["n_cand"]) == 16
    winners = collections.Counter(r["tx_type"] for S in searches.values() for r in S.want)
    assert len(winners) >= 6 and winners[0] < sum(winners.values())
    assert X.candidate_order(8, 8, 1, 0, 0, 6) == ([0, 10, 11, 3, 1, 2, 6, 9, 4, 5, 7, 8, 12, 13, 14, 15], 0b101011011)
    assert X.candidate_order(8, 8, 1, 0, 1, 2) == ([0, 9, 10, 11], 0b101) and X.candidate_order(32, 32, 0, 0, 0, 6) == ([0], 1)


def test_mirrors_match_the_header():
    names = ["sizeof(SvtHipTxtDesc)", "sizeof(SvtHipTxtResult)", "sizeof(SvtHipSpatialSrc)", "SVT_HIP_TXT_MAX_CAND", "SVT_HIP_TXT_EARLY_EXIT",
             "SVT_HIP_TXT_SPATIAL_SSE", "SVT_HIP_TXT_SEARCH_INVERSE", "offsetof(SvtHipTxtDesc, n_cand)", "offsetof(SvtHipTxtResult, cand)"]
    v = header_values(names, ["svt_hip_txfm.h"])
    assert [v[n] for n in names] == [C.sizeof(abi.TxtDesc), C.sizeof(abi.TxtResult), C.sizeof(abi.SpatialSrc), abi.TXT_MAX_CAND, abi.TXT_EARLY_EXIT,
                                     abi.TXT_SPATIAL_SSE, abi.TXT_SEARCH_INVERSE, abi.TxtDesc.n_cand.offset, abi.TxtResult.cand.offset]
    assert abi.TXT_DESC_DTYPE.itemsize == 72 and abi.TXT_RESULT_DTYPE.itemsize == 48 and abi.SPATIAL_SRC_DTYPE.itemsize == 16


@pytest.mark.parametrize("name", NAMES)
def test_export_is_not_an_rtcd_leaf(name):
    assert_not_rtcd_leaf(name)


def test_scratch_bytes_is_host_arithmetic():
    lib = abi.load()
    f = lib.svt_hip_txt_search_scratch_bytes
    assert f(0, 0) == 0 and f(1, 1) == 5 * 256 and f(16, 1) == f(16, 9)
    assert all(f(n + 1, 1) >= f(n, 1) >= n * (16 + 16 + 4 + 16 + 16) for n in (1, 15, 16, 17, 1000, 100000))


def test_refusals_need_no_device():
    """A process that never called svt_hip_init: a size that is no transform size, no table set, a NULL mandatory array with blocks to
    do, a mapping that does not exist and a scratch that is too small are bad parameters; an empty batch succeeds; NULL RDOQ arrays are
    allowed; anything else is SVT_HIP_ERR_NO_DEVICE.  Nothing is launched either way."""
    got = fresh_process("(lambda f, g, s, need: ("
                        # svt_hip_txt_select_batch(base, desc, tdesc, cdesc, tables, n_tables, result, rdoq, dist, cost, out, n_cand, n, w, h, stream)
                        "f(p, p, p, p, p, 1, p, p, p, p, p, 4, 1, 4, 32, None), f(p, p, p, p, p, 1, p, p, p, p, p, 4, 1, 12, 8, None),"
                        "f(p, p, p, p, p, 0, p, p, p, p, p, 4, 1, 8, 8, None), f(None, p, p, p, p, 1, p, p, p, p, p, 4, 1, 8, 8, None),"
                        "f(p, None, p, p, p, 1, p, p, p, p, p, 4, 1, 8, 8, None), f(p, p, None, p, p, 1, p, p, p, p, p, 4, 1, 8, 8, None),"
                        "f(p, p, p, None, p, 1, p, p, p, p, p, 4, 1, 8, 8, None), f(p, p, p, p, None, 1, p, p, p, p, p, 4, 1, 8, 8, None),"
                        "f(p, p, p, p, p, 1, None, p, p, p, p, 4, 1, 8, 8, None), f(p, p, p, p, p, 1, p, p, None, p, p, 4, 1, 8, 8, None),"
                        "f(p, p, p, p, p, 1, p, p, p, None, p, 4, 1, 8, 8, None), f(p, p, p, p, p, 1, p, p, p, p, None, 4, 1, 8, 8, None),"
                        "lib.svt_hip_txt_select_batch_mapped(p, p, p, p, p, 1, p, p, p, p, p, 4, 1, 8, 8, 2, None),"
                        # svt_hip_txt_search_batch(base, tdesc, rdesc, cdesc, tables, n_tables, desc, scratch, bytes, out, n_cand, n, w, h, flags, stream)
                        "g(p, p, p, p, p, 1, p, p, need, p, 4, 1, 8, 5, 0, None), g(p, p, p, p, p, 0, p, p, need, p, 4, 1, 8, 8, 0, None),"
                        "g(None, p, p, p, p, 1, p, p, need, p, 4, 1, 8, 8, 0, None), g(p, None, p, p, p, 1, p, p, need, p, 4, 1, 8, 8, 0, None),"
                        "g(p, p, p, None, p, 1, p, p, need, p, 4, 1, 8, 8, 0, None), g(p, p, p, p, None, 1, p, p, need, p, 4, 1, 8, 8, 0, None),"
                        "g(p, p, p, p, p, 1, None, p, need, p, 4, 1, 8, 8, 0, None), g(p, p, p, p, p, 1, p, None, need, p, 4, 1, 8, 8, 0, None),"
                        "g(p, p, p, p, p, 1, p, p, need, None, 4, 1, 8, 8, 0, None), g(p, p, p, p, p, 1, p, p, need - 1, p, 4, 1, 8, 8, 1, None),"
                        # svt_hip_txfm_spatial_distortion_batch(base, tdesc, src, out, n, w, h, stream)
                        "s(p, p, p, p, 1, 64, 8, None), s(None, p, p, p, 1, 8, 8, None), s(p, None, p, p, 1, 8, 8, None), s(p, p, None, p, 1, 8, 8, None),"
                        "s(p, p, p, None, 1, 8, 8, None),"
                        "f(None, None, None, None, None, 1, None, None, None, None, None, 0, 0, 16, 64, None),"
                        "g(None, None, None, None, None, 1, None, None, 0, None, 0, 0, 16, 64, 1, None), s(None, None, None, None, 0, 4, 16, None),"
                        "f(p, p, p, p, p, 1, p, None, p, p, p, 4, 1, 16, 64, None), g(p, p, None, p, p, 1, p, p, need, p, 4, 1, 64, 64, 1, None),"
                        "s(p, p, p, p, 1, 4, 4, None)))"
                        "(lib.svt_hip_txt_select_batch, lib.svt_hip_txt_search_batch, lib.svt_hip_txfm_spatial_distortion_batch,"
                        " lib.svt_hip_txt_search_scratch_bytes(4, 1))")
    assert got == [abi.SVT_HIP_ERR_BAD_PARAMETER] * 28 + [abi.SVT_HIP_OK] * 3 + [abi.SVT_HIP_ERR_NO_DEVICE] * 3
