"""CPU: the golden fixture of intra prediction / inter-intra / CfL (tests/intra_pred_cases.py) is what the reference computes, the
Python restatement of the edge preparation is what the reference's static functions do, and the cases reach what they are meant to
reach."""
import ast
import ctypes as C
import os

import numpy as np
import pytest

import intra_pred_cases as P
from support import assert_not_rtcd_leaf, build_pin, fresh_process, have_reference_tree
from svtav1_hip import abi


@pytest.fixture(scope="module")
def gold():
    return np.load(P.GOLD)


def test_intra_pred_golden_matches_reference(ref, gold):
    """Every case of the fixture, recomputed by the reference's own leaves; the counters are those the fixture records."""
    counters = P.new_counters()
    blocks, cfl = P.reference_outputs(ref, counters)
    P.check_against_golden(gold, blocks, cfl)
    assert np.array_equal(P.alpha_search_outputs(P.RefIntraPred(ref)), gold["cfl_alpha_search"])
    keys, values = P.counters_record(counters)
    assert keys.tolist() == gold["counter_keys"].tolist() and values.tolist() == gold["counter_values"].tolist()


def test_restatement_is_what_the_static_functions_do(ref, tmp_path):
    """build_intra_predictors / build_intra_predictors_high themselves (tests/intra_pred_pin_driver.c includes their file), with the
    reference's asserts on, against RefIntraPred.intra on every case."""
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    pin = build_pin(tmp_path, os.path.join(P.HERE, "intra_pred_pin_driver.c"))
    V, i = C.c_void_p, C.c_int32
    pin.pin_build_intra_predictors.argtypes = [V, V, V] + [i] * 11
    pin.pin_build_intra_predictors_high.argtypes = [V, V, V] + [i] * 12
    pin.pin_build_intra_predictors.restype = pin.pin_build_intra_predictors_high.restype = None
    orc = P.RefIntraPred(ref)
    for c in P.CASES:
        above, left, _ = P.case_inputs(c)
        want = np.zeros((c.h, c.w), P.sample_type(c.is16))
        size = want.itemsize
        args = (above.ctypes.data + P.ORG * size, left.ctypes.data + P.ORG * size, want.ctypes.data, c.w, c.mode, c.delta, c.fim,
                P.TX_INDEX[(c.w, c.h)], c.no_filter, c.n_top, c.n_tr, c.n_left, c.n_bl, c.filt_type)
        pin.pin_build_intra_predictors_high(*args, c.bd) if c.is16 else pin.pin_build_intra_predictors(*args)
        got = orc.intra(c, above, left)
        assert np.array_equal(got, want), c


def test_cases_reach_every_path(gold):
    """Conditions on the inputs, taken from the counters the composition kept while the fixture was written."""
    n = {ast.literal_eval(k): int(v) for k, v in zip(gold["counter_keys"].tolist(), gold["counter_values"].tolist())}
    for w, h in P.TX_SIZES:
        for mode, delta in P.MODE_VARIANTS:
            assert n.get(("pair", w, h, mode, delta), 0) >= 6, (w, h, mode, delta)   # 2 of the cross, 4 draws
    assert len(P.TX_SIZES) == 19 and len(P.MODE_VARIANTS) == 61
    assert n.get("upsample_above", 0) > 0 and n.get("upsample_left", 0) > 0
    for ft in (0, 1):
        for s in range(4):
            assert n.get(("strength", ft, s), 0) > 0, (ft, s)
    assert n.get(("corner", 0), 0) > 0 and n.get(("corner", 1), 0) > 0
    for which in range(4):
        assert n.get(("topleft", which), 0) > 0, which
    for which in ("above", "base+1", "left", "base-1"):
        assert n.get(("fill", which), 0) > 0, which
    assert n.get("z2_above", 0) > 0 and n.get("z2_left", 0) > 0
    for has_left in (0, 1):
        for has_top in (0, 1):
            for shape in ("1:1", "1:2", "1:4"):
                assert n.get(("dc", has_left, has_top, shape), 0) > 0, (has_left, has_top, shape)


def test_case_list_has_every_group_size_and_format():
    """Mixed sizes and depths in one list; every group has its cases."""
    by_group = {g: [c for c in P.CASES if c.group == g] for g in P.GROUPS}
    assert len(by_group["cross"]) == 19 * 61 * 2 and len(by_group["draws"]) == 19 * 61 * 4
    assert len(by_group["filter_intra"]) == 5 * 14 * 4 * 2 and len(by_group["inter_intra"]) == 4 * 14 * 2 + 1
    assert {(c.bd, c.is16) for c in P.CASES} == set(P.FORMATS)
    assert {(c.w, c.h) for c in by_group["inter_intra"]} == set(P.II_SIZES) | {(64, 64)}
    assert len(P.CFL_CASES) == 16 * 7 * 3 * 3 and {c.alpha for c in P.CFL_CASES} == {-16, -7, -1, 0, 1, 9, 16}


@pytest.mark.parametrize("name", ["svt_hip_intra_predict_batch", "svt_hip_intra_predict_batch_packed", "svt_hip_cfl_predict_batch"])
def test_intra_pred_export_is_not_an_rtcd_leaf(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf."""
    assert_not_rtcd_leaf(name)


def test_refusals_need_no_device():
    """A process that never called svt_hip_init: NULL / n == 0 are bad parameters, anything else SVT_HIP_ERR_NO_DEVICE; nothing is
    launched either way."""
    got = fresh_process("lib.svt_hip_intra_predict_batch(None, 1, None), lib.svt_hip_intra_predict_batch(p, 0, None),"
                        "lib.svt_hip_intra_predict_batch_packed(p, 1, 3, None), lib.svt_hip_cfl_predict_batch(None, 1, None), lib.svt_hip_cfl_predict_batch(p, 0, None),"
                        "lib.svt_hip_intra_predict_batch(p, 1, None), lib.svt_hip_intra_predict_batch_packed(p, 1, 1, None), lib.svt_hip_cfl_predict_batch(p, 1, None)")
    assert got == [abi.SVT_HIP_ERR_BAD_PARAMETER] * 5 + [abi.SVT_HIP_ERR_NO_DEVICE] * 3
