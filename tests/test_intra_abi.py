"""CPU: the golden fixture of the intra search is what the reference computes (when oracle/_ref/libsvtref.so is built) and reaches
what it is meant to reach."""
import numpy as np
import pytest

from support import assert_not_rtcd_leaf
from svtav1_hip import abi


def test_intra_golden_matches_reference(ref):
    """Every case of the golden fixture, recomputed by the reference's own functions."""
    import intra_cases as I
    gold = np.load(I.GOLD)
    orc = I.RefIntraSearch(ref)
    for i, case in enumerate(I.ALL_CASES):
        I.check_against_golden(gold, case[0], orc.run(I.case_plane(case, i), I.case_ctrls(case), all_modes=case in I.CASES))


def test_intra_golden_covers_every_mode_and_cost_form():
    """The cases reach every mode as a winner somewhere, both cost forms, every pf_shape and blocks that are not searched."""
    import intra_cases as I
    gold = np.load(I.GOLD)
    winners = set()
    for case in I.CASES:
        winners |= set(np.unique(gold[f"{case[0]}_best_mode"]).tolist())
    assert winners >= set(range(abi.INTRA_MODES)) | {I.NOT_SEARCHED}
    assert {c[5] for c in I.CASES} == {0, 1} and {c[6] for c in I.CASES if not c[5]} == {0, 1, 2}
    assert any(c[7] and (c[7], c[8]) != (c[2], c[3]) for c in I.CASES)


@pytest.mark.parametrize("name", ["svt_hip_intra_search_frames"])
def test_intra_export_is_not_an_rtcd_leaf(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf."""
    assert_not_rtcd_leaf(name)
