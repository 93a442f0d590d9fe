"""CPU: the golden fixture of OBMC motion refinement (tests/obmc_cases.py) is what the reference's calc_target_weighted_pred and
single_motion_search leave, the Python restatement equals it on every case, the cases reach what they are meant to reach,
svt_hip_obmc_mv_limits gives the limits the encoder would use, and the entry points refuse bad arguments without a device."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import obmc_cases as O
from support import assert_not_rtcd_leaf, fresh_process, have_reference_tree, header_values
from svtav1_hip import abi


def _golden_script():
    spec = importlib.util.spec_from_file_location("make_golden_obmc", os.path.join(O.HERE, "golden", "make_golden_obmc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gold():
    return O.Golden()


@pytest.fixture(scope="module")
def restated():
    return [O.Restated(c) for c in O.CASES]


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    return O.Pin(ref, tmp_path_factory.mktemp("obmc_pin"))


@pytest.mark.parametrize("name", ["svt_hip_obmc_target_batch", "svt_hip_obmc_search_batch", "svt_hip_obmc_mv_limits"])
def test_obmc_export_is_not_an_rtcd_leaf(name):
    assert_not_rtcd_leaf(name)


def test_constants_are_the_headers():
    names = ["SVT_HIP_OBMC_" + n for n in ("OK", "BAD_SIZE", "BAD_POINTER", "BAD_SEGMENT", "BAD_RANGE", "BAD_START_MV", "BAD_LIMITS", "BAD_FILTER", "BAD_COST",
                                          "MAX_NEIGHBOURS")]
    want = header_values(names)
    assert [want[n] for n in names] == [getattr(abi, n[len("SVT_HIP_"):]) for n in names]
    assert want["SVT_HIP_OBMC_OK"] == 0 and len({want[n] for n in names[:9]}) == 9 and want["SVT_HIP_OBMC_MAX_NEIGHBOURS"] == max(O.MAX_NEIGHBOR_OBMC) == 4


@pytest.mark.parametrize("mirror", [abi.ObmcNeighbour, abi.ObmcTargetDesc, abi.ObmcSearchDesc, abi.ObmcSearchResult], ids=lambda m: m.__name__)
def test_mirror_has_no_implicit_padding(mirror):
    end = 0
    for f, _ in mirror._fields_:
        assert getattr(mirror, f).offset == end, f"implicit padding before {mirror.__name__}.{f}"
        end += getattr(mirror, f).size
    assert end == C.sizeof(mirror)
    assert [C.sizeof(m) for m in (abi.ObmcNeighbour, abi.ObmcTargetDesc, abi.ObmcSearchDesc, abi.ObmcSearchResult)] == [2, 80, 96, 28]
    layout = header_values([f"sizeof(SvtHip{m.__name__})" for m in (abi.ObmcNeighbour, abi.ObmcTargetDesc, abi.ObmcSearchDesc, abi.ObmcSearchResult)])
    assert list(layout.values()) == [2, 80, 96, 28]


def test_mv_limits_are_the_fixtures(gold):
    """The host-only helper against what single_motion_search's set-up and svt_av1_set_mv_search_range gave: blocks at all four picture
    edges, ref_mv far enough out for the MAX_FULL_PEL_VAL clamp and for the MV_LOW / MV_UPP one; and the restatement the cases take their
    limits from."""
    lib = abi.load()
    clamped = 0
    for lc, want in zip(O.LIMIT_CASES, gold.limits):
        raw, fp, mv = (C.c_int32 * 4)(), (C.c_int32 * 4)(), abi.Mv(lc[6], lc[7])
        assert lib.svt_hip_obmc_mv_limits(*lc[:6], C.byref(mv), raw, fp) == abi.SVT_HIP_OK
        assert tuple(raw) + tuple(fp) == tuple(int(v) for v in want) == sum(O.mv_limits(*lc[:6], (lc[6], lc[7])), ()), lc
        clamped += want[4] == (lc[7] >> 3) - O.MAX_FULL_PEL_VAL + (lc[7] & 7 != 0) or want[5] == (lc[7] >> 3) + O.MAX_FULL_PEL_VAL
    assert clamped >= 2
    edges = {(lc[0] == 0, lc[1] == 0, lc[0] + lc[3] == lc[4], lc[1] + lc[2] == lc[5]) for lc in O.LIMIT_CASES}
    assert all(any(e[k] for e in edges) for k in range(4))
    mv, out = abi.Mv(0, 0), (C.c_int32 * 4)()
    assert lib.svt_hip_obmc_mv_limits(0, 0, 4, 4, 10, 10, None, out, out) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert lib.svt_hip_obmc_mv_limits(0, 0, 4, 4, 10, 10, C.byref(mv), None, out) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert lib.svt_hip_obmc_mv_limits(0, 0, 4, 4, 10, 10, C.byref(mv), out, None) == abi.SVT_HIP_ERR_BAD_PARAMETER


def test_both_mv_limit_exports_apply_one_range_rule():
    """Over the LIMIT_CASES of both families: the fp_limits of svt_hip_obmc_mv_limits are the full-pel range that svt_hip_subpel_mv_limits
    narrows from the same inputs, through the shared restatement of svt_av1_set_mv_search_range, and each export is its own restatement: the
    library's one copy of the rule, pinned from both sides."""
    import md_search_cases as M
    import subpel_cases as S
    lib = abi.load()
    cases = sorted({tuple(lc) for lc in S.LIMIT_CASES} | set(O.LIMIT_CASES))
    assert S.LIMIT_CASES and O.LIMIT_CASES
    for lc in cases:
        raw, fp, sub, ref_mv = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 4)(), (lc[6], lc[7])
        mv = abi.Mv(*ref_mv)
        assert lib.svt_hip_obmc_mv_limits(*lc[:6], C.byref(mv), raw, fp) == abi.SVT_HIP_OK
        assert lib.svt_hip_subpel_mv_limits(*lc[:6], C.byref(mv), sub) == abi.SVT_HIP_OK
        assert tuple(fp) == M.set_mv_search_range(M.block_mv_limits(*lc[:6]), ref_mv), lc
        assert tuple(sub) == M.set_subpel_mv_search_range(tuple(fp), ref_mv), lc
        assert (tuple(raw), tuple(fp)) == O.mv_limits(*lc[:6], ref_mv) and tuple(sub) == S.mv_limits(S.LimitCase(*lc)), lc


def test_restatement_matches_golden(gold, restated):
    """Without the reference: what every GPU test compares with is what the fixture holds."""
    for i, r in enumerate(restated):
        assert r.digests() == gold.digest(i) and r.record() == gold.record(i), (i, r.c)
        assert O.SAD_PER_BIT[r.c.qindex] == gold.sad_per_bit[i]
    assert (gold.digests[:, 0] != gold.digests[:, 1]).all() and len({tuple(d) for d in gold.digests}) > len(O.CASES) // 2


def test_cases_cover_their_list(restated):
    """The coverage conditions of the golden script, on the restatement's own account of each case"""
    events = _golden_script().coverage(restated)
    assert len(O.SIZES) == 22 and events[("tie",)] > 0


def test_ramps_are_the_blend_fixtures():
    """The ramps the target kernel and the restatement hold are those the blend tests read from the reference"""
    z = np.load(os.path.join(O.HERE, "golden", "inter_blend.npz"))
    for n, ramp in O.RAMPS.items():
        assert tuple(int(v) for v in z[f"obmc_{n}"]) == ramp


def test_restatement_is_what_the_reference_does(pin, restated):
    """The restatement against the reference on every case: calc_target_weighted_pred on the case's mode-info grid, the stage functions, and
    single_motion_search itself wherever its hard-wired controls are the case's; the constants and the ramps the header and the restatement state"""
    got = pin.constants()
    assert got[:12] == [1, 2, 3, O.MV_LOW, O.MV_UPP, O.MAX_FULL_PEL_VAL, 4, 4, 64, 6, 9, 6]
    assert got[12:] == [v for n in (1, 2, 4, 8, 16, 32) for v in O.RAMPS[n]]
    for lc in O.LIMIT_CASES:
        assert pin.limits(lc) == O.mv_limits(*lc[:6], (lc[6], lc[7])), lc
    pin_case = _golden_script().pin_case
    through_the_function = sum(pin_case(pin, r)[3] for r in restated)
    assert through_the_function * 2 > len(restated)


def test_golden_regenerates_byte_identical(pin, restated):
    with open(O.GOLD, "rb") as f:
        assert f.read() == _golden_script().build(pin, restated)


def test_refusals_need_no_device():
    """A process that never called svt_hip_init: NULL job, descriptors or results are bad parameters, an empty batch succeeds, anything
    else is SVT_HIP_ERR_NO_DEVICE.  Nothing is launched either way."""
    got = fresh_process("(lambda f, g: (f(None, p, p, 1, None), f(p, None, p, 1, None), f(p, p, None, 1, None), f(None, None, None, 0, None),"
                        "f(p, p, p, 0, None), f(p, p, p, 1, None), g(None, p, 1, None), g(p, None, 1, None), g(None, None, 0, None), g(p, p, 0, None),"
                        "g(p, p, 1, None)))(lib.svt_hip_obmc_search_batch, lib.svt_hip_obmc_target_batch)")
    bad, ok, none = abi.SVT_HIP_ERR_BAD_PARAMETER, abi.SVT_HIP_OK, abi.SVT_HIP_ERR_NO_DEVICE
    assert got == [bad] * 4 + [ok, none] + [bad] * 3 + [ok, none]
