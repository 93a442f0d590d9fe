"""CPU: the golden fixture of the sub-pel motion search (tests/subpel_cases.py) is what the reference's
svt_av1_find_best_sub_pixel_tree(_pruned) leave, the Python restatement equals it on every case, the cases reach what they are meant to
reach, svt_hip_subpel_mv_limits gives the limits the encoder would use, and the entry points refuse bad arguments without a device."""
import ctypes as C
import importlib.util
import os

import pytest

import subpel_cases as S
from support import assert_not_rtcd_leaf, fresh_process, have_reference_tree, header_values
from svtav1_hip import abi


def _golden_script():
    spec = importlib.util.spec_from_file_location("make_golden_subpel", os.path.join(S.HERE, "golden", "make_golden_subpel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gold():
    return S.Golden()


@pytest.fixture(scope="module")
def searches():
    return [S.Search(c) for c in S.CASES]


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    return S.Pin(ref, tmp_path_factory.mktemp("subpel_pin"))


@pytest.mark.parametrize("name", ["svt_hip_subpel_search_batch", "svt_hip_subpel_mv_limits"])
def test_subpel_export_is_not_an_rtcd_leaf(name):
    assert_not_rtcd_leaf(name)


def test_constants_are_the_headers():
    names = ["SVT_HIP_SUBPEL_" + n for n in ("TREE", "TREE_PRUNED", "USE_2_TAPS", "USE_4_TAPS", "USE_8_TAPS", "EXIT_NONE", "EXIT_EARLY", "EXIT_VARIANCE",
                                            "EXIT_ABS_TH", "EXIT_NO_ROUND", "EXIT_ROUND_DEV", "EXIT_END", "OK", "BAD_SIZE", "BAD_POINTER", "BAD_START_MV",
                                            "BAD_METHOD", "BAD_FILTER", "BAD_COST")]
    want = header_values(names)
    assert [want[n] for n in names] == [getattr(abi, n[len("SVT_HIP_"):]) for n in names]
    assert [want[n] for n in names[:5]] == [0, 1, 1, 2, 3] and want["SVT_HIP_SUBPEL_EXIT_NONE"] == 0 == want["SVT_HIP_SUBPEL_OK"]
    assert len({want[n] for n in names[5:12]}) == 7 and len({want[n] for n in names[12:]}) == 7


@pytest.mark.parametrize("mirror", [abi.SubpelJob, abi.SubpelDesc, abi.SubpelResult], ids=lambda m: m.__name__)
def test_mirror_has_no_implicit_padding(mirror):
    end = 0
    for f, _ in mirror._fields_:
        assert getattr(mirror, f).offset == end, f"implicit padding before {mirror.__name__}.{f}"
        end += getattr(mirror, f).size
    assert end == C.sizeof(mirror)
    assert [C.sizeof(m) for m in (abi.SubpelJob, abi.SubpelDesc, abi.SubpelResult)] == [32, 96, 24]


def test_mv_limits_are_the_fixtures(gold):
    """The host-only helper against what the reference's two range functions gave: blocks at all four picture edges, ref_mv far enough
    out for the MAX_FULL_PEL_VAL clamp and for the MV_LOW / MV_UPP one; and the restatement the cases take their limits from."""
    lib = abi.load()
    clamped = 0
    for lc, want in zip(S.LIMIT_CASES, gold.limits):
        out, mv = (C.c_int32 * 4)(), abi.Mv(lc.ref_row, lc.ref_col)
        assert lib.svt_hip_subpel_mv_limits(lc.mi_row, lc.mi_col, lc.mi_w, lc.mi_h, lc.mi_rows, lc.mi_cols, C.byref(mv), out) == abi.SVT_HIP_OK
        assert tuple(out) == tuple(int(v) for v in want) == S.mv_limits(lc), lc
        clamped += want[0] == lc.ref_col - 8 * S.MAX_FULL_PEL_VAL or want[1] == lc.ref_col + 8 * S.MAX_FULL_PEL_VAL
    assert clamped >= 2
    edges = {(lc.mi_row == 0, lc.mi_col == 0, lc.mi_row + lc.mi_h == lc.mi_rows, lc.mi_col + lc.mi_w == lc.mi_cols) for lc in S.LIMIT_CASES}
    assert all(any(e[k] for e in edges) for k in range(4))
    mv, out = abi.Mv(0, 0), (C.c_int32 * 4)()
    assert lib.svt_hip_subpel_mv_limits(0, 0, 4, 4, 10, 10, None, out) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert lib.svt_hip_subpel_mv_limits(0, 0, 4, 4, 10, 10, C.byref(mv), None) == abi.SVT_HIP_ERR_BAD_PARAMETER


def test_restatement_matches_golden(gold, searches):
    """Without the reference: what every GPU test compares with is what the fixture holds."""
    for i, s in enumerate(searches):
        assert s.record() == gold.record(i), (i, s.c)


def test_cases_cover_their_list(searches):
    """The coverage conditions of the golden script, on the restatement's own account of each search"""
    events = _golden_script().coverage(searches)
    assert len(S.SIZES) == 22 and events[("wrap", 110)] > 0


def test_restatement_is_what_the_reference_does(pin, searches):
    """The restatement against the two real functions on every case, and the constants it and the header state"""
    assert pin.constants() == [0, 1, 1, 2, 3, S.ENTROPY, S.L1_LOWRES, S.L1_MIDRES, S.L1_HDRES, S.OPT, S.NONE, 3, S.MV_LOW, S.MV_UPP, S.MAX_FULL_PEL_VAL, 1]
    for lc in S.LIMIT_CASES:
        assert pin.limits(lc) == S.mv_limits(lc), lc
    for i, s in enumerate(searches):
        assert pin.run(s.c) == s.record()[:6], (i, s.c)


def test_golden_regenerates_byte_identical(pin):
    with open(S.GOLD, "rb") as f:
        assert f.read() == _golden_script().build(pin)


def test_refusals_need_no_device():
    """A process that never called svt_hip_init: NULL job, descriptors or results are bad parameters, an empty batch succeeds, anything
    else is SVT_HIP_ERR_NO_DEVICE.  Nothing is launched either way."""
    got = fresh_process("(lambda f: (f(None, p, p, 1, None), f(p, None, p, 1, None), f(p, p, None, 1, None), f(None, None, None, 0, None),"
                        "f(p, p, p, 0, None), f(p, p, p, 1, None)))(lib.svt_hip_subpel_search_batch)")
    assert got == [abi.SVT_HIP_ERR_BAD_PARAMETER] * 4 + [abi.SVT_HIP_OK, abi.SVT_HIP_ERR_NO_DEVICE]
