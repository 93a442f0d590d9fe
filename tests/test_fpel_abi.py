"""CPU: the golden fixture of the full-pel motion search (tests/fpel_cases.py) is what the reference's md_full_pel_search, md_sq_motion_search
and md_nsq_motion_search leave, the Python restatement equals it on every case, the cases reach what they are meant to reach,
svt_hip_fpel_sq_windows gives the windows md_sq_motion_search derives, and the entry points refuse bad arguments without a device."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import pytest

import fpel_cases as F
from support import assert_not_rtcd_leaf, fresh_process, have_reference_tree, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

NAMES = ("svt_hip_fpel_search_batch", "svt_hip_fpel_sq_windows")


def _golden_script():
    spec = importlib.util.spec_from_file_location("make_golden_fpel", os.path.join(F.HERE, "golden", "make_golden_fpel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gold():
    return F.Golden()


@pytest.fixture(scope="module")
def searches():
    return [F.Search(c) for c in F.CASES]


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    return F.Pin(ref, tmp_path_factory.mktemp("fpel_pin"))


@pytest.mark.parametrize("name", NAMES)
def test_fpel_export_is_not_an_rtcd_leaf(name):
    assert_not_rtcd_leaf(name)


def test_constants_are_the_headers():
    names = ["SVT_HIP_FPEL_" + n for n in ("MVP", "SQ", "NSQ", "PME", "SAD", "VAR", "SSD", "MAX_MV", "MAX_MVP", "TILE", "MAX_EXTENT", "OK", "BAD_SIZE",
                                          "BAD_POINTER", "BAD_MODE", "BAD_DIST", "BAD_COST", "BAD_COUNT", "BAD_STEP", "BAD_WINDOW")]
    want = header_values(names)
    assert [want[n] for n in names] == [getattr(abi, n[len("SVT_HIP_"):]) for n in names]
    assert [want[n] for n in names[:11]] == [0, 1, 2, 3, 0, 1, 2, 6, 4, 32, 4095] and [want[n] for n in names[11:]] == list(range(9))
    status = header_values(["SVT_HIP_FPEL_STATUS(SVT_HIP_OK)", "SVT_HIP_FPEL_STATUS(SVT_HIP_ERR_BAD_PARAMETER)", "SVT_HIP_FPEL_STATUS(SVT_HIP_ERR_NO_DEVICE)",
                            "SVT_HIP_FPEL_STATUS(SVT_HIP_ERR_RUNTIME)"])
    assert list(status.values()) == [abi.fpel_status(s) for s in (abi.SVT_HIP_OK, abi.SVT_HIP_ERR_BAD_PARAMETER, abi.SVT_HIP_ERR_NO_DEVICE, abi.SVT_HIP_ERR_RUNTIME)]
    assert list(status.values())[0] == 0 and all(-32768 <= v < 0 for v in list(status.values())[1:]) and len(set(status.values())) == 4


@pytest.mark.parametrize("mirror", [abi.FpelLevel, abi.FpelDesc, abi.FpelResult, abi.FpelSqCtrls], ids=lambda m: m.__name__)
def test_mirror_has_no_implicit_padding(mirror):
    end = 0
    for f, _ in mirror._fields_:
        assert getattr(mirror, f).offset == end, f"implicit padding before {mirror.__name__}.{f}"
        end += getattr(mirror, f).size
    assert end == C.sizeof(mirror)
    assert [C.sizeof(m) for m in (abi.FpelLevel, abi.FpelDesc, abi.FpelResult, abi.FpelSqCtrls)] == [12, 128, 16, 36]


def test_records_have_the_sizes_and_offsets_the_header_states():
    want = header_values(["sizeof(SvtHipFpelDesc)", "sizeof(SvtHipFpelResult)", "sizeof(SvtHipFpelLevel)", "sizeof(SvtHipFpelSqCtrls)", "offsetof(SvtHipFpelDesc, mv)",
                          "offsetof(SvtHipFpelDesc, level)", "offsetof(SvtHipFpelDesc, mode)", "offsetof(SvtHipFpelDesc, nsq_search_width)",
                          "offsetof(SvtHipFpelResult, best_cost)", "offsetof(SvtHipFpelResult, aux_cost)", "offsetof(SvtHipFpelResult, status)"], ["svt_hip_inter.h"])
    assert list(want.values()) == [128, 16, 12, 36, 52, 76, 112, 119, 4, 8, 14]
    assert abi.FPEL_DESC_DTYPE.itemsize == 128 and abi.FPEL_RESULT_DTYPE.itemsize == 16
    assert abi.FPEL_DESC_DTYPE["mv"].shape == (6,) and abi.FPEL_DESC_DTYPE["level"].shape == (3,)
    # what feeds SvtHipSubpelDesc without a host step: a vector is 4 bytes on both sides, a distortion a uint32_t
    assert abi.FPEL_RESULT_DTYPE.fields["best_mv"][0].itemsize == abi.SUBPEL_DESC_DTYPE.fields["start_mv"][0].itemsize == 4
    assert abi.FPEL_RESULT_DTYPE.fields["best_cost"][0] == abi.SUBPEL_DESC_DTYPE.fields["best_mvp_dist"][0]


def test_restatement_matches_golden(gold, searches):
    """Without the reference: what every GPU test compares with is what the fixture holds."""
    for i, s in enumerate(searches):
        assert s.record() == gold.record(i), (i, s.c)


def test_cases_cover_their_list(searches):
    """The coverage conditions of the golden script, on the restatement's own account of each search"""
    events = _golden_script().coverage(searches)
    assert events["wrap"] > 0 and events["lev0_skip"] > 0
    sizes = {(c.w, c.h) for c in F.CASES}
    assert sizes >= {(4, 4), (4, 16), (16, 4), (8, 8), (16, 16), (64, 16), (64, 64), (128, 128)} and len(F.SIZES) == 22


def test_window_helper_gives_the_fixtures_windows(gold):
    """svt_hip_fpel_sq_windows and the restatement's sq_windows against what md_sq_motion_search itself was observed to search, for the four
    md_sq_mv_search_levels x search_area_multiplier 1 .. 3 x picture distances 1, 2, 8, 16; and on controls of the cases' own."""
    lib = abi.load()

    def helper(ct, sam, dist):
        prm, out = abi.FpelSqCtrls(), (abi.FpelLevel * 3)()
        for f in ("w", "h", "max_w", "max_h", "multiplier", "enabled", "step"):
            getattr(prm, f)[:] = list(getattr(ct, f))
        assert lib.svt_hip_fpel_sq_windows(C.byref(prm), sam, dist, out) is None
        return [F.Level(v.enabled, v.step, v.start_x, v.end_x, v.start_y, v.end_y) for v in out]
    seen = set()
    for (level, sam, dist), want in zip(F.WINDOW_CASES, gold.windows):
        ct = F.sq_level_ctrls(level)
        got = helper(ct, sam, F.scaled_distance(dist))
        assert got == F.sq_windows(ct, sam, F.scaled_distance(dist)), (level, sam, dist)
        assert [tuple(g[2:]) for g in got] == [tuple(int(v) for v in w) for w in want], (level, sam, dist)
        assert [(g.enabled, g.step) for g in got] == [(1, 4), (1, 2), (1, 1)]
        seen |= {tuple(g[2:]) for g in got}
    assert len(F.WINDOW_CASES) == 48 and (-372, 372, -372, 372) in seen and (-126, 126, -126, 126) in seen and (-1, 1, -1, 1) in seen
    assert [F.scaled_distance(d) for d in (1, 2, 8, 16)] == [1, 2, 5, 10]
    for c in F.CASES:
        if c.ctrls is not None:
            assert helper(c.ctrls, c.sam, F.scaled_distance(c.pocd)) == F.case_levels(c), c.name
    # a step of 0: an empty window that keeps its step; NULL pointers: nothing happens
    ct = F.sq_level_ctrls(1)._replace(step=(0, 2, 0))
    assert [(g.step, g[2:]) for g in helper(ct, 1, 1)] == [(0, (0, 0, 0, 0)), (2, (-10, 10, -10, 10)), (0, (0, 0, 0, 0))]
    lib.svt_hip_fpel_sq_windows(None, 1, 1, None)


def test_restatement_is_what_the_reference_does(pin, searches):
    """Every stage of every case through md_full_pel_search itself, md_sq_motion_search and md_nsq_motion_search themselves where they can
    be driven, and the constants and tables the restatement states"""
    assert pin.constants() == [F.SAD, F.VAR, F.SSD, F.ENTROPY, F.L1_LOWRES, F.L1_MIDRES, F.L1_HDRES, F.OPT, F.NONE, abi.FPEL_MAX_MV, abi.FPEL_MAX_MVP, 85,
                               256, 512, 2048, 6]
    assert pin.pu_table() == F.pu_table()
    assert [pin.lib.pin_scaled_distance(d) for d in range(1, 40)] == [F.scaled_distance(d) for d in range(1, 40)]
    g, whole = _golden_script(), 0
    for i, c in enumerate(F.CASES):
        s, w = g.pin_case(pin, c)
        assert s.record() == searches[i].record(), (i, c)
        whole += w
    assert whole >= 30


def test_golden_regenerates_byte_identical(pin):
    with open(F.GOLD, "rb") as f:
        assert f.read() == _golden_script().build(pin)


def test_fixture_is_small():
    assert os.path.getsize(F.GOLD) <= 16 * 1024


def test_new_names_are_exported_with_their_prototypes():
    lib = abi.load()
    for n in NAMES:
        assert n in PROTOTYPES and lib.svt_hip_rtcd_lookup(n[len("svt_hip_"):].encode()) is None
    assert PROTOTYPES["svt_hip_fpel_search_batch"] == ("c_int16", ("c_void_p", "c_void_p", "c_void_p", "c_uint32", "c_void_p"))
    assert PROTOTYPES["svt_hip_fpel_sq_windows"] == (None, ("c_void_p", "c_uint8", "c_uint16", "c_void_p"))
    assert lib.svt_hip_fpel_search_batch.restype is C.c_int16 and lib.svt_hip_fpel_sq_windows.restype is None


def test_status_exports_returning_int16_are_probed_here():
    """tests/test_tier_b_refusals.py takes its census from the exports that return int32_t, tests/test_wiener_pick_abi.py adds those that
    return int, tests/test_rest_pick_abi.py those that return int64_t.  svt_hip_fpel_search_batch returns int16_t (SVT_HIP_FPEL_STATUS of a
    SvtHipStatus): every svt_hip_* export with that return type is listed here with what the census's own child process (its probes, its
    marking of the error text) records for it."""
    import test_tier_b_refusals as T
    bad, none = abi.fpel_status(abi.SVT_HIP_ERR_BAD_PARAMETER), abi.fpel_status(abi.SVT_HIP_ERR_NO_DEVICE)
    assert (bad, none) == (-28667, -28672)
    want = {"svt_hip_fpel_search_batch": [[bad, "svt_hip_fpel_search_batch: bad argument"], [0, None], _no_device_row(none)]}
    assert {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_int16"} == set(want)
    assert not set(want) & set(T.census_names())
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(want)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == want


def _no_device_row(status):
    """What an export that asks for the device answers in a process that never called svt_hip_init: the census's own record of
    svt_hip_subpel_search_batch's third probe, with this export's name and status"""
    with open(os.path.join(F.HERE, "golden", "tier_b_refusals.json")) as f:
        rc, text = json.load(f)["svt_hip_subpel_search_batch"][2]
    assert rc == abi.SVT_HIP_ERR_NO_DEVICE
    return [status, text.replace("svt_hip_subpel_search_batch", "svt_hip_fpel_search_batch")]


def test_refusals_need_no_device():
    """A process that never called svt_hip_init: NULL job, descriptors or results are bad parameters, an empty batch succeeds, anything
    else is SVT_HIP_ERR_NO_DEVICE.  Nothing is launched either way."""
    got = fresh_process("(lambda f: (f(None, p, p, 1, None), f(p, None, p, 1, None), f(p, p, None, 1, None), f(None, None, None, 0, None),"
                        "f(p, p, p, 0, None), f(p, p, p, 1, None)))(lib.svt_hip_fpel_search_batch)")
    bad, none = abi.fpel_status(abi.SVT_HIP_ERR_BAD_PARAMETER), abi.fpel_status(abi.SVT_HIP_ERR_NO_DEVICE)
    assert got == [bad] * 4 + [0, none]
