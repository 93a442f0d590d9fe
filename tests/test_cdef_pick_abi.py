"""CPU: the fixture, the interface and the cases of svt_hip_cdef_pick_strengths (finish_cdef_search on the device).  No compute
call reaches a device here: the workspace helper is layout arithmetic and every refusal comes before the library looks for one."""
import ctypes as C
import os

import numpy as np
import pytest

import cdef_pick_cases as K
from support import assert_not_rtcd_leaf
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

NAMES = ("svt_hip_cdef_pick_strengths", "svt_hip_cdef_pick_workspace_bytes")
IDS = [c.name for c in K.CASES]


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_reference_leaf(ref, case):
    assert K.same(K.golden(case), K.drive(K.make_inputs(case), K.ref_search(ref))) == []


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_oracle_leaf(orc, case):
    assert K.same(K.golden(case), K.drive(K.make_inputs(case), K.orc_search(orc))) == []


def test_fixture_is_no_larger_than_the_leaves_fixture():
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(gold, "cdef_pick.npz")) <= os.path.getsize(os.path.join(gold, "leaves.npz"))


def test_workspace_helper_is_layout_arithmetic():
    """Monotone in both arguments, 0 for empty input, needs no device (the library is not initialised here)."""
    f = abi.load().svt_hip_cdef_pick_workspace_bytes
    assert f(0, 16) == 0 and f(2040, 0) == 0 and f(0, 0) == 0 and f(7, -3) == 0
    grids, lists = (1, 2, 12, 255, 256, 266, 2040, 8160, 1 << 20), range(1, 65)
    sizes = np.array([[f(g, n) for n in lists] for g in grids], np.uint64)
    assert (sizes > 0).all() and (np.diff(sizes.astype(np.int64), axis=0) >= 0).all() and (np.diff(sizes.astype(np.int64), axis=1) >= 0).all()
    assert sizes[0, 0] < sizes[-1, -1]
    # room for what the header promises to keep there: both cost tables, the totals of four widths, one byte per block
    for gi, g in enumerate(grids):
        for n in (1, 16, 64):
            assert sizes[gi, n - 1] >= 2 * g * n * 8 + 4 * n * n * 8 + g
    assert f(2 ** 32 - 1, 64) > 2 ** 32      # a 64-bit return


def test_new_names_are_exported_and_are_not_rtcd_leaves():
    lib = abi.load()
    for n in NAMES:
        assert_not_rtcd_leaf(n)
        assert n in PROTOTYPES and lib.svt_hip_rtcd_lookup(n[len("svt_hip_"):].encode()) is None
    assert PROTOTYPES["svt_hip_cdef_pick_workspace_bytes"] == ("c_uint64", ("c_uint32", "c_int32"))
    assert PROTOTYPES["svt_hip_cdef_pick_strengths"] == ("c_int32", ("c_void_p",) * 7 + ("c_uint64", "c_void_p"))


def test_every_refusal_comes_before_the_device():
    """Each bad call is refused with a message whether or not a device exists; the pointers are never followed."""
    lib = abi.load()
    x = K.make_inputs(K.CASES[3])
    need = lib.svt_hip_cdef_pick_workspace_bytes(x.n_fb, x.case.n)
    n = 0
    for label, change, null, short in K.rejections(x):
        prm = K.rejected_params(x, change)
        args = [C.addressof(prm)] + [0x1000 * (i + 1) for i in range(6)]
        if null:
            args[K.ARGS.index(null)] = None
        rc = lib.svt_hip_cdef_pick_strengths(*args, need - short, None)
        assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER, label
        assert b"svt_hip_cdef_pick_strengths" in lib.svt_hip_last_error(), label
        n += 1
    assert n == 7 + 3 + 3 + 3 + 5


def test_cases_cover_what_the_issue_lists():
    grids = {(c.cols, c.rows) for c in K.CASES}
    assert grids == {(1, 1), (4, 3), (17, 15), (19, 14), (60, 34)}
    assert {c.n for c in K.CASES} == {1, 4, 9, 16, 64}
    assert [c.n for c in K.CASES if (c.cols, c.rows) == (60, 34)] == [16]
    assert {(c.cols, c.rows) for c in K.CASES if c.n == 64} == {(4, 3), (17, 15)}
    assert {c.bits for c in K.CASES if c.kind in ("plain", "quant")} == {8, 24, 40}
    assert {"quant", "equal", "wrap"} <= {c.kind for c in K.CASES}
    assert {c.part for c in K.CASES} == {"all", "half", "one", "none"}
    assert {c.uv for c in K.CASES} == {0, 1} and {c.bias for c in K.CASES} == {0, 62, 63}
    for c in K.CASES:
        x = K.make_inputs(c)
        assert x.mse.shape == (3, c.cols * c.rows, c.n) and (-1 in x.strengths_uv) == bool(c.uv and c.n >= 3)
        part = K.takes_part(x.filt, c.cols, c.rows)
        assert int(part.sum()) == {"all": part.size, "one": 1, "none": 0}.get(c.part, int(part.sum())) == int(K.golden(c)["result"]["sb_count"])
        if c.part == "half":
            assert 0 < part.sum() < part.size
        if c.kind == "wrap":
            assert (x.mse == np.uint64(1 << 62)).all()
        if c.kind == "quant":
            assert not (x.mse % np.uint64(64)).any()


def test_cases_reach_what_they_are_meant_to_reach():
    """Conditions on the recorded results of the reference (not measurements of the code under test)."""
    gold = {c.name: K.golden(c) for c in K.CASES}
    res = {k: g["result"] for k, g in gold.items()}
    assert {int(r["cdef_bits"]) for r in res.values()} == {0, 1, 2, 3}
    refined = [k for k, g in gold.items()
               if not (np.array_equal(g["greedy0"], g["result"]["lev0"]) and np.array_equal(g["greedy1"], g["result"]["lev1"]))]
    assert len(refined) >= 3, refined
    assert sum(int(g["tied"]) >= 2 for g in gold.values()) >= 3
    twice = [k for k, r in res.items()
             if len({(int(a), int(b)) for a, b in zip(r["y_index"][:r["nb_strengths"]], r["uv_index"][:r["nb_strengths"]])}) < r["nb_strengths"]]
    assert twice, "no winner list holds a pair twice"
    none = [r for c, r in zip(K.CASES, res.values()) if c.part == "none"]
    assert none and all(r["sb_count"] == 0 and r["cdef_bits"] == 0 for r in none)
    for r in res.values():      # the record is consistent in itself
        assert r["nb_strengths"] == 1 << r["cdef_bits"] and r["best_cost"] == r["rd_cost"][r["cdef_bits"]] == r["rd_cost"].min()
        for i in range(4):
            assert not r["lev0"][i][1 << i:].any() and not r["lev1"][i][1 << i:].any()
