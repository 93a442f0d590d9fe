"""CPU: the fixture, the interface and the cases of svt_hip_dlf_pick_levels / svt_hip_dlf_apply_picked (search_filter_level on the
device).  No compute call reaches a device here: the workspace helper is layout arithmetic and every refusal comes before the library
looks for one."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dlf_pick_cases as K
import lf_cases as L
from support import assert_not_rtcd_leaf, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

NAMES = ("svt_hip_dlf_pick_levels", "svt_hip_dlf_apply_picked", "svt_hip_dlf_pick_workspace_bytes")
IDS = [c.name for c in K.CASES]


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_reference(ref, case):
    x = K.make_inputs(case)
    assert K.same(K.golden(case), K.drive(x, K.ref_filter(ref, x), K.ref_sse(ref, x))) == []


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_oracle(orc, case):
    x = K.make_inputs(case)
    assert K.same(K.golden(case), K.drive(x, K.orc_filter(orc, x), K.numpy_sse(x))) == []


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_mode_info_grid_is_the_reference_gather(ref, case):
    """dlf_pick_cases derives the SvtHipLfMi records from the AV1 specification's rules; the reference's tables give the same."""
    x = K.make_inputs(case)
    m = L.RefLfModeInfo(*[x.minfo[k].ctypes.data for k in ("bsize", "tx_depth", "skip", "ref_frame0", "mode", "segment_id")])
    flat = np.zeros((x.mi_rows, x.mi_stride), abi.LF_MI_DTYPE)
    ref.ref_lf_gather(x.mi_rows * x.mi_stride, C.byref(m), L.P(flat))
    assert flat.tobytes() == x.flat.tobytes()


def test_fixture_is_no_larger_than_the_frame_fixture():
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(gold, "dlf_pick.npz")) <= os.path.getsize(os.path.join(gold, "dlf.npz"))


def test_mirrors_constants_and_record_layout():
    """The device record has no implicit padding and the size the header states; abi.py states the header's constants."""
    end = 0
    for f, _ in abi.DlfPickResult._fields_:
        assert getattr(abi.DlfPickResult, f).offset == end, f"implicit padding before DlfPickResult.{f}"
        end += getattr(abi.DlfPickResult, f).size
    want = header_values(["SVT_HIP_DLF_PICK_RESULT_BYTES", "SVT_HIP_DLF_MAX_LEVEL", "SVT_HIP_DLF_PICK_DEFAULT_ROUNDS", "sizeof(SvtHipDlfPickResult)"])
    assert end == C.sizeof(abi.DlfPickResult) == want["sizeof(SvtHipDlfPickResult)"] == want["SVT_HIP_DLF_PICK_RESULT_BYTES"] == abi.DLF_PICK_RESULT_BYTES
    assert (abi.DLF_MAX_LEVEL, abi.DLF_PICK_DEFAULT_ROUNDS) == (want["SVT_HIP_DLF_MAX_LEVEL"], want["SVT_HIP_DLF_PICK_DEFAULT_ROUNDS"])
    assert abi.DLF_PICK_RESULT_DTYPE["ss_err"].shape == (3, 64) and abi.DLF_PICK_RESULT_DTYPE["hdr_level"].shape == (4,)
    # the recommended default: the largest `rounds` the fixture records, plus 4
    assert abi.DLF_PICK_DEFAULT_ROUNDS == max(int(K.golden(c)["record"]["rounds"].max()) for c in K.CASES) + 4


def test_workspace_helper_is_layout_arithmetic():
    """Monotone in both dimensions, 0 for an empty picture, a 64-bit return, no device (the library is not initialised here)."""
    f = abi.load().svt_hip_dlf_pick_workspace_bytes
    assert f(0, 0, 0) == 0 and f(0, 2160, 1) == 0 and f(3840, 0, 1) == 0
    dims = (8, 40, 200, 1920, 3840, 7680, 65536)
    for is16 in (0, 1):
        sizes = np.array([[f(w, h, is16) for w in dims] for h in dims], np.int64)
        assert (sizes >= 256).all() and (np.diff(sizes, axis=0) >= 0).all() and (np.diff(sizes, axis=1) >= 0).all()
    assert PROTOTYPES["svt_hip_dlf_pick_workspace_bytes"][0] == "c_uint64" and f.restype is C.c_uint64


def test_new_names_are_exported_and_are_not_rtcd_leaves():
    lib = abi.load()
    for n in NAMES:
        assert_not_rtcd_leaf(n)
        assert n in PROTOTYPES and lib.svt_hip_rtcd_lookup(n[len("svt_hip_"):].encode()) is None
    assert PROTOTYPES["svt_hip_dlf_pick_workspace_bytes"] == ("c_uint64", ("c_uint32", "c_uint32", "c_int32"))
    assert PROTOTYPES["svt_hip_dlf_pick_levels"] == ("c_uint32", ("c_void_p",) * 3 + ("c_uint64", "c_void_p"))
    assert PROTOTYPES["svt_hip_dlf_apply_picked"] == ("c_uint32", ("c_void_p",) * 3)


def test_every_refusal_comes_before_the_device():
    """Each bad call is refused with a message that names the function whether or not a device exists; no pointer is followed."""
    lib = abi.load()
    x = K.make_inputs(K.CASE["small_10bit_seg"])
    fake = [(0x10000 * (p + 1), x.recon[p].shape[1]) for p in range(3)]
    need = lib.svt_hip_dlf_pick_workspace_bytes(x.case.w, x.case.h, x.case.is16)
    n = n_apply = 0
    for label, change, null, short, applies in K.rejections(x):
        prm = K.params(x, fake, fake, 0x80000)
        if change:
            change(prm)
        args = [C.addressof(prm), 0x90000, 0xA0000]
        if null:
            args[K.ARGS.index(null)] = None
        rc = lib.svt_hip_dlf_pick_levels(*args, need - short, None)
        assert rc == K.BAD_PARAMETER, label
        assert b"svt_hip_dlf_pick_levels" in lib.svt_hip_last_error(), label
        n += 1
        if not applies:     # the frame call with picked levels reads neither the workspace, the search's own fields nor the source
            continue
        rc = lib.svt_hip_dlf_apply_picked(*args[:2], None)
        assert rc == K.BAD_PARAMETER, label
        assert b"svt_hip_dlf_apply_picked" in lib.svt_hip_last_error(), label
        n_apply += 1
    assert (n, n_apply) == (3 + 3 + 2 + 2 + 3 + 4 + 1 + 2 + 15, 2 + 2 + 2 + 15)
    for bad in (0x90004, 0x90001):      # record and workspace must be 8-byte aligned
        prm = K.params(x, fake, fake, 0x80000)
        assert lib.svt_hip_dlf_pick_levels(C.addressof(prm), bad, 0xA0000, need, None) == K.BAD_PARAMETER
        assert lib.svt_hip_dlf_pick_levels(C.addressof(prm), 0x90000, bad, need, None) == K.BAD_PARAMETER
        assert lib.svt_hip_dlf_apply_picked(C.addressof(prm), bad, None) == K.BAD_PARAMETER


def test_probes_of_an_uninitialised_library_match_their_fixture():
    """The three probes of the Tier B census (tests/test_tier_b_refusals.py), for the two status exports of this feature: the same
    return code and the same text, byte for byte, and every one a refusal that names its function before a device is asked for."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dlf_pick_refusals.json")) as f:
        gold = json.load(f)
    assert sorted(gold) == sorted(K.STATUS_NAMES) and K.refusal_probes() == gold
    # so that no export stays unprobed for the spelling of its return type: every svt_hip_* export that returns uint32_t is one of
    # these two or a count that takes no pointer
    others = {n for n, (restype, args) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_uint32"} - set(K.STATUS_NAMES)
    assert all("c_void_p" not in PROTOTYPES[n][1] for n in others), others
    for name, rows in gold.items():
        assert [rc for rc, _ in rows] == [K.BAD_PARAMETER] * 3 and all(text.startswith(name + ":") for _, text in rows)


def test_cases_cover_what_the_issue_lists():
    assert {(c.w, c.h) for c in K.CASES} >= {(40, 24), (200, 136)}
    assert {(c.bd, c.is16) for c in K.CASES} == {(8, 0), (10, 1), (8, 1)} and {c.sb for c in K.CASES} == {64, 128}
    assert {c.pitch > 0 for c in K.CASES} == {False, True} and {c.area for c in K.CASES} == {"aligned", "cropped"}
    assert {c.seg for c in K.CASES} == {0, 1} and {c.only4 for c in K.CASES} == {0, 1} and {c.conv for c in K.CASES} == {0, 1, 2}
    assert {c.mask for c in K.CASES} == {7, 1, 6}
    assert {s for c in K.CASES for p, s in enumerate(c.start) if (c.mask >> p) & 1} >= {0, 15, 16, 40, 63}
    for c in K.CASES:
        x = K.make_inputs(c)
        wa, ha = x.mi_cols * 4, x.mi_rows * 4
        assert (x.mi_stride > x.mi_cols) == (c.pitch > 0) and wa >= c.w and ha >= c.h
        smaller = [x.sse_w[p] < (wa >> (p > 0)) or x.sse_h[p] < (ha >> (p > 0)) for p in range(3)]
        assert all(smaller) == (c.area == "cropped") and any(smaller) == (c.area == "cropped"), c.name
        if (c.w, c.h) == (200, 136):    # at least 3 tiles of 64 x 64 each way, ragged on both sides
            assert wa > 3 * 64 and ha > 2 * 64 and wa % 64 and ha % 64
        for p in range(3):              # the reconstruction differs from the source in every plane
            assert not np.array_equal(x.recon[p], x.src[p])


def test_cases_reach_what_they_are_meant_to_reach():
    """Conditions on the recorded results of the reference (not measurements of the code under test)."""
    gold = {c.name: K.golden(c) for c in K.CASES}
    searched = [(c, p) for c in K.CASES for p in range(3) if (c.mask >> p) & 1]
    levels = [int(gold[c.name]["record"]["level"][p]) for c, p in searched]
    assert 0 in levels and any(1 <= v <= 15 for v in levels) and any(v >= 32 for v in levels)
    ups = downs = 0
    for c, p in searched:
        path = [int(v) for v in gold[c.name]["path"][p] if v >= 0]
        d = np.sign(np.diff(path))
        ups += any(d[i] > 0 and d[i + 1] > 0 for i in range(len(d) - 1))
        downs += any(d[i] < 0 and d[i + 1] < 0 for i in range(len(d) - 1))
    assert ups and downs
    assert any(gold[c.name]["conv_exit"][p] for c, p in searched)
    assert any(gold[c.name]["both"][p] for c, p in searched) and any(gold[c.name]["none"][p] for c, p in searched)
    assert any(int(gold[c.name]["record"]["level"][0]) == 0 for c in K.CASES if c.mask & 1)
    for c in K.CASES:
        rec = gold[c.name]["record"]
        assert int(rec["finished"]) == c.mask and int(rec["pad_"]) == 0
        for p in range(3):
            tried = int((rec["ss_err"][p] >= 0).sum())
            if (c.mask >> p) & 1:
                assert 3 <= tried <= 30 and tried == rec["trials"][p] and 1 <= rec["rounds"][p] <= rec["trials"][p]
                assert rec["best_err"][p] == rec["ss_err"][p][rec["level"][p]] >= 0
            else:
                assert tried == 0 and (rec["level"][p], rec["rounds"][p], rec["trials"][p], rec["best_err"][p]) == (0, 0, 0, 0)
        lv = [int(rec["level"][q]) if (c.mask >> q) & 1 else None for q in range(3)]
        want = [K.HOST_LEVELS[0] if lv[0] is None else lv[0], K.HOST_LEVELS[1] if lv[0] is None else lv[0],
                K.HOST_LEVELS[2] if lv[1] is None else lv[1], K.HOST_LEVELS[3] if lv[2] is None else lv[2]]
        assert list(rec["hdr_level"]) == want


def test_driver_stops_at_max_rounds(orc):
    """With two rounds the driver keeps what it measured, clears `finished`, and agrees with the full run on every entry it has."""
    case = K.CASE["tiles_8bit_harsh"]
    x = K.make_inputs(case)
    short, full = K.drive(x, K.orc_filter(orc, x), K.numpy_sse(x), max_rounds=2)["record"], K.golden(case)["record"]
    assert short["finished"] == 0 and (short["rounds"] == 2).all() and (full["rounds"] > 2).all()
    tried = short["ss_err"] >= 0
    assert (tried.sum(axis=1) == short["trials"]).all() and np.array_equal(short["ss_err"][tried], full["ss_err"][tried])
