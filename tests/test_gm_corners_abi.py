"""CPU: the fixture, the restatement and the interface of svt_hip_gm_detect_corners / svt_hip_gm_match_corners (the corner detection and the
correspondences of global motion on the device).  No compute call reaches a device here: the workspace query is layout arithmetic and every
refusal comes before the library looks for one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gm_cases as K
from support import assert_not_rtcd_leaf, fresh_process, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

NAMES = K.STATUS_NAMES + ("svt_hip_gm_corners_workspace_bytes",)


# ---- the fixture is the reference, the restatement is the fixture -------------------------------------------------------------

@pytest.mark.parametrize("plane", K.PLANES, ids=lambda p: p.name)
def test_restated_detection_equals_the_fixture(plane):
    buf = K.plane_buf(plane.name)
    assert buf.shape == (plane.h, plane.stride) and np.array_equal(buf, K.make_plane(plane))
    count, found, xy = K.detect(buf, plane.w)
    want = K.golden_corners(plane.name)
    assert (count, found) == want[:2] and np.array_equal(xy, want[2])


@pytest.mark.parametrize("case", K.MATCHES, ids=lambda m: m.name)
def test_restated_matching_equals_the_fixture(case):
    assert np.array_equal(K.restated_matches(case), K.golden_matches(case.name))


@pytest.mark.parametrize("plane", K.PLANES, ids=lambda p: p.name)
def test_fixture_is_the_reference_detection(ref, plane):
    count, found, xy = K.ref_detect(ref, K.plane_buf(plane.name), plane.w)
    want = K.golden_corners(plane.name)
    assert (count, found) == want[:2] and np.array_equal(xy, want[2])


@pytest.mark.parametrize("case", K.MATCHES, ids=lambda m: m.name)
def test_fixture_is_the_reference_matching(ref, case):
    assert np.array_equal(K.ref_matches(ref, case), K.golden_matches(case.name))


def test_cases_are_what_the_list_asks_for():
    """Conditions on the reference's recorded output (not measurements of the code under test)."""
    corners = {p.name: K.golden_corners(p.name) for p in K.PLANES}
    assert set(K.DETECT_LISTED) <= set(corners) and len({(K.PLANE[n].w, K.PLANE[n].h) for n in K.DETECT_BATCH}) == 3
    assert 150 <= corners["noise_64x48"][0] <= 400 and K.PLANE["noise_64x48"].stride == 80
    for n in ("tiny_7x7", "tiny_9x6", "flat_20x20", "flat_64x48"):
        assert corners[n][:2] == (0, 0), n
    assert corners["tiny_7x7_corner"][:2] == (1, 1)
    assert [tuple(v) for v in corners["hand_32x24"][2]] == K.HAND_CORNERS
    assert corners["dots_300x300"][:2] == (abi.GM_MAX_CORNERS, 5476) and len(corners["dots_300x300"][2]) == abi.GM_MAX_CORNERS
    for name, (count, found, xy) in corners.items():       # raster order, inside the tested rectangle
        p = K.PLANE[name]
        assert count == len(xy) == min(found, abi.GM_MAX_CORNERS)
        key = xy[:, 1].astype(np.int64) * 65536 + xy[:, 0]
        assert (np.diff(key) > 0).all() and ((xy >= 3) & (xy < np.array([p.w, p.h]) - 3)).all(), name
    traces = {}
    for m in K.MATCHES:
        traces[m.name] = {}
        K.restated_matches(m, traces[m.name])
    pts = {m.name: K.golden_matches(m.name) for m in K.MATCHES}
    assert all(len(pts[n]) >= 16 for n in K.NOISE_MATCHES)
    assert {(m.match_sz, m.frm_quarters) for m in K.MATCHES} >= {(7, 4), (13, 4), (7, 2), (13, 2)}
    assert sum(t["skipped"] for n, t in traces.items() if K.MATCH[n].match_sz == 13) > 0
    assert sum(t["moved1"] for t in traces.values()) > 0 and sum(t["moved2"] for t in traces.values()) > 0
    assert traces["sparse_sz7"]["nan"] > 0 and len(pts["sparse_sz7"]) == 20 and list(pts["sparse_sz7"][0]) == [10, 10, 13, 12]
    assert len(pts["dots_self"]) == abi.GM_MAX_CORNERS and (pts["dots_self"][:2] == 4).all()
    assert len(pts["empty_frm"]) == 0 and len(pts["empty_ref"]) == 0
    assert len({K.MATCH[n].frm for n in K.SHARED}) == 1 and len({K.MATCH[n].ref for n in K.SHARED}) >= 2


def test_fixture_is_small():
    assert os.path.getsize(K.GOLD) <= 256 * 1024


# ---- the interface --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [abi.GmPlane, abi.GmCorners, abi.GmMatchJob, abi.GmMatches], ids=lambda m: m.__name__)
def test_mirror_has_no_implicit_padding(mirror):
    end = 0
    for f, _ in mirror._fields_:
        assert getattr(mirror, f).offset == end, f"implicit padding before {mirror.__name__}.{f}"
        end += getattr(mirror, f).size
    assert end == C.sizeof(mirror)


def test_records_and_constants_are_the_headers():
    want = header_values(["sizeof(SvtHipGmPlane)", "sizeof(SvtHipGmCorners)", "sizeof(SvtHipGmMatchJob)", "sizeof(SvtHipGmMatches)",
                          "offsetof(SvtHipGmCorners, xy)", "offsetof(SvtHipGmMatches, pts)", "offsetof(SvtHipGmMatchJob, frm_corners)",
                          "offsetof(SvtHipGmMatchJob, match_sz)", "SVT_HIP_GM_MAX_CORNERS", "SVT_HIP_GM_MAX_PLANES", "SVT_HIP_GM_MAX_MATCH_SZ"],
                         ["svt_hip_inter.h"])
    assert list(want.values()) == [24, 8 + 8 * 4096, 72, 8 + 16 * 4096, 8, 8, 48, 66, 4096, 8, 13]
    assert [C.sizeof(m) for m in (abi.GmPlane, abi.GmCorners, abi.GmMatchJob, abi.GmMatches)] == list(want.values())[:4]
    assert (abi.GM_MAX_CORNERS, abi.GM_MAX_PLANES, abi.GM_MAX_MATCH_SZ) == tuple(want.values())[8:]
    assert abi.GM_CORNERS_DTYPE["xy"].shape == (8192,) and abi.GM_MATCHES_DTYPE["pts"].shape == (16384,)
    assert abi.GM_MATCHES_DTYPE.itemsize <= 64 * 1024 + 8       # what a caller downloads per pair
    status = header_values([f"SVT_HIP_GM_STATUS({s})" for s in ("SVT_HIP_OK", "SVT_HIP_ERR_NO_DEVICE", "SVT_HIP_ERR_BAD_PARAMETER", "SVT_HIP_ERR_RUNTIME")])
    assert list(status.values()) == [0, 0x1000, 0x1005, 0x1001]
    assert list(status.values()) == [abi.gm_status(s) for s in (abi.SVT_HIP_OK, abi.SVT_HIP_ERR_NO_DEVICE, abi.SVT_HIP_ERR_BAD_PARAMETER, abi.SVT_HIP_ERR_RUNTIME)]


def test_new_names_are_exported_with_their_prototypes():
    lib = abi.load()
    for n in NAMES:
        assert_not_rtcd_leaf(n)
        assert n in PROTOTYPES
    assert PROTOTYPES["svt_hip_gm_corners_workspace_bytes"] == ("c_uint64", ("c_uint32", "c_uint32", "c_uint32"))
    assert PROTOTYPES["svt_hip_gm_detect_corners"] == ("c_uint16", ("c_void_p", "c_uint32", "c_void_p", "c_void_p", "c_uint64", "c_void_p"))
    assert PROTOTYPES["svt_hip_gm_match_corners"] == ("c_uint16", ("c_void_p", "c_uint32", "c_void_p", "c_void_p"))
    assert lib.svt_hip_gm_detect_corners.restype is C.c_uint16 and lib.svt_hip_gm_match_corners.restype is C.c_uint16
    assert lib.svt_hip_gm_corners_workspace_bytes.restype is C.c_uint64


def test_workspace_query_is_layout_arithmetic():
    """No device (the library is not initialised here), monotonic in each argument, a 64-bit return, and the sum rule for a call over
    planes of different sizes."""
    f = abi.load().svt_hip_gm_corners_workspace_bytes
    dims, counts = (1, 7, 64, 131, 300, 1920, 3840, 16384), (0, 1, 2, 3, 8)
    sizes = np.array([[[f(w, h, n) for w in dims] for h in dims] for n in counts], np.int64)
    for axis in range(3):
        assert (np.diff(sizes, axis=axis) >= 0).all()
    assert (sizes[0] == 0).all() and (sizes[1] >= np.outer(dims, dims)).all()      # at least the byte score map
    assert f(16384, 16384, 8) > 2 ** 31 and f(3840, 2160, 3) == 3 * f(3840, 2160, 1)
    assert K.workspace_bytes(abi.load(), K.DETECT_BATCH) <= f(131, 97, 3)


# ---- refusals ---------------------------------------------------------------------------------------------------------------

FAKE = 0x10000      # never followed: every call below is refused before the library asks for a device


def _planes(*specs):
    arr = (abi.GmPlane * len(specs))()
    for i, (ptr, w, h, stride) in enumerate(specs):
        arr[i] = abi.GmPlane(ptr, w, h, stride, 0)
    return arr


def _job(**kw):
    j = abi.GmMatchJob(abi.GmPlane(FAKE, 64, 48, 64, 0), abi.GmPlane(2 * FAKE, 64, 48, 80, 0), 3 * FAKE, 4 * FAKE, 4, 4, 7)
    for k, v in kw.items():
        obj, _, field = k.rpartition("__")
        setattr(getattr(j, obj) if obj else j, field, v)
    return j


def test_every_detect_refusal_comes_before_the_device():
    lib = abi.load()
    f, ok = lib.svt_hip_gm_detect_corners, _planes((FAKE, 64, 48, 80))
    need = lib.svt_hip_gm_corners_workspace_bytes(64, 48, 1)
    nine = _planes(*[(FAKE, 64, 48, 80)] * 9)
    calls = {
        "NULL planes": (None, 1, 5 * FAKE, 6 * FAKE, need),
        "NULL records": (ok, 1, None, 6 * FAKE, need),
        "NULL workspace": (ok, 1, 5 * FAKE, None, need),
        "nine planes": (nine, 9, 5 * FAKE, 6 * FAKE, 9 * need),
        "NULL luma": (_planes((None, 64, 48, 80)), 1, 5 * FAKE, 6 * FAKE, need),
        "no width": (_planes((FAKE, 0, 48, 80)), 1, 5 * FAKE, 6 * FAKE, need),
        "no height": (_planes((FAKE, 64, 0, 80)), 1, 5 * FAKE, 6 * FAKE, need),
        "short stride": (_planes((FAKE, 64, 48, 63)), 1, 5 * FAKE, 6 * FAKE, need),
        "second plane empty": (_planes((FAKE, 64, 48, 80), (FAKE, 0, 0, 0)), 2, 5 * FAKE, 6 * FAKE, 2 * need),
        "workspace one byte short": (ok, 1, 5 * FAKE, 6 * FAKE, need - 1),
        "workspace for one plane of two": (_planes((FAKE, 64, 48, 80), (FAKE, 64, 48, 80)), 2, 5 * FAKE, 6 * FAKE, need),
    }
    for label, args in calls.items():
        assert f(*args, None) == K.BAD_PARAMETER, label
        assert lib.svt_hip_last_error().startswith(b"svt_hip_gm_detect_corners:"), label
    assert f(ok, 0, 5 * FAKE, 6 * FAKE, 0, None) == 0      # an empty call is fine and launches nothing


def test_every_match_refusal_comes_before_the_device():
    lib = abi.load()
    f = lib.svt_hip_gm_match_corners
    one = lambda **kw: (abi.GmMatchJob * 1)(_job(**kw))       # noqa: E731
    calls = {
        "NULL jobs": (None, 1, 5 * FAKE),
        "NULL records": (one(), 1, None),
        "nine jobs": ((abi.GmMatchJob * 9)(*[_job()] * 9), 9, 5 * FAKE),
        "NULL frame": (one(frm__luma=None), 1, 5 * FAKE),
        "NULL reference": (one(ref__luma=None), 1, 5 * FAKE),
        "NULL frame corners": (one(frm_corners=None), 1, 5 * FAKE),
        "NULL reference corners": (one(ref_corners=None), 1, 5 * FAKE),
        "empty frame": (one(frm__width=0, ref__width=0), 1, 5 * FAKE),
        "empty reference": (one(ref__height=0), 1, 5 * FAKE),
        "frame stride": (one(frm__stride=63), 1, 5 * FAKE),
        "reference stride": (one(ref__stride=60), 1, 5 * FAKE),
        "unequal widths": (one(ref__width=62), 1, 5 * FAKE),
        "unequal heights": (one(frm__height=40), 1, 5 * FAKE),
        "frame quarters 0": (one(frm_quarters=0), 1, 5 * FAKE),
        "frame quarters 5": (one(frm_quarters=5), 1, 5 * FAKE),
        "reference quarters 0": (one(ref_quarters=0), 1, 5 * FAKE),
        "reference quarters 5": (one(ref_quarters=5), 1, 5 * FAKE),
        "match_sz 8": (one(match_sz=8), 1, 5 * FAKE),
        "match_sz 15": (one(match_sz=15), 1, 5 * FAKE),
        "match_sz 1": (one(match_sz=1), 1, 5 * FAKE),
        "second job bad": ((abi.GmMatchJob * 2)(_job(), _job(match_sz=6)), 2, 5 * FAKE),
    }
    for label, args in calls.items():
        assert f(*args, None) == K.BAD_PARAMETER, label
        assert lib.svt_hip_last_error().startswith(b"svt_hip_gm_match_corners:"), label
    assert f(one(), 0, 5 * FAKE, None) == 0


def test_good_arguments_ask_for_the_device():
    """A process that never called svt_hip_init: what passes every check gets as far as SVT_HIP_ERR_NO_DEVICE, nothing is launched."""
    got = fresh_process(
        "(lambda pl, job: (lib.svt_hip_gm_detect_corners(pl, 1, 0x50000, 0x60000, lib.svt_hip_gm_corners_workspace_bytes(64, 48, 1), None),"
        " lib.svt_hip_gm_match_corners(job, 1, 0x50000, None)))"
        "((abi.GmPlane * 1)(abi.GmPlane(0x10000, 64, 48, 80, 0)),"
        " (abi.GmMatchJob * 1)(abi.GmMatchJob(abi.GmPlane(0x10000, 64, 48, 64, 0), abi.GmPlane(0x20000, 64, 48, 80, 0), 0x30000, 0x40000, 4, 4, 7)))")
    assert got == [K.NO_DEVICE, K.NO_DEVICE]


def test_status_exports_returning_uint16_are_probed_here():
    """tests/test_tier_b_refusals.py takes its census from the exports that return int32_t; the other spellings of the status are pinned
    by the ABI tests of their features.  The two exports here return uint16_t (SVT_HIP_GM_STATUS of a SvtHipStatus): every svt_hip_*
    export with that return type is listed with what the census's own child process (its three probes, its marking of the error text)
    records for it, and every probe is a refusal that names its function before a device is asked for."""
    import test_tier_b_refusals as T
    want = {
        "svt_hip_gm_detect_corners": [[K.BAD_PARAMETER, "svt_hip_gm_detect_corners: NULL argument"], [0, None],
                                      [K.BAD_PARAMETER, "svt_hip_gm_detect_corners: plane 0: NULL plane (0 x 0, stride 0)"]],
        "svt_hip_gm_match_corners": [[K.BAD_PARAMETER, "svt_hip_gm_match_corners: NULL argument"], [0, None],
                                     [K.BAD_PARAMETER, "svt_hip_gm_match_corners: job 0: frame: NULL plane (0 x 0, stride 0)"]],
    }
    assert {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_uint16"} == set(want) == set(K.STATUS_NAMES)
    assert not set(want) & set(T.census_names())
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(want)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == want
