"""CPU: the fixture, the interface and the cases of svt_hip_wiener_pick_plane (the Wiener decision of a plane on the device).  No
compute call reaches a device here: the workspace helper is layout arithmetic and every refusal comes before the library looks for one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wiener_pick_cases as K
from support import assert_not_rtcd_leaf, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

NAMES = ("svt_hip_wiener_pick_plane", "svt_hip_wiener_pick_workspace_bytes")
IDS = [c.name for c in K.CASES]


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_reference_leaves(ref, case):
    x = K.make_inputs(case)
    assert K.same(K.golden(case), K.drive(x, K.RefLeaves(x, ref))) == []


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_oracle_leaves(orc, case):
    x = K.make_inputs(case)
    assert K.same(K.golden(case), K.drive(x, K.OrcLeaves(x, orc))) == []


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    return K.Pin(ref, tmp_path_factory.mktemp("wiener_pick_pin"))


def test_restatement_is_what_the_reference_does(pin, ref):
    """The driver's integer solver, score, bit count and cost against the reference's own static functions (restoration_pick.c),
    over the statistics of every unit of every case and over random taps and costs."""
    assert pin.constants() == [*K.TAP_MIN, *K.TAP_MAX, *K.INIT[:4], 5, K.SCALE, K.STEP, 8, 9]
    n = 0
    for case in K.CASES:
        x = K.make_inputs(case)
        leaves = K.RefLeaves(x, ref)
        for limits in x.limits:
            M, H = leaves.stats(limits)
            v, h, score, _ = K.solve(case.win, M, H)
            assert (v, h, score) == pin.solve(case.win, M, H), (case.name, limits)
            n += 1
    assert n >= 50
    rng = np.random.default_rng(77)
    taps = lambda: [int(rng.integers(K.TAP_MIN[p], K.TAP_MAX[p] + 1)) for p in range(3)]      # noqa: E731
    for i in range(400):
        win = (7, 5)[i & 1]
        v, h, rv, rh = taps(), taps(), taps(), taps()
        assert K.count_wiener_bits(win, v, h, rv, rh) == pin.count_bits(win, v, h, rv, rh), (win, v, h, rv, rh)
    for p in range(3):          # every (reference, value) pair of every tap
        for r in range(K.TAP_MIN[p], K.TAP_MAX[p] + 1):
            for t in range(K.TAP_MIN[p], K.TAP_MAX[p] + 1):
                v, rv = list(K.INIT[:3]), list(K.INIT[:3])
                v[p], rv[p] = t, r
                assert K.count_wiener_bits(7, v, v, rv, rv) == pin.count_bits(7, v, v, rv, rv), (p, r, t)
    for _ in range(300):
        rdmult, rate, dist = int(rng.integers(1, 1 << 31)), int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 62))
        assert np.float64(K.rdcost_dbl(rdmult, rate, dist)).tobytes() == np.float64(pin.rdcost_dbl(rdmult, rate, dist)).tobytes()


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wiener_pick.npz")) <= 64 * 1024


def test_records_have_the_sizes_and_offsets_the_header_states():
    want = header_values(["SVT_HIP_WIENER_PICK_UNIT_BYTES", "sizeof(SvtHipWienerPickUnit)", "sizeof(SvtHipWienerPickResult)",
                          "sizeof(SvtHipWienerPickParams)", "offsetof(SvtHipWienerPickUnit, hfilter)", "offsetof(SvtHipWienerPickUnit, bits)",
                          "offsetof(SvtHipWienerPickUnit, trials)", "offsetof(SvtHipWienerPickResult, cost)"], ["svt_hip_lf.h"])
    assert list(want.values()) == [64, 64, 56, 40, 16, 48, 60, 40]
    assert abi.WIENER_PICK_UNIT_BYTES == C.sizeof(abi.WienerPickUnit) == K.UNIT_DTYPE.itemsize == 64
    assert C.sizeof(abi.WienerPickResult) == K.RESULT_DTYPE.itemsize == 56 and C.sizeof(abi.WienerPickParams) == 40
    for mirror in (abi.WienerPickParams, abi.WienerPickUnit, abi.WienerPickResult):      # no implicit padding
        end = 0
        for f, _ in mirror._fields_:
            assert getattr(mirror, f).offset == end, (mirror.__name__, f)
            end += getattr(mirror, f).size
        assert end == C.sizeof(mirror)
    assert K.RESULT_DTYPE["cost"].base == np.dtype("<f8") and K.UNIT_DTYPE["sse"].shape == (2,)


def test_workspace_helper_is_layout_arithmetic():
    """Monotone, 0 for an empty plane, needs no device (the library is not initialised here)."""
    f = abi.load().svt_hip_wiener_pick_workspace_bytes
    assert f(0) == 0
    sizes = np.array([f(n) for n in (1, 2, 6, 120, 121, 4096, 65535)], np.int64)
    assert (sizes > 0).all() and (np.diff(sizes) >= 0).all() and sizes[0] < sizes[-1]
    assert f(2 ** 32 - 1) > 2 ** 32      # a 64-bit return


def test_new_names_are_exported_and_are_not_rtcd_leaves():
    lib = abi.load()
    for n in NAMES:
        assert_not_rtcd_leaf(n)
        assert n in PROTOTYPES and lib.svt_hip_rtcd_lookup(n[len("svt_hip_"):].encode()) is None
    assert PROTOTYPES["svt_hip_wiener_pick_workspace_bytes"] == ("c_uint64", ("c_uint32",))
    assert PROTOTYPES["svt_hip_wiener_pick_plane"] == ("c_int", ("c_void_p", "c_void_p", "c_uint32") + ("c_void_p",) * 7 + ("c_uint64", "c_void_p"))


def test_status_exports_outside_the_int32_census_are_probed_here():
    """tests/test_tier_b_refusals.py takes its census from the exports that return int32_t.  svt_hip_wiener_pick_plane returns int, and so
    that no export can stay unprobed for the spelling of its return type, every svt_hip_* export that returns int is listed here
    with what the census's own child process (its probes, its marking of the error text) records for it."""
    import test_tier_b_refusals as T
    bad = abi.SVT_HIP_ERR_BAD_PARAMETER
    want = {"svt_hip_wiener_pick_plane": [[bad, "svt_hip_wiener_pick_plane: NULL argument"], [bad, "svt_hip_wiener_pick_plane: 0 units (1..65535)"],
                                          [bad, "svt_hip_wiener_pick_plane: wiener_win 0 is neither 7 nor 5"]]}
    assert {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_int"} == set(want)
    assert not set(want) & set(T.census_names())
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(want)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == want


def test_every_refusal_comes_before_the_device():
    """Each bad call is refused with a message whether or not a device exists; the device pointers are never followed."""
    lib = abi.load()
    x = K.make_inputs(K.CASES[0])
    n_units = len(x.limits)
    need = lib.svt_hip_wiener_pick_workspace_bytes(n_units)
    n = 0
    for label, change, limits, null, count, short in K.rejections(x):
        prm, units = K.params(x), K.wiener_units(x, 0x10000, 0x20000)
        for k, v in change.items():
            setattr(prm, k, v)
        for k, v in limits.items():
            setattr(units[0], k, v)
        args = dict(zip(K.ARGS, [C.addressof(prm), C.addressof(units)] + [0x1000 * (i + 3) for i in range(6)]))
        if null:
            args[null] = None
        rc = lib.svt_hip_wiener_pick_plane(args["prm"], args["units"], n_units if count is None else count, args["d_M"], args["d_H"], None,
                                           args["d_unit_records"], args["d_result"], args["d_lr_units"], args["d_workspace"], need - short, None)
        assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER, label
        assert b"svt_hip_wiener_pick_plane" in lib.svt_hip_last_error(), label
        n += 1
    assert n == 8 + 1 + 4 + 2 + 1 + 2 + 2 + 1


def test_cases_cover_what_the_issue_lists():
    shape = {c.name: (c.w, c.h, c.unit, len(K.unit_limits(c.w, c.h, c.unit, int(c.name.startswith("chroma"))))) for c in K.CASES}
    assert (200, 136, 64, 6) in shape.values() and (100, 68, 32, 6) in shape.values()
    assert K.unit_limits(200, 136, 64, 0)[2] == (128, 200, 0, 56) and K.unit_limits(200, 136, 64, 0)[5] == (128, 200, 56, 136)
    assert K.unit_limits(100, 68, 32, 1)[3] == (0, 32, 28, 68)                       # the offset is 8 >> ss_y
    assert any(n == 1 for *_, n in shape.values())
    tall = [c for c in K.CASES if any(ve - vs > c.unit for _, _, vs, ve in K.unit_limits(c.w, c.h, c.unit, 0)[-1:])]
    assert tall
    assert {(c.bd, c.is16) for c in K.CASES} == {(8, 0), (10, 1)} and {c.win for c in K.CASES} == {7, 5}
    assert {c.lvl for c in K.CASES} == {1, 2, 4, 6}
    assert {(c.win, c.bd) for c in K.CASES} == {(7, 8), (7, 10), (5, 8), (5, 10)}
    kinds = set()
    for c in K.CASES:
        x = K.make_inputs(c)
        kinds |= set(x.kinds)
        assert x.dgd.shape == (c.h + 2 * K.B, c.w + 2 * K.B) and x.src.shape == (c.h, c.w)
        inner = x.dgd[K.B:-K.B, K.B:-K.B]
        assert np.array_equal(x.dgd[:K.B, K.B:-K.B], np.broadcast_to(inner[0], (K.B, c.w)))        # replicated as svt_extend_frame leaves it
        assert np.array_equal(x.dgd[K.B:-K.B, -K.B:], np.broadcast_to(inner[:, -1:], (c.h, K.B)))
        assert (x.prev is not None) == (c.lvl == 6)
        if x.prev is not None:
            assert 0 < (x.prev["restoration_type"] == 1).sum() and (len(x.prev) == 1 or (x.prev["restoration_type"] != 1).any())
            if c.win == 5:
                assert not x.prev["hfilter"][:, 0].any() and not x.prev["vfilter"][:, 6].any()
            assert (x.prev["hfilter"][:, 3] == -2 * x.prev["hfilter"][:, :3].sum(axis=1)).all()
    assert kinds >= set("bsfhun")


def test_cases_reach_what_they_are_meant_to_reach():
    """Conditions on the recorded results of the reference (not measurements of the code under test)."""
    gold = {c.name: K.golden(c) for c in K.CASES}
    cover = {k: sum(int(g["cover"][:, i].sum()) for g in gold.values()) for i, k in enumerate(K.COVER)}
    for k in ("break", "repeat4", "move2", "move1", "rejected", "zero_pivot", "clip", "prev"):
        assert cover[k] >= 1, (k, cover)
    both = [n for n, g in gold.items() if g["result"]["frame_restoration_type"] == 1 and 0 < g["units"]["best_rtype"].sum() < len(g["units"])]
    assert both, "no plane decides WIENER while holding units of both types"
    assert any(g["result"]["frame_restoration_type"] == 0 for g in gold.values()), "no plane decides NONE"
    pairs = [n for n, g in gold.items() if (g["units"]["best_rtype"][:-1] & g["units"]["best_rtype"][1:]).any()]
    assert pairs, "no two consecutive Wiener units: ref never matters to the bits"
    for c in K.CASES:       # the records are consistent in themselves
        g = gold[c.name]
        u, r = g["units"], g["result"]
        rej = u["sse"][:, 1] == K.INT64_MAX
        assert (rej == (g["cover"][:, K.COVER.index("rejected")] == 1)).all()
        assert not u["hfilter"][rej].any() and not u["vfilter"][rej].any() and not u["trials"][rej].any() and not u["best_rtype"][rej].any()
        assert (u["bits"][rej] == c.cost[0]).all() and (u["trials"][~rej] >= 1).all()
        if not K.LEVELS[c.lvl][0]:
            assert (u["trials"][~rej] == 1).all()
        assert r["n_wiener"] == u["best_rtype"].sum() and r["sse"][0] == u["sse"][:, 0].sum() and r["bits"][0] == 0
        assert r["sse"][1] == np.where(u["best_rtype"] == 1, u["sse"][:, 1], u["sse"][:, 0]).sum()
        assert r["bits"][1] == np.where(u["best_rtype"] == 1, u["bits"], c.cost[0]).sum()
        assert r["frame_restoration_type"] == int(r["cost"][1] < r["cost"][0])
        lr = g["lr_units"]
        assert (lr["restoration_type"] == (u["best_rtype"] if r["frame_restoration_type"] else 0)).all()
        w = lr["restoration_type"] == 1
        assert np.array_equal(lr["hfilter"][w], u["hfilter"][w]) and np.array_equal(lr["vfilter"][w], u["vfilter"][w]) and not lr["hfilter"][~w].any()
        if c.win == 5:
            assert not u["hfilter"][:, 0].any() and not u["vfilter"][:, 0].any()
        assert (u["hfilter"][:, 3] == -2 * u["hfilter"][:, :3].sum(axis=1)).all() and not u["hfilter"][:, 7].any()
