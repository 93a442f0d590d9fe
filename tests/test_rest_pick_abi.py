"""CPU: the fixture, the interface and the cases of svt_hip_rest_pick_plane (the restoration decision of a plane with the self-guided
filter on the device).  No compute call reaches a device here: the workspace helper is layout arithmetic and every refusal comes
before the library looks for one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rest_pick_cases as K
from lf_cases import P, V
from support import assert_not_rtcd_leaf, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

NAMES = ("svt_hip_rest_pick_plane", "svt_hip_rest_pick_workspace_bytes")
IDS = [c.name for c in K.CASES]


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_reference_leaves(ref, case):
    x = K.make_inputs(case)
    gold = K.golden(case)
    wrecs = K.wiener_records(x, K.wiener_leaves(x, ref, "ref"))
    assert (wrecs is None) == (gold["wiener"] is None) and (wrecs is None or wrecs.tobytes() == gold["wiener"].tobytes())
    assert K.same(gold, K.drive(x, K.RefLeaves(x, ref), wrecs)) == []


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_fixture_is_the_driver_over_the_oracle_leaves(orc, case):
    assert K.same(K.golden(case), K.drive_orc(K.make_inputs(case), orc)) == []


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    return K.Pin(ref, tmp_path_factory.mktemp("rest_pick_pin"))


def test_decision_chain_is_what_the_reference_does(pin):
    """The driver's finish visitors and plane decision against the reference's own static search_wiener_finish, search_sgrproj_finish,
    search_switchable and RDCOST_DBL, called in raster order on the records of every case and on random records."""
    assert pin.constants() == [K.PRJ_MIN[0], K.PRJ_MAX[0], K.PRJ_MIN[1], K.PRJ_MAX[1], K.PRJ_BITS, 4, 4, *K.PRJ_DEFAULT, 64, 8, 384]

    def check(case, sse, taps, wbest, ep, xqd, tag):
        best, tested, tot_s, tot_b, cost, _, _, _ = K.decide(case, sse, taps, wbest, ep, xqd)
        p_best, p_sse, p_bits, p_cost = pin.decide(case, sse, taps, ep, xqd)
        assert (best, tot_s, tot_b, np.array(cost, np.float64).tobytes()) == (p_best, p_sse, p_bits, p_cost), tag
    for case in K.CASES:
        g = K.golden(case)
        u, w = g["units"], g["wiener"]
        taps = [([int(t) for t in r["vfilter"]], [int(t) for t in r["hfilter"]]) for r in w] if case.win else [None] * len(u)
        check(case, u["sse"].tolist(), taps, u["best_rtype"][:, 0].tolist(), u["ep"].tolist(), u["xqd"].tolist(), case.name)
    rng = np.random.default_rng(91)
    tap = lambda: [int(rng.integers(K.W.TAP_MIN[p], K.W.TAP_MAX[p] + 1)) for p in range(3)]      # noqa: E731

    def taps8():
        t = tap()
        return t + [-2 * sum(t)] + t[::-1] + [0]
    for i in range(200):                                 # random records: close SSEs, so that rates and references decide
        n, win = int(rng.integers(1, 9)), (7, 5, 0)[i % 3]
        case = K.Case("random", 0, 0, 0, 8, 0, 0, win, K.EP_ALL, int(rng.integers(1, 1 << 20)), tuple(rng.integers(0, 3000, 2).tolist()),
                      tuple(rng.integers(0, 3000, 2).tolist()), tuple(rng.integers(0, 3000, 3).tolist()), "", 0)
        base = rng.integers(5000, 1 << 30, n)
        sse = [[int(b), int(b - rng.integers(-50, 3000)), int(b - rng.integers(-50, 3000))] for b in base]
        taps = []
        for k in range(n):
            t = (taps8(), taps8())
            if win == 5:
                for f in t:
                    f[3] += 2 * f[0]
                    f[0] = f[6] = 0
            taps.append(t)
            if not win or rng.random() < 0.2:
                sse[k][1] = K.INT64_MAX
        ep = rng.integers(0, 16, n).tolist()
        xqd = [[int(rng.integers(K.PRJ_MIN[0], K.PRJ_MAX[0] + 1)), int(rng.integers(K.PRJ_MIN[1], K.PRJ_MAX[1] + 1))] for _ in range(n)]
        # best_rtype[WIENER - 1] as the Wiener call decides it: the reference's own pass, run alone
        wbest = [b[0] for b in pin.decide(case, sse, taps, ep, xqd)[0]]
        check(case, sse, taps if win else [None] * n, wbest, ep, xqd, (i, n, win))


def test_bit_count_and_encode_xq_are_what_the_reference_does(pin):
    rng = np.random.default_rng(92)
    for ep in range(16):
        for _ in range(60):
            xqd = [int(rng.integers(K.PRJ_MIN[0], K.PRJ_MAX[0] + 1)), int(rng.integers(K.PRJ_MIN[1], K.PRJ_MAX[1] + 1))]
            ref = [int(rng.integers(K.PRJ_MIN[0], K.PRJ_MAX[0] + 1)), int(rng.integers(K.PRJ_MIN[1], K.PRJ_MAX[1] + 1))]
            assert K.count_sgrproj_bits(ep, xqd, ref) == pin.count_bits(ep, xqd, ref), (ep, xqd, ref)
            xq = [int(rng.integers(-400, 400)), int(rng.integers(-400, 400))]
            assert K.encode_xq(xq, ep) == pin.encode_xq(xq, ep), (ep, xq)
    for p in range(2):              # every (reference, value) pair of both coefficients
        for r in range(K.PRJ_MIN[p], K.PRJ_MAX[p] + 1):
            for v in range(K.PRJ_MIN[p], K.PRJ_MAX[p] + 1):
                xqd, ref = list(K.PRJ_DEFAULT), list(K.PRJ_DEFAULT)
                xqd[p], ref[p] = v, r
                assert K.count_sgrproj_bits(0, xqd, ref) == pin.count_bits(0, xqd, ref), (p, r, v)


SEARCH_PINNED = [K.CASES[0], K.CASES[1], K.CASES[4], K.CASES[11]]      # every ep range with refinement, 8 / 10 / 12 bit, luma and chroma


@pytest.mark.parametrize("case", SEARCH_PINNED, ids=lambda c: c.name)
def test_search_is_what_the_reference_does(pin, ref, case):
    """Every unit's search against ref_sgr_search_unit (the reference's static search_selfguided_restoration), and the finer search of
    every candidate against the reference's static finer_search_pixel_proj_error on the same filtered planes."""
    x = K.make_inputs(case)
    lv = K.RefLeaves(x, ref)
    g = K.golden(case)
    start, end, inc, refine = case.ep
    pu = 64 >> x.ss
    for i, limits in enumerate(x.limits):
        hs, he, vs, ve = limits
        out = np.zeros(3, np.int32)
        dat, src = K._addr(x.dgd, K.B + vs, K.B + hs), K._addr(x.src, vs, hs)
        assert ref.ref_sgr_search_unit(K._enc(dat, case.is16), he - hs, ve - vs, x.dgd.shape[1], K._enc(src, case.is16), x.src.shape[1], case.is16, case.bd,
                                       pu, pu, start, end, inc, refine, P(out)) == 0
        assert out.tolist() == [int(g["units"]["ep"][i]), *g["units"]["xqd"][i].tolist()], (case.name, i)
    limits = x.limits[0]
    hs, he, vs, ve = limits
    w, h = he - hs, ve - vs
    fs = ((w + 7) & ~7) + 8
    f0, f1 = np.zeros((h, fs), np.int32), np.zeros((h, fs), np.int32)
    for ep in range(start, end, inc):
        for ii in range(0, h, pu):
            for j in range(0, w, pu):
                lv.filter(K._addr(x.dgd, K.B + vs + ii, K.B + hs + j), min(pu, w - j), min(pu, h - ii), x.dgd.shape[1], K._addr(f0, ii, j), K._addr(f1, ii, j), fs, ep)
        xqd = K.encode_xq(lv.subspace(K._addr(x.src, vs, hs), w, h, x.src.shape[1], K._addr(x.dgd, K.B + vs, K.B + hs), x.dgd.shape[1], f0, f1, fs, ep), ep)
        want = pin.finer_search(x, limits, f0, f1, fs, xqd, ep, refine)
        err, _, _ = K.finer_search(lambda q: lv.error(K._addr(x.src, vs, hs), w, h, x.src.shape[1], K._addr(x.dgd, K.B + vs, K.B + hs), x.dgd.shape[1], f0, f1, fs,
                                                       K.decode_xq(q, ep), ep), xqd, ep, refine)
        assert (err, xqd) == want, (case.name, ep)


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rest_pick.npz")) <= 64 * 1024


def test_records_have_the_sizes_and_offsets_the_header_states():
    want = header_values(["SVT_HIP_REST_PICK_UNIT_BYTES", "sizeof(SvtHipRestPickUnit)", "SVT_HIP_REST_PICK_RESULT_BYTES", "sizeof(SvtHipRestPickResult)",
                          "sizeof(SvtHipRestPickParams)", "offsetof(SvtHipRestPickUnit, search_err)", "offsetof(SvtHipRestPickUnit, ep)",
                          "offsetof(SvtHipRestPickUnit, xqd)", "offsetof(SvtHipRestPickUnit, best_rtype)", "offsetof(SvtHipRestPickUnit, trials)",
                          "offsetof(SvtHipRestPickResult, sse)", "offsetof(SvtHipRestPickResult, bits)", "offsetof(SvtHipRestPickResult, cost)",
                          "offsetof(SvtHipRestPickResult, n_units_of_type)", "offsetof(SvtHipRestPickResult, sg_frame_ep_cnt)"], ["svt_hip_lf.h"])
    assert list(want.values()) == [64, 64, 184, 184, 76, 24, 32, 36, 44, 56, 8, 40, 72, 104, 120]
    assert abi.REST_PICK_UNIT_BYTES == C.sizeof(abi.RestPickUnit) == K.UNIT_DTYPE.itemsize == 64
    assert abi.REST_PICK_RESULT_BYTES == C.sizeof(abi.RestPickResult) == K.RESULT_DTYPE.itemsize == 184 and C.sizeof(abi.RestPickParams) == 76
    for mirror in (abi.RestPickParams, abi.RestPickUnit, abi.RestPickResult):      # no implicit padding
        end = 0
        for f, _ in mirror._fields_:
            assert getattr(mirror, f).offset == end, (mirror.__name__, f)
            end += getattr(mirror, f).size
        assert end == C.sizeof(mirror)
    assert K.RESULT_DTYPE["cost"].base == np.dtype("<f8") and K.UNIT_DTYPE["sse"].shape == (3,)


def test_workspace_helper_is_layout_arithmetic():
    """What the header states, 0 for nothing to do, needs no device (the library is not initialised here)."""
    f = abi.load().svt_hip_rest_pick_workspace_bytes
    assert f(0, 64, 64, 1) == f(1, 0, 64, 1) == f(1, 64, 0, 1) == f(1, 64, 64, 0) == f(1, 64, 64, -3) == 0
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    for n, w, h, e in ((1, 72, 40, 1), (6, 200, 136, 16), (6, 100, 68, 2), (120, 3840, 2160, 16), (65535, 65536, 65536, 16)):
        assert f(n, w, h, e) == up(n * e * 64) + up(n * 16) + up(e * 2 * w * h * 4), (n, w, h, e)
    assert f(65535, 65536, 65536, 16) > 2 ** 38      # a 64-bit return


def test_new_names_are_exported_and_are_not_rtcd_leaves():
    lib = abi.load()
    for n in NAMES:
        assert_not_rtcd_leaf(n)
        assert n in PROTOTYPES and lib.svt_hip_rtcd_lookup(n[len("svt_hip_"):].encode()) is None
    assert PROTOTYPES["svt_hip_rest_pick_workspace_bytes"] == ("c_uint64", ("c_uint32", "c_uint32", "c_uint32", "c_int32"))
    assert PROTOTYPES["svt_hip_rest_pick_plane"] == ("c_int64", ("c_void_p", "c_void_p", "c_uint32") + ("c_void_p",) * 5 + ("c_uint64", "c_void_p"))


def test_status_exports_returning_int64_are_probed_here():
    """tests/test_tier_b_refusals.py takes its census from the exports that return int32_t, tests/test_wiener_pick_abi.py adds those that
    return int.  svt_hip_rest_pick_plane returns int64_t (launches, or a negative status): every svt_hip_* export with that return type
    is listed here with what the census's own child process (its probes, its marking of the error text) records for it."""
    import test_tier_b_refusals as T
    bad = abi.SVT_HIP_ERR_BAD_PARAMETER
    assert bad < 0
    want = {"svt_hip_rest_pick_plane": [[bad, "svt_hip_rest_pick_plane: NULL argument"], [bad, "svt_hip_rest_pick_plane: 0 units (1..65535)"],
                                        [bad, "svt_hip_rest_pick_plane: bit depth 0 with 8-bit samples"]]}
    assert {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_int64"} == set(want)
    assert not set(want) & set(T.census_names())
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(want)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == want


def test_every_refusal_comes_before_the_device():
    """Each bad call is refused with a negative status and a message whether or not a device exists; the device pointers are never
    followed."""
    lib = abi.load()
    x = K.make_inputs(K.CASES[0])
    n_units = len(x.limits)
    need = lib.svt_hip_rest_pick_workspace_bytes(n_units, x.case.w, x.case.h, K.n_ep(x.case))
    good = dict(zip(K.ARGS[2:], [0x1000 * (i + 3) for i in range(4)]), dgd=0x100000, src=0x200000)
    n = 0
    for rej in K.rejections(x):
        rc = K.call_rejection(lib, x, rej, good, n_units, 0x9000, need)
        assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER, rej[0]
        assert b"svt_hip_rest_pick_plane" in lib.svt_hip_last_error(), rej[0]
        n += 1
    assert n == 6 + 4 + 2 + 2 + 2 + 2 + 4 + 1 + 5 + 1
    # units that together hold more than the plane (each one inside it)
    prm, units = K.params(x), K.wiener_units(x, 0x100000, 0x200000)
    for u in units:
        u.h_start, u.h_end, u.v_start, u.v_end = 0, x.case.w, 0, x.case.h
    rc = lib.svt_hip_rest_pick_plane(C.byref(prm), units, n_units, None, *[good[a] for a in K.ARGS[2:]], need, None)
    assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER and b"svt_hip_rest_pick_plane: the units hold" in lib.svt_hip_last_error()


def test_cases_cover_what_the_issue_lists():
    limits = {c.name: K.W.unit_limits(c.w, c.h, c.unit, c.ss) for c in K.CASES}
    shape = {c.name: (c.w, c.h, c.unit, c.ss, len(limits[c.name])) for c in K.CASES}
    assert (200, 136, 64, 0, 6) in shape.values() and (100, 68, 32, 1, 6) in shape.values() and (72, 40, 64, 0, 1) in shape.values()
    assert K.W.unit_limits(200, 136, 64, 0)[2] == (128, 200, 0, 56) and K.W.unit_limits(200, 136, 64, 0)[5] == (128, 200, 56, 136)
    assert K.W.unit_limits(383, 40, 256, 0) == [(0, 383, 0, 40)]
    for base in ((200, 136, 64, 0), (100, 68, 32, 1), (72, 40, 64, 0), (383, 40, 256, 0)):
        assert {(c.bd, c.is16) for c in K.CASES if (c.w, c.h, c.unit, c.ss) == base} >= {(8, 0), (10, 1)}, base
    assert sum(c.bd == 12 for c in K.CASES) == 1
    assert {c.ep for c in K.CASES} == {(0, 16, 1, 1), (0, 16, 8, 1), (4, 5, 1, 0)}
    assert {c.win for c in K.CASES} == {0, 5, 7}
    kinds = set()
    for c in K.CASES:
        x = K.make_inputs(c)
        kinds |= set(x.kinds)
        assert x.limits == limits[c.name] and x.dgd.shape == (c.h + 2 * K.B, c.w + 2 * K.B) and x.src.shape == (c.h, c.w)
        inner = x.dgd[K.B:-K.B, K.B:-K.B]
        assert np.array_equal(x.dgd[:K.B, K.B:-K.B], np.broadcast_to(inner[0], (K.B, c.w)))        # replicated as svt_extend_frame leaves it
        assert np.array_equal(x.dgd[K.B:-K.B, -K.B:], np.broadcast_to(inner[:, -1:], (c.h, K.B)))
    assert kinds >= set("bnsfhu")           # blurred, noisy, identical, flat, unrelated


def test_cases_reach_what_they_are_meant_to_reach():
    """The issue's coverage conditions, on the recorded results of the reference (not measurements of the code under test)."""
    gold = {c.name: K.golden(c) for c in K.CASES}
    types = {n: int(g["result"]["frame_restoration_type"]) for n, g in gold.items()}
    assert set(types.values()) == {K.NONE, K.WIENER, K.SGRPROJ, K.SWITCHABLE}
    sw = [g for n, g in gold.items() if types[n] == K.SWITCHABLE]
    assert {int(t) for g in sw for t in g["units"]["best_rtype"][:, 2]} == {K.NONE, K.WIENER, K.SGRPROJ}
    assert {int(t) for g in sw for t in g["lr_units"]["restoration_type"]} == {K.NONE, K.WIENER, K.SGRPROJ}
    assert any((g["units"]["sse"][:, 1] == K.INT64_MAX).any() for g in sw), "no rejected Wiener record in a switchable plane"
    eps = [int(e) for g in gold.values() for e in g["units"]["ep"]]
    assert any(e <= 9 for e in eps) and any(10 <= e <= 13 for e in eps) and any(e >= 14 for e in eps)
    cover = {k: [int(v) for g in gold.values() for v in g["cover"][:, i]] for i, k in enumerate(K.COVER)}
    assert max(cover["clamp"]) >= 1, "no xqd ends on a clamp limit"
    flat = [int(v) for c in K.CASES for v, k in zip(gold[c.name]["cover"][:, K.COVER.index("full_tie")], K.make_inputs(c).kinds) if k == "f" and c.ep[3]]
    assert flat and max(flat) == 1, "no flat unit walks the full tie path"
    assert max(cover["keep2"]) >= 2, "the step-2 keep-moving branch is never taken twice in a row"
    assert max(cover["step1_only"]) == 1, "no search improves at step 1 only"
    chain = [n for n, g in gold.items() if types[n] == K.SWITCHABLE and g["chains"][0].sum() >= 2 and g["chains"][1].sum() >= 2
             and not np.array_equal(g["chains"][0], g["chains"][1])]
    assert chain, "no plane where ref changes in the sgrproj pass and differently in the switchable pass"
    for c in K.CASES:       # the records are consistent in themselves
        g = gold[c.name]
        u, r, lr = g["units"], g["result"], g["lr_units"]
        n = len(u)
        with_w, with_sw = bool(c.win), bool(c.win) and n > 1
        assert r["tested"] == 1 | with_w << 1 | 4 | with_sw << 3
        assert ((u["sse"][:, 1] == K.INT64_MAX).all() and not u["best_rtype"][:, 0].any()) if not with_w else np.array_equal(u["sse"][:, 1], g["wiener"]["sse"][:, 1])
        assert with_sw or not u["best_rtype"][:, 2].any()
        assert r["sg_frame_ep_cnt"].sum() == n and all(r["sg_frame_ep_cnt"][e] == (u["ep"] == e).sum() for e in range(16))
        assert set(u["ep"].tolist()) <= set(range(c.ep[0], c.ep[1], c.ep[2])) and (u["trials"] >= 1).all() and (u["trials"] <= 135).all()
        assert c.ep[3] or (u["trials"] == 1).all()
        assert r["sse"][0] == u["sse"][:, 0].sum() and r["bits"][0] == 0
        for t in (1, 2, 3):
            if r["tested"] >> t & 1:
                pick = u["best_rtype"][:, t - 1]
                assert r["sse"][t] == u["sse"][np.arange(n), pick].sum(), (c.name, t)
            else:
                assert r["sse"][t] == r["bits"][t] == 0 and r["cost"][t] == 0
        ft = int(r["frame_restoration_type"])
        assert r["tested"] >> ft & 1 and all(not (r["tested"] >> t & 1) or r["cost"][ft] <= r["cost"][t] for t in range(4))
        assert (lr["restoration_type"] == (u["best_rtype"][:, ft - 1] if ft else 0)).all()
        assert [int((lr["restoration_type"] == t).sum()) for t in range(3)] == r["n_units_of_type"].tolist()
        w, s = lr["restoration_type"] == 1, lr["restoration_type"] == 2
        assert not lr["hfilter"][~w].any() and not lr["vfilter"][~w].any() and not lr["ep"][~s].any() and not lr["xqd"][~s].any()
        assert np.array_equal(lr["ep"][s], u["ep"][s]) and np.array_equal(lr["xqd"][s], u["xqd"][s])
        if with_w:
            assert np.array_equal(lr["hfilter"][w], g["wiener"]["hfilter"][w]) and np.array_equal(lr["vfilter"][w], g["wiener"]["vfilter"][w])
