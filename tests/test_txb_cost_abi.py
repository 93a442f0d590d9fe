"""CPU: the golden fixture of the coefficient rate (tests/txb_cost_cases.py) is what the reference's svt_av1_cost_coeffs_txb returns, the
numpy restatement equals it on every case, the cases reach what they are meant to reach, and the entry point refuses bad arguments
without a device."""
import numpy as np
import pytest

import txb_cost_cases as T
from support import assert_not_rtcd_leaf, fresh_process, have_reference_tree
from svtav1_hip import abi


@pytest.fixture(scope="module")
def gold():
    return T.Golden()


@pytest.fixture(scope="module")
def blocks(gold):
    """(iscan, coefficients) of every case"""
    out = []
    for i, c in enumerate(T.CASES):
        iscan = gold.iscan(c.w, c.h, c.tx_type)
        out.append((iscan, T.coefficients(i, c, iscan)))
    return out


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    return T.Pin(ref, tmp_path_factory.mktemp("txb_cost_pin"))


def test_txb_cost_golden_matches_reference(pin, gold, blocks):
    """Tables, scans and every case's bits, recomputed by the reference's own functions now."""
    assert pin.tables().tobytes() == gold.tables.tobytes()
    for (s, t), iscan in gold.iscans.items():
        assert np.array_equal(pin.iscan(*T.SIZES[s], t), iscan), (s, t)
    for i, c in enumerate(T.CASES):
        assert pin.bits(c, blocks[i][1]) == int(gold.bits[i]), (i, c)


def test_restatement_is_what_the_reference_does(pin, gold, blocks):
    """restate_bits against the real function on every case, and the constants the descriptor's ranges rest on."""
    assert [pin.lib.pin_enum(k) for k in range(5)] == [T.NEARESTMV, T.NEW_NEWMV + 1, T.FILTER_INTRA_NONE, 6, len(T.SIZES)]
    for i, c in enumerate(T.CASES):
        iscan, q = blocks[i]
        assert T.restate_bits(gold.tables[c.table], c, q, iscan) == pin.bits(c, q), (i, c)
    for w, h in T.SIZES:
        for is_inter in (0, 1):
            for reduced in (0, 1):
                used = {t for t in range(16) if pin.allowed(w, h, t, is_inter, reduced)}
                assert used == T.EXT_TX_USED[T.ext_tx_set_type(w, h, is_inter, reduced)], (w, h, is_inter, reduced)


def test_restatement_matches_golden(gold, blocks):
    """The same without the reference: what every GPU test compares with is what the restatement gives."""
    for i, c in enumerate(T.CASES):
        iscan, q = blocks[i]
        assert iscan[0] == 0
        assert T.restate_bits(gold.tables[c.table], c, q, iscan) == int(gold.bits[i]), (i, c)
    assert len({g.tobytes() for g in gold.tables}) == len(T.QINDEX)   # the two table sets differ


def test_cases_reach_every_branch(blocks):
    """Counted on the inputs: sizes, classes, planes, eob edges, contexts, magnitudes, DC signs, c_start forms, the transform-type
    rate's paths, the closed forms and the launch properties."""
    n = {}

    def hit(*key):
        n[key] = n.get(key, 0) + 1
    for i, c in enumerate(T.CASES):
        iscan, q = blocks[i]
        assert T.type_allowed(c), c
        hit("size_class_plane", c.w, c.h, T.tx_class(c.tx_type), c.plane)
        hit("eob", c.w, c.h, c.eob)
        hit("skip_ctx", c.skip_ctx), hit("dc_sign_ctx", c.dc_sign_ctx), hit("table", c.table), hit("group", c.group)
        exact = not (c.est_mode == 2 or (c.est_mode == 1 and c.eob < (c.w * c.h) >> 6))
        hit("est", c.est_mode, c.eob < (c.w * c.h) >> 6)
        if not c.eob:
            assert not q.any()
            hit("all_zero")
            continue
        scan = T.scan_of(iscan)
        assert q[scan[c.eob - 1]] != 0
        if not exact:
            continue
        for m in set(np.abs(q[scan[:c.eob]]).tolist()):
            hit("magnitude", m)
        hit("dc", int(np.sign(q[0])), c.eob > 1)
        if q[scan[c.eob:]].any():
            hit("beyond_eob")
        div = c.fast - c.step
        hit("c_start", c.fast, c.step)
        hit("c_start_form", "max1" if div <= 0 else "div", "empty" if min(c.eob - 2, c.eob // max(1, div)) < 1 else "loop")
        if c.eob > 2 and c.eob // max(1, div) < c.eob - 2:
            hit("c_start_short")
        if c.plane == 0:
            inter = T.is_inter_mode(c.pred_mode)
            single = len(T.EXT_TX_USED[T.ext_tx_set_type(c.w, c.h, inter, c.reduced)]) == 1
            hit("tx_rate", "inter" if inter else "filter_intra" if c.fim != T.FILTER_INTRA_NONE else ("intra", c.pred_mode), c.reduced, single)
        else:
            hit("chroma_shift", bool(c.flags & abi.TXB_COST_NO_SHIFT), c.step > 0)
    for w, h in T.SIZES:
        size = min(w, 32) * min(h, 32)
        classes = {T.tx_class(t) for t in T.size_types(w, h)}
        assert classes == ({0, 1, 2} if max(w, h) <= 16 else {0})   # larger sizes allow no one-dimensional type
        for cls in classes:
            for plane in (0, 1):
                assert n.get(("size_class_plane", w, h, cls, plane), 0) >= 7, (w, h, cls, plane)
        for eob in T.eob_edges(size):
            assert n.get(("eob", w, h, eob), 0) >= 2, (w, h, eob)
    assert len(T.SIZES) == 19
    for key in [("skip_ctx", 0), ("skip_ctx", 12), ("dc_sign_ctx", 0), ("dc_sign_ctx", 1), ("dc_sign_ctx", 2), ("table", 0), ("table", 1), ("all_zero",),
                ("beyond_eob",), ("dc", -1, True), ("dc", 1, True), ("dc", 0, True), ("dc", -1, False), ("dc", 1, False), ("c_start_short",),
                ("c_start_form", "max1", "loop"), ("c_start_form", "max1", "empty"), ("c_start_form", "div", "empty"), ("c_start_form", "div", "loop"),
                ("tx_rate", "inter", 0, False), ("tx_rate", "inter", 1, False), ("tx_rate", "inter", 0, True), ("tx_rate", "filter_intra", 0, False),
                ("tx_rate", ("intra", 0), 0, False), ("tx_rate", ("intra", 1), 0, False), ("tx_rate", ("intra", 12), 1, False),
                ("tx_rate", ("intra", 0), 0, True), ("chroma_shift", True, True), ("chroma_shift", False, True)]:
        assert n.get(key, 0) > 0, key
    for m in (0,) + T.MAGNITUDES:
        assert n.get(("magnitude", m), 0) > 0, m
    assert {14, 15, 127, 128}.issubset(T.MAGNITUDES) and max(T.MAGNITUDES) > 1 << 15 and 1 << 15 in T.MAGNITUDES
    for fast in (1, 2, 3):
        for step in (0, 1, 2):
            assert n.get(("c_start", fast, step), 0) > 0, (fast, step)
    for est_mode in (1, 2):
        for below in (True, False):
            assert n.get(("est", est_mode, below), 0) > 0, (est_mode, below)
    # launch properties: no size's batch fills its last workgroup (256 lanes, min(n, 64) lanes per block)
    for w, h in T.SIZES:
        per_wg = 256 // min(min(w, 32) * min(h, 32), 64)
        assert sum((c.w, c.h) == (w, h) for c in T.CASES) % per_wg != 0, (w, h)


@pytest.mark.parametrize("name", ["svt_hip_txb_cost_batch", "svt_hip_txb_cost_batch_placed"])
def test_txb_cost_export_is_not_an_rtcd_leaf(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf."""
    assert_not_rtcd_leaf(name)


def test_refusals_need_no_device():
    """A process that never called svt_hip_init: a size that is no transform size, no table set, and NULL arrays with blocks to do are
    bad parameters; an empty batch succeeds; anything else is SVT_HIP_ERR_NO_DEVICE.  Nothing is launched either way."""
    got = fresh_process("(lambda f: ("
                        "f(p, p, p, 1, None, None, p, 1, 4, 32, None), f(p, p, p, 1, None, None, p, 1, 12, 8, None), f(p, p, p, 1, None, None, p, 0, 64, 8, None),"
                        "f(p, p, p, 0, None, None, p, 1, 8, 8, None), f(p, p, p, 0, None, None, p, 0, 8, 8, None), f(p, None, p, 1, None, None, p, 1, 8, 8, None),"
                        "f(p, p, None, 1, None, None, p, 1, 8, 8, None), f(p, p, p, 1, None, None, None, 1, 8, 8, None),"
                        "lib.svt_hip_txb_cost_batch_placed(p, p, p, 1, None, None, None, 1, 8, 8, 1, None),"
                        "f(None, None, None, 1, None, None, None, 0, 16, 64, None), f(p, p, p, 1, None, None, p, 1, 16, 64, None)))(lib.svt_hip_txb_cost_batch)")
    assert got == [abi.SVT_HIP_ERR_BAD_PARAMETER] * 9 + [abi.SVT_HIP_OK, abi.SVT_HIP_ERR_NO_DEVICE]
