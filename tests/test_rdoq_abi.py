"""CPU: the golden fixture of the RDOQ stage (tests/rdoq_cases.py) is what the reference's svt_aom_quantize_inv_quantize leaves, the Python
restatement equals it on every case, the cases reach every branch they are meant to reach, the scans have the dependency order the
walk rests on, and the entry point refuses bad arguments without a device."""
import collections
import os
import subprocess

import numpy as np
import pytest

import rdoq_cases as R
import txb_cost_cases as T
from support import assert_not_rtcd_leaf, fresh_process, have_reference_tree
from svtav1_hip import abi


@pytest.fixture(scope="module")
def gold():
    return R.Golden()


@pytest.fixture(scope="module")
def counted(gold, orc):
    """(every case's Block, the restatement's branch counters)"""
    hits = collections.Counter()
    return [R.Block(gold, orc, i, lambda *k: hits.update([k])) for i in range(len(R.CASES))], hits


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    return R.Pin(ref, tmp_path_factory.mktemp("rdoq_pin"))


def test_rdoq_golden_matches_reference(pin, gold, counted):
    """Quantiser tables, matrices and every case's result, recomputed by the reference's own functions now."""
    assert np.array_equal(pin.quant_tables(), gold.quant)
    for (plane, s), (qm, iqm) in gold.qms.items():
        got = pin.qm(plane, *T.SIZES[s])
        assert np.array_equal(got[0], qm) and np.array_equal(got[1], iqm), (plane, s)
    for i, c in enumerate(R.CASES):
        q, dq, eob, cul = pin.run(c, counted[0][i].coeff)
        assert (eob, cul, R.digest(q), R.digest(dq)) == (gold.eob[i], gold.cul_level[i], gold.q_digest[i], gold.dq_digest[i]), (i, c)


def test_restatement_is_what_the_reference_does(pin, counted):
    """The restatement against the real function on every case, array for array, and the constants it states."""
    assert [pin.lib.pin_enum(k) for k in range(4)] == [6, 1, 5, R.NO_QM_LEVEL + 1]
    for i, c in enumerate(R.CASES):
        b = counted[0][i]
        q, dq, eob, cul = pin.run(c, b.coeff)
        assert np.array_equal(q, b.q) and np.array_equal(dq, b.dq) and (eob, cul) == (b.eob, b.cul), (i, c)


def test_restatement_matches_golden(gold, counted):
    """The same without the reference: what every GPU test compares with is what the fixture holds."""
    for i, b in enumerate(counted[0]):
        assert (b.eob, b.cul, b.path, b.changed, R.digest(b.q), R.digest(b.dq)) == \
            (gold.eob[i], gold.cul_level[i], gold.path[i], gold.changed[i], gold.q_digest[i], gold.dq_digest[i]), (i, b.c)


def test_cases_reach_every_branch(counted):
    """Counted on `path` and on the restatement's branch counters: every item of the case list has a non-zero count."""
    blocks, n = counted
    paths = collections.Counter((b.path & abi.RDOQ_PATH_MASK, bool(b.path & abi.RDOQ_PATH_FAST_TRIM), bool(b.path & abi.RDOQ_PATH_SKIP)) for b in blocks)
    by_way = collections.Counter(b.path & abi.RDOQ_PATH_MASK for b in blocks)
    for way in (abi.RDOQ_PATH_NOT_FLAGGED, abi.RDOQ_PATH_EOB_ZERO, abi.RDOQ_PATH_REQUANT_SATD, abi.RDOQ_PATH_REQUANT_EOB, abi.RDOQ_PATH_EARLY_EXIT,
                abi.RDOQ_PATH_TRELLIS):
        assert by_way[way] > 0, way
    assert paths[(abi.RDOQ_PATH_TRELLIS, True, False)] and paths[(abi.RDOQ_PATH_TRELLIS, False, True)] and paths[(abi.RDOQ_PATH_EOB_ZERO, True, False)]
    assert paths[(abi.RDOQ_PATH_EARLY_EXIT, True, False)] + paths[(abi.RDOQ_PATH_EARLY_EXIT, False, False)] == by_way[abi.RDOQ_PATH_EARLY_EXIT]
    assert sum(b.changed for b in blocks if (b.path & abi.RDOQ_PATH_MASK) in (abi.RDOQ_PATH_NOT_FLAGGED, abi.RDOQ_PATH_EARLY_EXIT)
               and not b.path & abi.RDOQ_PATH_FAST_TRIM) == 0
    # sizes, classes, planes, eob edges, among the blocks the trellis walks
    assert len(T.SIZES) == 19
    for w, h in T.SIZES:
        size = min(w, 32) * min(h, 32)
        classes = {T.tx_class(t) for t in T.size_types(w, h)}
        assert classes == ({0, 1, 2} if max(w, h) <= 16 else {0})   # larger sizes allow no one-dimensional type
        for cls in classes:
            for plane in (0, 1):
                assert n[("trellis", "size", w, h, cls, plane)] >= 5, (w, h, cls, plane)
        for eob in T.eob_edges(size):
            if eob:
                assert n[("trellis", "eob", w, h, eob)] >= 1, (w, h, eob)
        # a batch that does not fill its last wavefront (64 lanes, min(n, 64) lanes to a block)
        assert sum((b.c.w, b.c.h) == (w, h) for b in blocks) % (64 // min(size, 64)) != 0 or size >= 64, (w, h)
    must = [("trellis", "iqm", True), ("trellis", "iqm", False), ("trellis", "bd", 8), ("trellis", "bd", 10), ("trellis", "sharp", 1),
            ("trellis", "sharp", 0), ("trellis", "plane", 0), ("trellis", "plane", 1), ("trellis", "inter", 0), ("trellis", "inter", 1),
            ("last", "one"), ("last", "keep"), ("last", "lower"),
            ("head", "zero"), ("head", "keep"), ("head", "lower"), ("head", "new_eob"), ("head", "new_eob_lower"),
            ("head_end", "skip_reached", 1), ("head_end", "skip_reached", 2), ("head_end", "skip_reached", 3), ("head_end", "skip_reached", 4),
            ("head_end", "skip_not_reached", 5), ("head_end", "skip_not_reached", "fast"), ("skip", "taken"), ("skip", "not_taken"),
            ("simple", "below"), ("simple", "keep"), ("simple", "lower"), ("golomb_table",), ("golomb_r32", "pow2"), ("golomb_r32", "other"),
            ("dc", "zero"), ("dc", "keep"), ("dc", "lower"), ("dc_sign", -1), ("dc_sign", 0), ("dc_sign", 1),
            ("trim", "fast_mode"), ("trim", "eob_fast_th", 0), ("trim", "eob_fast_th", 30), ("trim", "emptied_in_trellis"),
            ("eob_fast_th", "above"), ("eob_fast_th", "below"), ("eob_th", "above"), ("eob_th", "below"),
            ("satd", "passed"), ("satd", "refused"), ("satd_picture_depth", "decides", "passed"), ("satd_picture_depth", "agrees", "refused"),
            ("satd_picture_depth", "agrees", "passed"), ("requant", "redone"), ("requant", "kept"), ("early_exit", "taken"), ("early_exit", "not_taken")]
    must += [("trellis", "class", k) for k in range(3)] + [("trellis", "log_scale", k) for k in range(3)]
    must += [("simple_level", m) for m in R.MAGNITUDES if m < 1 << 15] + [("simple_level", "big")]
    for key in must:
        assert n[key] > 0, key
    assert {1, 2, 3, 14, 15, 16, 45, 46, 47, 127, 128}.issubset(R.MAGNITUDES) and max(R.MAGNITUDES) > 1 << 15
    # the switches that are off somewhere too, and every lambda on a block the trellis walks
    cs = [b.c for b in blocks]
    assert {c.eob_fast_th for c in cs} == {0, 30, 255} and {c.eob_th for c in cs} == {85, 255} and {c.satd_factor for c in cs} >= {255}
    assert {b.c.lam for b in blocks if (b.path & abi.RDOQ_PATH_MASK) == abi.RDOQ_PATH_TRELLIS} == set(R.LAMBDAS) and min(R.LAMBDAS) == 0
    # a first quantiser of either family, and blocks whose eob the first quantiser left differs from the final one
    assert {b.mode for b in blocks} == {abi.QUANT_B, abi.QUANT_B_HBD, abi.QUANT_FP, abi.QUANT_FP_HBD}
    assert sum(b.eob != b.eob0 for b in blocks) > 50 and sum(b.eob == b.eob0 and b.changed > 0 for b in blocks) > 50


def neighbours_follow(iscan, w, h, tx_type):
    iscan = iscan.astype(np.int64)
    iw, ih = T.retained(w, h)
    grid = np.full((ih + 4, iw + 4), iw * ih, np.int64)   # outside the block: the pad, never written
    grid[:ih, :iw] = iscan.reshape(ih, iw)
    nz, br = R.neighbours(T.tx_class(tx_type))
    row, col = np.divmod(np.arange(iw * ih), iw)
    return all((grid[row + dr, col + dc] > iscan).all() and dr >= 0 and dc >= 0 and dr + dc > 0 for dr, dc in set(nz) | set(br))


def test_neighbours_follow_in_every_scan_of_the_reference(pin):
    """The kernel takes the rounds for any tx_type without a fall-back to scan order; the fixture holds one type per class.  Here every
    one of the 16 types of every size, from the reference's av1_scan_orders: the property holds for all of them, and the types of a
    class share the class's scan (what lets one type stand for its class in the cases)."""
    for w, h in T.SIZES:
        by_class = {}
        for tx_type in range(16):
            iscan = pin.iscan(w, h, tx_type)
            assert neighbours_follow(iscan, w, h, tx_type), (w, h, tx_type)
            by_class.setdefault(T.tx_class(tx_type), set()).add(iscan.tobytes())
        assert all(len(v) == 1 for v in by_class.values()), (w, h)


def test_neighbours_follow_in_scan_order(gold):
    """What lets update_coeff_simple read FINAL levels: every neighbour that get_lower_levels_ctx / get_br_ctx read from a position
    lies later in scan order than the position, for every (size, type) scan the cases use; so a walk from eob - 1 down has
    finished with them; and every neighbour lies on a later anti-diagonal, so positions that share one never read each other."""
    pairs = {(c.w, c.h, c.tx_type) for c in R.CASES}
    assert len(pairs) >= 19
    for w, h, tx_type in sorted(pairs):
        iscan = gold.iscan(w, h, tx_type).astype(np.int64)
        iw, ih = T.retained(w, h)
        cls = T.tx_class(tx_type)
        grid = np.full((ih + 4, iw + 4), iw * ih, np.int64)   # outside the block: the pad, never written
        grid[:ih, :iw] = iscan.reshape(ih, iw)
        nz, br = R.neighbours(cls)
        row, col = np.divmod(np.arange(iw * ih), iw)
        for dr, dc in set(nz) | set(br):
            assert (grid[row + dr, col + dc] > iscan).all(), (w, h, tx_type, dr, dc)
            assert dr >= 0 and dc >= 0 and dr + dc > 0   # a later anti-diagonal in every class: one diagonal's positions are independent


GEOMETRY_FIELDS = "valid sw sh orient sqr sqr_up txs_ctx pixels tx_scale iw ih retained sqrt_retained".split()
GEOMETRY_PROGRAM = """
#include "txb_geometry.hpp"
#include <cstdio>
#include <cstdlib>
using namespace svthip;
static_assert(TxbGeometry(64, 16).retained == 512 && grid_blocks(9, 4, 100) == 3 && grid_blocks(8, 4, 100) == 2 && grid_blocks(9, 4, 2) == 2, "");
int main(int argc, char **argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        const uint32_t w = (uint32_t)atoi(argv[i]), h = (uint32_t)atoi(argv[i + 1]);
        const TxbGeometry g(w, h);
        int got_w = -1, got_h = -1;
        const bool listed = for_retained_shape(w, h, [&](auto W, auto H) { got_w = decltype(W)::value, got_h = decltype(H)::value; });
        printf("%d %d %d %d %d %d %d %u %d %u %u %u %u %d %d %d\\n", (int)g.valid, g.sw, g.sh, g.orient, g.sqr, g.sqr_up, g.txs_ctx, g.pixels, g.tx_scale, g.iw,
               g.ih, g.retained, g.sqrt_retained, (int)listed, got_w, got_h);
    }
    printf("%u %u %u %u\\n", group_lanes(16), group_lanes(32), group_lanes(64), group_lanes(1024));
    return 0;
}
"""


def test_geometry_header(tmp_path):
    """csrc/txb_geometry.hpp by a host compiler alone, against the Python restatements: which (w, h) are transform sizes, every field
    of the 19 that are, and that the list of retained shapes holds exactly the 14 of them (each handed on as itself)."""
    src, exe = tmp_path / "geometry.cpp", tmp_path / "geometry"
    src.write_text(GEOMETRY_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(abi.PKG_ROOT, "csrc"), str(src), "-o", str(exe)], check=True)
    sides = (4, 8, 16, 32, 64)
    sizes = [(w, h) for w in sides for h in sides] + [(3, 4), (12, 8), (128, 128), (0, 0)]
    shapes = sorted({T.retained(w, h) for w, h in T.SIZES}) + [(64, 64), (4, 32), (2, 2)]
    out = subprocess.run([str(exe)] + [str(v) for s in sizes + shapes for v in s], check=True, capture_output=True, text=True).stdout
    rows = [list(map(int, line.split())) for line in out.splitlines()]
    assert rows.pop() == [16, 32, 64, 64]   # group_lanes: 4, 2 and 1 blocks to a wavefront, then one block to 64 lanes
    assert len(rows) == len(sizes) + len(shapes)
    for (w, h), row in zip(sizes, rows):
        g = dict(zip(GEOMETRY_FIELDS, row))
        assert g["valid"] == ((w, h) in T.SIZES), (w, h)
        if g["valid"]:
            sw, sh = T.size_index(w), T.size_index(h)
            want = dict(valid=1, sw=sw, sh=sh, orient=(w > h) - (w < h), sqr=min(sw, sh), sqr_up=max(sw, sh),
                        txs_ctx=(T.size_index(min(w, h)) + T.size_index(max(w, h)) + 1) >> 1, pixels=w * h, tx_scale=T.tx_scale(w, h),
                        iw=T.retained(w, h)[0], ih=T.retained(w, h)[1], retained=T.retained(w, h)[0] * T.retained(w, h)[1],
                        sqrt_retained=R.SQRT_TX_PIXELS[(w, h)])
            assert g == want, (w, h)
    assert len(shapes) == 14 + 3
    for (iw, ih), row in zip(shapes, rows[len(sizes):]):
        listed = (iw, ih) in shapes[:14]
        assert row[13:] == ([1, iw, ih] if listed else [0, -1, -1]), (iw, ih)


@pytest.mark.parametrize("name", ["svt_hip_rdoq_batch", "svt_hip_rdoq_batch_mapped"])
def test_rdoq_export_is_not_an_rtcd_leaf(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf."""
    assert_not_rtcd_leaf(name)


def test_refusals_need_no_device():
    """A process that never called svt_hip_init: a size that is no transform size, no table set, and NULL arrays with blocks to do are
    bad parameters, and so are a mapping that does not exist or does not exist for the size; an empty batch succeeds; anything else is SVT_HIP_ERR_NO_DEVICE.  Nothing is launched either way."""
    got = fresh_process("(lambda f: ("
                        "f(p, p, p, p, 1, p, p, 1, 4, 32, None), f(p, p, p, p, 1, p, p, 1, 12, 8, None), f(p, p, p, p, 1, p, p, 0, 64, 8, None),"
                        "f(p, p, p, p, 0, p, p, 1, 8, 8, None), f(p, p, p, p, 0, p, p, 0, 8, 8, None), f(None, p, p, p, 1, p, p, 1, 8, 8, None),"
                        "f(p, None, p, p, 1, p, p, 1, 8, 8, None), f(p, p, None, p, 1, p, p, 1, 8, 8, None), f(p, p, p, None, 1, p, p, 1, 8, 8, None),"
                        "f(p, p, p, p, 1, None, p, 1, 8, 8, None), f(p, p, p, p, 1, p, None, 1, 8, 8, None),"
                        "lib.svt_hip_rdoq_batch_mapped(p, p, p, p, 1, p, None, 1, 8, 8, 1, None), lib.svt_hip_rdoq_batch_mapped(p, p, p, p, 1, p, p, 1, 8, 5, 0, None),"
                        "lib.svt_hip_rdoq_batch_mapped(p, p, p, p, 1, p, p, 1, 16, 16, 2, None), lib.svt_hip_rdoq_batch_mapped(p, p, p, p, 1, p, p, 1, 4, 4, 3, None),"
                        "f(None, None, None, None, 1, None, None, 0, 16, 64, None), f(p, p, p, p, 1, p, p, 1, 16, 64, None)))(lib.svt_hip_rdoq_batch)")
    assert got == [abi.SVT_HIP_ERR_BAD_PARAMETER] * 15 + [abi.SVT_HIP_OK, abi.SVT_HIP_ERR_NO_DEVICE]
