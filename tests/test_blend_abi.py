"""CPU: the golden
fixture of tests/blend_cases.py is what the reference computes (when oracle/_ref/libsvtref.so is built), and its cases reach what
they are meant to reach."""
import numpy as np
import pytest

import blend_cases as B
from support import assert_not_rtcd_leaf
from svtav1_hip import abi


@pytest.mark.parametrize("name", ["svt_hip_blend_batch", "svt_hip_compound_mask_search_batch"])
def test_blend_exports_are_not_rtcd_leaves(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf."""
    assert_not_rtcd_leaf(name)


def test_blend_golden_matches_reference(ref):
    """Every entry of the golden fixture, recomputed by the reference's own functions."""
    gold = np.load(B.GOLD)
    rec = B.golden_entries(ref)
    assert set(rec) == set(gold.files)
    for k, v in rec.items():
        v = np.asarray(v)
        assert gold[k].dtype == v.dtype and gold[k].shape == v.shape and np.array_equal(gold[k], v), k


def test_blend_fixture_tables_have_the_reference_layout():
    """The wedge masks are 32 per size in the order 2 * index + sign with weights 0 .. 64, and the ramps are the OBMC lengths."""
    gold = np.load(B.GOLD)
    total = 0
    for (w, h) in B.WEDGE_BSIZE:
        m = gold[f"wedge_{w}x{h}"]
        assert m.dtype == np.uint8 and m.shape == (2 * abi.WEDGE_TYPES, w * h) and m.max() == 64 and m.min() == 0
        assert np.array_equal(m[0::2].astype(int) + m[1::2], np.full((abi.WEDGE_TYPES, w * h), 64))
        assert len({m[2 * i].tobytes() for i in range(abi.WEDGE_TYPES)}) == abi.WEDGE_TYPES
        total += m.size
    assert total == 100352
    for n in B.OBMC_LENGTHS:
        r = gold[f"obmc_{n}"]
        assert r.shape == (n,) and r[-1] == 64 and (np.diff(r.astype(int)) >= 0).all() and r.min() >= 32


def test_blend_cases_cover_the_interface():
    """Kinds, sub-samplings, sample formats, mask types, strides, misaligned rows and block sizes of the blend cases."""
    gold = np.load(B.GOLD)
    cases = B.BLEND_CASES
    assert len(cases) > 100 and len({c[0] for c in cases}) == len(cases)
    assert {c[1] for c in cases} == set(range(5))
    for kind in (abi.BLEND_D16, abi.BLEND_MASK):
        assert {(c[6], c[7]) for c in cases if c[1] == kind} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for kind in range(5):
        assert {(c[4], c[5]) for c in cases if c[1] == kind} == set(B.FORMATS), kind
    assert {(c[8], c[4], c[5]) for c in cases if c[1] == abi.BLEND_D16_DIFFWTD} == {(t, bd, s) for t in (0, 1) for bd, s in B.FORMATS}
    sizes = {(c[1], c[2], c[3]) for c in cases}
    assert (abi.BLEND_D16, 4, 4) in sizes and (abi.BLEND_D16, 128, 128) in sizes and (abi.BLEND_MASK, 128, 128) in sizes
    assert (abi.BLEND_HMASK, 2, 8) in sizes and (abi.BLEND_VMASK, 8, 1) in sizes
    wider, odd, inplace, clipped_lo, clipped_hi, built = 0, 0, 0, 0, 0, set()
    for i, case in enumerate(cases):
        inp = B.BlendInputs(case, i, gold)
        bufs = (inp.src0, inp.src1, inp.dst)
        wider += any(b.stride > b.w for b in bufs)
        odd += any((b.byte_offset // b.a.itemsize) % 2 or b.stride % 2 for b in bufs)
        inplace += inp.dst is inp.src0
        name = f"blend_{case[0]}_dst"
        if name in gold.files and case[1] <= abi.BLEND_D16_DIFFWTD:   # the d16 blends clip at both ends of the range somewhere
            clipped_lo += int((gold[name] == 0).any())
            clipped_hi += int((gold[name] == (1 << case[4]) - 1).any())
        if f"blend_{case[0]}_mask" in gold.files:
            built |= set(np.unique(gold[f"blend_{case[0]}_mask"]).tolist())
    assert wider > 50 and odd > 50 and inplace >= 6 and clipped_lo >= 3 and clipped_hi >= 3
    assert min(built) < 26 and max(built) == 64 and len(built) > 10    # both mask types, a spread of weights


def test_search_cases_cover_the_search():
    """Asserted on the reference's recorded results and on counters taken from its intermediates."""
    gold = np.load(B.GOLD)
    res, cases = gold["search_results"], B.SEARCH_CASES
    assert len(res) == len(cases) and res.dtype == B.RESULT_DTYPE
    wedge = np.array([bool(c[6]) for c in cases])
    assert {(c[1], c[2]) for c in cases if c[6]} == set(B.WEDGE_BSIZE)
    assert {(c[3], c[4]) for c in cases if c[6]} == set(B.FORMATS)
    assert any(max(c[1], c[2]) == 128 for c in cases) and any(not c[6] and (c[1], c[2]) in B.WEDGE_BSIZE for c in cases)
    assert set(res["wedge_sign"][wedge].ravel().tolist()) == {0, 1} and set(res["best_wedge_sign"][wedge].tolist()) == {0, 1}
    assert len(set(res["best_wedge_index"][wedge].tolist())) >= 8
    assert (res["best_wedge_index"][~wedge] == -1).all() and (res["wedge_sse"][~wedge] == 0).all()
    assert set(res["best_diffwtd_type"].tolist()) == {0, 1}
    # an exact tie between wedge indices: pred0 == pred1 makes every SSE equal, the first index wins
    flat = np.array([c[5] == "flat" for c in cases])
    assert flat.sum() >= 9 and (res["wedge_sse"][flat] == res["wedge_sse"][flat][:, :1]).all() and (res["wedge_sse"][flat] > 0).all()
    assert (res["best_wedge_index"][flat] == 0).all() and (res["best_diffwtd_type"][flat] == 0).all() and (res["pred0_to_pred1_dist"][flat] == 0).all()
    # strict <: the winner is the first minimum everywhere
    assert (res["best_wedge_index"][wedge] == res["wedge_sse"][wedge].argmin(axis=1)).all()
    ds_saturated, t_clamped, t_clamped_10bit = gold["search_counters"].tolist()
    assert ds_saturated > 100 and t_clamped_10bit > 100
    # strides larger than w and rows at odd sample offsets
    inputs = [B.SearchInputs(c, i) for i, c in enumerate(cases)]
    assert sum(any(b.stride > b.w for b in inp.buffers()) for inp in inputs) > 50
    assert sum(any(b.off % 2 or b.stride % 2 for b in inp.buffers()) for inp in inputs) > 50


def test_picture_and_pipeline_cases():
    gold = np.load(B.GOLD)
    best = gold["picture_best"]
    assert best.shape == (3, len(B.picture_blocks())) and len(B.picture_blocks()) == 120 * 67
    assert len(set(best[0].tolist())) >= 8 and set(best[1].tolist()) == {0, 1} and set(best[2].tolist()) == {0, 1}
    assert {(c[3], c[4], c[5]) for c in B.PIPE_CASES} == {(bd, s, t) for bd, s in ((8, 0), (10, 1)) for t in (B.COMPOUND_WEDGE, B.COMPOUND_DIFFWTD)}
    for c in B.PIPE_CASES:
        y, u = gold[f"pipe_{c[0]}_y"], gold[f"pipe_{c[0]}_u"]
        assert y.shape == (c[2], c[1]) and u.shape == (c[2] // 2, c[1] // 2) and y.dtype == (np.uint16 if c[4] else np.uint8)
        if c[5] == B.COMPOUND_DIFFWTD:
            m = gold[f"pipe_{c[0]}_mask"]
            assert m.shape == y.shape and len(np.unique(m)) > 3
