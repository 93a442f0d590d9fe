"""CPU: svt_hip_warp_shear_params is svt_get_shear_params,
the golden fixture of tests/warp_cases.py is what the reference computes (when oracle/_ref/libsvtref.so is built), and its cases
reach what they are meant to reach."""
import ctypes as C
import os

import numpy as np
import pytest

import blend_cases as B
import warp_cases as W
from support import assert_not_rtcd_leaf
from svtav1_hip import abi

ONE = W.ONE


@pytest.mark.parametrize("name", ["svt_hip_warp_batch", "svt_hip_warp_error_batch", "svt_hip_gm_refine", "svt_hip_warp_shear_params",
                                  "svt_hip_warp_error_workspace_bytes"])
def test_warp_exports_are_not_rtcd_leaves(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf."""
    assert_not_rtcd_leaf(name)


def shear_models():
    """Seeded models: near identity, wide (gamma / delta clamp to int16), mat[2] <= 0, huge, and the hand-built ones."""
    rng = np.random.default_rng(20261)
    n = 25000
    ident = np.array([0, 0, ONE, 0, 0, ONE])
    near = ident + np.concatenate([rng.integers(-1 << 20, 1 << 20, (n, 2)), rng.integers(-6000, 6001, (n, 4))], axis=1)
    wide = ident + np.concatenate([rng.integers(-1 << 20, 1 << 20, (n, 2)), rng.integers(-120000, 120001, (n, 4))], axis=1)
    small = wide.copy()
    small[:, 2] = rng.integers(-3000, 3000, n)            # mat[2] <= 0 and tiny divisors
    huge = rng.integers(-(1 << 23), 1 << 23, (n, 6))      # alpha / beta clamp as well; products stay far inside int64
    edge = ident + np.concatenate([np.zeros((n, 2), np.int64), rng.integers(-2, 3, (n, 4)) * 8192 + rng.integers(-70, 71, (n, 4))], axis=1)
    hand = [[0, 0] + list(m) for m in W.LIMIT_MODELS] + [[0, 0, 0, 0, 0, ONE], [0, 0, -ONE, 5, 5, ONE], [0, 0, 1, 0, 40000, ONE],
                                                        [0, 0, ONE + 32767, 32767, 0, ONE], [0, 0, ONE + 32736, -32736, 0, ONE]]
    return np.concatenate([near, wide, small, huge, edge, np.array(hand)]).astype(np.int64)


def test_shear_params_match_reference(ref):
    """svt_hip_warp_shear_params against svt_get_shear_params: the return value and all four parameters (where the reference
    leaves the model alone -- mat[2] <= 0 -- so does the library)."""
    lib = abi.load()
    get = B._fn(ref, "svt_get_shear_params", C.c_int, C.c_void_p)
    models = shear_models()
    assert len(models) >= 100000 and (models[:, 2] <= 0).sum() > 5000
    wm, mat, out = W.WarpedMotionParams(), (C.c_int32 * 6)(), (C.c_int16 * 4)()
    valid = clamped = 0
    for m in models.tolist():
        wm.wmtype, wm.wmmat[:6] = W.AFFINE, m
        wm.alpha, wm.beta, wm.gamma, wm.delta = out[:] = (11, -22, 33, -44)
        mat[:] = m
        want = get(C.addressof(wm))
        got = lib.svt_hip_warp_shear_params(mat, out)
        assert (got, list(out)) == (want, [wm.alpha, wm.beta, wm.gamma, wm.delta]), m
        valid += want
        clamped += m[2] > 0 and (abs(m[2] - ONE) > 32767 or abs(m[3]) > 32767 or 32704 in (abs(wm.gamma), abs(wm.delta)) or -32768 in (wm.gamma, wm.delta))
    assert valid > 10000 and clamped > 5000, (valid, clamped)
    for m in W.LIMIT_MODELS:
        ok, shear = W.lib_shear([0, 0] + list(m))
        assert ok == 1 and max(4 * abs(shear[0]) + 7 * abs(shear[1]), 4 * abs(shear[2]) + 4 * abs(shear[3])) >= 65280


def test_workspace_helper():
    lib = abi.load()
    ws = lib.svt_hip_warp_error_workspace_bytes
    assert ws(0, 8, 1) == ws(8, 0, 1) == ws(8, 8, 0) == 0
    last = 0
    for w, h, n in ((1, 1, 1), (24, 16, 1), (32, 32, 1), (33, 32, 1), (104, 88, 1), (104, 88, 44), (1920, 1080, 1), (1920, 1080, 8), (7680, 4320, 64)):
        blocks = -(-w // 32) * -(-h // 32)
        assert ws(w, h, n) >= n * blocks * 4 and ws(w, h, n) >= last
        last = ws(w, h, n)
    for w in range(1, 200, 7):
        assert ws(w, 90, 3) <= ws(w + 1, 90, 3) and ws(90, w, 3) <= ws(90, w + 1, 3) and ws(w, w, 3) <= ws(w, w, 4)


def test_warp_golden_matches_reference(ref):
    """Every entry of the golden fixture, recomputed by the reference's own functions."""
    gold = np.load(W.GOLD)
    rec = W.golden_entries(ref)
    assert set(rec) == set(gold.files)
    for k, v in rec.items():
        v = np.asarray(v)
        assert gold[k].dtype == v.dtype and gold[k].shape == v.shape and np.array_equal(gold[k], v), k
    assert os.path.getsize(W.GOLD) <= os.path.getsize(B.GOLD)


def test_warp_cases_cover_the_interface():
    """Sizes, formats, compound modes, models, window positions and both clip ends, on the reference's recorded blocks."""
    gold = np.load(W.GOLD)
    cases = W.WARP_CASES
    assert gold["warped_filter"].shape == (193, 8) and gold["warped_filter"].dtype == np.int16 and (gold["warped_filter"].sum(axis=1) == 128).all()
    assert len(cases) > 100 and len({c[0] for c in cases}) == len(cases)
    assert {(c[1], c[2], c[3]) for c in cases} == {(0, 8, 8), (0, 8, 16), (0, 16, 8), (0, 32, 32), (0, 64, 64), (0, 128, 128), (1, 4, 4), (1, 4, 8),
                                                   (1, 8, 4), (1, 16, 16), (1, 32, 32)}
    assert {(c[4], c[5]) for c in cases if c[2] < 128} == {(f, c) for f in range(3) for c in range(4)}
    assert {c[6] for c in cases if c[5] == 3} == {0, 1, 2}
    for f in range(3):
        assert {c[7] for c in cases if c[4] == f} == set(W.MODELS) and {c[8] for c in cases if c[4] == f} == set(W.POSITIONS)
    # every size meets every model and every window position, and checkerboards as well as random content
    for size in {(c[1], c[2], c[3]) for c in cases if c[2] < 128}:
        mine = [c for c in cases if (c[1], c[2], c[3]) == size]
        assert {c[7] for c in mine} == set(W.MODELS) and {c[8] for c in mine} == set(W.POSITIONS), size
        assert {c[9] for c in mine} == {False, True}, size
    def classes(x0, x1, y0, y1, Wp, Hp):
        """Where one 15 x 15 source window lies; "cross": over an edge with part of it on the plane."""
        out = {"inside"} if x0 >= 0 and x1 < Wp and y0 >= 0 and y1 < Hp else set()
        out |= ({"left"} if x0 < 0 <= x1 else set()) | ({"right"} if x0 < Wp <= x1 else set())
        out |= ({"top"} if y0 < 0 <= y1 else set()) | ({"bottom"} if y0 < Hp <= y1 else set())
        out |= {"cross"} if out - {"inside"} and x1 >= 0 and x0 < Wp and y1 >= 0 and y0 < Hp else set()
        return out | ({("out", x1 < 0, y1 < 0)} if (x1 < 0 or x0 >= Wp) and (y1 < 0 or y0 >= Hp) else set())

    seen, clip_lo, clip_hi, wider, odd = set(), 0, 0, 0, 0
    big = set()   # window classes over the 8 x 8 blocks of the 64 x 64 cases, which are recorded as digests
    real = {}     # size -> window classes of each of its cases whose recorded block is real filter output (> 4 distinct samples)
    for i, case in enumerate(cases):
        mine = set().union(*(classes(*win, *(W.CHROMA if case[1] else W.LUMA)) for win in W.block_windows(case, i)))
        seen |= mine
        big |= mine if case[2] == 64 else set()
        seen |= {"pcol"} if W.case_model(case, i)[1] and W.case_model(case, i)[2] else set()
        inp = W.WarpInputs(case, i)
        wider += all(b.stride > b.w for b in inp.buffers())
        odd += any((b.byte_offset // b.a.itemsize) % 2 or b.stride % 2 for b in inp.buffers())
        name = f"warp_{case[0]}"
        if name in gold.files and case[5] != 1:
            assert gold[name].shape == (case[3], case[2]) and gold[name].dtype == (np.uint16 if W.FORMATS[case[4]][1] else np.uint8)
            if len(np.unique(gold[name])) > 4:
                real.setdefault(case[1:4], []).append(mine)
            clip_lo += int((gold[name] == 0).any())
            clip_hi += int((gold[name] == (1 << W.FORMATS[case[4]][0]) - 1).any())
    assert seen >= {"inside", "left", "right", "top", "bottom", "pcol"} | {("out", a, b) for a in (False, True) for b in (False, True)}
    assert clip_lo >= 6 and clip_hi >= 6 and wider > 50 and odd > 50
    # The arithmetic of every size whose blocks are recorded in full (the 4-wide and 4-high ones among them) is pinned by data, not
    # by the constant block of an all-clamped window: of the 8 or 9 pixel-writing cases of a size, 6 of 10 positions keep the window
    # on the plane, so at least three varied blocks, one with a window wholly inside and one crossing an edge, must be there.
    full = {(c[1], c[2], c[3]) for c in cases if c[2] * c[3] <= W.FULL_LIMIT}
    assert full >= {(1, 4, 4), (1, 4, 8), (1, 8, 4), (0, 8, 8), (1, 16, 16), (0, 32, 32)} and set(real) == full
    for size in full:
        assert len(real[size]) >= 3 and any("inside" in m for m in real[size]) and any("cross" in m for m in real[size]), (size, real[size])
    assert big >= {"inside", "left", "right", "top", "bottom"}
    assert {c[1] for c in W.INTER_CASES} == {"warp_conv", "conv_warp", "warp_warp_wedge"} and {c[4] for c in W.INTER_CASES} == {8, 10}
    for c in W.INTER_CASES:
        assert gold[f"inter_{c[0]}"].shape == (c[3], c[2]) and len(np.unique(gold[f"inter_{c[0]}"])) > 20


def test_error_cases_cover_the_walk():
    """Asserted on the reference's recorded results: early exits, full walks, a spread of blocks_summed, refused models."""
    gold = np.load(W.GOLD)
    assert W.ERROR_PICTURES == ((104, 88), (32, 32), (24, 16), (96, 64))
    n_valid = len(W.ERROR_MODELS) * len(W.THRESHOLDS)
    for k, (w, h) in enumerate(W.ERROR_PICTURES):
        for chess in (0, 1):
            best, res = gold[f"error_{k}_{chess}_best"], gold[f"error_{k}_{chess}_results"]
            assert len(best) == len(res) >= 40 and res.dtype == abi.WARP_ERROR_RESULT_DTYPE
            assert (res["status"][n_valid:] == abi.WARP_ERROR_BAD_SHEAR).all() and len(res) - n_valid == 2 and (res["error"][n_valid:] == 0).all()
            assert (res["status"][:n_valid] == 0).all()
            full = np.repeat(res["error"][:n_valid:len(W.THRESHOLDS)], len(W.THRESHOLDS))   # the "max" threshold of each model
            err, blocks = res["error"][:n_valid], res["blocks_summed"][:n_valid]
            early = (err < full) & (err > best[:n_valid])
            visited = sum(1 for r in range(-(-h // 32)) for c in range(-(-w // 32)) if not chess or (r + c) & 1)
            assert (blocks[~early] == visited).all() and (blocks[early] < visited if chess == 0 else blocks[early] <= visited).all()
            if visited > 2:   # the pictures of more than a few blocks
                assert 3 * early.sum() >= n_valid and 3 * (~early).sum() >= n_valid and len(set(blocks.tolist())) >= (2 if chess else 3)
            if chess and visited:
                assert (err[~early] % 2 == 0).all()


def test_refine_cases_move_the_model():
    gold = np.load(W.GOLD)
    assert {(c[2], c[3]) for c in W.REFINE_CASES} >= {(W.ROTZOOM, 0), (W.ROTZOOM, 1), (W.AFFINE, 0), (W.AFFINE, 1)}
    assert {c[1] for c in W.REFINE_CASES} == {0, 1, 2} and W.N_REFINEMENTS == 5 and W.REFINE_SIZE == (104, 88)
    for c in W.REFINE_CASES:
        got, start = gold[f"refine_{c[0]}"], W.refine_start(c)
        n_params = 2 * c[2]   # the parameters the hill climb searches: mat[4], mat[5] of a ROTZOOM model only mirror mat[3], mat[2]
        assert sum(int(a != b) for a, b in zip(got[:n_params], start[:n_params])) >= 2 and got[6] == c[2] and got[7] > 1
