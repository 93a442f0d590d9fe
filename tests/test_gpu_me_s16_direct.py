"""GPU parity of the direct search of 16-sample-wide blocks (wg_s16_search: HME level 0 and the wide pre-HME region read from the
1/16 reference plane, descriptor by descriptor, beside descriptors of the same call that stay staged) against the oracle,
bit-exact: small pictures chosen for the paths of that search.  `descriptor_shapes` restates the geometry of hme_round for pre-HME
and level 0 (prehme_rules, hme_l0_rules), their zero-MV-SAD exits and the kernel's shape test on the host, so that test_cases_reach_their_paths can say
without a GPU how many descriptors of every case are searched and by which path.  The library as built sends level 0 there
(SVT_HIP_ME_S16_DIRECT = 1); the wide pre-HME region takes the same path in builds with bit 1 of that switch, which these cases
cover as well: a build is tested by naming it in SVTAV1_HIP_LIB."""
import numpy as np
import pytest

import me_cases
from svtav1_hip import frames
from test_gpu_me_l1_direct import run_hip_me

S16_MAX_W, S16_MAX_ROWS = 384, 8  # sad_device.hpp
SEED = 47

# name: (clip kind, width, height, pictures, params key, cur, list 0, list 1, temporal layer, parameter overrides)
CASES = {
    # the benchmark's reference structure: 5 references x 4 quadrants = 20 level-0 descriptors; the 1/16 plane is 80 samples
    # wide, so every wide pre-HME window is clipped
    "bench_refs": ("pan", 320, 192, 6, "m8_4k_tl2", 3, [2, 1, 0], [4, 5], 2, {}),
    # 16 x 2 b64: the interior ones search the full 96- and 192-position rows, the outer ones start at negative, odd origins
    # or are clipped on the right (widths that are no multiple of eight, a partial last item, come with the narrow planes of
    # the other cases: 80 + 15 = 95 in bench_refs)
    "wide_unclipped": ("fastpan", 1024, 128, 6, "m8_4k_tl2", 3, [2, 1, 0], [4, 5], 2, {}),
    # every SAD ties across items, rows, the lanes of an item and descriptors: the first minimum in raster order has to win
    # (a constant picture has zero-MV SAD 0, under every early-exit threshold: without me_early_exit_th = 0 nothing is searched)
    "ties": ("flat", 128, 128, 6, "m8_4k_tl2", 3, [2, 1, 0], [4, 5], 2, dict(me_early_exit_th=0)),
    # last b64 row with b64_h = 8: one sub-sampled block row at 1/16, too few to split over lanes
    "bottom_edge": ("blocks", 192, 136, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # last b64 column with b64_w = 8: a 2-sample-wide block keeps the staged path; both paths in one launch
    "right_edge": ("noise", 200, 128, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # full SAD: 16 block rows at the raw stride, the most a 16-bit lane of the packed accumulator holds; noise makes SADs large
    "full_sad": ("noise", 256, 192, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, dict(hme_search_method=1, me_search_method=1)),
    # early exits and pruned references leave descriptors without a search
    "inactive": ("static", 192, 128, 5, "m8_360p_tl0", 3, [2, 1, 0], [], 0, {}),
    # the same with a threshold that lets level 0 search some (b64, reference) pairs and not others
    "part_inactive": ("static", 192, 128, 5, "m8_360p_tl0", 3, [2, 1, 0], [], 0, dict(me_early_exit_th=26200)),
    # temporal layer 0 with two lists: list 1 has a pre-HME round of its own that mirrors list 0's vectors and searches nothing
    "tl0_two_lists": ("pan", 192, 128, 5, "m8_360p_tl0", 2, [1, 0], [3, 4], 0, {}),
    # reference distances 1 and 8 in one job: the distant references' level-0 quadrants are taller than the limit and stay
    # staged beside direct ones in the same call
    "mixed_sizes": ("pan", 256, 128, 10, "m8_360p_tl2", 8, [7, 0], [9], 2, {}),
    # prehme_skip_search_line: the wide pre-HME descriptors carry `skip` and stay staged, level 0 is direct
    "skip_lines": ("pan", 256, 192, 5, "m10_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
}

_inputs = {}


def case_inputs(orc, name):
    """(params, pyramids, oracle outputs) of a case, computed once."""
    if name not in _inputs:
        kind, w, h, n, key, cur, l0, l1, tl, over = CASES[name]
        ck = ("clip", kind, w, h, n)
        if ck not in _inputs:
            _inputs[ck] = me_cases.build_pyramids(orc, me_cases.make_clip(kind, w, h, n, seed=SEED))
        pyrs = _inputs[ck]
        want = me_cases.run_cpu(orc.orc_me_frame_range, case_params(name), pyrs, cur, l0, l1, w, h)
        _inputs[name] = (case_params(name), pyrs, want)
    return _inputs[name]


def case_params(name):
    _, _, _, _, key, cur, l0, l1, tl, over = CASES[name]
    prm = me_cases.scenario_params(key, cur, l0, l1, tl, 1)
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


def scaled_dist(d):
    return d * 5 // 8 + (0 if d % 8 == 0 else 1)


def clamp_axis(org, o, sa, pad, size, round8):
    """One axis of clamp_window: (origin offset, area) of a search area clipped by the padded plane."""
    if org + o < -pad:  # (the origin moves; the area keeps its size, as in the reference)
        o = -pad - org
    if org + o > size - 1:
        o -= (org + o) - (size - 1)
    if org + o + sa > size:
        sa = max(1, sa - ((org + o + sa) - size))
    if round8 and sa >= 8:
        sa &= ~7
    return o, sa


def zz_sad(src, ref, bx, by, b64_w, b64_h):
    """zz_sad_all: zero-MV SAD of a b64 on every other row, scaled to 64 x 64 samples."""
    a = src[64 * by:64 * by + b64_h:2, 64 * bx:64 * bx + b64_w].astype(np.int64)
    b = ref[64 * by:64 * by + b64_h:2, 64 * bx:64 * bx + b64_w].astype(np.int64)
    return (int(np.abs(a - b).sum()) << 1) * 64 * 64 // (b64_w * b64_h)


def descriptor_shapes(prm, width, height, l0, l1, clip):
    """Every descriptor the pre-HME and level-0 rounds set up, with the exits that follow from the zero-MV SADs of the clip:
    (stage, b64 column, b64 row, list, reference, block width, block rows, sa_w, sa_h, x origin offset, skip, direct, searched).
    `direct` is the kernel's shape test on the area the descriptor gets when it is searched; `searched` is false when the
    zz-SAD early exit of its stage (check_prehme_early_exit, the head of hme_l0_rules) or the zz-SAD pruning of the reference
    (zz_prune_lane0) takes the search away.  The pruning behind pre-HME (phme_prune_lane0) depends on search results and is not
    restated: it can take further level-0 searches of references other than the first away, never add one."""
    th, searching = prm.me_early_exit_th, lambda li: prm.temporal_layer_index > 0 or li == 0  # noqa: E731
    assert not prm.me_safe_limit_zz_th and not prm.prev_me_stage_based_exit_th  # exits this restatement leaves out
    W, H, pad = width >> 2, height >> 2, frames.SIXTEENTH_PAD - 1
    sub = prm.hme_search_method == 0
    assert not (prm.reduce_hme_l0_sr_th_min and prm.reduce_hme_l0_sr_th_max)  # else the level-0 area depends on vectors
    out = []
    for by in range((height + 63) // 64):
        for bx in range((width + 63) // 64):
            b64_w, b64_h = min(64, width - 64 * bx), min(64, height - 64 * by)
            bw, bh = b64_w >> 2, ((b64_h >> 2) >> 1 if sub else b64_h >> 2)
            ox16, oy16 = 16 * bx, 16 * by
            zz = {(li, ri): zz_sad(clip[prm.picture_number], clip[poc], bx, by, b64_w, b64_h)
                  for li, pocs in enumerate((l0, l1)) for ri, poc in enumerate(pocs) if th and searching(li)}
            best = min(zz.values(), default=0)
            for li, pocs in enumerate((l0, l1)):
                for ri, poc in enumerate(pocs):
                    z = zz.get((li, ri))
                    pruned = (z is not None and ri >= 1 and prm.temporal_layer_index > 0 and best < prm.zz_sad_th and
                              (z - best) * 100 > prm.zz_sad_pct * best)
                    alive = {"prehme": not pruned and not (z is not None and z < th),
                             "l0": not pruned and not (z is not None and z < (th >> 2))}
                    factor = scaled_dist(abs(prm.picture_number - poc))
                    shapes = []
                    if prm.prehme_enable and (prm.temporal_layer_index > 0 or li == 0):
                        for si in range(2):
                            sa_w = min(prm.prehme_sa_min[si].width * factor, prm.prehme_sa_max[si].width)
                            sa_h = min(prm.prehme_sa_min[si].height * factor, prm.prehme_sa_max[si].height)
                            ox, sa_w = clamp_axis(ox16, -(sa_w >> 1), sa_w, pad, W, False)
                            _, sa_h = clamp_axis(oy16, -(sa_h >> 1), sa_h, pad, H, False)
                            skip = bool(prm.prehme_skip_search_line and bw == 16 and bh <= 16)
                            shapes.append(("prehme%d" % si, sa_w, sa_h, ox, skip))
                    if prm.enable_hme_flag and prm.enable_hme_level0_flag and (prm.temporal_layer_index > 0 or li == 0):
                        mn = [prm.hme_l0_sa_min.width, prm.hme_l0_sa_min.height]
                        mx = [prm.hme_l0_sa_max.width, prm.hme_l0_sa_max.height]
                        if prm.enable_me_sr_adjustment and prm.distance_based_hme_resizing:
                            mn, mx = [v // (1 + ri) for v in mn], [v // (1 + ri) for v in mx]
                        nw, nh = prm.num_hme_sa_w, prm.num_hme_sa_h
                        w = min((mn[0] // nw * factor + 15) & ~15, (mx[0] // nw + 15) & ~15)
                        h = min(mn[1] // nh * factor, mx[1] // nh)
                        w = (w + 7) & ~7
                        for qy in range(nh):
                            for qx in range(nw):
                                ox, sa_w = clamp_axis(ox16, -((w * nw) >> 1) + w * qx, w, pad, W, True)
                                _, sa_h = clamp_axis(oy16, -((h * nh) >> 1) + h * qy, h, pad, H, False)
                                shapes.append(("l0", sa_w, sa_h, ox, False))
                    for stage, sa_w, sa_h, ox, skip in shapes:
                        direct = (bw == 16 and bh <= 16 and not skip and 0 < sa_w <= S16_MAX_W and 0 < sa_h <= S16_MAX_ROWS)
                        out.append((stage, bx, by, li, ri, bw, bh, sa_w, sa_h, ox, skip, direct, alive[stage[:6] if stage != "l0" else stage]))
    return out


def shapes_of(name):
    kind, w, h, n, _, _, l0, l1, _, _ = CASES[name]
    return descriptor_shapes(case_params(name), w, h, l0, l1, me_cases.make_clip(kind, w, h, n, seed=SEED))


def test_cases_reach_their_paths():
    """Host only: which descriptors of every case are searched at all, and which of those the kernel's shape test sends to the
    direct search.  (A search width under
    8 cannot reach it: a 16-sample block means a 1/16 plane at least 16 wide past the b64's origin, a window clipped on the left keeps
    its size, and one clipped on the right still reaches from its origin, at most 16 x (column) - 16 + 16, to the plane's edge.)"""
    sh = {name: shapes_of(name) for name in CASES}
    count = {}  # name: {stage: (descriptors searched by the direct path, searched staged, not searched)}
    for name, rows in sh.items():
        count[name] = {st: (sum(r[11] and r[12] for r in rows if r[0] == st), sum(not r[11] and r[12] for r in rows if r[0] == st),
                            sum(not r[12] for r in rows if r[0] == st)) for st in ("prehme0", "prehme1", "l0")}
        print(name, count[name], sorted({(r[0], r[5], r[6], r[7], r[8], r[11]) for r in rows if r[12]}))
    for name in sh:
        c = count[name]
        if name == "inactive":  # every zero-MV SAD is under both thresholds: rounds of descriptors with nothing to search
            assert all(v[0] + v[1] == 0 and v[2] > 0 for v in c.values()), (name, c)
        elif name == "part_inactive":  # level 0's threshold lies inside the spread of the zero-MV SADs: calls of both kinds
            assert c["l0"][0] > 0 and c["l0"][2] > 0 and c["prehme1"][0] == 0, (name, c)
        else:  # the others search what they set up (`bottom_edge` loses a few b64 of still content), the cases about
            assert all(v[0] + v[1] > 4 * v[2] for v in c.values()), (name, c)  # level 0 all of it
            assert name == "bottom_edge" or c["l0"][2] == 0, (name, c)
    # `ties`: with no early-exit threshold nothing depends on the zero-MV SADs, and equal SADs prune no reference (the pruning
    # rules ask for a SAD above the best one): 2 x 2 b64 x 5 references x 4 quadrants, all direct
    assert case_params("ties").me_early_exit_th == 0 and count["ties"]["l0"] == (80, 0, 0) and count["ties"]["prehme1"] == (20, 0, 0)
    sh = {name: [r for r in rows if r[12]] for name, rows in sh.items()}  # from here on: the descriptors that are searched
    is_dir = lambda r: r[11]                       # noqa: E731
    wide = lambda r: r[0] == "prehme1"              # noqa: E731
    tall = lambda r: r[0] == "prehme0"              # noqa: E731
    lev0 = lambda r: r[0] == "l0"                   # noqa: E731
    for name, rows in sh.items():  # the tall region never qualifies
        assert not any(is_dir(r) for r in rows if tall(r)), name
    b = sh["bench_refs"]
    one = [r for r in b if lev0(r) and (r[1], r[2]) == (2, 1)]
    assert len(one) == 20 and all(is_dir(r) for r in one) and {(r[7], r[8]) for r in one} == {(16, 8), (16, 4)}
    assert all(is_dir(r) and r[7] < (96, 192, 192)[r[4]] for r in b if wide(r) and r[3] == 0)
    u = [r for r in sh["wide_unclipped"] if wide(r)]
    assert all(is_dir(r) for r in u)
    assert {(96, 3), (192, 3)} <= {(r[7], r[8]) for r in u}
    assert any(r[9] + 16 * r[1] < 0 for r in u) and any(r[7] < 96 for r in u)
    assert any(r[7] % 8 for r in b if wide(r))
    assert all(is_dir(r) for r in sh["ties"] if not tall(r))
    e = [r for r in sh["bottom_edge"] if r[2] == 2 and not tall(r)]
    assert e and all(is_dir(r) and r[6] == 1 for r in e)
    e = sh["right_edge"]
    assert {r[5] for r in e} == {16, 2} and not any(is_dir(r) for r in e if r[5] == 2) and any(is_dir(r) for r in e if r[5] == 16)
    assert all(r[6] == 16 and is_dir(r) for r in sh["full_sad"] if not tall(r))
    assert any(is_dir(r) for r in sh["tl0_two_lists"])
    assert not any(r[3] == 1 for r in sh["tl0_two_lists"])  # list 1 mirrors list 0 at temporal layer 0
    m = [r for r in sh["mixed_sizes"] if lev0(r)]
    assert any(is_dir(r) for r in m) and any(not is_dir(r) and r[8] > S16_MAX_ROWS for r in m)
    s = sh["skip_lines"]
    assert all(r[10] and not is_dir(r) for r in s if wide(r)) and all(is_dir(r) for r in s if lev0(r))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_s16_direct(hip, orc, name):
    _, w, h, _, _, cur, l0, l1, _, _ = CASES[name]
    prm, pyrs, want = case_inputs(orc, name)
    got = run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h)[0]
    me_cases.assert_same(want, got, name)


@pytest.mark.gpu
def test_s16_direct_repeatable(hip, orc):
    """The same job three times in one launch: three identical results, each equal to the oracle's."""
    name = "bench_refs"
    _, w, h, _, _, cur, l0, l1, _, _ = CASES[name]
    prm, pyrs, want = case_inputs(orc, name)
    got = run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h, n_copies=3)
    assert len(got) == 3
    for i, g in enumerate(got):
        me_cases.assert_same(want, g, f"{name} copy {i}")
        me_cases.assert_same(got[0], g, f"{name} copy {i} vs copy 0")
