"""GPU parity of the direct HME level-1 search (wg_direct_search, taken by me_b64_kernel when every level-1 window is at most
8 x 4 positions of a 32-sample-wide block) against the oracle, bit-exact: small pictures chosen for the paths of that search."""
import ctypes as C

import numpy as np
import pytest

import me_cases
from svtav1_hip import abi, device, frames

pytestmark = pytest.mark.gpu

# name: (clip kind, width, height, pictures, params key, cur, list 0, list 1, temporal layer, parameter overrides)
CASES = {
    # 3 x 3 b64, bottom row with b64_h = 8: 2 block rows at level 1, too few to split over lanes
    "bottom_edge": ("blocks", 192, 136, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # right column with b64_w = 8: a 4-sample-wide level-1 block keeps the staged search; both paths in one launch
    "right_edge": ("noise", 200, 128, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # every SAD ties: the first minimum in raster order has to survive the lane split and the cross-lane sum
    "ties": ("flat", 128, 128, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # clamp_window clips windows at all four borders: fewer than 8 columns / 3 rows, negative origins
    "clipped": ("fastpan", 256, 192, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # full SAD: block rows step by the raw stride and there are 32 of them (16-bit accumulators: 8 rows at most)
    "full_sad": ("fastpan", 256, 192, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, dict(hme_search_method=1, me_search_method=1)),
    # early exits and pruned references leave descriptors without a search
    "inactive": ("static", 192, 128, 5, "m8_360p_tl0", 3, [2, 1, 0], [], 0, {}),
    # the benchmark's reference structure: 5 references x 4 quadrants = 20 descriptors
    "bench_refs": ("pan", 320, 192, 6, "m8_4k_tl2", 3, [2, 1, 0], [4, 5], 2, {}),
}

_inputs = {}


def case_inputs(orc, name):
    """(params, pyramids, oracle outputs) of a case, computed once."""
    if name not in _inputs:
        kind, w, h, n, key, cur, l0, l1, tl, over = CASES[name]
        ck = ("clip", kind, w, h, n)
        if ck not in _inputs:
            _inputs[ck] = me_cases.build_pyramids(orc, me_cases.make_clip(kind, w, h, n, seed=31))
        pyrs = _inputs[ck]
        prm = me_cases.scenario_params(key, cur, l0, l1, tl, 1)
        for k, v in over.items():
            setattr(prm, k, v)
        want = me_cases.run_cpu(orc.orc_me_frame_range, prm, pyrs, cur, l0, l1, w, h)
        _inputs[name] = (prm, pyrs, want)
    return _inputs[name]


def run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h, n_copies=1):
    nb = frames.b64_count(w, h)
    dpyr = {i: device.DevicePyramid(hip, pyrs[i]) for i in set([cur] + l0 + l1)}
    outs, jobs = [], []
    for _ in range(n_copies):
        o = device.DeviceMeOut(hip, prm, nb)
        job = abi.MeFrameJob()
        job.prm = prm
        job.src = dpyr[cur].desc()
        for r, poc in enumerate(l0):
            job.ref[0][r] = dpyr[poc].desc()
        for r, poc in enumerate(l1):
            job.ref[1][r] = dpyr[poc].desc()
        job.out = o.desc()
        outs.append(o)
        jobs.append(job)
    device.me_frames(hip, jobs)
    return [o.download() for o in outs]


def test_cases_are_eligible():
    """The parameter sets used here give level-1 windows the direct search accepts (8 x 3, at most 32 descriptors); that the
    kernel takes that path shows in its level-1 counters and its time, not here."""
    for name, (_, w, h, _, key, cur, l0, l1, tl, over) in CASES.items():
        prm = me_cases.scenario_params(key, cur, l0, l1, tl, 1)
        assert prm.enable_hme_flag and prm.enable_hme_level1_flag, name
        assert (prm.hme_l1_sa.width + 7) // 8 * 8 <= 8 and prm.hme_l1_sa.height <= 4, name
        assert 4 * (len(l0) + len(l1)) <= 32, name


@pytest.mark.parametrize("name", list(CASES))
def test_l1_direct(hip, orc, name):
    _, w, h, _, _, cur, l0, l1, _, _ = CASES[name]
    prm, pyrs, want = case_inputs(orc, name)
    got = run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h)[0]
    me_cases.assert_same(want, got, name)


def test_l1_direct_repeatable(hip, orc):
    """The same job three times in one launch: three identical results, each equal to the oracle's."""
    name = "bench_refs"
    _, w, h, _, _, cur, l0, l1, _, _ = CASES[name]
    prm, pyrs, want = case_inputs(orc, name)
    got = run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h, n_copies=3)
    assert len(got) == 3
    for i, g in enumerate(got):
        me_cases.assert_same(want, g, f"{name} copy {i}")
        me_cases.assert_same(got[0], g, f"{name} copy {i} vs copy 0")
