"""GPU parity of the direct full-pel search (fullpel_direct_all, taken by me_b64_kernel when every reference's final window is
small: all references in one pass, windows read from the reference planes) against the oracle, bit-exact on every output array:
small pictures chosen for the ways that search can go wrong."""
import numpy as np
import pytest

import me_cases
from svtav1_hip import abi, device, frames

gpu = pytest.mark.gpu

# the limits of fullpel_direct_all (me_frame.hip: FPD_MAX_W, FPD_MAX_ROWS): widest / tallest final window it takes
FPD_MAX_W, FPD_MAX_ROWS = 24, 9

# name: (clip kind, width, height, pictures, params key, cur, list 0, list 1, temporal layer, parameter overrides)
CASES = {
    # bottom b64 row with b64_h = 8: the 16 block lanes of an item read into the padding
    "bottom_edge": ("blocks", 192, 136, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # right column with b64_w = 8
    "right_edge": ("noise", 200, 128, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # every SAD ties: the first minimum in raster order has to survive the flat item range, the 16-lane groups and the 64-bit
    # minima of several references side by side
    "ties": ("flat", 128, 128, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # clamp_me_window cuts windows at all four borders: widths that are no multiple of 4, negative origins
    "clipped": ("fastpan", 256, 192, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, {}),
    # zz_sad below me_early_exit_th / 6: 1 x 1 windows, and pruned references, which have no items at all
    "one_by_one": ("static", 192, 128, 5, "m8_360p_tl0", 3, [2, 1, 0], [], 0, {}),
    # full SAD: 16 rows per block, the 16-bit accumulators at their bound
    "full_sad": ("fastpan", 256, 192, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, dict(me_search_method=1, hme_search_method=1)),
    # the benchmark's slot layout: list 0 = 3 references, list 1 = 2
    "bench_refs": ("pan", 320, 192, 6, "m8_4k_tl2", 3, [2, 1, 0], [4, 5], 2, {}),
    # the parameter bound exceeds the limits: the loop over the references is still right (whether both paths occur in one
    # launch depends on the content)
    "staged_fallback": ("fastpan", 256, 192, 5, "m8_360p_tl2", 2, [1, 0], [3, 4], 2, dict(me_sa_min=(32, 16), me_sa_max=(64, 32))),
}
ELIGIBLE = [n for n in CASES if n != "staged_fallback"]

_inputs = {}


def make_params(name):
    _, _, _, _, key, cur, l0, l1, tl, over = CASES[name]
    prm = me_cases.scenario_params(key, cur, l0, l1, tl, 1)
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(prm, k).width, getattr(prm, k).height = v
        else:
            setattr(prm, k, v)
    return prm


def case_inputs(orc, name):
    """(params, pyramids, oracle outputs) of a case, computed once."""
    if name not in _inputs:
        kind, w, h, n, _, cur, l0, l1, _, _ = CASES[name]
        ck = ("clip", kind, w, h, n)
        if ck not in _inputs:
            _inputs[ck] = me_cases.build_pyramids(orc, me_cases.make_clip(kind, w, h, n, seed=31))
        pyrs = _inputs[ck]
        prm = make_params(name)
        want = me_cases.run_cpu(orc.orc_me_frame_range, prm, pyrs, cur, l0, l1, w, h)
        _inputs[name] = (prm, pyrs, want)
    return _inputs[name]


def make_job(prm, descs, cur, l0, l1, out):
    job = abi.MeFrameJob()
    job.prm = prm
    job.src = descs[cur]
    for r, poc in enumerate(l0):
        job.ref[0][r] = descs[poc]
    for r, poc in enumerate(l1):
        job.ref[1][r] = descs[poc]
    job.out = out.desc()
    return job


def run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h, n_copies=1):
    nb = frames.b64_count(w, h)
    dpyr = {i: device.DevicePyramid(hip, pyrs[i]) for i in set([cur] + l0 + l1)}
    descs = {i: d.desc() for i, d in dpyr.items()}
    outs = [device.DeviceMeOut(hip, prm, nb) for _ in range(n_copies)]
    device.me_frames(hip, [make_job(prm, descs, cur, l0, l1, o) for o in outs])
    return [o.download() for o in outs]


def window_bound(prm, l0, l1):
    """Largest final window the parameters allow (fullpel_prepare_all before the variance rule, which only shrinks)."""
    wmax = hmax = 0
    for li, refs in enumerate((l0, l1)):
        for ri in range(len(refs)):
            dist = abs(int(prm.picture_number) - int(prm.ref_picture_number[li][ri]))
            scaled = dist * 5 // 8 + (0 if dist % 8 == 0 else 1)
            wmax = max(wmax, (min(prm.me_sa_min.width * scaled, prm.me_sa_max.width) + 7) & ~7)
            hmax = max(hmax, min(prm.me_sa_min.height * scaled, prm.me_sa_max.height))
    return wmax, hmax


def test_cases_are_eligible():
    """From the parameters alone: the windows of every case but staged_fallback are within the limits of the direct search and
    the references are prepared in one pass (me_early_exit_th != 0); staged_fallback's bound is beyond the limits.  That the kernel
    takes the direct search shows in its full-pel counters and its time, not here."""
    for name in CASES:
        _, _, _, _, _, _, l0, l1, _, _ = CASES[name]
        prm = make_params(name)
        wmax, hmax = window_bound(prm, l0, l1)
        assert prm.me_early_exit_th != 0, name
        assert not prm.mv_sa_adj_enabled, name  # (it would widen the windows beyond the bound above)
        if name in ELIGIBLE:
            assert wmax <= FPD_MAX_W and hmax <= FPD_MAX_ROWS, (name, wmax, hmax)
        else:
            assert wmax > FPD_MAX_W or hmax > FPD_MAX_ROWS, (name, wmax, hmax)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fullpel_direct(hip, orc, name):
    _, w, h, _, _, cur, l0, l1, _, _ = CASES[name]
    prm, pyrs, want = case_inputs(orc, name)
    got = run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h)[0]
    me_cases.assert_same(want, got, name)


@gpu
def test_fullpel_direct_exact_planes(hip, orc):
    """The `clipped` job on planes of EXACTLY stride * (height + 2 * org_y) bytes, packed back to back in one allocation (the
    memory contract of include/svt_hip_me.h, as tests/test_gpu_me.py::test_me_frame_exact_size_planes): a byte read past a plane
    belongs to the next plane, and past the last one to a sentinel area filled with 0x00 and then with 0xFF.  The run finishes
    and gives the oracle's results both times."""
    name = "clipped"
    _, w, h, _, _, cur, l0, l1, _, _ = CASES[name]
    prm, pyrs, want = case_inputs(orc, name)
    planes = [pl for p in pyrs for pl in p.planes()]
    total = sum(pl.nbytes for pl in planes)
    SENT = 4096
    big = device.DeviceBuffer(hip, total + SENT)
    nb = frames.b64_count(w, h)
    for sentinel in (0x00, 0xFF):
        host = np.full(total + SENT, sentinel, np.uint8)
        descs, off = [], 0
        for pl in planes:
            host[off:off + pl.nbytes] = pl.buf.reshape(-1)
            descs.append(pl.desc(big.ptr + off))
            off += pl.nbytes
        big.upload(host)
        pyr_desc = [abi.Pyramid8(*descs[3 * i:3 * i + 3]) for i in range(len(pyrs))]
        out = device.DeviceMeOut(hip, prm, nb)
        device.me_frames(hip, [make_job(prm, pyr_desc, cur, l0, l1, out)])
        me_cases.assert_same(want, out.download(), f"exact-size planes, sentinel {sentinel:#x}")


@gpu
def test_fullpel_direct_repeatable(hip, orc):
    """The same job three times in one launch: three identical results, each equal to the oracle's."""
    name = "bench_refs"
    _, w, h, _, _, cur, l0, l1, _, _ = CASES[name]
    prm, pyrs, want = case_inputs(orc, name)
    got = run_hip_me(hip, prm, pyrs, cur, l0, l1, w, h, n_copies=3)
    assert len(got) == 3
    for i, g in enumerate(got):
        me_cases.assert_same(want, g, f"{name} copy {i}")
        me_cases.assert_same(got[0], g, f"{name} copy {i} vs copy 0")
