"""svt_hip_analysis_frames through its fused kernel (csrc/pyramid.hip): both decimated planes, their padding and the block
statistics from one read of the full plane.  Every case compares whole buffers, padding included, with the oracle's
orc_pyramid_frame / orc_variance_frame; decimated planes and outputs start as 0xA5 on both sides."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import analysis_cases as ac
from svtav1_hip import abi, device, frames

pytestmark = pytest.mark.gpu

# 64x64: one tile, every edge at once.  200x136: partial blocks both ways.  130x70: odd quarter size 65x35.
# 206x142: width no multiple of 4, 8 or 16.  648x360: several tiles per row, a last tile with one block.
SIZES = [(64, 64), (200, 136), (130, 70), (206, 142), (648, 360)]
MODES = [(1, 0), (1, 1), (0, 0), (0, 1)]    # (hme_level1_enabled, full_precision)


def check_job(dj, case, l1, fp, what):
    ac.assert_equal(dj.results(), ac.reference(*case, l1, fp), what)


@pytest.mark.parametrize("l1,fp", MODES)
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_and_modes(hip, w, h, l1, fp):
    """Two pictures of one size in a batch, the first with `mean`, the second with mean == NULL."""
    cases = [("noise", w, h, 31), ("pan", w, h, 32)]
    djobs = [ac.DeviceJob(hip, *c, with_mean=(i == 0)) for i, c in enumerate(cases)]
    ac.run(hip, [d.job() for d in djobs], l1, fp)
    for i, (d, c) in enumerate(zip(djobs, cases)):
        check_job(d, c, l1, fp, f"{w}x{h} l1={l1} fp={fp} job {i}")


@pytest.mark.parametrize("l1,fp", MODES)
def test_mixed_sizes_one_batch(hip, l1, fp):
    """Jobs of different sizes share the launch: the grid is sized by the largest job, which comes last; a 64x64 job first."""
    cases = [("noise", 64, 64, 33), ("pan", 200, 136, 34), ("noise", 130, 70, 35), ("pan", 648, 360, 36)]
    djobs = [ac.DeviceJob(hip, *c, with_mean=(i % 2 == 1)) for i, c in enumerate(cases)]
    ac.run(hip, [d.job() for d in djobs], l1, fp)
    for i, (d, c) in enumerate(zip(djobs, cases)):
        check_job(d, c, l1, fp, f"mixed batch l1={l1} fp={fp} job {i}")


@pytest.mark.parametrize("l1,fp", [(1, 0), (0, 1)])
def test_batch_of_one(hip, l1, fp):
    case = ("pan", 206, 142, 37)
    dj = ac.DeviceJob(hip, *case)
    ac.run(hip, [dj.job()], l1, fp)
    check_job(dj, case, l1, fp, f"batch of one l1={l1} fp={fp}")


@pytest.mark.parametrize("l1,fp", [(1, 0), (0, 1)])
def test_batch_of_25_then_3(hip, l1, fp):
    """More jobs than the benchmark's 21, three sizes interleaved; then a batch of 3 on the same planes, whose descriptor
    table follows the first one through the staging ring."""
    cases = [("noise" if i % 2 else "pan", (64, 130, 200)[i % 3], (64, 70)[i % 2], 50 + i % 4) for i in range(25)]
    djobs = [ac.DeviceJob(hip, *c, with_mean=(i % 3 != 2)) for i, c in enumerate(cases)]
    ac.run(hip, [d.job() for d in djobs], l1, fp)
    for i, (d, c) in enumerate(zip(djobs, cases)):
        check_job(d, c, l1, fp, f"25 jobs l1={l1} fp={fp} job {i}")
    for d in djobs[:3]:
        d.refill()
    ac.run(hip, [d.job() for d in djobs[:3]], l1, fp)
    for i, (d, c) in enumerate(zip(djobs[:3], cases)):
        check_job(d, c, l1, fp, f"3 jobs after 25 l1={l1} fp={fp} job {i}")


@pytest.mark.parametrize("l1,fp", [(1, 1), (0, 0)])
def test_exact_size_planes_back_to_back(hip, l1, fp):
    """include/svt_hip_me.h "Memory contract": the planes of two pictures packed into one allocation with 64 guard bytes
    between them, the last plane (a full plane, whose bottom padding the statistics read) ending at the allocation's last
    byte.  Results equal the oracle's and every guard byte is intact."""
    cases = [("noise", 130, 70, 38), ("pan", 200, 136, 39)]
    GUARD = 64
    guard = (np.arange(GUARD) * 7 + 3).astype(np.uint8)
    hps = [ac.prefilled_pyramid(ac.luma_of(*c)) for c in cases]
    order = [hps[0].full, hps[0].quarter, hps[0].sixteenth, hps[1].sixteenth, hps[1].quarter, hps[1].full]
    total = sum(p.nbytes for p in order) + GUARD * (len(order) - 1)
    host, offs, off = np.empty(total, np.uint8), {}, 0
    for k, p in enumerate(order):
        host[off:off + p.nbytes] = p.buf.reshape(-1)
        offs[id(p)] = off
        off += p.nbytes
        if k + 1 < len(order):
            host[off:off + GUARD] = guard
            off += GUARD
    assert off == total
    big = device.DeviceBuffer(hip, total)
    big.upload(host)
    outs, jobs = [], []
    for hp, (_, w, h, _) in zip(hps, cases):
        nb = frames.b64_count(w, h)
        dv, dm = device.DeviceBuffer(hip, nb * 85 * 2), device.DeviceBuffer(hip, nb * 85 * 8)
        pyr = abi.Pyramid8(*[p.desc(big.ptr + offs[id(p)]) for p in hp.planes()])
        jobs.append(abi.AnalysisJob(pyr, dv.ptr, dm.ptr))
        outs.append((dv, dm, nb))
    ac.run(hip, jobs, l1, fp)
    got = big.download(np.uint8, (total,))
    for k, p in enumerate(order[:-1]):
        g0 = offs[id(p)] + p.nbytes
        assert np.array_equal(got[g0:g0 + GUARD], guard), f"guard after plane {k} overwritten"
    for i, (hp, c, (dv, dm, nb)) in enumerate(zip(hps, cases, outs)):
        res = {"quarter": got[offs[id(hp.quarter)]:][:hp.quarter.nbytes].reshape(hp.quarter.buf.shape),
               "sixteenth": got[offs[id(hp.sixteenth)]:][:hp.sixteenth.nbytes].reshape(hp.sixteenth.buf.shape),
               "variance": dv.download(np.uint16, (nb, 85)), "mean": dm.download(np.uint64, (nb, 85))}
        ac.assert_equal(res, ac.reference(*c, l1, fp), f"packed planes l1={l1} fp={fp} job {i}")
        assert np.array_equal(got[offs[id(hp.full)]:][:hp.full.nbytes], hp.full.buf.reshape(-1)), "full plane changed"


@pytest.mark.parametrize("fp", [0, 1])
def test_level1_off_leaves_quarter_alone(hip, fp):
    """hme_level1_enabled = 0: not one byte of the quarter plane changes (and its descriptor may be anything)."""
    case = ("pan", 200, 136, 40)
    dj = ac.DeviceJob(hip, *case)
    before = dj.dp.quarter.download()
    assert (before == ac.FILL).all()
    ac.run(hip, [dj.job()], 0, fp)
    assert np.array_equal(dj.dp.quarter.download(), before)
    check_job(dj, case, 0, fp, f"l1=0 fp={fp}")


@pytest.mark.parametrize("fp", [0, 1])
def test_other_descriptor_sizes_take_the_three_launches(hip, fp):
    """A quarter descriptor one column narrower than width >> 1 is not the reference's geometry: the batch goes through the
    three launches and equals svt_hip_pyramid_frame + svt_hip_variance_frame for the same job on the same device."""
    kind, w, h, seed = "noise", 200, 136, 44
    narrow = ((w >> 1) - 1, h >> 1)
    a, b = (ac.DeviceJob(hip, kind, w, h, seed, quarter_size=narrow) for _ in range(2))
    ac.run(hip, [a.job()], 1, fp)
    d = b.dp.desc()
    device.check(hip, hip.svt_hip_pyramid_frame(C.byref(d.full), C.byref(d.quarter), C.byref(d.sixteenth), 1, None), "svt_hip_pyramid_frame")
    device.check(hip, hip.svt_hip_variance_frame(C.byref(d.full), C.c_void_p(b.dv.ptr), C.c_void_p(b.dm.ptr), fp, None), "svt_hip_variance_frame")
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    want = b.results()
    assert not (want["quarter"] == ac.FILL).all()
    ac.assert_equal(a.results(), want, f"narrow quarter fp={fp}")


def test_switch_off_gives_the_same_buffers(hip, tmp_path):
    """SVTAV1_HIP_ANALYSIS_FUSED=0 is read once per process: a child process runs the batch with the switch off, this
    process with the fused path, and every buffer is equal (and equal to the oracle's)."""
    out = str(tmp_path / "unfused.npz")
    env = dict(os.environ, SVTAV1_HIP_ANALYSIS_FUSED="0")
    r = subprocess.run([sys.executable, os.path.join(ac.HERE, "analysis_cases.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, f"child exit status {r.returncode}\nstdout:\n{r.stdout[-3000:]}\nstderr:\n{r.stderr[-6000:]}"
    assert os.environ.get("SVTAV1_HIP_ANALYSIS_FUSED", "1") != "0", "this process must run the fused path"
    off = np.load(out)
    for l1, fp in ((1, 0), (0, 1)):
        on = ac.switch_batch_results(hip, l1, fp)
        ac.assert_equal(on, {k: off[k] for k in on}, f"switch on vs off l1={l1} fp={fp}")
        for i, c in enumerate(ac.SWITCH_BATCH):
            ac.assert_equal({k.split("_", 2)[2]: v for k, v in on.items() if k.startswith(f"{i}_")}, ac.reference(*c, l1, fp),
                            f"switch batch job {i} l1={l1} fp={fp}")
