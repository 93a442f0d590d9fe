"""GPU parity: svt_hip_intra_search_frames (the open-loop intra search of TPL level 1, include/svt_hip_intra.h) against the
reference's own functions (tests/intra_cases.py, when oracle/_ref/libsvtref.so is built) and the golden fixture recorded from them,
bit-exact: best mode and cost of every 16x16 block, every mode's cost and every prediction byte."""
import ctypes as C

import numpy as np
import pytest

import intra_cases as I
import pyorc
from arena import GUARD
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(I.GOLD)


@pytest.fixture(scope="module")
def oracle():
    return I.RefIntraSearch(pyorc.ref()) if pyorc.have_ref() else None


def setup_jobs(hip, cases):
    """(planes on the device, outputs, jobs) of ALL_CASES entries; the small cases with every mode's cost and prediction."""
    keep, jobs = [], []
    for case in cases:
        i = I.ALL_CASES.index(case)
        plane = I.case_plane(case, i)
        buf = device.DeviceBuffer(hip, plane.buf.nbytes)
        buf.upload(plane.buf)
        out = device.DeviceIntraOut(hip, plane.width, plane.height, all_modes=case in I.CASES)
        job = abi.IntraSearchJob()
        job.src, job.ctrls = plane.desc(buf.ptr), I.case_ctrls(case)
        out.fill_job(job)
        keep.append((case, plane, buf, out))
        jobs.append(job)
    return keep, jobs


def check(gold, oracle, case, plane, got):
    name = case[0]
    assert set(np.unique(got["best_mode"])) <= set(range(abi.INTRA_MODES)) | {I.NOT_SEARCHED}, name
    I.check_against_golden(gold, name, got)
    if oracle is not None:
        want = oracle.run(plane, I.case_ctrls(case), all_modes="pred" in got)
        for k, v in want.items():
            assert np.array_equal(got[k], v), (name, k, int((got[k] != v).sum()))


@pytest.mark.parametrize("case", I.CASES, ids=lambda c: c[0])
def test_intra_search_case(hip, gold, oracle, case):
    keep, jobs = setup_jobs(hip, [case])
    device.intra_search_frames(hip, jobs)
    c, plane, _, out = keep[0]
    got = out.download()
    # modes after intra_mode_end: INT64_MAX cost, prediction untouched (the 0xA5 fill)
    end = case[4]
    searched = got["best_mode"] != I.NOT_SEARCHED
    assert (got["mode_cost"][:, :, end + 1:] == I.INT64_MAX).all()
    assert (got["pred"][searched][:, end + 1:] == GUARD).all()
    assert (got["pred"][~searched] == GUARD).all()
    got["pred"][~searched] = 0  # the oracle leaves the predictions of blocks it does not search at 0
    got["pred"][:, :, end + 1:] = 0
    check(gold, oracle, case, plane, got)


def test_intra_search_pictures_of_different_sizes_in_one_call(hip, gold, oracle):
    keep, jobs = setup_jobs(hip, I.CASES)
    device.intra_search_frames(hip, jobs)
    for case, plane, _, out in keep:
        got = out.download()
        searched = got["best_mode"] != I.NOT_SEARCHED
        got["pred"][~searched] = 0
        got["pred"][:, :, case[4] + 1:] = 0
        check(gold, oracle, case, plane, got)


@pytest.mark.parametrize("case", I.BIG_CASES, ids=lambda c: c[0])
def test_intra_search_whole_picture(hip, gold, oracle, case):
    keep, jobs = setup_jobs(hip, [case])
    device.intra_search_frames(hip, jobs)
    _, plane, _, out = keep[0]
    got = out.download()
    assert (got["best_mode"] != I.NOT_SEARCHED).all()
    check(gold, oracle, case, plane, got)


def _bad_jobs():
    """(what, mutate(jobs)) of every job set the entry point must refuse before it launches anything."""
    def ctrl(field, value):
        return lambda jobs: setattr(jobs[-1].ctrls, field, value)
    return [
        ("intra_mode_end", ctrl("intra_mode_end", abi.PAETH_PRED + 1)),
        ("use_sad", ctrl("use_sad", 2)),
        ("pf_shape", ctrl("pf_shape", 3)),
        ("subsample_tx", ctrl("subsample_tx", 1)),
        ("src", lambda jobs: setattr(jobs[-1].src, "buf", None)),
        ("best_mode", lambda jobs: setattr(jobs[-1], "best_mode", None)),
        ("best_cost", lambda jobs: setattr(jobs[-1], "best_cost", None)),
        ("stride", lambda jobs: setattr(jobs[-1].src, "stride", I.PAD + ((jobs[-1].src.width + 15) & ~15) - 1)),
        ("width", lambda jobs: setattr(jobs[-1].src, "width", 0)),
    ]


@pytest.mark.parametrize("what,mutate", _bad_jobs(), ids=lambda v: v if isinstance(v, str) else "")
def test_intra_search_bad_parameter(hip, what, mutate):
    """The second of two jobs is bad: nothing is launched, neither job's outputs change."""
    keep, jobs = setup_jobs(hip, I.CASES[:2])
    mutate(jobs)
    arr = (abi.IntraSearchJob * 2)(*jobs)
    rc = hip.svt_hip_intra_search_frames(arr, 2, None)
    assert rc == abi.SVT_HIP_ERR_BAD_PARAMETER, what
    assert b"svt_hip_intra_search_frames" in hip.svt_hip_last_error()
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    for _, _, _, out in keep:
        for k, v in out.download().items():
            assert (v.view(np.uint8) == GUARD).all(), (what, k)


def test_intra_search_bad_job_array(hip):
    job = abi.IntraSearchJob()
    assert hip.svt_hip_intra_search_frames(None, 1, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert hip.svt_hip_intra_search_frames(C.byref(job), 0, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
