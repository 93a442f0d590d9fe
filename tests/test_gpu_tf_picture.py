"""GPU parity: svt_hip_tf_filter_picture (ME_MCTF -> sub-pel refinement -> 64/32/16 decisions -> predictions -> accumulate ->
normalise, all device-resident) against the oracle's restatement of produce_temporally_filtered_pic and against the golden
pictures the reference itself produced, bit-exact: the filtered picture, the per-block refinement state and the counters."""
import ctypes as C

import numpy as np
import pytest

import tf_picture_cases as tpc
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
GOLD = tpc.GOLD


def run_gpu(hip, pics, case, decay):
    name, kind, w, h, n_refs, bd, key, ctl = case
    dev = tpc.DevWindow(hip, pics)
    job = tpc.make_job(pics, w, h, bd, key, ctl, decay, dev.ptrs)
    states, tot = device.tf_read_back(hip, job, *device.tf_filter_picture(hip, job))
    return dev.centre_arrays(), states, tot


@pytest.mark.parametrize("case", tpc.CASES, ids=lambda c: c[0])
def test_filter_picture(hip, orc, case):
    gold = np.load(GOLD)
    name = case[0]
    decay = tuple(int(x) for x in gold[f"{name}_decay"])
    got, states, tot = run_gpu(hip, tpc.case_window(orc, case), case, decay)
    pics = tpc.case_window(orc, case)
    ostates, otot = tpc.run_oracle(orc, pics, case, decay)
    assert tot == otot == tuple(int(x) for x in gold[f"{name}_tot"])
    ost = tpc.states_to_array(ostates)
    bad = np.argwhere((ost != states).any(axis=1))
    assert len(bad) == 0, (name, "state of (ref, b64) entries", bad[:8].ravel().tolist())
    for k, v in pics[0].arrays().items():
        assert np.array_equal(got[k], v), (name, k, int((got[k] != v).sum()))
        assert np.array_equal(got[k], gold[f"{name}_{k}"]), (name, k, "golden")


def test_argument_checks(hip, orc):
    case = tpc.CASES[0]
    name, kind, w, h, n_refs, bd, key, ctl = case
    pics = tpc.case_window(orc, case)
    dev = tpc.DevWindow(hip, pics)
    job = tpc.make_job(pics, w, h, bd, key, ctl, (1, 1, 1), dev.ptrs)
    assert hip.svt_hip_tf_filter_picture(C.byref(job), None) == abi.SVT_HIP_ERR_BAD_PARAMETER  # no workspace
    ws = device.tf_workspace(hip, job)
    job.workspace, job.workspace_bytes = ws.ptr, ws.nbytes
    job.ctrls.enable_8x8_pred = 2   # a flag: 0 or 1
    assert hip.svt_hip_tf_filter_picture(C.byref(job), None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert b"8x8" in hip.svt_hip_last_error()
    # 8x8 prediction refines the ME's 8x8 vectors: the ME must store all 85 PUs of a b64
    for me16, me8 in ((1, 0), (0, 1), (0, 0)):
        job.ctrls.enable_8x8_pred, job.me.enable_me_16x16, job.me.enable_me_8x8 = 1, me16, me8
        assert hip.svt_hip_tf_filter_picture(C.byref(job), None) == abi.SVT_HIP_ERR_BAD_PARAMETER, (me16, me8)
        assert b"8x8" in hip.svt_hip_last_error()
    job.me.enable_me_16x16 = job.me.enable_me_8x8 = 1
    job.ctrls.enable_8x8_pred, job.n_refs = 0, 0
    assert hip.svt_hip_tf_filter_picture(C.byref(job), None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    job.n_refs, job.bit_depth = n_refs, 12
    assert hip.svt_hip_tf_filter_picture(C.byref(job), None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert hip.svt_hip_tf_filter_picture(None, None) == abi.SVT_HIP_ERR_BAD_PARAMETER


def test_filter_picture_4k(hip, orc):
    """BASELINE size: one 3840x2160 8-bit picture against one neighbour (tf level 6 controls, luma + chroma), GPU == oracle on
    every plane and every (b64) refinement state; and the size-independent property that a window of identical pictures
    leaves the centre picture unchanged (every prediction is the picture itself, (sum w * x + sum w / 2) / sum w == x)."""
    case = ("pan_4k", "pan", 3840, 2160, 1, 8, "m8_4k_tl2", tpc.LVL6)
    decay = (2247286, 6156426, 6156426)
    got, states, tot = run_gpu(hip, tpc.case_window(orc, case), case, decay)
    pics = tpc.case_window(orc, case)
    ostates, otot = tpc.run_oracle(orc, pics, case, decay)
    assert tot == otot
    assert np.array_equal(tpc.states_to_array(ostates), states)
    for k, v in pics[0].arrays().items():
        assert np.array_equal(got[k], v), (k, int((got[k] != v).sum()))
    # identical pictures
    same = tpc.case_window(orc, case)
    for k, v in same[1].arrays().items():
        v[...] = same[0].arrays()[k]
    d = same[1].pyr.desc()
    orc.orc_pyramid_frame(C.byref(d.full), C.byref(d.quarter), C.byref(d.sixteenth), 1)
    before = {k: v.copy() for k, v in same[0].arrays().items()}
    got, _, _ = run_gpu(hip, same, case, decay)
    for k, v in before.items():
        assert np.array_equal(got[k], v), k


@pytest.mark.parametrize("case", [
    # the m8 4K preset stores 21 PUs per b64; 8x8 prediction needs all 85 (svt_hip_tf_filter_picture refuses it otherwise)
    ("blocks_8x8_me8x8_4k", "blocks", 3840, 2160, 1, 8, "m8_4k_tl2", dict(tpc.LVL1, enable_8x8_pred=1, me=dict(enable_me_8x8=1))),
    ("fastpan_ld_4k_10bit", "fastpan", 3840, 2160, 2, 10, "m8_4k_tl2", dict(tpc.LVL8, low_delay=1, chroma=1)),
], ids=lambda c: c[0])
def test_filter_picture_variants_4k(hip, orc, case):
    """BASELINE size for the variants added in round 3: tf level 1 with 8x8 prediction (tens of thousands of 16x16 blocks split into 8x8) and
    the low-delay filter on a 10-bit picture with two neighbours — GPU == oracle on every plane and every refinement state."""
    decay = (2247286, 6156426, 6156426)
    got, states, tot = run_gpu(hip, tpc.case_window(orc, case), case, decay)
    pics = tpc.case_window(orc, case)
    ostates, otot = tpc.run_oracle(orc, pics, case, decay)
    assert tot == otot
    assert np.array_equal(tpc.states_to_array(ostates), states)
    if case[7].get("enable_8x8_pred"):
        assert sum(sum(s.split16) for s in ostates) > 1000     # the 8x8 path is what this case is about
    for k, v in pics[0].arrays().items():
        assert np.array_equal(got[k], v), (k, int((got[k] != v).sum()))
