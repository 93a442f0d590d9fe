"""GPU parity: svt_hip_warp_batch, svt_hip_warp_error_batch and svt_hip_gm_refine (include/svt_hip_inter.h) against the golden
fixture recorded from the reference's own functions (tests/warp_cases.py) and, when oracle/_ref/libsvtref.so is built, against
those functions themselves — bit-exact: every sample of the block, every byte around it, every input buffer unchanged, every field
of the error records, the refined model."""
import ctypes as C

import numpy as np
import pytest

import blend_cases as B
import conv_cases as K
import pyorc
import warp_cases as W
from arena import GUARD, OnDevice
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
V = C.c_void_p


@pytest.fixture(scope="module")
def gold():
    return np.load(W.GOLD)


@pytest.fixture(scope="module")
def ref():
    return pyorc.ref() if pyorc.have_ref() else None


@pytest.fixture(scope="module")
def filt(hip, gold):
    """The filter table on the device, uploaded once as the encoder would."""
    d = device.DeviceBuffer(hip, abi.WARP_FILTER_BYTES)
    d.upload(gold["warped_filter"])
    return d


# ---- 1. prediction ----------------------------------------------------------------------------------------------------------
def check_warp(gold, ref, index, inp, dev):
    case = inp.case
    for b in inp.buffers():
        dev.fetch(b)
    B.check_record(gold, W.warp_record(inp), case[0])
    fresh = W.WarpInputs(case, index)
    for name in ("ref", "dst", "cbuf"):
        got, was = getattr(inp, name), getattr(fresh, name)
        if got is inp.out:
            assert got.outside_untouched(), (case[0], name, "bytes outside the block")
        else:
            assert np.array_equal(got.a, was.a), (case[0], name, "a buffer that is only read changed")
    if ref is not None:
        W.RefWarp(ref).run(fresh)
        assert np.array_equal(inp.out.a, fresh.out.a), (case[0], int((inp.out.a != fresh.out.a).sum()))


@pytest.mark.parametrize("index", range(len(W.WARP_CASES)), ids=lambda i: W.WARP_CASES[i][0])
def test_warp_case(hip, gold, ref, filt, index):
    inp = W.WarpInputs(W.WARP_CASES[index], index)
    dev = OnDevice(hip, inp.buffers())
    device.warp_batch(hip, [inp.desc(dev.ptrs)], filt.ptr)
    check_warp(gold, ref, index, inp, dev)


def test_warp_all_cases_in_one_call(hip, gold, ref, filt):
    """Mixed sizes, formats, compound modes and models in one launch, with empty descriptors in between."""
    inputs = [W.WarpInputs(c, i) for i, c in enumerate(W.WARP_CASES)]
    dev = OnDevice(hip, [b for inp in inputs for b in inp.buffers()])
    descs = []
    for i, inp in enumerate(inputs):
        descs.append(inp.desc(dev.ptrs))
        if i % 7 == 0:   # the same block again, but empty: nothing may happen
            d = inp.desc(dev.ptrs)
            d.p_width, d.p_height = (0, d.p_height) if i % 2 else (d.p_width, 0)
            descs.append(d)
    assert len(descs) > 100
    device.warp_batch(hip, descs, filt.ptr)
    for i, inp in enumerate(inputs):
        check_warp(gold, ref, i, inp, dev)


def _skipped_descs():
    """(what, index of the case it is made from, mutate(desc)): descriptors the kernel is specified to skip."""
    def field(name, value):
        return lambda d: setattr(d, name, value)
    first = {c: next(i for i, k in enumerate(W.WARP_CASES) if k[5] == c and k[4] == 0 and k[2] >= 8) for c in range(4)}
    hb = next(i for i, k in enumerate(W.WARP_CASES) if k[4] == 1 and k[5] == 2)
    return [("w == 0", first[0], field("p_width", 0)), ("h == 0", first[1], field("p_height", 0)), ("NULL ref", first[2], field("ref", None)),
            ("shear alpha", first[0], field("alpha", 16384)), ("shear beta", first[3], field("beta", -9408)),
            ("shear gamma + delta", first[1], lambda d: (setattr(d, "gamma", 8192), setattr(d, "delta", -8192))),
            ("shear -32768", hb, field("delta", -32768)), ("NULL dst", first[0], field("dst", None)), ("NULL cbuf", first[1], field("cbuf", None)),
            ("w 2", first[0], field("p_width", 2)), ("h 129", first[2], field("p_height", 129)), ("compound 4", first[3], field("compound", 4)),
            ("bit_depth 9", hb, field("bit_depth", 9)), ("10 bits in uint8", first[0], field("bit_depth", 10)), ("is_16bit 2", hb, field("is_16bit", 2)),
            ("subsampling", first[0], field("subsampling_x", 2)), ("round_0 0", first[0], field("round_0", 0)), ("rounds", first[2], field("round_1", 12)),
            ("width 0", first[0], field("width", 0)), ("height 0", first[3], field("height", 0)), ("p_col < 0", first[0], field("p_col", -8))]


def test_warp_skips_descriptors(hip, gold, ref, filt):
    """Empty, NULL, out-of-range and disallowed-shear descriptors between good ones: their dst and cbuf keep every byte, their
    neighbours are predicted."""
    bad = _skipped_descs()
    good_idx = sorted({i for _, i, _ in bad})
    good = [W.WarpInputs(W.WARP_CASES[i], i) for i in good_idx]
    victims = [W.WarpInputs(W.WARP_CASES[i], i) for _, i, _ in bad]
    dev = OnDevice(hip, [b for inp in good + victims for b in inp.buffers()])
    descs = []
    for k, ((what, _, mutate), inp) in enumerate(zip(bad, victims)):
        d = inp.desc(dev.ptrs)
        mutate(d)
        descs.append(d)
        if k < len(good):
            descs.append(good[k].desc(dev.ptrs))
    assert len(bad) >= len(good)
    device.warp_batch(hip, descs, filt.ptr)
    for (what, i, _), inp in zip(bad, victims):
        fresh = W.WarpInputs(W.WARP_CASES[i], i)
        for b, was in zip(inp.buffers(), fresh.buffers()):
            dev.fetch(b)
            assert np.array_equal(b.a, was.a), (what, "a skipped descriptor wrote")
    for i, inp in zip(good_idx, good):
        check_warp(gold, ref, i, inp, dev)


# ---- 2. interplay with the interpolation and the blends -------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(W.INTER_CASES)), ids=lambda i: W.INTER_CASES[i][0])
def test_warp_with_convolve_and_blend(hip, gold, ref, filt, index):
    case = W.INTER_CASES[index]
    name, kind, w, h, bd, is16 = case
    inp = W.InterInputs(case, index)
    px = 2 if is16 else 1
    dev = OnDevice(hip, inp.planes)
    d_dst, d_cb = device.DeviceBuffer(hip, w * h * px), [device.DeviceBuffer(hip, w * h * 2) for _ in range(2)]
    for d in [d_dst] + d_cb:
        d.fill(GUARD)

    def warp(j, cb, compound):
        p = inp.planes[j]
        d = abi.WarpDesc(dev.ptrs[id(p)] + p.byte_offset, d_dst.ptr, cb.ptr, p.stride, w, w, p.w, p.h, W.INTER_POS[0], W.INTER_POS[1], w, h,
                         (C.c_int32 * 6)(*inp.mats[j]), *inp.shears[j], 0, 0, inp.r0, inp.r1, bd, is16, compound, 0, 0)
        return device.warp_batch(hip, [d], filt.ptr)

    def conv(j, cb, compound):
        p = inp.planes[j]
        t = np.array(K.TABLES["sub_pel_filters_8"], np.int16)
        d = abi.ConvolveDesc(dev.ptrs[id(p)] + p.byte_offset + inp.conv_src_offset(p) * px, d_dst.ptr, p.stride, w, w, h, (C.c_int16 * 8)(*t[inp.phase[0]]),
                             (C.c_int16 * 8)(*t[inp.phase[1]]), 8, 8, inp.r0, inp.r1, bd, is16, compound, 0, 0, (C.c_uint8 * 3)(), cb.ptr, w, 0)
        d_desc = device.upload_descriptors(hip, [d])
        device.check(hip, hip.svt_hip_convolve_batch(V(d_desc.ptr), 1, None), "svt_hip_convolve_batch")
        device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")

    if kind == "warp_conv":
        warp(0, d_cb[0], 1), conv(1, d_cb[0], 2)
    elif kind == "conv_warp":
        conv(0, d_cb[0], 1), warp(1, d_cb[0], 2)
    else:
        warp(0, d_cb[0], 1), warp(1, d_cb[1], 1)
        assert (d_dst.download(np.uint8, (w * h * px,)) == GUARD).all()   # compound 1 leaves dst alone
        d_mask = device.DeviceBuffer(hip, w * h)
        d_mask.upload(np.load(B.GOLD)["wedge_16x16"][W.INTER_WEDGE])
        device.blend_batch(hip, [abi.BlendDesc(d_cb[0].ptr, d_cb[1].ptr, d_dst.ptr, d_mask.ptr, w, w, w, w, w, h, abi.BLEND_D16, 0, 0, 0,
                                               inp.r0, inp.r1, bd, is16, 0)])
    got = d_dst.download(np.uint16 if is16 else np.uint8, (h, w))
    assert np.array_equal(got, gold[f"inter_{name}"]), (name, int((got != gold[f"inter_{name}"]).sum()))
    if ref is not None:
        assert np.array_equal(got, W.RefInter(ref, np.load(B.GOLD)).run(W.InterInputs(case, index))), name


# ---- 3. the global-motion error -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chess", (0, 1))
@pytest.mark.parametrize("k", range(len(W.ERROR_PICTURES)), ids=lambda k: "%dx%d" % W.ERROR_PICTURES[k])
def test_warp_error_picture(hip, gold, ref, filt, k, chess):
    """More than 40 candidates in one call; thresholds from the reference's own full error of each candidate."""
    pair = W.error_pair(k)
    dev = OnDevice(hip, pair)
    best, want = gold[f"error_{k}_{chess}_best"], gold[f"error_{k}_{chess}_results"]
    cand = W.error_candidates(best)
    assert len(cand) >= 40
    job = W.error_job(*pair, chess, filt.ptr, dev.ptrs)
    ws = device.warp_error_workspace(hip, job, len(cand))
    got = device.warp_error_batch(hip, job, cand)
    for f in ("status", "error", "blocks_summed", "pad_"):
        assert np.array_equal(got[f], want[f]), (f, np.nonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))[0][:8].tolist())
    fresh = W.error_pair(k)
    for b, was in zip(pair, fresh):
        dev.fetch(b)
        assert np.array_equal(b.a, was.a), "an input picture changed"
    if ref is not None:
        orc = W.RefError(ref)
        models = [m for m in W.ERROR_MODELS for _ in W.THRESHOLDS]
        for i, m in enumerate(models):
            assert got["error"][i] == orc.error(m, W.AFFINE, *fresh, chess, int(best[i])), (i, m)
    del ws


# ---- 4. the refinement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(W.REFINE_CASES)), ids=lambda i: W.REFINE_CASES[i][0])
def test_gm_refine(hip, gold, ref, filt, index):
    case = W.REFINE_CASES[index]
    name, pair_index, wmtype, chess, best, _ = case
    pair = W.refine_pair(pair_index)
    dev = OnDevice(hip, pair)
    job = W.error_job(*pair, chess, filt.ptr, dev.ptrs)
    ws = device.warp_error_workspace(hip, job, 1)
    mat, wt, err = device.gm_refine(hip, job, W.refine_start(case), wmtype, W.N_REFINEMENTS, best)
    got = np.array(mat[:6] + [wt, err], np.int64)
    assert np.array_equal(got, gold[f"refine_{name}"]), (got.tolist(), gold[f"refine_{name}"].tolist())
    assert mat[6:] == [0, 0]
    if ref is not None:
        assert np.array_equal(got, W.ref_refine(W.RefError(ref), case))
    del ws


def test_gm_refine_of_an_invalid_model(hip, filt):
    """A start model that fails the shear check evaluates to error 1, as in the reference, and every step from it as well."""
    pair = W.refine_pair(0)
    dev = OnDevice(hip, pair)
    job = W.error_job(*pair, 0, filt.ptr, dev.ptrs)
    ws = device.warp_error_workspace(hip, job, 1)
    start = [0, 0, W.ONE + 30000, 0, 0, W.ONE + 30000, 0, 0]
    mat, wt, err = device.gm_refine(hip, job, start, W.ROTZOOM, 1, W.INT64_MAX)
    assert err == 1 and mat == start and wt == W.ROTZOOM
    del ws


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments(hip, filt):
    d = device.DeviceBuffer(hip, 4096)
    bad = abi.SVT_HIP_ERR_BAD_PARAMETER
    assert hip.svt_hip_warp_batch(None, 1, V(filt.ptr), None) == bad
    assert b"svt_hip_warp_batch" in hip.svt_hip_last_error()
    assert hip.svt_hip_warp_batch(V(d.ptr), 0, V(filt.ptr), None) == bad
    assert hip.svt_hip_warp_batch(V(d.ptr), 1, None, None) == bad
    pair = W.error_pair(1)
    dev = OnDevice(hip, pair)
    job = W.error_job(*pair, 0, filt.ptr, dev.ptrs)
    ws = device.warp_error_workspace(hip, job, 2)
    assert hip.svt_hip_warp_error_batch(C.byref(job), None, V(d.ptr), 1, None) == bad
    assert b"svt_hip_warp_error_batch" in hip.svt_hip_last_error()
    assert hip.svt_hip_warp_error_batch(C.byref(job), V(d.ptr), None, 1, None) == bad
    assert hip.svt_hip_warp_error_batch(C.byref(job), V(d.ptr), V(d.ptr), 0, None) == bad
    assert hip.svt_hip_warp_error_batch(None, V(d.ptr), V(d.ptr), 1, None) == bad
    for name, value in (("ref", None), ("cur", None), ("filter", None), ("workspace", None), ("workspace_bytes", ws.nbytes - 257), ("cur_width", 0),
                        ("ref_height", 0), ("ref_stride", pair[0].w - 1), ("chess_refn", 2)):
        j = W.error_job(*pair, 0, filt.ptr, dev.ptrs)
        j.workspace, j.workspace_bytes = ws.ptr, ws.nbytes
        setattr(j, name, value)
        assert hip.svt_hip_warp_error_batch(C.byref(j), V(d.ptr), V(d.ptr), 2, None) == bad, name
    mat, wt, err = (C.c_int32 * 8)(0, 0, W.ONE, 0, 0, W.ONE), C.c_int32(W.AFFINE), C.c_int64(0)
    assert hip.svt_hip_gm_refine(C.byref(job), None, C.byref(wt), 5, 0, C.byref(err), None) == bad
    assert b"svt_hip_gm_refine" in hip.svt_hip_last_error()
    assert hip.svt_hip_gm_refine(C.byref(job), mat, C.byref(C.c_int32(4)), 5, 0, C.byref(err), None) == bad
    assert hip.svt_hip_gm_refine(C.byref(job), mat, C.byref(wt), -1, 0, C.byref(err), None) == bad
    assert hip.svt_hip_gm_refine(C.byref(job), mat, C.byref(wt), 5, 0, None, None) == bad
