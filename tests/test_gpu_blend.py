"""GPU parity: svt_hip_blend_batch and svt_hip_compound_mask_search_batch (include/svt_hip_inter.h) against the golden fixture
recorded from the reference's own functions (tests/blend_cases.py) and, when oracle/_ref/libsvtref.so is built, against those
functions themselves — bit-exact: every sample of dst, every byte around the block, every field of the search record."""
import ctypes as C

import numpy as np
import pytest

import blend_cases as B
import conv_cases as K
import pyorc
from arena import GUARD, OnDevice
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
V = C.c_void_p


@pytest.fixture(scope="module")
def gold():
    return np.load(B.GOLD)


@pytest.fixture(scope="module")
def ref():
    return pyorc.ref() if pyorc.have_ref() else None


@pytest.fixture(scope="module")
def wedge_dev(hip, gold):
    """The wedge masks of the nine sizes on the device, uploaded once as the encoder would: ({(w, h): address}, keep-alive)."""
    bufs = {}
    for (w, h) in B.WEDGE_BSIZE:
        bufs[(w, h)] = device.DeviceBuffer(hip, 32 * w * h)
        bufs[(w, h)].upload(gold[f"wedge_{w}x{h}"])
    return {k: b.ptr for k, b in bufs.items()}, bufs


def on_device(hip, inputs):
    """Device copies of the host buffers of a list of inputs"""
    return OnDevice(hip, [b for inp in inputs for b in inp.buffers()])


# ---- 1. blends --------------------------------------------------------------------------------------------------------------
def check_blend(gold, ref, index, inp, dev):
    """inp's buffers after the GPU blend against the fixture, the bytes around every block, and the reference."""
    case = inp.case
    for b in inp.buffers():
        dev.fetch(b)
    B.check_record(gold, B.blend_record(case[0], inp), case[0])
    fresh = B.BlendInputs(case, index, gold)
    for name in ("src0", "src1", "dst", "mask"):
        got, was = getattr(inp, name), getattr(fresh, name)
        assert got.outside_untouched(), (case[0], name, "bytes outside the block")
        written = name == "dst" or (name == "src0" and inp.inplace) or (name == "mask" and case[1] == abi.BLEND_D16_DIFFWTD)
        assert written or np.array_equal(got.a, was.a), (case[0], name, "an input changed")
    if ref is not None:
        B.RefBlend(ref).run(fresh)
        assert np.array_equal(inp.dst.a, fresh.dst.a), (case[0], int((inp.dst.a != fresh.dst.a).sum()))
        assert np.array_equal(inp.mask.a, fresh.mask.a), (case[0], "mask")


@pytest.mark.parametrize("index", range(len(B.BLEND_CASES)), ids=lambda i: B.BLEND_CASES[i][0])
def test_blend_case(hip, gold, ref, index):
    inp = B.BlendInputs(B.BLEND_CASES[index], index, gold)
    dev = on_device(hip, [inp])
    device.blend_batch(hip, [inp.desc(dev.ptrs)])
    check_blend(gold, ref, index, inp, dev)


def test_blend_all_cases_in_one_call(hip, gold, ref):
    """Mixed kinds, sizes and formats in one launch, with empty descriptors (w == 0 / h == 0) in between."""
    inputs = [B.BlendInputs(c, i, gold) for i, c in enumerate(B.BLEND_CASES)]
    dev = on_device(hip, inputs)
    descs = []
    for i, inp in enumerate(inputs):
        descs.append(inp.desc(dev.ptrs))
        if i % 7 == 0:   # the same block again, but empty: nothing may happen
            d = inp.desc(dev.ptrs)
            d.w, d.h = (0, d.h) if i % 2 else (d.w, 0)
            descs.append(d)
    assert len(descs) > 100
    device.blend_batch(hip, descs)
    for i, inp in enumerate(inputs):
        check_blend(gold, ref, i, inp, dev)


# ---- 2. search --------------------------------------------------------------------------------------------------------------
def check_search(gold, ref, indices, got):
    want = gold["search_results"][indices]
    assert (got["status"] == 0).all()
    for f in B.RESULT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (f, [B.SEARCH_CASES[i][0] for i in np.array(indices)[np.nonzero(got[f] != want[f])[0]]][:5])
    if ref is not None:
        orc = B.RefSearch(ref, gold)
        for k, i in enumerate(indices):
            r = orc.run_inputs(B.SearchInputs(B.SEARCH_CASES[i], i))
            assert got[k].tobytes() == r.tobytes(), B.SEARCH_CASES[i][0]


@pytest.mark.parametrize("index", range(len(B.SEARCH_CASES)), ids=lambda i: B.SEARCH_CASES[i][0])
def test_search_case(hip, gold, ref, wedge_dev, index):
    inp = B.SearchInputs(B.SEARCH_CASES[index], index)
    dev = on_device(hip, [inp])
    got = device.compound_mask_search_batch(hip, [inp.desc(wedge_dev[0], dev.ptrs)])
    check_search(gold, ref, [index], got)


def test_search_all_cases_in_one_call(hip, gold, ref, wedge_dev):
    inputs = [B.SearchInputs(c, i) for i, c in enumerate(B.SEARCH_CASES)]
    dev = on_device(hip, inputs)
    got = device.compound_mask_search_batch(hip, [inp.desc(wedge_dev[0], dev.ptrs) for inp in inputs])
    check_search(gold, ref, list(range(len(inputs))), got)


# ---- 3. the pipeline --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(B.PIPE_CASES)), ids=lambda i: B.PIPE_CASES[i][0])
def test_convolve_then_masked_compound(hip, gold, ref, wedge_dev, index):
    """svt_hip_convolve_batch compound-1 descriptors for both references of Y, U and V, then the masked compound: luma in one
    call (building the mask of a difference-weighted compound), the chroma planes reading that mask in the next."""
    case = B.PIPE_CASES[index]
    name, w, h, bd, is16, ctype, widx, wsign, mask_type = case
    inp = B.PipeInputs(case, index)
    r0, r1 = K.conv_rounds_compound(bd)
    px = 2 if is16 else 1
    keep, conv, planes = [], [], []
    scrap = device.DeviceBuffer(hip, w * h * px)   # dst of a compound-1 descriptor: not written
    for pw, ph, refs, phases in inp.planes:
        cbs = []
        for j in range(2):
            d_ref, d_cb = device.DeviceBuffer(hip, refs[j].nbytes), device.DeviceBuffer(hip, pw * ph * 2)
            d_ref.upload(refs[j])
            d_cb.fill(GUARD)
            sx, sy, ti = phases[j]
            t = np.array(K.TABLES[B.PIPE_TABLES[ti]], np.int16)
            conv.append(abi.ConvolveDesc(d_ref.ptr + (8 * refs[j].shape[1] + 8) * px, scrap.ptr, refs[j].shape[1], pw, pw, ph,
                                         (C.c_int16 * 8)(*t[sx]), (C.c_int16 * 8)(*t[sy]), 8, 8, r0, r1, bd, is16, 1, 0, 0,
                                         (C.c_uint8 * 3)(), d_cb.ptr, pw, 0))
            keep += [d_ref, d_cb]
            cbs.append(d_cb)
        d_dst = device.DeviceBuffer(hip, pw * ph * px)
        d_dst.fill(GUARD)
        planes.append((pw, ph, cbs, d_dst))
    d_conv = device.upload_descriptors(hip, conv)
    device.check(hip, hip.svt_hip_convolve_batch(V(d_conv.ptr), len(conv), None), "svt_hip_convolve_batch")
    d_mask = device.DeviceBuffer(hip, w * h)
    d_mask.fill(GUARD)
    if ctype == B.COMPOUND_WEDGE:
        mask_ptr, kind = wedge_dev[0][(w, h)] + (2 * widx + wsign) * w * h, abi.BLEND_D16
    else:
        mask_ptr, kind = d_mask.ptr, abi.BLEND_D16_DIFFWTD

    def blend(plane, kind, sub):
        pw, ph, cbs, d_dst = planes[plane]
        return abi.BlendDesc(cbs[0].ptr, cbs[1].ptr, d_dst.ptr, mask_ptr, pw, pw, pw, w, pw, ph, kind, sub, sub,
                             mask_type if kind == abi.BLEND_D16_DIFFWTD else 0, r0, r1, bd, is16, 0)
    luma_descs = device.blend_batch(hip, [blend(0, kind, 0)], sync=False)   # kept until the next call has synchronised
    device.blend_batch(hip, [blend(1, abi.BLEND_D16, 1), blend(2, abi.BLEND_D16, 1)])
    dt = np.uint16 if is16 else np.uint8
    got = {k: planes[i][3].download(dt, (planes[i][1], planes[i][0])) for i, k in enumerate("yuv")}
    if ctype == B.COMPOUND_DIFFWTD:
        got["mask"] = d_mask.download(np.uint8, (h, w))
    else:
        assert (d_mask.download(np.uint8, (h, w)) == GUARD).all()
    wants = [{k: gold[f"pipe_{name}_{k}"] for k in got}] + ([B.RefPipe(ref).run(inp)] if ref is not None else [])
    for want in wants:
        assert set(want) == set(got)
        for k in got:
            assert np.array_equal(got[k], want[k]), (name, k, int((got[k] != want[k]).sum()))


# ---- 4. refusals and skipped descriptors ------------------------------------------------------------------------------------
def test_bad_arguments(hip):
    d = device.DeviceBuffer(hip, 4096)
    assert hip.svt_hip_blend_batch(None, 1, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert b"svt_hip_blend_batch" in hip.svt_hip_last_error()
    assert hip.svt_hip_blend_batch(V(d.ptr), 0, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert hip.svt_hip_compound_mask_search_batch(None, V(d.ptr), 1, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert b"svt_hip_compound_mask_search_batch" in hip.svt_hip_last_error()
    assert hip.svt_hip_compound_mask_search_batch(V(d.ptr), None, 1, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert hip.svt_hip_compound_mask_search_batch(V(d.ptr), V(d.ptr), 0, None) == abi.SVT_HIP_ERR_BAD_PARAMETER


def _bad_blend_descs():
    """(what, index of the case it is made from, mutate(desc)): descriptors the kernel is specified to skip."""
    def field(name, value):
        return lambda d: setattr(d, name, value)
    first = {kind: next(i for i, c in enumerate(B.BLEND_CASES) if c[1] == kind and c[2] >= 8 and c[3] >= 8) for kind in range(5)}
    d16, dw, mk, vm, hm = (first[k] for k in range(5))
    assert not B.BLEND_CASES[d16][5]
    return [("kind", d16, field("kind", 5)), ("kind 255", mk, field("kind", 255)), ("subw", d16, field("subw", 2)), ("subh", mk, field("subh", 2)),
            ("w", mk, field("w", 129)), ("h", d16, field("h", 200)), ("src0", d16, field("src0", None)), ("src1", mk, field("src1", None)),
            ("mask", vm, field("mask", None)), ("bit_depth", mk, field("bit_depth", 9)), ("is_16bit", hm, field("is_16bit", 2)),
            ("10 bits in uint8", d16, field("bit_depth", 10)),
            ("d16 w < 4", d16, field("w", 2)), ("d16 h < 4", dw, field("h", 3)), ("mask_type", dw, field("mask_type", 2)),
            ("mask_type of a plain blend", mk, field("mask_type", 1)), ("rounds", d16, field("round_0", 12)),
            ("subw of a vmask", vm, field("subw", 1)), ("subh of a diffwtd", dw, field("subh", 1))]


def test_blend_skips_out_of_range_descriptors(hip, gold, ref):
    """Out-of-range descriptors between good ones: their dst (and mask) keep every byte, their neighbours are blended."""
    bad = _bad_blend_descs()
    good_idx = sorted({i for _, i, _ in bad})
    good = [B.BlendInputs(B.BLEND_CASES[i], i, gold) for i in good_idx]
    victims = [B.BlendInputs(B.BLEND_CASES[i], i, gold) for _, i, _ in bad]
    dev = on_device(hip, good + victims)
    descs = []
    for k, ((what, _, mutate), inp) in enumerate(zip(bad, victims)):
        d = inp.desc(dev.ptrs)
        mutate(d)
        descs.append(d)
        if k < len(good):
            descs.append(good[k].desc(dev.ptrs))
    assert len(bad) >= len(good)
    d_null = victims[0].desc(dev.ptrs)
    d_null.dst = None
    descs.append(d_null)
    device.blend_batch(hip, descs)
    for (what, i, _), inp in zip(bad, victims):
        fresh = B.BlendInputs(B.BLEND_CASES[i], i, gold)
        for b, was in zip(inp.buffers(), fresh.buffers()):
            dev.fetch(b)
            assert np.array_equal(b.a, was.a), (what, "a skipped descriptor wrote")
    for i, inp in zip(good_idx, good):
        check_blend(gold, ref, i, inp, dev)


def test_search_skips_out_of_range_descriptors(hip, gold, ref, wedge_dev):
    idx = [0, 1, 2, 3, 4]
    inputs = [B.SearchInputs(B.SEARCH_CASES[i], i) for i in idx]
    big = next(i for i, c in enumerate(B.SEARCH_CASES) if (c[1], c[2]) == (64, 64))
    inputs.append(B.SearchInputs(B.SEARCH_CASES[big], big))
    dev = on_device(hip, inputs)
    descs = [inp.desc(wedge_dev[0], dev.ptrs) for inp in inputs]
    bad = []
    for what, k, name, value, status in (("w", 0, "w", 12, 2), ("h", 1, "h", 256, 2), ("src", 2, "src", None, 2), ("pred1", 3, "pred1", None, 2),
                                         ("bit_depth", 4, "bit_depth", 9, 2), ("is_16bit", 0, "is_16bit", 2, 2), ("w == 0", 1, "w", 0, 2),
                                         ("wedges for 64x64", 5, "wedge_masks", wedge_dev[0][(32, 32)], 1)):
        d = inputs[k].desc(wedge_dev[0], dev.ptrs)
        setattr(d, name, value)
        bad.append((what, d, status))
    mixed, where = [], {}
    for k, d in enumerate(descs):
        mixed.append(d)
        where[("good", k)] = len(mixed) - 1
        for what, b, status in bad[k::len(descs)]:
            mixed.append(b)
            where[what] = len(mixed) - 1
    got = device.compound_mask_search_batch(hip, mixed)
    for what, _, status in bad:
        r = got[where[what]]
        assert r["status"] == status, what
        r = r.copy()
        r["status"] = 0
        assert r.tobytes() == bytes(B.RESULT_DTYPE.itemsize), (what, "result not zeroed")
    check_search(gold, ref, idx + [big], got[[where[("good", k)] for k in range(len(descs))]])


# ---- 5. a whole picture -----------------------------------------------------------------------------------------------------
def test_search_whole_picture(hip, gold, ref, wedge_dev):
    """Every 16x16 block of a 1080p picture in one launch."""
    planes = B.picture_planes()
    devs = []
    for p in planes:
        d = device.DeviceBuffer(hip, p.nbytes)
        d.upload(p)
        devs.append(d)
    stride = planes[0].shape[1]
    descs = [abi.MaskSearchDesc(*(d.ptr + y * stride + x for d in devs), wedge_dev[0][(16, 16)], stride, stride, stride, 16, 16, 8, 0)
             for x, y in B.picture_blocks()]
    got = device.compound_mask_search_batch(hip, descs)
    assert (got["status"] == 0).all()
    assert np.array_equal(np.stack([got["best_wedge_index"], got["best_wedge_sign"], got["best_diffwtd_type"].astype(np.int8)]), gold["picture_best"])
    assert B.digest(got) == str(gold["picture_sha256"])
    if ref is not None:
        want = B.picture_oracle(B.RefSearch(ref, gold), planes)
        for f in B.RESULT_DTYPE.names:
            assert np.array_equal(got[f], want[f]), f
