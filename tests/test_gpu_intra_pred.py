"""GPU parity: svt_hip_intra_predict_batch (with its inter-intra epilogue) and svt_hip_cfl_predict_batch (include/svt_hip_intra.h)
against the golden fixture recorded from the reference's own functions (tests/intra_pred_cases.py) and, when
oracle/_ref/libsvtref.so is built, against those functions themselves — bit-exact: every sample of dst and every byte around it."""
import ctypes as C

import numpy as np
import pytest

import blend_cases as B
import intra_pred_cases as P
import pyorc
from arena import GUARD
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
V = C.c_void_p


@pytest.fixture(scope="module")
def gold():
    return np.load(P.GOLD)


@pytest.fixture(scope="module")
def orc():
    return P.RefIntraPred(pyorc.ref()) if pyorc.have_ref() else None


def on_device(hip, host):
    d = device.DeviceBuffer(hip, host.nbytes)
    d.upload(host)
    return d


def filled(hip, nbytes):
    d = device.DeviceBuffer(hip, nbytes)
    d.fill(GUARD)
    return d


def run_batch(hip, batch, order=None, waves=None):
    """The output buffer of a PredBatch after one call over its descriptors (in `order`)."""
    d_in, d_out = on_device(hip, batch.arena.build()), filled(hip, batch.out.nbytes())
    descs = batch.descs(d_in.ptr, d_out.ptr)
    device.intra_predict_batch(hip, descs if order is None else descs[order], waves_per_workgroup=waves)
    return d_out.download(np.uint8, (batch.out.nbytes(),))


@pytest.fixture(scope="module")
def whole(hip):
    """The whole case list in one call: (batch, raw output buffer, blocks)."""
    batch = P.PredBatch(P.CASES)
    raw = run_batch(hip, batch)
    return batch, raw, batch.blocks(raw)


@pytest.fixture(scope="module")
def live(orc):
    """The live composition's block of every case, computed once."""
    return [orc.predict(c, *P.case_inputs(c)) for c in P.CASES] if orc is not None else None


def first_difference(cases, got, want):
    for c, g, w in zip(cases, got, want):
        if not np.array_equal(g, w):
            return c, int((g != w).sum()), g.tolist()[:2], w.tolist()[:2]
    return None


# ---- 1. the case list -----------------------------------------------------------------------------------------------------
def test_whole_case_list_in_one_call(gold, live, whole):
    """Mixed sizes, modes and bit depths in one launch: the golden digests, the reference itself, and not a byte outside the blocks."""
    batch, raw, blocks = whole
    cases = P.CASES
    assert len({(c.w, c.h) for c in cases}) == 19 and len({(c.bd, c.is16) for c in cases}) == 4
    assert sum((a.w, a.h, a.is16) != (b.w, b.h, b.is16) for a, b in zip(cases, cases[1:])) > 3000   # neighbours in the list differ
    if live is not None:
        assert first_difference(cases, blocks, live) is None
    P.check_against_golden(gold, blocks)
    assert batch.out.untouched_outside(raw)


def test_shuffled_order_gives_the_same_bytes(hip, whole):
    batch, raw, _ = whole
    order = np.random.default_rng(5).permutation(len(P.CASES))
    assert np.array_equal(run_batch(hip, batch, order), raw)


@pytest.mark.parametrize("waves", [1, 2])
def test_packing_does_not_change_the_result(hip, whole, waves):
    """svt_hip_intra_predict_batch_packed with one and two descriptors per workgroup."""
    batch, raw, _ = whole
    assert np.array_equal(run_batch(hip, batch, waves=waves), raw)


# ---- 2. edges straight from a plane -----------------------------------------------------------------------------------------
def plane_cases():
    out, k = [], 0
    for w, h in ((4, 4), (8, 8), (16, 4), (4, 16), (32, 32), (16, 64), (64, 64)):
        for mode, delta in ((abi.DC_PRED, 0), (abi.H_PRED, 0), (abi.D45_PRED, -2), (abi.D135_PRED, 1), (abi.D203_PRED, 3), (abi.D157_PRED, -3),
                            (abi.SMOOTH_PRED, 0), (abi.PAETH_PRED, 0)):
            is16 = int(k % 3 != 0)
            out.append(P.Case("plane", w, h, mode, delta, 5, 0, k & 1, w, w, h, h, 10 if is16 else 8, is16, 0, k, -1, 0))
            k += 1
    return out


def test_edges_read_straight_from_a_plane(hip, orc):
    """above / left point into a padded reconstructed plane (left_stride = the plane's stride); the same blocks fed from neighbour arrays
    give the same samples."""
    cases = plane_cases()
    stride, rows = 200, 200
    rng = np.random.default_rng(77)
    planes = {is16: rng.integers(0, 1024 if is16 else 256, (rows, stride)).astype(P.sample_type(is16)) for is16 in (0, 1)}
    d_planes = {k: on_device(hip, p) for k, p in planes.items()}
    arena, out_a, out_b = P.input_arena(), P.OutLayout(), P.OutLayout()
    rel, inputs = [], []
    for k, c in enumerate(cases):
        x, y, size, p = 5 + 3 * (k % 7), 3 + 2 * (k % 11), 2 if c.is16 else 1, planes[c.is16]
        above, left = np.zeros(P.EDGE_LEN, p.dtype), np.zeros(P.EDGE_LEN, p.dtype)
        above[P.ORG - 1:P.ORG + 2 * c.w] = p[y - 1, x - 1:x + 2 * c.w]
        left[P.ORG:P.ORG + 2 * c.h] = p[y:y + 2 * c.h, x - 1]
        inputs.append((above, left))
        rel.append((((y - 1) * stride + x) * size, (y * stride + x - 1) * size,
                    arena.add(f"above {k}", above, **P.PACKED) + P.ORG * size, arena.add(f"left {k}", left, **P.PACKED) + P.ORG * size,
                    out_a.add(c.w, c.h, size, 3)[0], out_b.add(c.w, c.h, size, 3)[0]))
    d_in, d_a, d_b = on_device(hip, arena.build()), filled(hip, out_a.nbytes()), filled(hip, out_b.nbytes())
    descs = np.zeros(2 * len(cases), P.DESC_DTYPE)
    for k, (c, (pa, pl, aa, al, oa, ob)) in enumerate(zip(cases, rel)):
        descs[2 * k] = P.pred_desc(c, d_planes[c.is16].ptr + pa, d_planes[c.is16].ptr + pl, d_a.ptr + oa, c.w + 3, stride)
        descs[2 * k + 1] = P.pred_desc(c, d_in.ptr + aa, d_in.ptr + al, d_b.ptr + ob, c.w + 3, 1)
    device.intra_predict_batch(hip, descs)
    raw_a, raw_b = d_a.download(np.uint8, (out_a.nbytes(),)), d_b.download(np.uint8, (out_b.nbytes(),))
    assert np.array_equal(raw_a, raw_b) and out_a.untouched_outside(raw_a)
    blocks = [out_a.read(raw_a, k) for k in range(len(cases))]
    assert len({b.tobytes() for b in blocks}) > len(cases) // 2
    if orc is not None:
        assert first_difference(cases, blocks, [orc.predict(c, a, l) for c, (a, l) in zip(cases, inputs)]) is None


# ---- 3. unaligned dst ---------------------------------------------------------------------------------------------------------
def test_unaligned_dst(hip, whole):
    """Odd addresses and odd strides: the same samples as in the aligned run, guard bytes around every block untouched."""
    _, _, blocks = whole
    picked = [i for i, c in enumerate(P.CASES) if c.group in ("cross", "filter_intra", "inter_intra") and
              (c.w, c.h) in ((4, 4), (4, 16), (16, 4), (64, 64)) and (c.group != "cross" or (c.mode, c.delta) in
                                                                      ((0, 0), (1, 0), (3, 0), (4, -3), (7, 2), (9, 0), (12, 0)))]
    assert len(picked) > 60 and {P.CASES[i].is16 for i in picked} == {0, 1}
    batch = P.PredBatch([P.CASES[i] for i in picked], layout=lambda k: ((1, 3, 5, 7)[k % 4], (1, 3, 1, 5)[(k // 4) % 4]))
    assert all(off % 2 == 1 for (off, _, _, _, size) in batch.out.blocks if size == 1)
    assert all(off % 4 == 2 for (off, _, _, _, size) in batch.out.blocks if size == 2)
    raw = run_batch(hip, batch)
    assert first_difference(batch.cases, batch.blocks(raw), [blocks[i] for i in picked]) is None
    assert batch.out.untouched_outside(raw)


# ---- 4. a large batch -----------------------------------------------------------------------------------------------------------
def test_large_batch(hip, whole):
    """300 000 copies of a handful of 4 x 4 and 8 x 8 descriptors in one call (more than 65 535 workgroups, a tail that does not fill
    the last workgroup), every output checked."""
    _, _, blocks = whole
    want = [(i, c) for i, c in enumerate(P.CASES) if c.group == "cross" and (c.w, c.h) in ((4, 4), (8, 8)) and
            (c.mode, c.delta, c.is16) in ((0, 0, 0), (3, 1, 0), (12, 0, 1), (5, -2, 0), (9, 0, 1))]
    picked = [next(i for i, c in want if (c.w, c.h) == s and c.mode == m) for s, m in (((4, 4), 0), ((8, 8), 3), ((4, 4), 12), ((8, 8), 5), ((4, 4), 9))]
    n, slot = 300001, 128
    batch = P.PredBatch([P.CASES[i] for i in picked])
    d_in, d_out = on_device(hip, batch.arena.build()), filled(hip, n * slot)
    base = batch.descs(d_in.ptr, 0)
    descs = base[np.arange(n) % len(picked)]
    descs["dst"] = d_out.ptr + np.arange(n, dtype=np.uint64) * slot
    descs["dst_stride"] = descs["w"]
    device.intra_predict_batch(hip, descs)
    raw = d_out.download(np.uint8, (n, slot))
    for j, i in enumerate(picked):
        expect = np.full(slot, GUARD, np.uint8)
        expect[:blocks[i].nbytes] = blocks[i].view(np.uint8).reshape(-1)
        assert (raw[j::len(picked)] == expect).all(), (j, P.CASES[i])


# ---- 5. refusals and skipped descriptors ---------------------------------------------------------------------------------------
def test_host_argument_checks(hip):
    d = filled(hip, 4096)
    for call in (lambda: hip.svt_hip_intra_predict_batch(None, 1, None), lambda: hip.svt_hip_intra_predict_batch(V(d.ptr), 0, None),
                 lambda: hip.svt_hip_intra_predict_batch_packed(V(d.ptr), 1, 3, None), lambda: hip.svt_hip_intra_predict_batch_packed(None, 1, 4, None)):
        assert call() == abi.SVT_HIP_ERR_BAD_PARAMETER
        assert b"svt_hip_intra_predict_batch" in hip.svt_hip_last_error()
    assert hip.svt_hip_cfl_predict_batch(None, 1, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    assert b"svt_hip_cfl_predict_batch" in hip.svt_hip_last_error()
    assert hip.svt_hip_cfl_predict_batch(V(d.ptr), 0, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
    device.check(hip, hip.svt_hip_stream_sync(None), "sync")
    assert (d.download(np.uint8, (4096,)) == GUARD).all()   # nothing was launched over the "descriptors"


INVALID = [("shape 12 x 8", "dr", {"w": 12}), ("shape 64 x 8", "dr", {"w": 64}), ("shape 8 x 2", "dr", {"h": 2}), ("mode 13", "dr", {"mode": 13}),
           ("delta on DC", "dc", {"angle_delta": 1}), ("delta 4", "dr", {"angle_delta": 4}), ("delta -4", "dr", {"angle_delta": -4}),
           ("filter-intra 64 wide", "dc64", {"filter_intra_mode": 0}), ("filter-intra on D45", "dr", {"filter_intra_mode": 1}),
           ("filter-intra mode 6", "dc", {"filter_intra_mode": 6}), ("n_top_px", "dr", {"n_top_px": 9}), ("n_left_px", "dr", {"n_left_px": 9}),
           ("n_topright_px", "dr", {"n_topright_px": 9}), ("n_bottomleft_px", "dr", {"n_bottomleft_px": 9}),
           ("top-right without the whole top", "dr", {"n_top_px": 4}), ("bottom-left without the whole left", "dr", {"n_left_px": 4}),
           ("bit depth 9", "dr", {"bit_depth": 9}), ("10 bits in uint8", "dr", {"bit_depth": 10}), ("is_16bit 2", "dr", {"is_16bit": 2}),
           ("filt_type 2", "dr", {"filt_type": 2}), ("NULL dst", "dr", {"dst": 0}), ("NULL above", "dr", {"above": 0}), ("NULL left", "dr", {"left": 0})]


def test_invalid_descriptors_are_skipped(hip, whole):
    """One invalid descriptor per field that can be invalid, between two valid ones: it leaves dst at its fill, both neighbours are
    computed."""
    _, _, blocks = whole
    find = lambda w, mode: next(i for i, c in enumerate(P.CASES) if c.group == "cross" and (c.w, c.h, c.mode, c.delta, c.is16) == (w, w, mode, 0, 0))  # noqa: E731
    base = {"dr": find(8, abi.D45_PRED), "dc": find(8, abi.DC_PRED), "dc64": find(64, abi.DC_PRED)}
    idx = []
    for _, which, _ in INVALID:
        idx += [base["dr"], base[which], base["dc"]]
    batch = P.PredBatch([P.CASES[i] for i in idx], layout=lambda k: (0, 0))
    d_in, d_out = on_device(hip, batch.arena.build()), filled(hip, batch.out.nbytes())
    descs = batch.descs(d_in.ptr, d_out.ptr)
    for k, (what, _, change) in enumerate(INVALID):
        for name, value in change.items():
            descs[name][3 * k + 1] = value
    device.intra_predict_batch(hip, descs)
    got = batch.blocks(d_out.download(np.uint8, (batch.out.nbytes(),)))
    for k, (what, which, change) in enumerate(INVALID):
        assert np.array_equal(got[3 * k], blocks[base["dr"]]) and np.array_equal(got[3 * k + 2], blocks[base["dc"]]), (what, "a neighbour")
        assert (got[3 * k + 1] == GUARD).all(), (what, "was not skipped")


# ---- 6. inter-intra ---------------------------------------------------------------------------------------------------------------
def test_smooth_interintra_epilogue(gold, live, whole):
    """The epilogue against svt_aom_combine_interintra[_highbd]: the fixture keeps this group in full."""
    _, _, blocks = whole
    n = 0
    for i, c in enumerate(P.CASES):
        if c.group == "inter_intra":
            assert np.array_equal(blocks[i], gold[f"full_{i}"]), c
            assert live is None or np.array_equal(blocks[i], live[i]), c
            n += 1
    assert n == 4 * 14 * 2 + 1


@pytest.mark.parametrize("w, h, bd, is16", [(16, 16, 8, 0), (8, 16, 10, 1), (32, 32, 10, 1), (32, 8, 8, 0)])
def test_wedge_interintra_through_the_blend(hip, orc, w, h, bd, is16):
    """The wedge form needs no code of its own: a plain prediction, then SVT_HIP_BLEND_MASK in a second call on the same stream."""
    c = P.Case("wedge", w, h, abi.SMOOTH_PRED, 0, 5, 0, 0, w, 0, h, 0, bd, is16, 0, 555 + w + h, 2, 0)
    above, left, inter = P.case_inputs(c)
    plain = c._replace(ii_mode=-1)
    batch = P.PredBatch([plain], layout=lambda k: (0, 0))
    d_in, d_intra = on_device(hip, batch.arena.build()), filled(hip, batch.out.nbytes())
    keep = device.intra_predict_batch(hip, batch.descs(d_in.ptr, d_intra.ptr), sync=False)
    wedge_index, wedge_sign = 5, 1
    mask = np.load(B.GOLD)[f"wedge_{w}x{h}"][2 * wedge_index + wedge_sign]
    d_mask, d_inter, d_dst = on_device(hip, mask), on_device(hip, inter), filled(hip, inter.nbytes)
    off = batch.out.blocks[0][0]
    device.blend_batch(hip, [abi.BlendDesc(d_intra.ptr + off, d_inter.ptr, d_dst.ptr, d_mask.ptr, w, w, w, w, w, h, abi.BLEND_MASK, 0, 0, 0, 0, 0,
                                           bd, is16, 0)])
    del keep
    got = d_dst.download(inter.dtype, (h, w))
    intra = batch.blocks(d_intra.download(np.uint8, (batch.out.nbytes(),)))[0].astype(np.int64)
    m = mask.reshape(h, w).astype(np.int64)
    assert np.array_equal(got, (m * intra + (64 - m) * inter + 32) >> 6)   # AOM_BLEND_A64
    if orc is not None:
        pyorc.ref().svt_av1_init_wedge_masks()
        ref_intra, out = orc.intra(plain, above, left), np.zeros_like(inter)
        assert np.array_equal(intra, ref_intra)
        bs = P.BSIZE[(w, h)]
        args = (2, 1, wedge_index, wedge_sign, bs, bs, out.ctypes.data, w, inter.ctypes.data, w, ref_intra.ctypes.data, w)
        orc.ii_high(*args, bd) if is16 else orc.ii(*args)
        assert np.array_equal(got, out)


# ---- 7. CfL ---------------------------------------------------------------------------------------------------------------------
def test_cfl_cases(hip, gold, orc):
    """Prediction and ac_out of every CfL case in one call (test_cfl_alpha_search runs without ac_out)."""
    arena, out = P.input_arena(), P.OutLayout()
    rel = []
    for k, c in enumerate(P.CFL_CASES):
        luma, pred = P.cfl_inputs(c)
        size, extra = 2 if c.is16 else 1, (0, 2, 8, 5)[k % 4]
        lp = np.full((2 * c.h, 2 * c.w + extra), 0, luma.dtype)
        lp[:, :2 * c.w] = luma
        rel.append((arena.add(f"luma {k}", lp, **P.PACKED), 2 * c.w + extra, arena.add(f"pred {k}", pred, **P.PACKED), out.add(c.w, c.h, size, extra)[0], c.w + extra,
                    out.add(abi.CFL_BUF_LINE, c.h, 2)[0]))
    d_in, d_out = on_device(hip, arena.build()), filled(hip, out.nbytes())
    descs = np.zeros(len(rel), P.CFL_DESC_DTYPE)
    for k, (c, (lu, ls, pr, ds, dstride, ac)) in enumerate(zip(P.CFL_CASES, rel)):
        descs[k] = P.cfl_desc(c, d_in.ptr + lu, d_in.ptr + pr, d_out.ptr + ds, d_out.ptr + ac, ls, c.w, dstride)
    device.cfl_predict_batch(hip, descs)
    raw = d_out.download(np.uint8, (out.nbytes(),))
    got = [(out.read(raw, 2 * k), out.read(raw, 2 * k + 1).view(np.int16)) for k in range(len(P.CFL_CASES))]
    assert P.digest(d for d, _ in got) == str(gold["sha256_cfl_dst"]) and P.digest(a for _, a in got) == str(gold["sha256_cfl_ac"])
    assert out.untouched_outside(raw)
    if orc is not None:
        for c, (dst, ac) in zip(P.CFL_CASES, got):
            want_dst, want_ac = orc.cfl(c, *P.cfl_inputs(c))
            assert np.array_equal(dst, want_dst), c
            assert np.array_equal(ac, want_ac), (c, "ac_out")


def test_cfl_alpha_search(hip, gold, orc):
    """33 descriptors over one luma block, alpha -16 .. 16, in one call."""
    c = P.ALPHA_SEARCH
    luma, pred = P.cfl_inputs(c)
    d_luma, d_pred, d_out = on_device(hip, luma), on_device(hip, pred), filled(hip, 33 * pred.nbytes)
    descs = np.zeros(33, P.CFL_DESC_DTYPE)
    for k, a in enumerate(range(-16, 17)):
        descs[k] = P.cfl_desc(c._replace(alpha=a), d_luma.ptr, d_pred.ptr, d_out.ptr + k * pred.nbytes, 0, 2 * c.w, c.w, c.w)
    device.cfl_predict_batch(hip, descs)
    got = d_out.download(pred.dtype, (33, c.h, c.w))
    assert np.array_equal(got, gold["cfl_alpha_search"])
    assert np.array_equal(got[16], pred) and len({g.tobytes() for g in got}) > 20
    if orc is not None:
        assert np.array_equal(got, P.alpha_search_outputs(orc))


def test_cfl_invalid_descriptors_are_skipped(hip, gold):
    c = P.ALPHA_SEARCH._replace(alpha=5)
    luma, pred = P.cfl_inputs(c)
    bad = [{"w": 64}, {"h": 12}, {"alpha_q3": 17}, {"alpha_q3": -17}, {"bit_depth": 9}, {"is_16bit": 2}, {"luma": 0}, {"pred": 0}]
    d_luma, d_pred, d_out = on_device(hip, luma), on_device(hip, pred), filled(hip, (2 * len(bad) + 1) * pred.nbytes)
    descs = np.zeros(2 * len(bad) + 1, P.CFL_DESC_DTYPE)
    for k in range(len(descs)):
        descs[k] = P.cfl_desc(c, d_luma.ptr, d_pred.ptr, d_out.ptr + k * pred.nbytes, 0, 2 * c.w, c.w, c.w)
    for k, change in enumerate(bad):
        for name, value in change.items():
            descs[name][2 * k + 1] = value
    device.cfl_predict_batch(hip, descs)
    got = d_out.download(pred.dtype, (len(descs), c.h, c.w))
    for k in range(len(descs)):
        if k % 2:
            assert (got[k].view(np.uint8) == GUARD).all(), bad[k // 2]
        else:
            assert np.array_equal(got[k], gold["cfl_alpha_search"][16 + 5])
