"""GPU parity: svt_hip_obmc_target_batch and svt_hip_obmc_search_batch (include/svt_hip_inter.h) against the golden fixture of
tests/obmc_cases.py, which holds what the reference's calc_target_weighted_pred and single_motion_search leave on every case, and against
the Python restatement; and one OBMC candidate from neighbour vectors to final prediction through the existing entry points."""
import ctypes as C

import numpy as np
import pytest

import md_search_cases as M
import obmc_cases as O
from arena import GUARD, check_containment
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restated():
    """Every case's samples, segments and results from the restatement: computed once, read by all tests"""
    return [O.Restated(c) for c in O.CASES]


class Loaded(M.Loaded):
    """The samples and cost tables of a list of cases on the device, with room for every case's wsrc and mask"""

    def __init__(self, lib, cases, restated, layout=lambda i: (0, 0)):
        super().__init__(lib, O.Arena(cases, layout, restated), device.obmc_search_batch)
        self.target_descs, self.search_descs = self.arena.target_descs(self.buf.ptr), self.descs

    def target(self, descs):
        """(status words, whether the guard bytes around them kept their fill)"""
        return M.guarded(device.obmc_target_batch(self.lib, descs, fill=GUARD))

    search = M.Loaded.run

    def outputs(self, i):
        """(wsrc, mask) of case i as they are on the device now, int32 [h][w]"""
        c = self.arena.cases[i]
        return [self.buf.download(np.int32, (c.h, c.w), offset=at) for at in self.arena.outputs[i]]


@pytest.fixture(scope="module")
def gold():
    return O.Golden()


@pytest.fixture(scope="module")
def loaded(hip, restated):
    return Loaded(hip, O.CASES, restated)


def target_of_one(loaded, i):
    """The target of case i in a call of its own: the digests of what it left, which the case's search then reads"""
    status, clean = loaded.target(loaded.target_descs[i:i + 1])
    assert clean and status[0] == abi.OBMC_OK, (i, status)
    return tuple(O.digest(a) for a in loaded.outputs(i))


one_by_one = M.one_by_one_fixture(before=target_of_one)      # (digests, records)


def test_every_case_equals_the_fixture(one_by_one, gold):
    digests, records = one_by_one
    for i, r in enumerate(records):
        assert digests[i] == gold.digest(i), (i, O.CASES[i])
        assert r["status"] == abi.OBMC_OK and not r["pad_"].any(), (i, O.CASES[i])
        assert O.result_tuple(r) == gold.record(i), (i, O.CASES[i])


def test_all_cases_in_one_call(hip, restated, one_by_one):
    """The whole list shuffled in one call of each entry point on a fresh copy of the inputs, then every descriptor 27 times over: 8262
    descriptors, more than the 32 workgroups per compute unit that a 256-unit device's grid holds, so workgroups take a second descriptor.
    Then the 4 x 4 and 8 x 8 targets alone, more often than that grid holds workgroups, so that one workgroup of the single-wave target
    kernel computes two.  Results as one by one; nothing outside the wsrc and mask arrays and the results is written."""
    digests, records = one_by_one
    ld = Loaded(hip, O.CASES, restated)
    order = np.random.RandomState(7).permutation(len(O.CASES))
    status, clean = ld.target(ld.target_descs[order])
    assert clean and not status.any()
    after = ld.image()
    check_containment(ld.arena.host, after, ld.arena.regions, ld.arena.declared(), "svt_hip_obmc_target_batch")
    for i in order[:40]:
        assert tuple(O.digest(a) for a in ld.outputs(i)) == digests[i], i
    out, clean = ld.search(ld.search_descs[order])
    assert clean and out.tobytes() == records[order].tobytes()
    many = np.repeat(order, 27)
    assert len(many) > 32 * 256
    status, clean = ld.target(ld.target_descs[many])
    assert clean and not status.any()
    out, clean = ld.search(ld.search_descs[many])
    assert clean and out.tobytes() == records[many].tobytes()
    assert (ld.image() == after).all()
    # the small blocks alone, so that a workgroup of the single-wave target kernel computes a second target: its grid holds 32 x 256
    small = [i for i, c in enumerate(O.CASES) if (c.w, c.h) in ((4, 4), (8, 8))]
    many = np.tile(small, 32 * 256 // len(small) + 1)
    assert small and len(many) > 32 * 256
    for at, nbytes in ld.arena.declared(small):      # poisoned, so that the pass has to write them again
        device.check(hip, hip.svt_hip_memset(ld.buf.ptr + at, GUARD, nbytes, None), "svt_hip_memset")
    assert not (ld.image() == after).all()
    status, clean = ld.target(ld.target_descs[many])      # (the status words start as GUARD too: each is written by the workgroup that took it)
    assert clean and not status.any()
    assert (ld.image() == after).all()


def test_unaligned_pointers_and_odd_strides(hip, restated):
    """Source, neighbour buffers and reference at odd addresses with strides that are no multiple of anything (wsrc and mask stay 4-byte
    aligned, as the header asks), for the narrow and the flat sizes and two of the four-wave kernel's, against the restatement"""
    sizes = ((4, 4), (4, 16), (16, 4), (8, 8), (64, 16), (16, 64))
    picks = [i for i, c in enumerate(O.CASES) if (c.w, c.h) in sizes and c.group in ("size", "stop", "descent", "limit")]
    assert {(O.CASES[i].w, O.CASES[i].h) for i in picks} == set(sizes)
    ld = Loaded(hip, [O.CASES[i] for i in picks], [restated[i] for i in picks], layout=lambda i: (1 + 2 * (i % 16), 1 + 2 * (i % 5)))
    for f in ("src", "above", "left"):
        assert {int(d[f]) % 4 for d in ld.target_descs} == {1, 3} and all(int(d[f + "_stride"]) % 2 == 1 for d in ld.target_descs)
    assert all(int(d["ref"]) % 2 == 1 and int(d["ref_stride"]) % 2 == 1 for d in ld.search_descs)
    assert all(int(d["wsrc"]) % 4 == 0 and int(d["mask"]) % 4 == 0 for d in ld.search_descs)
    status, clean = ld.target(ld.target_descs)
    assert clean and not status.any()
    out, clean = ld.search(ld.search_descs)
    assert clean
    for k, i in enumerate(picks):
        wsrc, mask = ld.outputs(k)
        assert (wsrc == restated[i].wsrc).all() and (mask == restated[i].mask).all(), O.CASES[i]
        assert out[k]["status"] == abi.OBMC_OK and O.result_tuple(out[k]) == restated[i].record(), O.CASES[i]


def test_bad_target_descriptors_among_good_ones(hip, restated):
    """A bad descriptor gets its status; its wsrc and mask are zero where they could be written and untouched otherwise; its neighbours'
    arrays are what they are without it"""
    picks = [i for i, c in enumerate(O.CASES) if c.group in ("size", "count") and c.up and c.left][:36]
    ld = Loaded(hip, [O.CASES[i] for i in picks], [restated[i] for i in picks])
    descs, bad = ld.target_descs.copy(), {}

    def spoil(k, status, written, **fields):
        for f, v in fields.items():
            if f in ("above_nb", "left_nb"):
                for j, (rel, n) in enumerate(v):
                    descs[k][f][j]["rel_mi"], descs[k][f][j]["mi_len"] = rel, n
            else:
                descs[k][f] = v
        bad[k] = (status, written)

    spoil(1, abi.OBMC_BAD_SIZE, False, w=12)
    spoil(3, abi.OBMC_BAD_SIZE, False, w=4, h=64)
    spoil(5, abi.OBMC_BAD_SIZE, False, h=0)
    spoil(7, abi.OBMC_BAD_POINTER, True, src=0)
    spoil(9, abi.OBMC_BAD_POINTER, False, wsrc=int(descs[9]["wsrc"]) + 2)
    spoil(11, abi.OBMC_BAD_POINTER, False, mask=0)
    spoil(13, abi.OBMC_BAD_POINTER, True, above=0, n_above=1, above_nb=[(0, 1)])
    spoil(15, abi.OBMC_BAD_SEGMENT, True, n_above=5)
    spoil(17, abi.OBMC_BAD_SEGMENT, True, n_left=2, left_nb=[(0, 1), (0, 1)])                             # overlapping
    spoil(19, abi.OBMC_BAD_SEGMENT, True, n_above=1, above_nb=[(0, int(descs[19]["w"]) // 4 + 1)])        # past the block
    spoil(21, abi.OBMC_BAD_SEGMENT, True, n_left=1, left_nb=[(int(descs[21]["h"]) // 4, 1)])              # starts behind it
    spoil(23, abi.OBMC_BAD_SEGMENT, True, n_above=1, above_nb=[(0, 0)])                                   # empty
    spoil(25, abi.OBMC_BAD_SEGMENT, True, n_left=2, left_nb=[(1, 1), (0, 1)])                             # descending
    assert {ld.arena.cases[k].w * ld.arena.cases[k].h > 256 for k in bad} == {True, False}
    status, clean = ld.target(descs)
    assert clean
    after = ld.image()
    check_containment(ld.arena.host, after, ld.arena.regions, ld.arena.declared([k for k in range(len(picks)) if k not in bad or bad[k][1]]), "bad descriptors")
    for k, i in enumerate(picks):
        wsrc, mask = ld.outputs(k)
        if k in bad:
            assert status[k] == bad[k][0], (k, status[k])
            if bad[k][1]:
                assert not wsrc.any() and not mask.any(), k
        else:
            assert status[k] == abi.OBMC_OK and (wsrc == restated[i].wsrc).all() and (mask == restated[i].mask).all(), k


def test_bad_search_descriptors_among_good_ones(loaded, one_by_one):
    """A bad descriptor gets its status code and zeroes, whichever kernel its size would have put it in; its neighbours are untouched by it"""
    records = one_by_one[1]
    picks = [i for i, c in enumerate(O.CASES) if c.group == "size"][:40]
    descs, bad = loaded.search_descs[picks].copy(), {}

    def spoil(k, status, **fields):
        for f, v in fields.items():
            if f in ("start_row", "start_col"):
                descs[k]["start_mv"][f[6:]] = v
            elif f in ("fp_limits", "raw_limits"):
                descs[k][f][:] = v
            else:
                descs[k][f] = v
        bad[k] = status

    spoil(1, abi.OBMC_BAD_SIZE, w=12)
    spoil(4, abi.OBMC_BAD_SIZE, w=4, h=64)
    spoil(7, abi.OBMC_BAD_SIZE, w=128, h=256)
    spoil(10, abi.OBMC_BAD_POINTER, ref=0)
    spoil(13, abi.OBMC_BAD_POINTER, wsrc=int(descs[13]["wsrc"]) + 1)
    spoil(16, abi.OBMC_BAD_POINTER, mask=0)
    spoil(19, abi.OBMC_BAD_RANGE, fpel_search_range=17)
    spoil(22, abi.OBMC_BAD_RANGE, fpel_search_range=255, do_full_refine=0)
    spoil(25, abi.OBMC_BAD_START_MV, start_row=1 << 14)
    spoil(28, abi.OBMC_BAD_START_MV, start_col=-(1 << 14))
    spoil(31, abi.OBMC_BAD_LIMITS, fp_limits=(5, 4, -10, 10))
    spoil(33, abi.OBMC_BAD_LIMITS, raw_limits=(-10, 10, 3, 2))
    spoil(34, abi.OBMC_BAD_LIMITS, fp_limits=(-2049, 10, -10, 10))
    spoil(36, abi.OBMC_BAD_FILTER, subpel_search_type=0)
    spoil(37, abi.OBMC_BAD_FILTER, subpel_search_type=4, do_frac_refine=0)
    assert {O.CASES[picks[k]].w * O.CASES[picks[k]].h > 256 for k in bad} == {True, False}
    out, clean = loaded.search(descs)
    assert clean
    zero = np.zeros((), abi.OBMC_SEARCH_RESULT_DTYPE)
    for k, r in enumerate(out):
        if k in bad:
            zero["status"] = bad[k]
            assert r.tobytes() == zero.tobytes(), (k, r)
        else:
            assert r.tobytes() == records[picks[k]].tobytes(), k
    # the entropy costs without the job's tables
    entropy = [i for i, c in enumerate(O.CASES) if not c.approx][:2] + [i for i, c in enumerate(O.CASES) if c.approx][:1]
    out, _ = loaded.search(loaded.search_descs[entropy], job=abi.SubpelJob())
    assert [int(r["status"]) for r in out] == [abi.OBMC_BAD_COST, abi.OBMC_BAD_COST, abi.OBMC_OK]
    assert out[2].tobytes() == records[entropy[2]].tobytes()


def test_call_level_errors(hip, loaded):
    """NULL job, descriptors, status words or results: SVT_HIP_ERR_BAD_PARAMETER; an empty batch is fine and writes nothing"""
    d_search, d_target = device.upload_descriptors(hip, loaded.search_descs[:1]), device.upload_descriptors(hip, loaded.target_descs[:1])
    M.assert_call_level_errors(hip, "svt_hip_obmc_search_batch", abi.SVT_HIP_ERR_BAD_PARAMETER, [C.byref(loaded.job), C.c_void_p(d_search.ptr)])
    M.assert_call_level_errors(hip, "svt_hip_obmc_target_batch", abi.SVT_HIP_ERR_BAD_PARAMETER, [C.c_void_p(d_target.ptr)])


# ---- one OBMC candidate from neighbour vectors to final prediction ----------------------------------------------------------------
def predict_sr(ref, y, x, mv, w, h):
    """svt_av1_convolve_2d_sr_c / _x_sr_c / _y_sr_c / _2d_copy_sr_c with the regular 8-tap filter and the ConvolveParams of a single
    reference at 8 bits (round_0 3, round_1 11): the w x h block at (y, x) of ref moved by mv (1/8 units)"""
    y, x, sy, sx = y + (mv[0] >> 3), x + (mv[1] >> 3), mv[0] & 7, mv[1] & 7
    fx, fy = O.FILTERS[2][sx].astype(np.int64), O.FILTERS[2][sy].astype(np.int64)
    r = ref.astype(np.int64)
    if not sx and not sy:
        return r[y:y + h, x:x + w]
    if not sy:
        s = sum(fx[k] * r[y:y + h, x - 3 + k:x - 3 + k + w] for k in range(8))
        return np.clip((((s + 4) >> 3) + 8) >> 4, 0, 255)
    if not sx:
        s = sum(fy[k] * r[y - 3 + k:y - 3 + k + h, x:x + w] for k in range(8))
        return np.clip((s + 64) >> 7, 0, 255)
    im = (sum(fx[k] * r[y - 3:y + h + 4, x - 3 + k:x - 3 + k + w] for k in range(8)) + 4) >> 3      # the offsets of the C code cancel exactly
    return np.clip((sum(fy[k] * im[k:k + h] for k in range(8)) + 1024) >> 11, 0, 255)


def conv_desc(src, src_stride, dst, dst_stride, mv, w, h):
    """The single-reference descriptor of that prediction; src: the device address of the block's co-located sample"""
    d = abi.ConvolveDesc()
    d.src, d.src_stride, d.dst, d.dst_stride, d.w, d.h = src + (mv[0] >> 3) * src_stride + (mv[1] >> 3), src_stride, dst, dst_stride, w, h
    d.filter_x[:], d.filter_y[:] = [int(v) for v in O.FILTERS[2][mv[1] & 7]], [int(v) for v in O.FILTERS[2][mv[0] & 7]]
    d.taps_x, d.taps_y, d.round_0, d.round_1, d.bit_depth = 8 if mv[1] & 7 else 0, 8 if mv[0] & 7 else 0, 3, 11, 8
    return d


@pytest.mark.parametrize("w,h", [(16, 16), (32, 8)])
def test_one_candidate_from_neighbour_vectors_to_final_prediction(hip, w, h):
    """svt_hip_convolve_batch makes the neighbour predictions, svt_hip_obmc_target_batch the target from them, svt_hip_obmc_search_batch the
    vector, svt_hip_convolve_batch the block's prediction at it and svt_hip_blend_batch the vmask / hmask blends of
    build_obmc_inter_pred_above / _left: the buffers each entry point leaves are the ones the next reads, and the final prediction is the
    restatement's."""
    c = next(c for c in O.CASES if (c.w, c.h) == (w, h) and c.group == "size" and c.full and c.frac and not c.approx)
    # 8-sample neighbours above (more than nb_max of them over the 32 x 8), one neighbour to the left
    c = c._replace(above_tiles=((2, 1),) * (w // 8), above_from=c.mi_col, left_tiles=((h // 4, 1),), left_from=c.mi_row)
    ref, src, _, _ = O.pictures(c)
    seg_above, seg_left = O.segments(c)
    assert seg_above and seg_left
    ov_above, ov_left = min(h, 64) >> 1, min(w, 64) >> 1
    vectors = [((7 * k + 3) % 19 - 9, (5 * k + 8) % 19 - 9) for k in range(8)]
    vectors[1] = (vectors[1][0] & ~7, vectors[1][1])      # one neighbour without a vertical fraction
    # restatement
    B = O.BORDER
    above, left = np.full((h, w), GUARD, np.int64), np.full((h, w), GUARD, np.int64)
    for k, (rel, n) in enumerate(seg_above):
        above[:ov_above, rel * 4:(rel + n) * 4] = predict_sr(ref, B, B + rel * 4, vectors[k], n * 4, ov_above)
    for k, (rel, n) in enumerate(seg_left):
        left[rel * 4:(rel + n) * 4, :ov_left] = predict_sr(ref, B + rel * 4, B, vectors[4 + k], ov_left, n * 4)
    wsrc, mask = O.target(c, src, above, left, (seg_above, seg_left))
    search = O.Search(c, ref, wsrc, mask)
    want = predict_sr(ref, B, B, search.best, w, h).copy()
    for rel, n in seg_above:
        m = np.array(O.RAMPS[ov_above], np.int64)[:, None]
        cols = slice(rel * 4, (rel + n) * 4)
        want[:ov_above, cols] = (m * want[:ov_above, cols] + (64 - m) * above[:ov_above, cols] + 32) >> 6
    for rel, n in seg_left:
        m = np.array(O.RAMPS[ov_left], np.int64)[None, :]
        rows = slice(rel * 4, (rel + n) * 4)
        want[rows, :ov_left] = (m * want[rows, :ov_left] + (64 - m) * left[rows, :ov_left] + 32) >> 6
    # the device: one buffer with the reference, the source, the two neighbour buffers, the prediction, wsrc, mask, the ramps and the tables
    import arena as A
    ab = A.Arena(fill=GUARD, tail=64)
    at = {name: ab.add(name, arr) for name, arr in (("ref", ref), ("src", src))}
    for name in ("above", "left", "pred"):
        at[name] = ab.add(name, nbytes=w * h)
    for name in ("wsrc", "mask"):
        at[name] = ab.add(name, nbytes=4 * w * h)
    at["ramp_above"], at["ramp_left"] = ab.add("ramp above", np.array(O.RAMPS[ov_above], np.uint8)), ab.add("ramp left", np.array(O.RAMPS[ov_left], np.uint8))
    mvj, row, col = O.mv_cost_tables()
    tables = [ab.add(name, t) - 4 * O.MV_LOW for name, t in (("mvcost row", row), ("mvcost col", col))]
    host = ab.build()
    buf = device.DeviceBuffer(hip, host.nbytes)
    buf.upload(host)
    base, ref_stride = buf.ptr, ref.shape[1]
    ref0 = base + at["ref"] + B * ref_stride + B
    conv = [conv_desc(ref0 + rel * 4, ref_stride, base + at["above"] + rel * 4, w, vectors[k], n * 4, ov_above) for k, (rel, n) in enumerate(seg_above)]
    conv += [conv_desc(ref0 + rel * 4 * ref_stride, ref_stride, base + at["left"] + rel * 4 * w, w, vectors[4 + k], ov_left, n * 4) for k, (rel, n) in enumerate(seg_left)]
    device.convolve_batch(hip, conv)
    t = np.zeros(1, abi.OBMC_TARGET_DESC_DTYPE)
    for f in ("src", "above", "left", "wsrc", "mask"):
        t[0][f] = base + at[f]
    t[0]["src_stride"], t[0]["above_stride"], t[0]["left_stride"], t[0]["w"], t[0]["h"], t[0]["up_available"], t[0]["left_available"] = w, w, w, w, h, 1, 1
    for side, segs in (("above", seg_above), ("left", seg_left)):
        t[0]["n_" + side] = len(segs)
        for k, (rel, n) in enumerate(segs):
            t[0][side + "_nb"][k]["rel_mi"], t[0][side + "_nb"][k]["mi_len"] = rel, n
    status, _ = device.obmc_target_batch(hip, t, fill=GUARD)
    assert status[0] == abi.OBMC_OK
    job = abi.SubpelJob()
    job.mvjcost[:] = [int(v) for v in mvj]
    job.mvcost[0], job.mvcost[1] = base + tables[0], base + tables[1]
    s = np.zeros(1, abi.OBMC_SEARCH_DESC_DTYPE)
    s[0] = O.fill_search_desc(c, base + at["wsrc"], base + at["mask"], ref0, ref_stride)
    out, _ = device.obmc_search_batch(hip, job, s, fill=GUARD)
    assert out[0]["status"] == abi.OBMC_OK and O.result_tuple(out[0]) == search.record()
    best = (int(out[0]["best_mv"]["row"]), int(out[0]["best_mv"]["col"]))
    device.convolve_batch(hip, [conv_desc(ref0, ref_stride, base + at["pred"], w, best, w, h)])

    def blend(kind, off, bw, bh, neighbour, ramp):
        d = abi.BlendDesc()
        d.src0 = d.dst = base + at["pred"] + off
        d.src1, d.mask, d.src0_stride, d.src1_stride, d.dst_stride, d.w, d.h, d.kind, d.bit_depth = base + at[neighbour] + off, base + at[ramp], w, w, w, bw, bh, kind, 8
        return d

    device.blend_batch(hip, [blend(abi.BLEND_VMASK, rel * 4, n * 4, ov_above, "above", "ramp_above") for rel, n in seg_above])
    device.blend_batch(hip, [blend(abi.BLEND_HMASK, rel * 4 * w, ov_left, n * 4, "left", "ramp_left") for rel, n in seg_left])
    after = buf.download(np.uint8, (host.nbytes,))
    got = after[at["pred"]:at["pred"] + w * h].reshape(h, w)
    assert (got == want).all()
    assert (after[at["wsrc"]:at["wsrc"] + 4 * w * h].view(np.int32).reshape(h, w) == wsrc).all()
    declared = [(at[name], w * h) for name in ("above", "left", "pred")] + [(at[name], 4 * w * h) for name in ("wsrc", "mask")]
    check_containment(host, after, ab.regions, declared, "the chain")
