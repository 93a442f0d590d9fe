"""GPU parity: svt_hip_fpel_search_batch (include/svt_hip_inter.h) against the golden fixture of tests/fpel_cases.py, which holds what the
reference's md_full_pel_search leaves on every case as its callers chain it, and against the Python restatement."""
import ctypes as C

import numpy as np
import pytest

import fpel_cases as F
import md_search_cases as M
import subpel_cases as S
from arena import GUARD
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu


def Loaded(lib, cases, layout=lambda i: (0, 0)):
    """The pictures and cost tables of a list of cases on the device"""
    return M.Loaded(lib, F.Arena(cases, layout), device.fpel_search_batch)


@pytest.fixture(scope="module")
def gold():
    return F.Golden()


@pytest.fixture(scope="module")
def loaded(hip):
    return Loaded(hip, F.CASES)


one_by_one = M.one_by_one_fixture()


def test_every_case_equals_the_fixture(one_by_one, gold):
    for i, r in enumerate(one_by_one):
        assert r["status"] == abi.FPEL_OK and not r["pad_"], (i, F.CASES[i])
        assert F.result_tuple(r) == gold.record(i), (i, F.CASES[i])


def test_windows_span_tiles_of_the_size_the_kernel_states():
    """One window per distortion type (and per scan for the SAD) is larger than the LDS tile of SVT_HIP_FPEL_TILE x SVT_HIP_FPEL_TILE positions
    that the kernel walks, its winner lies in a tile other than the first and ties with a position in yet another tile"""
    assert abi.FPEL_TILE == F.TILE == 32
    seen = set()
    for c in F.CASES:
        if c.name == "tiles" and c.mode == F.PME:
            (ay, ax, _), (by, bx, _) = c.pic[2]["at"]
            lv = c.levels[0]
            tiles = {((x - lv.start_x) // F.TILE, (y - lv.start_y) // F.TILE) for x, y in ((ax, ay), (bx, by))}
            assert len(tiles) == 2 and (0, 0) not in tiles and lv.end_x - lv.start_x >= 2 * F.TILE and lv.end_y - lv.start_y >= 2 * F.TILE
            s = F.Search(c)
            assert s.result[2] == 0 and (s.result[0] // 8, s.result[1] // 8) in ((ay, ax), (by, bx))
            seen.add((c.dist, c.psad))
    assert seen == {(F.SAD, 0), (F.SAD, 1), (F.VAR, 0), (F.SSD, 0)}


def test_all_cases_in_one_call(loaded, one_by_one):
    """The whole list shuffled, and then every descriptor 9 times over: 2124 descriptors, more than the 8 workgroups per compute unit that a
    256-unit device's grid holds, so workgroups take a second descriptor.  Records as one by one; nothing written past the last."""
    order = np.random.RandomState(7).permutation(len(F.CASES))
    out, clean = loaded.run(loaded.descs[order])
    assert clean and out.tobytes() == one_by_one[order].tobytes()
    many = np.repeat(order, 9)
    assert len(many) > 8 * 256
    out, clean = loaded.run(loaded.descs[many])
    assert clean and out.tobytes() == one_by_one[many].tobytes()
    loaded.assert_untouched("all cases in one call")


def test_unaligned_pointers_and_odd_strides(hip):
    """src and ref at odd addresses, strides that are no multiple of anything, for the narrow and the flat sizes and one wide one, against the
    restatement run on the same widened planes (the psad overshoot reads the stride padding)"""
    sizes = ((4, 4), (4, 16), (16, 4), (8, 8), (64, 16))
    cases = [c for c in F.CASES if (c.w, c.h) in sizes and c.name in ("size", "size_psad", "single", "nine", "pm2", "nsq", "clip_right", "psad_width", "tiles")]
    assert {(c.w, c.h) for c in cases} == set(sizes) and {c.mode for c in cases} == {F.SQ, F.NSQ, F.PME} and {c.psad for c in cases} == {0, 1}
    ld = Loaded(hip, cases, layout=lambda i: (1 + 2 * (i % 16), 1 + 2 * (i % 5)))
    assert all(int(d["src"]) % 2 == 1 or int(d["ref"]) % 2 == 1 for d in ld.descs) and all(int(d["ref_stride"]) % 2 == 1 for d in ld.descs)
    assert {int(d["src"]) % 4 for d in ld.descs} == {1, 3} and {int(d["src_stride"]) % 4 for d in ld.descs} == {1, 3}
    out, clean = ld.run(ld.descs)
    assert clean
    for c, r, (src, ref) in zip(cases, out, ld.arena.views):
        assert r["status"] == abi.FPEL_OK and F.result_tuple(r) == F.Search(c, src, ref).record(), c
    ld.assert_untouched("odd strides")


def test_bad_descriptors_among_good_ones(loaded, one_by_one):
    """A bad descriptor gets its status code and zeroes; its neighbours are untouched by it"""
    picks = [i for m in (F.PME, F.SQ, F.NSQ, F.MVP) for i in [i for i, c in enumerate(F.CASES) if c.mode == m and c.name in ("size", "cost", "subset", "nsq", "mvp")][:12]]
    descs = loaded.descs[picks].copy()
    mode = lambda m: next(k for k, i in enumerate(picks) if F.CASES[i].mode == m and k not in bad and 2 < k)      # noqa: E731
    bad = {}

    def spoil(k, status, **fields):
        for f, v in fields.items():
            if f.startswith("level"):
                descs[k]["level"][int(f[5])][f[7:]] = v
            else:
                descs[k][f] = v
        bad[k] = status

    spoil(1, abi.FPEL_BAD_SIZE, w=12)
    spoil(mode(F.PME), abi.FPEL_BAD_SIZE, w=4, h=64)
    spoil(mode(F.PME), abi.FPEL_BAD_SIZE, w=128, h=256)
    spoil(mode(F.PME), abi.FPEL_BAD_SIZE, w=0)
    spoil(mode(F.PME), abi.FPEL_BAD_POINTER, src=0)
    spoil(mode(F.NSQ), abi.FPEL_BAD_POINTER, ref=0)
    spoil(mode(F.PME), abi.FPEL_BAD_MODE, mode=4)
    spoil(mode(F.PME), abi.FPEL_BAD_DIST, dist_type=3)
    spoil(mode(F.NSQ), abi.FPEL_BAD_COST, mv_cost_type=6)
    spoil(mode(F.NSQ), abi.FPEL_BAD_COUNT, n_mv=0)
    spoil(mode(F.NSQ), abi.FPEL_BAD_COUNT, n_mv=7)
    spoil(mode(F.MVP), abi.FPEL_BAD_COUNT, n_mv=5)
    spoil(mode(F.MVP), abi.FPEL_BAD_COUNT, n_mv=0)
    spoil(mode(F.SQ), abi.FPEL_BAD_STEP, level0_enabled=1, level0_step=0)
    spoil(mode(F.SQ), abi.FPEL_BAD_WINDOW, level2_enabled=1, level2_step=1, level2_start_x=-2048, level2_end_x=2048)
    spoil(mode(F.PME), abi.FPEL_BAD_WINDOW, level0_start_y=-4000, level0_end_y=96)
    assert len(bad) == 16
    out, clean = loaded.run(descs)
    assert clean
    zero = np.zeros((), abi.FPEL_RESULT_DTYPE)
    for k, r in enumerate(out):
        if k in bad:
            zero["status"] = bad[k]
            assert r.tobytes() == zero.tobytes(), (k, r)
        else:
            assert r.tobytes() == one_by_one[picks[k]].tobytes(), k
    # a disabled level may hold anything; MVP mode reads no cost type; MV_COST_ENTROPY without the job's tables
    k = next(i for i, c in enumerate(F.CASES) if c.name == "pm2")
    d = loaded.descs[k:k + 1].copy()
    d["level"][0][0]["step"], d["level"][0][0]["start_x"], d["level"][0][2]["end_y"] = 0, -30000, 30000
    assert loaded.run(d)[0].tobytes() == one_by_one[k:k + 1].tobytes()
    job = abi.SubpelJob()
    pick = ([i for i, c in enumerate(F.CASES) if c.cost_type == F.ENTROPY and c.mode != F.MVP][:2] +
            [i for i, c in enumerate(F.CASES) if c.cost_type == F.NONE and c.mode != F.MVP][:1] + [i for i, c in enumerate(F.CASES) if c.mode == F.MVP][:1])
    d = loaded.descs[pick].copy()
    d["mv_cost_type"][3] = F.ENTROPY
    out, _ = device.fpel_search_batch(loaded.lib, job, d, fill=GUARD)
    assert [int(r["status"]) for r in out] == [abi.FPEL_BAD_COST, abi.FPEL_BAD_COST, abi.FPEL_OK, abi.FPEL_OK]
    assert out[2:].tobytes() == one_by_one[pick[2:]].tobytes()
    loaded.assert_untouched("bad descriptors")


def test_call_level_errors(hip, loaded):
    """NULL job, descriptors or results: SVT_HIP_ERR_BAD_PARAMETER in 16 bits; an empty batch is fine and writes nothing"""
    d_desc = device.upload_descriptors(hip, loaded.descs[:1])
    M.assert_call_level_errors(hip, "svt_hip_fpel_search_batch", abi.fpel_status(abi.SVT_HIP_ERR_BAD_PARAMETER), [C.byref(loaded.job), C.c_void_p(d_desc.ptr)])


@pytest.mark.parametrize("w,h", [(16, 16), (32, 8)])
def test_chain_from_mvp_to_sub_pel_without_a_download(hip, w, h):
    """MVP scoring and the SQ search in one call, their records copied on the device into a sub-pel descriptor (best_mv -> start_mv, the
    best MVP -> best_mvp, its distortion -> best_mvp_dist), svt_hip_subpel_search_batch on that: against the two restatements chained."""
    pic = ("tex", 4242 + w, {"shift": (3, -2), "cell": 8})
    common = dict(w=w, h=h, cost_type=F.ENTROPY, epb=300, ref_mv=(6, -10), geo=F.Geo(w + 64, h + 64, 16, 16, 32, 32), levels=None, pocd=1, sq_size=max(w, h),
                  nsq=(0, 0), sub=None, geom_org=(0, 0), pic=pic, psad=0)
    mvp = F.Case(name="chain", mode=F.MVP, dist=F.VAR, mvs=[(0, 0), (19, -13), (-16, 24)], ctrls=None, sam=0, th=0, **common)
    sq = F.Case(name="chain", mode=F.SQ, dist=F.VAR, mvs=[(8, -8)], ctrls=F.sq_level_ctrls(4), sam=2, th=0, **common)
    ld = Loaded(hip, [mvp, sq])
    want_mvp, want_sq = F.Search(mvp).record(), F.Search(sq).record()
    assert want_sq[4] == 1 and want_sq[:2] != (8, -8) and want_mvp[5] != 0
    # the sub-pel search that follows, with the mvp_th rule on so that best_mvp and best_mvp_dist matter
    sc = S.Case("chain", w, h, S.TREE, taps=3, iters=2, forced_stop=0, allow_hp=1, bias_fp=0, skip_diag=0, pred_var_th=0, abs_th_mult=0, round_dev_th=S.INT_MAX,
                qp=40, cost_type=S.ENTROPY, epb=300, early_exit_th=1500, early_exit=0, mvp_th=20, hp_mv_th=12, mvp_dist=want_mvp[2], mvp=want_mvp[:2],
                start=want_sq[:2], ref_mv=(6, -10), true_mv=None, limits=(-400, 400, -400, 400), kind="", noise=0, seed=0)
    src, ref = F.pictures(sq)
    g = sq.geo
    oy, ox = g.org_y + g.blk_y - S.BORDER, g.org_x + g.blk_x - S.BORDER
    want = S.Search(sc, src[oy:, ox:], ref[oy:, ox:]).record()
    sd = S.fill_desc(sc._replace(start=(0, 0), mvp=(0, 0), mvp_dist=0), int(ld.descs[1]["src"]), int(ld.descs[1]["ref"]), int(ld.descs[1]["src_stride"]),
                     int(ld.descs[1]["ref_stride"]), S.case_limits(sc)).reshape(1)
    d_fpel, d_sub = device.upload_descriptors(hip, ld.descs), device.upload_descriptors(hip, sd)
    d_res = device.Guarded(hip, 2 * C.sizeof(abi.FpelResult), 64, GUARD)
    d_out = device.Guarded(hip, C.sizeof(abi.SubpelResult), 64, GUARD)
    assert hip.svt_hip_fpel_search_batch(C.byref(ld.job), d_fpel.ptr, d_res.ptr, 2, None) == 0, hip.svt_hip_last_error()
    rsz, off = C.sizeof(abi.FpelResult), lambda f: getattr(abi.SubpelDesc, f).offset      # noqa: E731
    for dst, src_at in ((off("best_mvp"), abi.FpelResult.best_mv.offset), (off("best_mvp_dist"), abi.FpelResult.best_cost.offset),
                        (off("start_mv"), rsz + abi.FpelResult.best_mv.offset)):
        device.check(hip, hip.svt_hip_copy(d_sub.ptr + dst, d_res.ptr + src_at, 4, None), "svt_hip_copy")
    device.check(hip, hip.svt_hip_subpel_search_batch(C.byref(ld.job), d_sub.ptr, d_out.ptr, 1, None), "svt_hip_subpel_search_batch")
    (res, g1), (out, g2) = d_res.read(abi.FPEL_RESULT_DTYPE), d_out.read(abi.SUBPEL_RESULT_DTYPE)
    assert (g1 == GUARD).all() and (g2 == GUARD).all()
    assert F.result_tuple(res[0]) == want_mvp and F.result_tuple(res[1]) == want_sq
    assert out[0]["status"] == abi.SUBPEL_OK and S.result_tuple(out[0]) == want
    ld.assert_untouched("chain")
