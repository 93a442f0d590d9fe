"""GPU parity: svt_hip_subpel_search_batch (include/svt_hip_inter.h) against the golden fixture of tests/subpel_cases.py, which holds what
the reference's svt_av1_find_best_sub_pixel_tree(_pruned) leave on every case, and against the Python restatement."""
import ctypes as C

import numpy as np
import pytest

import md_search_cases as M
import subpel_cases as S
from arena import GUARD
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu


def Loaded(lib, cases, layout=lambda i: (0, 0)):
    """The pictures and cost tables of a list of cases on the device"""
    return M.Loaded(lib, S.Arena(cases, layout), device.subpel_search_batch)


@pytest.fixture(scope="module")
def gold():
    return S.Golden()


@pytest.fixture(scope="module")
def loaded(hip):
    return Loaded(hip, S.CASES)


one_by_one = M.one_by_one_fixture()


def test_every_case_equals_the_fixture(one_by_one, gold):
    for i, r in enumerate(one_by_one):
        assert r["status"] == abi.SUBPEL_OK and not r["pad_"].any(), (i, S.CASES[i])
        assert S.result_tuple(r) == gold.record(i), (i, S.CASES[i])


def test_all_cases_in_one_call(loaded, one_by_one):
    """The whole list shuffled, and then every descriptor 24 times over: 9168 descriptors, more than the 32 workgroups per compute unit
    that a 256-unit device's grid holds, so workgroups take a second descriptor.  Records as one by one; nothing written past the last."""
    order = np.random.RandomState(7).permutation(len(S.CASES))
    out, clean = loaded.run(loaded.descs[order])
    assert clean and out.tobytes() == one_by_one[order].tobytes()
    many = np.repeat(order, 24)
    assert len(many) > 32 * 256
    out, clean = loaded.run(loaded.descs[many])
    assert clean and out.tobytes() == one_by_one[many].tobytes()


def test_unaligned_pointers_and_odd_strides(hip):
    """src and ref at odd addresses, strides that are no multiple of anything, for the narrow and the flat sizes and one of the four-wave
    kernel's, against the restatement"""
    sizes = ((4, 4), (4, 16), (16, 4), (8, 8), (64, 16))
    cases = [c for c in S.CASES if (c.w, c.h) in sizes and c.group in ("size", "taps", "skip_diag", "reach")]
    assert {(c.w, c.h, c.method) for c in cases} == {(w, h, m) for w, h in sizes for m in (S.TREE, S.PRUNED)}
    ld = Loaded(hip, cases, layout=lambda i: (1 + 2 * (i % 16), 1 + 2 * (i % 5)))
    assert all(int(d["src"]) % 2 == 1 or int(d["ref"]) % 2 == 1 for d in ld.descs) and all(int(d["ref_stride"]) % 2 == 1 for d in ld.descs)
    assert {int(d["src"]) % 4 for d in ld.descs} == {1, 3} and {int(d["src_stride"]) % 4 for d in ld.descs} == {1, 3}
    out, clean = ld.run(ld.descs)
    assert clean
    for c, r in zip(cases, out):
        assert r["status"] == abi.SUBPEL_OK and S.result_tuple(r) == S.Search(c).record(), c


def test_bad_descriptors_among_good_ones(loaded, one_by_one):
    """A bad descriptor gets its status code and zeroes, whichever kernel its size would have put it in; its neighbours are untouched by it"""
    picks = [i for i, c in enumerate(S.CASES) if c.group == "size"][:40]
    descs = loaded.descs[picks].copy()
    bad = {}

    def spoil(k, status, **fields):
        for f, v in fields.items():
            if f in ("start_row", "start_col"):
                descs[k]["start_mv"][f[6:]] = v
            else:
                descs[k][f] = v
        bad[k] = status

    spoil(1, abi.SUBPEL_BAD_SIZE, w=12)
    spoil(4, abi.SUBPEL_BAD_SIZE, w=4, h=64)
    spoil(7, abi.SUBPEL_BAD_SIZE, w=128, h=256)
    spoil(10, abi.SUBPEL_BAD_SIZE, w=0)
    spoil(13, abi.SUBPEL_BAD_POINTER, src=0)
    spoil(16, abi.SUBPEL_BAD_POINTER, ref=0)
    spoil(19, abi.SUBPEL_BAD_START_MV, start_row=int(descs[19]["start_mv"]["row"]) + 4)
    spoil(22, abi.SUBPEL_BAD_START_MV, start_col=int(descs[22]["start_mv"]["col"]) + 1)
    spoil(25, abi.SUBPEL_BAD_METHOD, method=2)
    spoil(28, abi.SUBPEL_BAD_FILTER, subpel_search_type=0)
    spoil(31, abi.SUBPEL_BAD_FILTER, subpel_search_type=4)
    spoil(34, abi.SUBPEL_BAD_COST, mv_cost_type=6)
    spoil(37, abi.SUBPEL_BAD_FILTER, subpel_search_type=9, method=abi.SUBPEL_TREE_PRUNED)
    assert {S.CASES[picks[k]].w * S.CASES[picks[k]].h > 256 for k in bad} == {True, False}
    out, clean = loaded.run(descs)
    assert clean
    zero = np.zeros((), abi.SUBPEL_RESULT_DTYPE)
    for k, r in enumerate(out):
        if k in bad:
            zero["status"] = bad[k]
            assert r.tobytes() == zero.tobytes(), (k, r)
        else:
            assert r.tobytes() == one_by_one[picks[k]].tobytes(), k
    # MV_COST_ENTROPY without the job's tables
    job = abi.SubpelJob()
    entropy = [i for i, c in enumerate(S.CASES) if c.cost_type == S.ENTROPY][:2] + [i for i, c in enumerate(S.CASES) if c.cost_type == S.NONE][:1]
    out, _ = device.subpel_search_batch(loaded.lib, job, loaded.descs[entropy], fill=GUARD)
    assert [int(r["status"]) for r in out] == [abi.SUBPEL_BAD_COST, abi.SUBPEL_BAD_COST, abi.SUBPEL_OK]
    assert out[2].tobytes() == one_by_one[entropy[2]].tobytes()


def test_call_level_errors(hip, loaded):
    """NULL job, descriptors or results: SVT_HIP_ERR_BAD_PARAMETER; an empty batch is fine and writes nothing"""
    d_desc = device.upload_descriptors(hip, loaded.descs[:1])
    M.assert_call_level_errors(hip, "svt_hip_subpel_search_batch", abi.SVT_HIP_ERR_BAD_PARAMETER, [C.byref(loaded.job), C.c_void_p(d_desc.ptr)])
