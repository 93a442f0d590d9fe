"""CPU: the interpolation filter search's fixture, restatement and C-ABI (svt_hip_ifs_search_batch, include/svt_hip_inter.h).  The fixture
tests/golden/ifs.npz equals what the reference's own functions leave (tests/ifs_pin_driver.c) wherever oracle/_ref/libsvtref.so is built,
the numpy restatement of tests/ifs_cases.py equals the fixture on every case, and the conditions the case list is there for are reached."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

import ifs_cases as I
import pyorc
from support import assert_not_rtcd_leaf, fresh_process, have_reference_tree, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

NAME = "svt_hip_ifs_search_batch"


@pytest.fixture(scope="module")
def gold():
    return I.Golden()


@pytest.fixture(scope="module")
def found():
    return [I.search(c) for c in I.CASES]


@pytest.mark.skipif(not (have_reference_tree() and pyorc.have_ref()), reason="needs the reference tree and oracle/_ref/libsvtref.so")
def test_fixture_is_what_the_reference_functions_leave(gold, tmp_path):
    pin = I.Pin(tmp_path)
    assert np.array_equal(pin.banks(), gold.banks)
    for i, c in enumerate(I.CASES):
        assert pin.search(c) == gold.record(i), (i, c)


def test_restatement_equals_the_fixture_on_every_case(gold, found):
    assert np.array_equal(gold.banks, I.BANKS)
    for i, c in enumerate(I.CASES):
        assert I.found_tuple(found[i], c) == gold.record(i), (i, c)


def test_the_cases_reach_what_they_are_there_for(found):
    by = lambda group: [(c, f) for c, f in zip(I.CASES, found) if c.group == group]
    job = lambda c: I.JOBS[c.job]
    tested = lambda c: [i for i, (fy, fx) in enumerate(I.FILTER_SETS) if job(c).dual or fy == fx]
    # all 22 sizes single and compound at both depths, both components fractional; the 4-tap banks in each direction; several tiles
    for bd in (8, 10):
        for comp in (False, True):
            got = {(c.w, c.h) for c, _ in by("size") if job(c).bd == bd and bool(c.compound) == comp}
            assert got == set(I.SIZES) and len(I.SIZES) == 22
    assert all(c.phases[0] and c.phases[1] and (not c.compound or (c.phases[2] and c.phases[3])) for c, _ in by("size"))
    assert {(c.w <= 4, c.h <= 4) for c, _ in by("size")} == {(False, False), (True, False), (False, True), (True, True)}
    assert {(c.w, c.h) for c, _ in by("size")} >= {(128, 64), (64, 128), (128, 128)}
    # the four families in sr and in jnt form, on both shapes
    for shape in ((8, 8), (4, 16)):
        for comp in (False, True):
            fam = {(bool(c.phases[0]), bool(c.phases[1])) for c, _ in by("phase") if (c.w, c.h) == shape and bool(c.compound) == comp}
            assert len(fam) == 4
            assert len({c.phases[:2] for c, _ in by("phase") if (c.w, c.h) == shape and bool(c.compound) == comp}) == 64
    # the weight pairs and their reverses, one reference at zero phases, the other not
    w3 = [c for c, _ in by("weights") if c.compound == 3]
    assert {(c.fwd, c.bck) for c in w3} == set(I.WEIGHTS) | {(b, a) for a, b in I.WEIGHTS} and all(c.fwd + c.bck == 16 for c in w3)
    assert {c.phases[:2] == (0, 0) for c in w3} == {True, False} and all((c.phases[:2] == (0, 0)) != (c.phases[2:] == (0, 0)) for c in w3)
    assert {c.compound for c in I.CASES} == {0, 2, 3}
    # the controls
    assert {(j.bd, j.dual) for j in I.JOBS} == {(8, 0), (8, 1), (10, 0), (10, 1)}
    assert {c.h for c, _ in by("sub")} >= {16, 32} and all(job(c).sub for c, _ in by("sub"))
    assert all(f.sse[i] % 2 == 0 for c, f in by("sub") if c.h > 16 for i in tested(c))
    assert any(f.sse[i] % 2 for c, f in by("sub") if c.h == 16 for i in tested(c))
    assert {job(c).skip for c in I.CASES} == {0, 1} and {job(c).bias for c in I.CASES} == {0, 110, 130}
    assert all(f.rd[i] == f.sse[i] * 10 * 128 + ((int(I.rate_table("random")[c.ctx[0]][i // 3] + I.rate_table("random")[c.ctx[1]][i % 3]) * job(c).lam + 256) >> 9)
               for c, f in by("skip") for i in tested(c))
    # the quantizer's ends at both depths: qstep 0 at the lowest
    q = {(job(c).bd, job(c).q >> (job(c).bd - 5)) for c, _ in by("quantizer")}
    assert q == {(8, 0), (8, 228), (10, 0), (10, 228)} and {job(c).q >> (job(c).bd - 5) for c in I.CASES} > {0, 228}
    # the clamp is reached where it is meant to be, and not everywhere
    assert all(f.clamped and 0 < max(f.sse) < 10000 for c, f in by("clamp")) and not all(f.clamped for c, f in by("size"))
    # sse == 0: the model answers (0, 0), the rate alone decides
    for c, f in by("zero"):
        assert all(f.sse[i] == 0 for i in tested(c)) and f.best == min(tested(c), key=lambda i: (f.rd[i], i))
    assert any(f.rd[f.best] > 0 for c, f in by("zero"))
    # 64-bit sums
    assert all(max(f.sse[i] for i in tested(c)) > 1 << 32 for c, f in by("contrast")) and {job(c).bd for c, _ in by("contrast")} == {10}
    # flat references: nine equal SSEs; unequal rates decide, equal rates leave the first
    for c, f in by("flat"):
        assert len({f.sse[i] for i in tested(c)}) == 1
        if job(c).rates == "equal":
            assert f.best == 0 and len(set(f.rd)) == 1
        else:
            rates = I.rate_table("random")
            assert len({f.rd[i] for i in tested(c)}) == 9
            assert f.best == min(range(9), key=lambda i: int(rates[c.ctx[0]][i // 3]) + int(rates[c.ctx[1]][i % 3]))
    assert any(f.best != 0 for c, f in by("flat"))
    assert {job(c).rates for c, _ in by("flat")} == {"equal", "random"}
    # a zero x phase with dual filter on: three groups of three equal SSEs
    zx = [(c, f) for c, f in by("phase") if not c.compound and c.phases[0] == 0 and c.phases[1]]
    assert len(zx) == 14
    for c, f in zx:
        assert all(len(set(f.sse[3 * fy:3 * fy + 3])) == 1 for fy in range(3)) and len({f.sse[0], f.sse[3], f.sse[6]}) == 3
    # the lambda's ends: the distortion decides under the small one, the rate term under the large one
    for c, f in by("lambda"):
        if job(c).lam < 10:
            assert f.best == min(range(9), key=lambda i: (f.sse[i], i)) and len(set(f.sse)) > 1
    large = [f for c, f in by("lambda") if job(c).lam > 1 << 20]        # the rate term (switchable + modelled) outweighs the distortion
    assert len(large) == 8 and sum(f.best != min(range(9), key=lambda i: (f.sse[i], i)) for f in large) >= 4
    # every pair wins somewhere, at both depths
    for bd in (8, 10):
        assert {f.best for c, f in by("winner") if job(c).bd == bd} == set(range(9))
    assert {f.best for f in found} == set(range(9))


def test_mirrors_and_constants():
    for m, size in ((abi.IfsJob, 32), (abi.IfsDesc, 64), (abi.IfsResult, 32), (abi.IfsTrace, 144)):
        end = 0
        for f, _ in m._fields_:
            assert getattr(m, f).offset == end, f"implicit padding before {m.__name__}.{f}"
            end += getattr(m, f).size
        assert end == C.sizeof(m) == size == abi.record_dtype(m).itemsize
    names = ["SVT_HIP_IFS_COMBOS", "SVT_HIP_IFS_FILTER_BANKS", "SVT_HIP_IFS_CONTEXTS", "SVT_HIP_IFS_OK", "SVT_HIP_IFS_BAD_SIZE", "SVT_HIP_IFS_BAD_POINTER",
             "SVT_HIP_IFS_BAD_PHASE", "SVT_HIP_IFS_BAD_CTX", "SVT_HIP_IFS_BAD_COMPOUND", "SVT_HIP_IFS_BAD_WEIGHT"]
    got = header_values(names + ["SVT_HIP_IFS_STATUS(SVT_HIP_ERR_BAD_PARAMETER) == 0x80001005u", "SVT_HIP_IFS_STATUS(SVT_HIP_OK) == 0", "sizeof(SVT_HIP_IFS_STATUS(0))"])
    assert [got[n] for n in names] == [getattr(abi, n[len("SVT_HIP_"):]) for n in names] == [9, 5, 16, 0, 1, 2, 3, 4, 5, 6]
    assert list(got.values())[-3:] == [1, 1, C.sizeof(C.c_size_t)]
    assert abi.ifs_status(abi.SVT_HIP_ERR_BAD_PARAMETER) == 0x80001005 and abi.ifs_status(0) == 0
    assert I.BANKS.shape == (abi.IFS_FILTER_BANKS, 16, 8) and I.rate_table("random").shape == (abi.IFS_CONTEXTS, 3)
    assert len(I.FILTER_SETS) == abi.IFS_COMBOS


def test_prototype_and_not_an_rtcd_leaf():
    assert PROTOTYPES[NAME] == ("c_size_t", ("c_void_p", "c_void_p", "c_void_p", "c_void_p", "c_uint32", "c_void_p"))
    assert abi.load().svt_hip_ifs_search_batch.restype is C.c_size_t
    assert_not_rtcd_leaf(NAME)


_JOB = ("(lambda **kw: abi.IfsJob(**{**dict(d_switchable_rate=0x10000, d_filters=0x20000, full_lambda=100, quantizer=100, bit_depth=8,"
        " enable_dual_filter=1), **kw}))")


def test_refusals_in_a_process_that_never_initialised_the_library():
    """Refused before any device is looked for: a NULL argument, a NULL table in the job, a bit depth that is neither 8 nor 10.  An empty
    batch under a good job is fine on that side of the device question (as svt_hip_subpel_search_batch has it); a good call gets as far
    as SVT_HIP_ERR_NO_DEVICE.  A NULL trace is no error."""
    got = fresh_process(
        "(lambda J, f: (f(None, p, p, p, 1, None), f(C.byref(J()), None, p, p, 1, None), f(C.byref(J()), p, None, p, 1, None),"
        " f(C.byref(J(d_switchable_rate=None)), p, p, p, 1, None), f(C.byref(J(d_filters=None)), p, p, p, 0, None),"
        " f(C.byref(J(bit_depth=9)), p, p, p, 1, None), f(C.byref(J(bit_depth=12)), p, p, p, 1, None), f(C.byref(J(bit_depth=0)), p, p, p, 0, None),"
        " f(C.byref(J()), p, p, p, 0, None), f(C.byref(J(bit_depth=10)), p, p, None, 0, None),"
        " f(C.byref(J()), p, p, p, 1, None), f(C.byref(J(bit_depth=10)), p, p, None, 1, None)))"
        f"({_JOB}, lib.{NAME})")
    bad, none = abi.ifs_status(abi.SVT_HIP_ERR_BAD_PARAMETER), abi.ifs_status(abi.SVT_HIP_ERR_NO_DEVICE)
    assert got == [bad] * 8 + [0, 0] + [none] * 2
    texts = fresh_process  # the texts, each in a process of its own
    for call, text in (("f(None, p, p, p, 1, None)", "svt_hip_ifs_search_batch: NULL argument"),
                       ("f(C.byref(J(d_filters=None)), p, p, p, 1, None)", "svt_hip_ifs_search_batch: NULL table in the job"),
                       ("f(C.byref(J(bit_depth=9)), p, p, p, 1, None)", "svt_hip_ifs_search_batch: bit depth 9 is neither 8 nor 10")):
        assert texts(f"(lambda J, f: ({call}, lib.svt_hip_last_error() == {text.encode()!r}))({_JOB}, lib.{NAME})") == [bad, 1], call


def test_status_exports_returning_size_t_are_probed_here():
    """tests/test_tier_b_refusals.py takes its census from the exports that return int32_t, and the ABI tests of earlier features close the
    sets of the other return types.  svt_hip_ifs_search_batch returns size_t (SVT_HIP_IFS_STATUS: the 32 bits of the SvtHipStatus): every
    svt_hip_* export with that return type is either layout arithmetic, named here, or this one, listed with what the census's own child
    process (its three probes, its marking of the error text) records for it."""
    import test_tier_b_refusals as T
    layout = {"svt_hip_resize_workspace_bytes", "svt_hip_sgr_search_work_bytes", "svt_hip_txt_search_scratch_bytes"}
    bad = abi.ifs_status(abi.SVT_HIP_ERR_BAD_PARAMETER)
    want = {NAME: [[bad, "svt_hip_ifs_search_batch: NULL argument"], [bad, "svt_hip_ifs_search_batch: NULL table in the job"],
                   [bad, "svt_hip_ifs_search_batch: NULL table in the job"]]}
    assert {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_size_t"} == set(want) | layout
    assert not set(want) & set(T.census_names())
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(want)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == want
