"""GPU parity: svt_hip_ifs_search_batch (include/svt_hip_inter.h) against the golden fixture of tests/ifs_cases.py, which holds what the
reference's own functions leave on every case (all nine (sse, rd) pairs, the winner, the winner's prediction), and against the Python
restatement.  A call has one job, so the cases run job by job: each job's cases in one guarded arena."""
import ctypes as C
import zlib

import numpy as np
import pytest

import ifs_cases as I
from arena import GUARD
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return I.Golden()


@pytest.fixture(scope="module")
def loaded(hip):
    """{job index: (indices into I.CASES, Loaded)}"""
    out = {}
    for j in range(len(I.JOBS)):
        idx = [i for i, c in enumerate(I.CASES) if c.job == j]
        out[j] = (idx, I.Loaded(hip, [I.CASES[i] for i in idx]))
    assert sum(len(idx) for idx, _ in out.values()) == len(I.CASES)
    return out


@pytest.fixture(scope="module")
def one_by_one(loaded):
    """{job index: (records, traces)} of one call per case, each checked for containment"""
    out = {}
    for j, (idx, ld) in loaded.items():
        recs, trs = [], []
        for k in range(len(idx)):
            r, t, guards = device.ifs_search_batch(ld.lib, ld.job, ld.descs[k:k + 1], fill=GUARD)
            assert (guards == GUARD).all(), (j, k)
            recs.append(r[0]), trs.append(t[0])
        out[j] = (np.array(recs), np.array(trs))
    return out


def test_every_case_equals_the_fixture(loaded, one_by_one, gold):
    """Trace and winner of every case, one call each; then, per job, what the calls left in the arena: every winner's prediction in its
    dst rectangle and not a byte changed elsewhere."""
    seen = 0
    for j, (idx, ld) in loaded.items():
        recs, trs = one_by_one[j]
        ld.after = ld.buf.download(np.uint8, (ld.before.nbytes,))
        I.check_containment(ld.before, ld.after, ld.regions, ld.declared, f"job {I.JOBS[j].name}")
        for k, i in enumerate(idx):
            r, t, c = recs[k], trs[k], I.CASES[i]
            assert r["status"] == abi.IFS_OK and not r["pad_"].any(), (i, c)
            sse, rd, rec, crc = gold.record(i)
            assert I.record_tuple(r, t) == (sse, rd, rec), (i, c)
            assert (int(r["rd"]), int(r["sse"])) == (rd[rec[0]], sse[rec[0]]), (i, c)
            assert zlib.crc32(np.ascontiguousarray(ld.dst(k)).tobytes()) == crc, (i, c)
            seen += 1
        ld.reset()
    assert seen == len(I.CASES)


def test_all_cases_of_a_job_in_one_call(loaded, one_by_one):
    """Every job's list shuffled in one call, then the largest job's list repeated past 32 x 256 descriptors, more than the grid of the
    single-wave kernel holds on a 256-unit device, so workgroups take more than one.  Records and traces as one by one; the same call
    twice gives the same bytes; with a NULL trace the records are the same."""
    for j, (idx, ld) in loaded.items():
        recs, trs = one_by_one[j]
        order = np.random.RandomState(7 + j).permutation(len(idx))
        out, tr, clean = ld.run(ld.descs[order])
        assert clean and out.tobytes() == recs[order].tobytes() and tr.tobytes() == trs[order].tobytes(), I.JOBS[j].name
        again, tr2, clean = ld.run(ld.descs[order])
        assert clean and again.tobytes() == out.tobytes() and tr2.tobytes() == tr.tobytes()
        bare, none, clean = ld.run(ld.descs[order], trace=False)
        assert clean and none is None and bare.tobytes() == out.tobytes()
    j = max(loaded, key=lambda j: len(loaded[j][0]))
    idx, ld = loaded[j]
    recs, trs = one_by_one[j]
    small = np.array([k for k, i in enumerate(idx) if I.CASES[i].w * I.CASES[i].h <= 256])
    many = np.tile(small, -(-(32 * 256 + 1) // len(small)))
    assert len(many) > 32 * 256
    out, tr, clean = ld.run(ld.descs[many])
    assert clean and out.tobytes() == recs[many].tobytes() and tr.tobytes() == trs[many].tobytes()
    large = np.array([k for k, i in enumerate(idx) if I.CASES[i].w * I.CASES[i].h > 256])
    many = np.tile(large, -(-(8 * 256 + 1) // len(large)))      # the four-wave kernel's grid
    out, tr, clean = ld.run(ld.descs[many], trace=False)
    assert clean and out.tobytes() == recs[many].tobytes()


def test_unaligned_pointers_and_odd_strides(hip):
    """src, the references and dst at odd sample addresses, strides that are no multiple of anything, against the restatement"""
    for job in ("main8", "main10"):
        sizes = ((4, 4), (4, 16), (16, 4), (8, 8), (64, 16), (128, 128))
        mine = [c for c in I.CASES if c.job == I.JOB[job] and (c.w, c.h) in sizes]
        cases = [c for c in mine if c.group == "size"] + [c for c in mine if c.group == "phase"][::5]
        assert {(c.w, c.h) for c in cases} == set(sizes) and {bool(c.compound) for c in cases} == {True, False}
        ld = I.Loaded(hip, cases, layout=lambda i: (1 + 2 * (i % 16), 1 + 2 * (i % 5)))
        px = 2 if I.JOBS[I.JOB[job]].bd > 8 else 1
        assert all(int(d[f]) // px % 2 == 1 for d in ld.descs for f in ("src", "ref0", "dst")) and all(int(d["ref0_stride"]) % 2 == 1 for d in ld.descs)
        out, tr, clean = ld.run(ld.descs)
        assert clean
        for k, c in enumerate(cases):
            f = I.search(c)
            assert out[k]["status"] == abi.IFS_OK and I.record_tuple(out[k], tr[k]) == I.found_tuple(f, c)[:3], c
            assert np.array_equal(ld.dst(k), f.pred), c


def test_bad_descriptors_among_good_ones(loaded, one_by_one):
    """A bad descriptor gets its status code, a zeroed record and a zeroed trace, whichever kernel its size would have put it in; it touches
    neither its dst nor its neighbours' records"""
    j = I.JOB["main8"]
    idx, ld = loaded[j]
    recs, trs = one_by_one[j]
    ld.reset()
    picks = [k for k, i in enumerate(idx) if I.CASES[i].group == "size"][:44]
    descs = ld.descs[picks].copy()
    bad = {}

    def spoil(k, status, **fields):
        for f, v in fields.items():
            descs[k][f] = v
        bad[k] = status

    spoil(1, abi.IFS_BAD_SIZE, w=12)
    spoil(2, abi.IFS_BAD_SIZE, w=4, h=64)
    spoil(5, abi.IFS_BAD_SIZE, w=128, h=256)
    spoil(8, abi.IFS_BAD_SIZE, w=0)
    spoil(11, abi.IFS_BAD_POINTER, src=0)
    spoil(14, abi.IFS_BAD_POINTER, ref0=0)
    spoil(17, abi.IFS_BAD_POINTER, ref1=0, compound=2)
    spoil(20, abi.IFS_BAD_PHASE, subpel_x0=16)
    spoil(23, abi.IFS_BAD_PHASE, subpel_y1=255)
    spoil(26, abi.IFS_BAD_CTX, ctx=(16, 0))
    spoil(29, abi.IFS_BAD_CTX, ctx=(3, 200))
    spoil(32, abi.IFS_BAD_COMPOUND, compound=1)
    spoil(35, abi.IFS_BAD_COMPOUND, compound=4)
    spoil(38, abi.IFS_BAD_WEIGHT, compound=3, fwd_offset=9, bck_offset=8)
    spoil(41, abi.IFS_BAD_WEIGHT, compound=3, fwd_offset=0, bck_offset=0)
    assert {I.CASES[idx[picks[k]]].w * I.CASES[idx[picks[k]]].h > 256 for k in bad} == {True, False}
    # a bad descriptor's dst rectangle stays as it was: only the good ones' are declared
    declared, ld.declared = ld.declared, []
    for k in range(len(picks)):
        if k not in bad:
            o, stride = ld.dst_at[picks[k]]
            c = I.CASES[idx[picks[k]]]
            ld.declared += I.rows(o, stride, c.w, c.h)
    try:
        out, tr, clean = ld.run(descs)
    finally:
        ld.declared = declared
    assert clean
    zero, zero_trace = np.zeros((), abi.IFS_RESULT_DTYPE), np.zeros((), abi.IFS_TRACE_DTYPE)
    for k in range(len(picks)):
        if k in bad:
            zero["status"] = bad[k]
            assert out[k].tobytes() == zero.tobytes() and tr[k].tobytes() == zero_trace.tobytes(), (k, out[k])
        else:
            assert out[k].tobytes() == recs[picks[k]].tobytes() and tr[k].tobytes() == trs[picks[k]].tobytes(), k
    ld.reset()


def test_dst_is_what_convolve_batch_writes_for_the_winner(hip, loaded, one_by_one):
    """The winner's prediction in dst, byte for byte what svt_hip_convolve_batch writes on the device for the same references, phases and
    the winner's filters: single reference, plain average and distance-weighted average, at both depths"""
    for job in ("main8", "main10"):
        j = I.JOB[job]
        idx, ld = loaded[j]
        recs, _ = one_by_one[j]
        bd = I.JOBS[j].bd
        px, dt = (2, np.uint16) if bd > 8 else (1, np.uint8)
        picks = [k for k, i in enumerate(idx) if I.CASES[i].group in ("size", "weights")]
        assert {I.CASES[idx[k]].compound for k in picks} == {0, 2, 3}
        out, _, clean = ld.run(ld.descs[picks], trace=False)
        assert clean and out.tobytes() == recs[picks].tobytes()
        outs = device.DeviceBuffer(hip, sum(I.CASES[idx[k]].w * I.CASES[idx[k]].h for k in picks) * (px + 2))
        first, second, at, o = [], [], [], 0
        for n, k in enumerate(picks):
            c, d = I.CASES[idx[k]], ld.descs[k]
            fy, fx = I.FILTER_SETS[int(out[n]["best"])]
            cd = abi.ConvolveDesc(dst=outs.ptr + o, dst_stride=c.w, w=c.w, h=c.h, round_0=3, round_1=7 if c.compound else 11, bit_depth=bd, is_16bit=int(bd > 8),
                                  fwd_offset=c.fwd, bck_offset=c.bck, cbuf=outs.ptr + o + c.w * c.h * px, cbuf_stride=c.w)
            at.append(o)
            o += c.w * c.h * (px + 2)
            for r in range(2 if c.compound else 1):
                e = abi.ConvolveDesc.from_buffer_copy(cd)
                e.src, e.src_stride, sx, sy = int(d[f"ref{r}"]), int(d[f"ref{r}_stride"]), c.phases[2 * r], c.phases[2 * r + 1]
                e.taps_x, e.taps_y = 8 * bool(sx), 8 * bool(sy)
                e.filter_x, e.filter_y = (C.c_int16 * 8)(*map(int, I.BANKS[I.bank_of(fx, c.w)][sx])), (C.c_int16 * 8)(*map(int, I.BANKS[I.bank_of(fy, c.h)][sy]))
                e.compound = (c.compound if r else 1) if c.compound else 0
                (second if r else first).append(e)
        device.convolve_batch(hip, first)
        device.convolve_batch(hip, second)
        raw = outs.download(np.uint8, (outs.nbytes,))
        for n, k in enumerate(picks):
            c = I.CASES[idx[k]]
            want = raw[at[n]:at[n] + c.w * c.h * px].view(dt).reshape(c.h, c.w)
            assert np.array_equal(ld.dst(k), want), c
        ld.reset()


def test_call_level_errors(hip, loaded):
    """NULL job, descriptors or results, a NULL table, a bit depth of 9: SVT_HIP_ERR_BAD_PARAMETER as the size_t the call returns, nothing
    launched; an empty batch is fine and writes nothing"""
    idx, ld = loaded[I.JOB["main8"]]
    d_desc = device.upload_descriptors(hip, ld.descs[:1])
    out = device.Guarded(hip, 32, 64, GUARD)
    f, bad = hip.svt_hip_ifs_search_batch, abi.ifs_status(abi.SVT_HIP_ERR_BAD_PARAMETER)
    assert f(None, d_desc.ptr, out.ptr, None, 1, None) == f(C.byref(ld.job), None, out.ptr, None, 1, None) == f(C.byref(ld.job), d_desc.ptr, None, None, 1, None) == bad
    for field, value in (("d_filters", None), ("d_switchable_rate", None), ("bit_depth", 9)):
        job = abi.IfsJob.from_buffer_copy(ld.job)
        setattr(job, field, value)
        assert f(C.byref(job), d_desc.ptr, out.ptr, None, 1, None) == bad and hip.svt_hip_last_error().startswith(b"svt_hip_ifs_search_batch:")
    assert f(C.byref(ld.job), d_desc.ptr, out.ptr, None, 0, None) == 0
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    rec, guards = out.read(np.uint8)
    assert (rec == GUARD).all() and (guards == GUARD).all()
