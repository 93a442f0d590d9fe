"""GPU: the transform-type search (svt_hip_txt_select_batch, svt_hip_txfm_spatial_distortion_batch, svt_hip_txt_search_batch) against the
Python restatement of tx_type_search's decision (tests/txt_search_cases.py), numpy, the fixture tests/golden/txt_search.npz and the five
public per-candidate calls run one by one.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import rdoq_cases as R
import txt_search_cases as X
from arena import GUARD, PATTERN, Arena, check_containment
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
V = C.c_void_p


@pytest.fixture(scope="module")
def gold():
    return R.Golden()


@pytest.fixture(scope="module")
def fixture():
    return np.load(X.GOLD)


@pytest.fixture(scope="module")
def sets(gold):
    """The select-only inputs with their restated records, made once"""
    return [(s, X.synthetic_expected(gold, s)) for s in X.synthetic_sets(gold)]


@pytest.fixture(scope="module")
def searches(gold, orc):
    """The whole searches of every size with what the oracle's stages and the restated decision make of them, made once"""
    return {s: X.Search(gold, orc, *s) for s in X.SEARCH_SIZES}


def grid_cap(hip):
    """The most workgroups a stage-2 launch takes: 16 per compute unit of the device the test runs on"""
    cus = hip.svt_hip_compute_units()
    assert cus > 0
    return cus * 16


def records(want):
    """decide()'s dictionaries as the record array the device leaves"""
    out = np.zeros(len(want), abi.TXT_RESULT_DTYPE)
    for r, x in zip(out, want):
        for f in X.RESULT_FIELDS:
            r[f] = x[f]
        r["distortion"] = x["distortion"]
    return out


def select(hip, gold, s, descs, mapping, d_base=None, d_tdesc=None):
    """svt_hip_txt_select_batch over the uploaded records of a Synthetic -> records; the guards are checked"""
    up = [device.upload_descriptors(hip, a) for a in (s.results, s.rdoq, s.dist, s.cost)]
    keep = [device.DeviceBuffer(hip, 256), device.upload_descriptors(hip, np.zeros(len(s.cdescs), abi.TXFM_DESC_DTYPE))]
    out, guard = device.txt_select_batch(hip, d_base or keep[0].ptr, descs, d_tdesc or keep[1].ptr, s.cdescs, gold.tables, up[0].ptr, up[1].ptr, up[2].ptr,
                                         up[3].ptr, len(s.cdescs), s.w, s.h, mapping=mapping)
    assert (guard == GUARD).all(), "bytes around d_out were written"
    return out


@pytest.mark.parametrize("mapping", [None, 0, 1])
def test_select_matches_restatement(hip, gold, sets, mapping):
    """Candidate counts 1, 2 and 16 and ragged mixes, 1, 63 and 65 blocks (65 crosses a wavefront), ragged first_cand, small value ranges:
    every field of every record, the two masks among them, with both work splits."""
    for s, want in sets:
        got = select(hip, gold, s, s.descs, mapping)
        bad = [k for k in range(len(want)) if not X.same_record(got[k], want[k])]
        assert not bad, (s.w, s.h, len(want), bad[:5], got[bad[0]], want[bad[0]])


def test_select_without_rdoq_results_and_beyond_the_arrays(hip, gold, sets):
    """d_rdoq_result NULL gives cul_level 0; a block whose candidates start beyond the per-candidate arrays has none, one that runs over
    their end is cut there, a count above 16 is clamped."""
    s, _ = sets[4]
    descs = s.descs.copy()
    descs["first_cand"][3], descs["n_cand"][5], descs["n_cand"][7] = len(s.cdescs) + 5, 200, 16
    descs["first_cand"][7] = len(s.cdescs) - 2
    no_rdoq = s._replace(rdoq=None)
    want = X.synthetic_expected(gold, no_rdoq._replace(descs=descs))
    up = [device.upload_descriptors(hip, a) for a in (s.results, s.dist, s.cost)]
    keep = [device.DeviceBuffer(hip, 256), device.upload_descriptors(hip, np.zeros(len(s.cdescs), abi.TXFM_DESC_DTYPE))]
    got, guard = device.txt_select_batch(hip, keep[0].ptr, descs, keep[1].ptr, s.cdescs, gold.tables, up[0].ptr, None, up[1].ptr, up[2].ptr, len(s.cdescs),
                                         s.w, s.h)
    assert (guard == GUARD).all()
    assert all(X.same_record(g, w) for g, w in zip(got, want))
    assert want[3]["cand"] == abi.TXT_NO_CAND and want[3]["cost"] == X.M64 and not any(w["cul_level"] for w in want)


@pytest.mark.parametrize("mapping", [0, 1])
def test_select_longer_than_one_pass_of_the_grid(hip, gold, sets, mapping):
    """The grid is capped at 16 workgroups per compute unit; a workgroup takes 64 blocks per step when it also copies and 256 when it only
    replays.  A launch this long makes every workgroup come round again.  The blocks of one set repeated (they share its candidates)."""
    s, want = sets[4]
    repeat = grid_cap(hip) * (64 if mapping == 0 else 256) // len(want) + 2
    assert len(want) * repeat > grid_cap(hip) * (64 if mapping == 0 else 256)
    got = select(hip, gold, s, np.tile(s.descs, repeat), mapping)
    assert got.tobytes() == np.tile(records(want), repeat).tobytes()


def coefficient_arrays(S, descs):
    """(offset, bytes) of what a search without the inverse pass may write: the candidates' coefficient arrays and the blocks' destinations"""
    return [(int(d[f]), 4 * S.n) for d in S.tdescs for f in ("coeff_off", "qcoeff_off", "dqcoeff_off")] + \
           [(int(b[f]), 4 * S.n) for b in descs for f in ("dst_qcoeff_off", "dst_dqcoeff_off")]


def pixels(buf, off, rows, stride, w, pix):
    n = np.dtype(pix).itemsize
    return buf[int(off):int(off) + rows * stride * n].view(pix).reshape(rows, stride)[:, :w]


@pytest.mark.parametrize("w, h", [(4, 4), (4, 16), (16, 4), (64, 64)], ids=lambda v: str(v))
def test_spatial_distortion_matches_numpy(hip, w, h):
    """Every crop of 4 x 4, and at the other sizes the whole block and crops that cut the last row, the last column and both; uint8 and uint16
    samples; odd strides and offsets that are no multiple of 4."""
    rng = np.random.default_rng(w * 100 + h)
    crops = [(cw, ch) for cw in range(1, 5) for ch in range(1, 5)] if (w, h) == (4, 4) else [(w, h), (w - 1, h), (w, h - 1), (w - 1, h - 1), (1, h), (w, 1), (0, 0)]
    ab = Arena(fill=PATTERN)
    tdescs, srcs, want = np.zeros(2 * len(crops), abi.TXFM_DESC_DTYPE), np.zeros(2 * len(crops), abi.SPATIAL_SRC_DTYPE), []
    for i in range(len(tdescs)):
        pix16 = i % 2
        pix, (cw, ch) = (np.uint16 if pix16 else np.uint8), crops[i // 2]
        strides = (w + 1 + 2 * (i % 3), w + 3, w + 5)
        arrays = [rng.integers(0, 1024 if pix16 else 256, size=(h, st)).astype(pix) for st in strides]
        offs = [ab.add(f"{name} of candidate {i}", a, skew=np.dtype(pix).itemsize * (1 + i % 5)) for name, a in zip(("pred", "recon", "src"), arrays)]
        d, s = tdescs[i], srcs[i]
        d["pred_off"], d["recon_off"], d["pred_stride"], d["recon_stride"], d["flags"] = offs[0], offs[1], strides[0], strides[1], abi.TX_PIXEL16 * pix16
        s["src_off"], s["src_stride"], s["crop_w"], s["crop_h"] = offs[2], strides[2], cw, ch
        cw, ch = cw or w, ch or h
        src = arrays[2][:ch, :cw].astype(np.int64)
        want.append((int(((src - arrays[1][:ch, :cw]) ** 2).sum()) << 4, int(((src - arrays[0][:ch, :cw]) ** 2).sum()) << 4))
    tdescs["pred_off"][-1] = abi.NO_OFFSET               # a candidate without a prediction gets {0, 0}
    want[-1] = (0, 0)
    arena = ab.build()
    d_arena, d_tdesc = device.DeviceBuffer(hip, arena.nbytes), device.upload_descriptors(hip, tdescs)
    d_arena.upload(arena)
    got, guard = device.spatial_distortion_batch(hip, d_arena.ptr, d_tdesc.ptr, srcs, w, h)
    assert (guard == GUARD).all()
    assert [tuple(int(v) for v in g) for g in got] == want
    check_containment(arena, d_arena.download(np.uint8, (arena.nbytes,)), ab.regions, [], "svt_hip_txfm_spatial_distortion_batch")


def check_search(S, fixture, got_arena, out):
    """The records, the arrays at the destinations and everything else in the arena after a whole search"""
    w, h, n = S.w, S.h, S.n
    for bi, (b, want) in enumerate(zip(S.descs, S.want)):
        assert X.same_record(out[bi], want), (bi, S.cases[bi], out[bi], want)
        assert tuple(int(fixture[f][S.case_index[bi]]) for f in X.FIXTURE_FIELDS) == S.summary(bi), (bi, S.cases[bi])
        win = S.winner(bi)
        if win is None:
            continue
        pix = win["rec"].dtype
        q, dq = (got_arena[int(b[f]):int(b[f]) + 4 * n].view(np.int32) for f in ("dst_qcoeff_off", "dst_dqcoeff_off"))
        assert np.array_equal(q, win["q"]) and np.array_equal(dq, win["dq"]), (bi, S.cases[bi])
        assert np.array_equal(pixels(got_arena, b["dst_recon_off"], h, int(b["dst_recon_stride"]), w, pix), win["rec"]), (bi, S.cases[bi])
    check_containment(S.arena, got_arena, S.regions, S.written, "svt_hip_txt_search_batch")
    for i, c in enumerate(S.cand):             # the candidates' own arrays are what the chain leaves, except where a winner was copied over them
        d = S.tdescs[i]
        if not any(int(b["dst_qcoeff_off"]) == int(d["qcoeff_off"]) and S.winner(bi) is not None for bi, b in enumerate(S.descs)):
            assert np.array_equal(got_arena[int(d["qcoeff_off"]):int(d["qcoeff_off"]) + 4 * n].view(np.int32), c["q"]), i


def run_search(hip, gold, S):
    d_arena = device.DeviceBuffer(hip, S.arena.nbytes + 256)
    d_arena.upload(S.arena)
    out, guard = device.txt_search_batch(hip, d_arena.ptr, S.tdescs, S.rdescs, S.cdescs, gold.tables, S.descs, S.w, S.h, inverse=True)
    assert (guard == GUARD).all(), "bytes around d_out or the scratch were written"
    return d_arena.download(np.uint8, (S.arena.nbytes,)), out


@pytest.mark.parametrize("w, h", X.SEARCH_SIZES, ids=lambda v: str(v))
def test_search_matches_fixture(hip, gold, fixture, searches, w, h):
    """The whole search of every case of the size in one call: the record of every block as restated and as the fixture holds it, the
    winner's qcoeff, dqcoeff and reconstruction at the destinations, nothing written elsewhere."""
    S = searches[(w, h)]
    check_search(S, fixture, *run_search(hip, gold, S))


@pytest.mark.parametrize("w, h", X.SEARCH_SIZES, ids=lambda v: str(v))
def test_search_in_reversed_order(hip, gold, orc, fixture, w, h):
    """The same blocks in reversed order give the same results: no block depends on its place in the batch."""
    S = X.Search(gold, orc, w, h, order=lambda n: range(n - 1, -1, -1))
    check_search(S, fixture, *run_search(hip, gold, S))


@pytest.mark.parametrize("w, h", [(4, 4), (16, 16)], ids=lambda v: str(v))
def test_search_without_the_inverse_pass(hip, gold, searches, w, h):
    """flags = 0: the blocks that measure in the transform domain, without a recon destination.  The same records and coefficient arrays
    as with the pass; no reconstruction is written anywhere."""
    S = searches[(w, h)]
    keep = [bi for bi, c in enumerate(S.cases) if not c.spatial]
    descs = S.descs[keep].copy()
    descs["dst_recon_off"] = abi.NO_OFFSET
    d_arena = device.DeviceBuffer(hip, S.arena.nbytes + 256)
    d_arena.upload(S.arena)
    out, guard = device.txt_search_batch(hip, d_arena.ptr, S.tdescs, S.rdescs, S.cdescs, gold.tables, descs, w, h, inverse=False)
    assert (guard == GUARD).all()
    got = d_arena.download(np.uint8, (S.arena.nbytes,))
    assert 2 <= len(keep) < len(S.cases)
    for k, bi in enumerate(keep):
        assert X.same_record(out[k], S.want[bi]), (bi, S.cases[bi], out[k], S.want[bi])
        win, b = S.winner(bi), descs[k]
        q, dq = (got[int(b[f]):int(b[f]) + 4 * S.n].view(np.int32) for f in ("dst_qcoeff_off", "dst_dqcoeff_off"))
        assert np.array_equal(q, win["q"]) and np.array_equal(dq, win["dq"]), (bi, S.cases[bi])
    check_containment(S.arena, got, S.regions, coefficient_arrays(S, descs), "svt_hip_txt_search_batch without the inverse pass")


@pytest.mark.parametrize("w, h", [(4, 4), (16, 16)], ids=lambda v: str(v))
def test_search_without_the_inverse_pass_ignores_spatial_sse(hip, gold, searches, w, h):
    """flags = 0 over ALL blocks of the size, those with SVT_HIP_TXT_SPATIAL_SSE and recon destinations included: the call has no spatial
    sums and no reconstructions, so every block is decided on the transform-domain distortion, as if the flag were clear, and no
    reconstruction is copied.  Expected: the restated decision, SPATIAL_SSE cleared, on the downloaded outputs of the public per-candidate
    calls; the winner's coefficient arrays at the destinations; nothing else written."""
    S = searches[(w, h)]
    n_cand = len(S.tdescs)
    d_arena, d_fwd = device.DeviceBuffer(hip, S.arena.nbytes + 256), device.upload_descriptors(hip, S.tdescs)
    d_arena.upload(S.arena)
    d_res, d_dist = device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_cand), device.DeviceBuffer(hip, 16 * n_cand)
    device.check(hip, hip.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_res.ptr), n_cand, w, h, None), "svt_hip_txfm_quant_batch")
    rdoq, _ = device.rdoq_batch(hip, d_arena.ptr, d_fwd.ptr, S.rdescs, gold.tables, d_res.ptr, w, h)
    device.check(hip, hip.svt_hip_txfm_distortion_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_dist.ptr), n_cand, w, h, None), "svt_hip_txfm_distortion_batch")
    cost, _ = device.txb_cost_batch(hip, d_arena.ptr, S.cdescs, gold.tables, w, h, d_txfm_result=d_res.ptr, d_distortion=d_dist.ptr)
    dist, results = d_dist.download(np.uint64, (n_cand, 2)), d_res.download(np.dtype(abi.TXFM_RESULT_DTYPE), (n_cand,))
    plain = S.descs.copy()
    plain["flags"] &= ~np.uint8(abi.TXT_SPATIAL_SSE)
    want = [X.decide(gold.tables, w, h, b, S.cdescs, results, rdoq, dist, cost) for b in plain]
    assert any(c.spatial for c in S.cases) and any(want[bi] != S.want[bi] for bi, c in enumerate(S.cases) if c.spatial)
    assert all(want[bi] == S.want[bi] for bi, c in enumerate(S.cases) if not c.spatial)
    d_arena.upload(S.arena)
    out, guard = device.txt_search_batch(hip, d_arena.ptr, S.tdescs, S.rdescs, S.cdescs, gold.tables, S.descs, w, h, inverse=False)
    assert (guard == GUARD).all()
    got = d_arena.download(np.uint8, (S.arena.nbytes,))
    for bi, b in enumerate(S.descs):
        assert X.same_record(out[bi], want[bi]), (bi, S.cases[bi], out[bi], want[bi])
        if want[bi]["cand"] != abi.TXT_NO_CAND:
            win = S.cand[int(b["first_cand"]) + want[bi]["cand"]]
            q, dq = (got[int(b[f]):int(b[f]) + 4 * S.n].view(np.int32) for f in ("dst_qcoeff_off", "dst_dqcoeff_off"))
            assert np.array_equal(q, win["q"]) and np.array_equal(dq, win["dq"]), (bi, S.cases[bi])
    check_containment(S.arena, got, S.regions, coefficient_arrays(S, S.descs), "svt_hip_txt_search_batch without the inverse pass")


@pytest.mark.parametrize("mapping", [0, 1])
def test_copies_in_a_launch_longer_than_one_pass_of_the_grid(hip, gold, searches, mapping):
    """The blocks of the 4 x 4 search repeated until every workgroup comes round again (64 blocks per step where one kernel replays and
    copies, 4 per step in the copying kernel of the two-kernel split), every copy of a block with destinations of its own packed behind the
    arena: the winner's arrays arrive at every one of them, and nothing else changes."""
    S = searches[(4, 4)]
    n, w, h = S.n, S.w, S.h
    arena = S.arena.copy()
    pix = {}
    for d, c in zip(S.tdescs, S.cand):
        arena[int(d["qcoeff_off"]):int(d["qcoeff_off"]) + 4 * n] = c["q"].view(np.uint8)
        arena[int(d["dqcoeff_off"]):int(d["dqcoeff_off"]) + 4 * n] = c["dq"].view(np.uint8)
        pixels(arena, d["recon_off"], h, int(d["recon_stride"]), w, c["rec"].dtype)[:] = c["rec"]
    nb0 = len(S.descs)
    repeat = grid_cap(hip) * (64 if mapping == 0 else 4) // nb0 + 2
    assert nb0 * repeat > grid_cap(hip) * (64 if mapping == 0 else 4)
    per = 8 * n + 2 * w * h                                  # qcoeff, dqcoeff, recon (room for 16-bit samples, pitch w)
    descs = np.tile(S.descs, repeat)
    at = np.uint64(arena.nbytes) + np.arange(len(descs), dtype=np.uint64) * np.uint64(per)
    descs["dst_qcoeff_off"], descs["dst_dqcoeff_off"], descs["dst_recon_off"], descs["dst_recon_stride"] = at, at + np.uint64(4 * n), at + np.uint64(8 * n), w
    big = np.concatenate([arena, np.full(len(descs) * per, 0x3C, np.uint8)])
    d_arena, d_tdesc = device.DeviceBuffer(hip, big.nbytes), device.upload_descriptors(hip, S.tdescs)
    d_arena.upload(big)
    s = X.Synthetic(w, h, descs, S.cdescs, *S.records)
    out = select(hip, gold, s, descs, mapping, d_arena.ptr, d_tdesc.ptr)
    got = d_arena.download(np.uint8, (big.nbytes,))
    assert out.tobytes() == np.tile(records(S.want), repeat).tobytes()
    check_containment(arena, got[:arena.nbytes], S.regions, [], "svt_hip_txt_select_batch")
    one = np.full((nb0, per), 0x3C, np.uint8)
    for bi in range(nb0):
        win = S.winner(bi)
        if win is not None:
            one[bi, :4 * n], one[bi, 4 * n:8 * n] = win["q"].view(np.uint8), win["dq"].view(np.uint8)
            rec = np.ascontiguousarray(win["rec"]).view(np.uint8).reshape(-1)
            one[bi, 8 * n:8 * n + rec.size] = rec
    bad = np.nonzero((got[arena.nbytes:].reshape(repeat, nb0, per) != one[None]).any(axis=2))
    assert bad[0].size == 0, (bad[0][:5], bad[1][:5])


@pytest.mark.parametrize("mapping", [0, 1])
def test_select_copies_the_winner(hip, gold, searches, mapping):
    """Both work splits of svt_hip_txt_select_batch over the restated records of a whole search, the candidates' arrays in place: the
    same records and the same bytes at the destinations."""
    S = searches[(8, 8)]
    arena = S.arena.copy()
    for d, c in zip(S.tdescs, S.cand):
        arena[int(d["qcoeff_off"]):int(d["qcoeff_off"]) + 4 * S.n] = c["q"].view(np.uint8)
        arena[int(d["dqcoeff_off"]):int(d["dqcoeff_off"]) + 4 * S.n] = c["dq"].view(np.uint8)
        pixels(arena, d["recon_off"], S.h, int(d["recon_stride"]), S.w, c["rec"].dtype)[:] = c["rec"]
    d_arena, d_tdesc = device.DeviceBuffer(hip, arena.nbytes), device.upload_descriptors(hip, S.tdescs)
    d_arena.upload(arena)
    s = X.Synthetic(S.w, S.h, S.descs, S.cdescs, *S.records)
    out = select(hip, gold, s, S.descs, mapping, d_arena.ptr, d_tdesc.ptr)
    got = d_arena.download(np.uint8, (arena.nbytes,))
    want_arena = arena.copy()
    for bi, b in enumerate(S.descs):
        assert X.same_record(out[bi], S.want[bi]), bi
        win = S.winner(bi)
        if win is not None:
            want_arena[int(b["dst_qcoeff_off"]):int(b["dst_qcoeff_off"]) + 4 * S.n] = win["q"].view(np.uint8)
            want_arena[int(b["dst_dqcoeff_off"]):int(b["dst_dqcoeff_off"]) + 4 * S.n] = win["dq"].view(np.uint8)
            pixels(want_arena, b["dst_recon_off"], S.h, int(b["dst_recon_stride"]), S.w, win["rec"].dtype)[:] = win["rec"]
    assert np.array_equal(got, want_arena)


@pytest.mark.parametrize("w, h", X.SEARCH_SIZES, ids=lambda v: str(v))
def test_search_equals_the_public_calls_one_by_one(hip, gold, searches, w, h):
    """svt_hip_txfm_quant_batch -> svt_hip_rdoq_batch -> svt_hip_txfm_quant_batch (INV only, its own descriptors and results) ->
    svt_hip_txfm_distortion_batch -> svt_hip_txb_cost_batch, the spatial distortion for the blocks that use it, all downloaded, and the
    restated decision on them: the records svt_hip_txt_search_batch leaves in one call."""
    S = searches[(w, h)]
    n_cand = len(S.tdescs)
    inv = S.tdescs.copy()
    inv["quant_mode"], inv["flags"] = abi.QUANT_NONE, abi.TX_INV | (S.tdescs["flags"] & abi.TX_PIXEL16)
    d_arena, d_fwd, d_inv = device.DeviceBuffer(hip, S.arena.nbytes + 256), device.upload_descriptors(hip, S.tdescs), device.upload_descriptors(hip, inv)
    d_arena.upload(S.arena)
    d_res, d_res_inv, d_dist = (device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_cand), device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_cand),
                                device.DeviceBuffer(hip, 16 * n_cand))
    device.check(hip, hip.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_res.ptr), n_cand, w, h, None), "svt_hip_txfm_quant_batch")
    rdoq, _ = device.rdoq_batch(hip, d_arena.ptr, d_fwd.ptr, S.rdescs, gold.tables, d_res.ptr, w, h)
    device.check(hip, hip.svt_hip_txfm_quant_batch(V(d_arena.ptr), V(d_inv.ptr), V(d_res_inv.ptr), n_cand, w, h, None), "svt_hip_txfm_quant_batch (INV)")
    device.check(hip, hip.svt_hip_txfm_distortion_batch(V(d_arena.ptr), V(d_fwd.ptr), V(d_dist.ptr), n_cand, w, h, None), "svt_hip_txfm_distortion_batch")
    cost, _ = device.txb_cost_batch(hip, d_arena.ptr, S.cdescs, gold.tables, w, h, d_txfm_result=d_res.ptr, d_distortion=d_dist.ptr)
    srcs = np.zeros(n_cand, abi.SPATIAL_SRC_DTYPE)
    dist = d_dist.download(np.uint64, (n_cand, 2))
    for b in S.descs:
        sl = slice(int(b["first_cand"]), int(b["first_cand"]) + int(b["n_cand"]))
        srcs["src_off"][sl], srcs["src_stride"][sl], srcs["crop_w"][sl], srcs["crop_h"][sl] = b["src_off"], b["src_stride"], b["crop_w"], b["crop_h"]
    spatial, _ = device.spatial_distortion_batch(hip, d_arena.ptr, d_fwd.ptr, srcs, w, h)
    for b in S.descs:
        if b["flags"] & abi.TXT_SPATIAL_SSE:
            sl = slice(int(b["first_cand"]), int(b["first_cand"]) + int(b["n_cand"]))
            dist[sl] = spatial[sl]
    results = d_res.download(np.dtype(abi.TXFM_RESULT_DTYPE), (n_cand,))
    want = [X.decide(gold.tables, w, h, b, S.cdescs, results, rdoq, dist, cost) for b in S.descs]
    _, out = run_search(hip, gold, S)
    for bi in range(len(want)):
        assert X.same_record(out[bi], want[bi]), (bi, S.cases[bi], out[bi], want[bi])
        assert want[bi] == S.want[bi], (bi, "the public calls differ from the oracle's stages")
