"""CPU: the fixture, the restatement and the interface of svt_hip_palette_search_batch, svt_hip_palette_predict_batch and
svt_hip_sc_classify (the luma palette of mode decision and the screen-content decision on the device).  No compute call reaches a device
here: every refusal comes before the library looks for one."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import palette_cases as K
from support import assert_not_rtcd_leaf, build_pin, fresh_process, have_reference_tree, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

MIRRORS = [abi.PaletteRates, abi.PaletteCtrls, abi.PaletteCand, abi.PaletteRecord, abi.PaletteDesc, abi.PalettePredDesc, abi.ScClass]


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    if not have_reference_tree():
        pytest.skip("the reference tree is not present")
    return build_pin(tmp_path_factory.mktemp("palette_pin"), K.DRIVER)


@pytest.fixture(scope="module")
def restated():
    """Every case restated once, with its log: {name: (Result, Counter)}"""
    ysize, ycolor = K.golden_rates()
    out = {}
    for c in K.CASES:
        log = Counter()
        out[c.name] = (K.search(c, K.make_block(c), ysize, ycolor, log), log)
    return out


# ---- the fixture is the reference, the restatement is the fixture -------------------------------------------------------------

@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_restated_search_equals_the_fixture(restated, case):
    res = restated[case.name][0]
    rec, maps = K.golden_record(case.name)
    assert np.array_equal(K.record_bytes(res), rec) and np.array_equal(K.maps_array(case, res), maps)


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_fixture_is_the_reference_search(pin, restated, case):
    """search_palette_luma and the rate functions themselves; under another cap than 50, svt_av1_k_means_dim1_c run by run"""
    blk = K.make_block(case)
    res, ref = restated[case.name][0], K.ref_search(pin, case, blk)
    assert (res.colors, res.cache) == ref[:2]
    if case.max_itr == 50:
        assert K.same_as_reference(res, ref)
    if 2 < res.colors <= 64:
        data = blk[:case.rows, :case.cols].reshape(-1).astype(np.int64)
        lb, ub = int(data.min()), int(data.max())
        for n in range(min(res.colors, 8), 1, -1):
            init = [lb + (2 * i + 1) * (ub - lb) // n // 2 for i in range(n)]
            cen, idx = K.k_means(data, init, case.max_itr, Counter())
            ref_cen, ref_idx = K.ref_k_means(pin, data, init, case.max_itr)
            assert cen == ref_cen and np.array_equal(idx, ref_idx), n


def test_fixture_holds_the_reference_rate_table(pin):
    ysize, ycolor = K.ref_rates(pin)
    assert np.array_equal(ysize, K.golden_rates()[0]) and np.array_equal(ycolor, K.golden_rates()[1])


@pytest.mark.parametrize("plane", K.SC_PLANES, ids=lambda p: p.name)
def test_restated_classifier_equals_the_fixture_and_the_reference(plane, request):
    buf = K.make_sc_plane(plane)
    c1, c2, blocks, cls = K.sc_classify(buf, plane.w, plane.h)
    assert np.array_equal(K.sc_record_bytes(c1, c2, blocks, cls), K.gold()["sc_" + plane.name])
    import pyorc
    if pyorc.have_ref() and have_reference_tree():
        assert cls == K.ref_sc_classes(request.getfixturevalue("pin"), buf, plane.w, plane.h)


def test_cases_are_what_the_list_asks_for(restated):
    """Conditions on the reference's recorded output and on the restatement's log of it (not measurements of the code under test)."""
    logs = {n: log for n, (_, log) in restated.items()}
    n_cands = {c.name: len(K.golden_record(c.name)[1]) for c in K.CASES}
    colors = {c.name: int(K.golden_record(c.name)[0].view(abi.PALETTE_RECORD_DTYPE)[0]["colors"]) for c in K.CASES}
    assert {(c.w, c.h, c.bd) for c in K.CASES} >= {(w, h, bd) for w, h in K.SIZES for bd in (8, 10)} and len(K.SIZES) == 14
    assert [colors[n] for n in ("colors_1", "colors_2", "colors_3", "colors_8", "colors_9", "colors_64", "colors_65")] == [1, 2, 3, 8, 9, 64, 65]
    assert [n_cands[n] for n in ("colors_1", "colors_2", "colors_65", "colors_65_10")] == [0] * 4 and n_cands["colors_64"] > 0 and n_cands["colors_64_10"] > 0
    assert logs["colors_2"]["rejected"] == 2
    for n in ("short_9x13", "short_3x5", "short_cols", "short_rows"):
        c, m = K.CASE[n], K.golden_record(n)[1][0]
        assert (m[:, c.cols:] == m[:, c.cols - 1:c.cols]).all() and (m[c.rows:, :] == m[c.rows - 1:c.rows, :]).all() and len(np.unique(m[:c.rows, :c.cols])) > 1
    assert {c.step for c in K.CASES if n_cands[c.name]} == {1, 2}
    assert [len(restated[n][0].cache) for n in ("colors_3", "cache_1", "cache_16")] == [0, 1, 16]
    assert logs["cache_1"]["snap"] > 0 and logs["cache_16"]["no_snap_at_2"] > 0 and logs["cache_snap_merge"]["dup"] > 0
    assert logs["tie_top"]["tie_top"] > 0 and logs["tie_nearest"]["tie_nearest"] > 0
    assert logs["empties"]["two_empties"] > 0 and logs["empties_10"]["two_empties"] > 0 and logs["empties_10"]["wrap"] > 0
    assert logs["dups"]["dup"] > 0 and any(log["slot_reuse"] for log in logs.values())
    assert max(n_cands.values()) == 12 == n_cands["full_12"] == n_cands["full_12_10"] and n_cands["one_cand"] == 1
    assert logs["itr_1"]["exit_cap"] > 0 and logs["itr_2"]["exit_cap"] > 0 and logs["itr_50"]["exit_cap"] == 0
    assert len({K.golden_record(n)[0].tobytes() for n in ("itr_1", "itr_2", "itr_50")}) == 3
    assert sum(log["exit_worse"] for log in logs.values()) == 0
    sc = {p.name: K.gold()["sc_" + p.name].view(abi.SC_CLASS_DTYPE)[0] for p in K.SC_PLANES}
    assert [list(sc[n]["sc_class"]) for n in ("noise", "text", "ragged")] == [[0] * 4, [1] * 4, [1] * 4] and list(sc["between"]["sc_class"][:2]) == [1, 0]


def test_fixture_is_small():
    assert os.path.getsize(K.GOLD) <= 256 * 1024


# ---- the interface --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", MIRRORS, ids=lambda m: m.__name__)
def test_mirror_has_no_implicit_padding(mirror):
    end = 0
    for f, _ in mirror._fields_:
        assert getattr(mirror, f).offset == end, f"implicit padding before {mirror.__name__}.{f}"
        end += getattr(mirror, f).size
    assert end == C.sizeof(mirror)


def test_records_and_constants_are_the_headers():
    want = header_values(["sizeof(SvtHipPaletteRates)", "sizeof(SvtHipPaletteCtrls)", "sizeof(SvtHipPaletteCand)", "sizeof(SvtHipPaletteRecord)",
                          "sizeof(SvtHipPaletteDesc)", "sizeof(SvtHipPalettePredDesc)", "sizeof(SvtHipScClass)", "offsetof(SvtHipPaletteRecord, cand)",
                          "offsetof(SvtHipPaletteCand, palette_colors)", "offsetof(SvtHipPaletteCand, map_bits)", "offsetof(SvtHipPaletteDesc, above)",
                          "SVT_HIP_PALETTE_MAX_SIZE", "SVT_HIP_PALETTE_MAX_CANDS", "SVT_HIP_PALETTE_DOMINANT", "SVT_HIP_PALETTE_KMEANS"], ["svt_hip_intra.h"])
    assert list(want.values()) == [4 * (49 + 280), 16, 32, 48 + 14 * 32, 80, 40, 24, 48, 4, 28, 48, 8, 14, 0, 1]
    assert [C.sizeof(m) for m in MIRRORS] == list(want.values())[:7]
    assert (abi.PALETTE_MAX_SIZE, abi.PALETTE_MAX_CANDS, abi.PALETTE_DOMINANT, abi.PALETTE_KMEANS) == tuple(want.values())[11:]
    assert abi.PALETTE_RECORD_DTYPE.itemsize == K.RECORD_BYTES == 496 and abi.SC_CLASS_DTYPE.itemsize == 24


def test_new_names_are_exported_with_their_prototypes():
    lib = abi.load()
    for n in K.NAMES:
        assert_not_rtcd_leaf(n)
        assert PROTOTYPES[n][0] == "c_uint64" and getattr(lib, n).restype is C.c_uint64
    status = header_values([f"SVT_HIP_PALETTE_STATUS({s}) == {v}ull" for s, v in (("SVT_HIP_OK", 0), ("SVT_HIP_ERR_NO_DEVICE", 0x80001000),
                                                                                   ("SVT_HIP_ERR_BAD_PARAMETER", 0x80001005), ("SVT_HIP_ERR_RUNTIME", 0x80001001))])
    assert list(status.values()) == [1] * 4
    assert [abi.palette_status(s) for s in (abi.SVT_HIP_OK, abi.SVT_HIP_ERR_NO_DEVICE, abi.SVT_HIP_ERR_BAD_PARAMETER, abi.SVT_HIP_ERR_RUNTIME)] == \
        [0, 0x80001000, 0x80001005, 0x80001001]
    assert PROTOTYPES["svt_hip_palette_search_batch"][1] == ("c_void_p", "c_void_p", "c_uint32", "c_void_p")
    assert PROTOTYPES["svt_hip_palette_predict_batch"][1] == ("c_void_p", "c_uint32", "c_void_p")
    assert PROTOTYPES["svt_hip_sc_classify"][1] == ("c_void_p", "c_uint32", "c_uint32", "c_uint32", "c_void_p", "c_void_p")


# ---- refusals ---------------------------------------------------------------------------------------------------------------

FAKE = 0x10000      # never followed: every call below is refused before the library asks for a device


def _desc(**kw):
    d = abi.PaletteDesc(FAKE, 2 * FAKE, 3 * FAKE, 80, 4, 2, 16, 16, 16, 16, 2, 1)
    d.above[0], d.above[1], d.left[0] = 10, 200, 60
    for k, v in kw.items():
        if k in ("above", "left"):
            getattr(d, k)[:len(v)] = v
        else:
            setattr(d, k, v)
    return d


def test_every_search_refusal_names_its_descriptor():
    lib = abi.load()
    f = lib.svt_hip_palette_search_batch
    ctrls = lambda **kw: C.byref(abi.PaletteCtrls(**{"d_rates": 4 * FAKE, "dominant_color_step": 1, "bit_depth": 8, "max_itr": 50, **kw}))      # noqa: E731
    one = lambda **kw: (abi.PaletteDesc * 1)(_desc(**kw))       # noqa: E731
    calls = {
        "NULL ctrls": (None, one(), 1), "NULL descriptors": (ctrls(), None, 1), "no descriptor": (ctrls(), one(), 0),
        "NULL table": (ctrls(d_rates=None), one(), 1), "misaligned table": (ctrls(d_rates=4 * FAKE + 2), one(), 1),
        "bit depth 12": (ctrls(bit_depth=12), one(), 1), "bit depth 9": (ctrls(bit_depth=9), one(), 1),
        "step 0": (ctrls(dominant_color_step=0), one(), 1), "step 3": (ctrls(dominant_color_step=3), one(), 1),
        "max_itr 0": (ctrls(max_itr=0), one(), 1), "max_itr 51": (ctrls(max_itr=51), one(), 1),
    }
    for label, args in calls.items():
        assert f(*args, None) == K.BAD_PARAMETER, label
        assert lib.svt_hip_last_error().startswith(b"svt_hip_palette_search_batch:"), label
    per_desc = {
        "NULL source": dict(src=None), "NULL record": dict(record=None), "NULL maps": dict(maps=None),
        "width 4": dict(width=4), "width 128": dict(width=128), "height 4": dict(height=4), "width 24": dict(width=24, cols=16),
        "8 x 64": dict(width=8, height=64, rows=8, cols=8), "64 x 8": dict(width=64, height=8, rows=8),
        "no rows": dict(rows=0), "no cols": dict(cols=0), "rows beyond": dict(rows=17), "cols beyond": dict(cols=17),
        "above of 9": dict(above_n=9), "left of 9": dict(left_n=9), "colour beyond 8 bits": dict(left=(256,)),
        "record at 4": dict(record=2 * FAKE + 4), "maps at 2": dict(maps=3 * FAKE + 2), "stride": dict(stride=19),
    }
    for label, kw in per_desc.items():
        assert f(ctrls(), (abi.PaletteDesc * 3)(_desc(), _desc(), _desc(**kw)), 3, None) == K.BAD_PARAMETER, label
        assert lib.svt_hip_last_error().startswith(b"svt_hip_palette_search_batch: descriptor 2:"), (label, lib.svt_hip_last_error())
    assert f(ctrls(bit_depth=10), one(src=FAKE + 1), 1, None) == K.BAD_PARAMETER
    assert lib.svt_hip_last_error() == b"svt_hip_palette_search_batch: descriptor 0: odd uint16 plane"
    assert f(ctrls(), one(rows=17), 1, None) == K.BAD_PARAMETER
    assert lib.svt_hip_last_error() == b"svt_hip_palette_search_batch: descriptor 0: 17 rows, 16 cols of a 16 x 16 block"


def test_predict_and_classify_refusals():
    lib = abi.load()
    for args in ((None, 1), (FAKE, 0)):
        assert lib.svt_hip_palette_predict_batch(*args, None) == K.BAD_PARAMETER
        assert lib.svt_hip_last_error().startswith(b"svt_hip_palette_predict_batch:")
    calls = {"NULL plane": (None, 64, 64, 64, FAKE), "NULL record": (FAKE, 64, 64, 64, None), "no width": (FAKE, 0, 64, 64, FAKE),
             "no height": (FAKE, 64, 0, 64, FAKE), "too wide": (FAKE, 16385, 16, 16385, FAKE), "too many pixels": (FAKE, 8192, 8192, 8192, FAKE),
             "short stride": (FAKE, 64, 64, 63, FAKE), "record at 2": (FAKE, 64, 64, 64, FAKE + 2)}
    for label, args in calls.items():
        assert lib.svt_hip_sc_classify(*args, None) == K.BAD_PARAMETER, label
        assert lib.svt_hip_last_error().startswith(b"svt_hip_sc_classify:"), label


def test_good_arguments_ask_for_the_device():
    """A process that never called svt_hip_init: what passes every check gets as far as SVT_HIP_ERR_NO_DEVICE, nothing is launched."""
    got = fresh_process(
        "(lib.svt_hip_palette_search_batch(C.byref(abi.PaletteCtrls(0x40000, 2, 10, 1)),"
        " (abi.PaletteDesc * 1)(abi.PaletteDesc(0x10000, 0x20000, 0x30000, 80, 4, 2, 64, 16, 9, 33, 0, 0)), 1, None),"
        " lib.svt_hip_palette_predict_batch(0x10000, 3, None), lib.svt_hip_sc_classify(0x10000, 1920, 1080, 1920, 0x20000, None))")
    assert got == [K.NO_DEVICE] * 3


def test_status_exports_returning_uint64_are_probed_here():
    """tests/test_tier_b_refusals.py takes its census from the exports that return int32_t; the other spellings of the status are pinned
    by the ABI tests of their features.  The three exports here return uint64_t (SVT_HIP_PALETTE_STATUS of a SvtHipStatus): every
    svt_hip_* export with that return type is one of them or a size / offset query that takes no pointer, and each is listed with what
    the census's own child process (its three probes, its marking of the error text) records for it."""
    import json
    import subprocess
    import sys

    import test_tier_b_refusals as T
    bad, none = K.BAD_PARAMETER, K.NO_DEVICE
    not_ready = "library not initialised: call svt_hip_init(device_ordinal) first"
    want = {
        "svt_hip_palette_search_batch": [[bad, "svt_hip_palette_search_batch: NULL argument or no descriptor"],
                                         [bad, "svt_hip_palette_search_batch: NULL argument or no descriptor"],
                                         [bad, "svt_hip_palette_search_batch: NULL or misaligned rate table"]],
        "svt_hip_palette_predict_batch": [[bad, "svt_hip_palette_predict_batch: NULL descriptors or none"],
                                          [bad, "svt_hip_palette_predict_batch: NULL descriptors or none"], [none, not_ready]],
        "svt_hip_sc_classify": [[bad, "svt_hip_sc_classify: NULL argument"],
                                [bad, "svt_hip_sc_classify: plane of 0 x 0, 1 .. 16384 each and at most 2^31 / 50 pixels"], [none, not_ready]],
    }
    wide = {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_uint64"}
    assert set(want) == set(K.NAMES) <= wide and all("c_void_p" not in PROTOTYPES[n][1] for n in wide - set(want)), wide
    assert not set(want) & set(T.census_names())
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(want)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == {n: want[n] for n in sorted(want)}
