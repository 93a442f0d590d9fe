"""CPU: the fixture, the restatement, the host helpers and the interface of reference scaling (include/svt_hip_scale.h):
svt_hip_resize_planes, svt_hip_superres_upscale_planes, svt_hip_convolve_scale_batch, svt_hip_scale_factors, svt_hip_scaled_block_position
and svt_hip_scaled_size.  No compute call reaches a device here: the helpers and the workspace query are arithmetic, and every refusal
comes before the library looks for a device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scale_cases as K
from support import assert_not_rtcd_leaf, fresh_process, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

HELPERS = ("svt_hip_resize_workspace_bytes", "svt_hip_scale_factors", "svt_hip_scaled_block_position", "svt_hip_scaled_size")
DIMS = list(range(1, 301)) + [1920, 3840, 16384]
DENOMS = range(8, 18)
KINDS = [("resize", K.RESIZE, K.restate_resize), ("superres", K.SUPERRES, K.restate_superres), ("scaled", K.SCALED, K.restate_scaled),
         ("scaled", [ch.first for ch in K.CHAINS], K.restate_scaled), ("chain", K.CHAINS, K.restate_chain)]
ALL = [pytest.param(kind, c, f, id=f"{kind}/{c.name}") for kind, cases, f in KINDS for c in cases]


@pytest.fixture(scope="module")
def pin(ref, tmp_path_factory):
    return K.build_pin(tmp_path_factory.mktemp("scale_pin"))


# ---- the restatement is the fixture, the fixture is the reference ------------------------------------------------------------------

@pytest.mark.parametrize("kind,case,restate", ALL)
def test_restatement_equals_the_fixture(kind, case, restate):
    g, key = K.golden(), f"{kind}/{case.name}"
    got = restate(case)
    if "out/" + key in g:
        assert got.dtype == g["out/" + key].dtype and np.array_equal(got, g["out/" + key])
    else:
        assert got.nbytes > K.ARRAY_MAX_BYTES and K.digest(got) == g["sha/" + key].tobytes().hex()


@pytest.mark.parametrize("kind,case,restate", ALL)
def test_fixture_is_the_reference(ref, pin, kind, case, restate):
    got = {"resize": lambda: K.reference_resize(ref, case), "superres": lambda: K.reference_superres(pin, case),
           "scaled": lambda: K.reference_scaled(ref, case), "chain": lambda: K.reference_chain(ref, case)}[kind]()
    store = {}
    K.record(store, "k", got)
    g, key = K.golden(), f"{kind}/{case.name}"
    (name, want), = store.items()
    assert np.array_equal(g[name.replace("k", key, 1)], want)


def test_fixture_holds_the_reference_banks_and_nothing_else(ref, pin):
    g = K.golden()
    banks, half = K.reference_banks(pin)
    assert np.array_equal(g["banks"], banks) and np.array_equal(g["half"], half)
    assert [int(banks[b].sum(axis=1).min()) for b in range(5)] == [128] * 5 == [int(banks[b].sum(axis=1).max()) for b in range(5)]
    keys = {f"{kind}/{c.name}" for kind, cases, _ in KINDS for c in cases}
    assert {k.split("/", 1)[1] for k in g if "/" in k} == keys and set(g) - {"banks", "half"} == {k for k in g if k[:4] in ("out/", "sha/")}


def test_fixture_is_small():
    assert os.path.getsize(K.GOLD) <= K.GOLD_MAX_BYTES == 256 * 1024


# ---- the helpers against the reference ------------------------------------------------------------------------------------------

class RefScaleFactors(C.Structure):      # ScaleFactors (definitions.h:2013)
    _fields_ = [("x_scale_fp", C.c_int32), ("y_scale_fp", C.c_int32), ("x_step_q4", C.c_int32), ("y_step_q4", C.c_int32),
                ("scale_value_x", C.c_void_p), ("scale_value_y", C.c_void_p)]


def lib_scaled_size(lib, dim, denom):
    d = C.c_uint16(dim)
    lib.svt_hip_scaled_size(C.byref(d), denom)
    return d.value


def lib_factors(lib, ow, oh, tw, th):
    sf = abi.ScaleFactors(7, 7, 7, 7)
    lib.svt_hip_scale_factors(ow, oh, tw, th, C.byref(sf))
    return sf


def size_pairs():
    """(other, this): every dimension against its scaled size at every denominator, both ways round, and the ends of the valid range"""
    for dim in DIMS:
        for denom in DENOMS:
            s = K.scaled_size(dim, denom)
            yield dim, s
            yield s, dim
        yield from ((dim, (dim + 1) // 2), (dim, max(1, (dim + 1) // 2 - 1)), (dim, 16 * dim), (dim, 16 * dim + 1))


def test_scaled_size_is_the_references(ref):
    lib = abi.load()
    for dim in DIMS + [65535]:
        for denom in DENOMS:
            d = C.c_uint16(dim)
            ref.calculate_scaled_size_helper(C.byref(d), C.c_uint8(denom))
            assert lib_scaled_size(lib, dim, denom) == d.value == K.scaled_size(dim, denom), (dim, denom)


def test_scaled_size_is_the_restatement():
    lib = abi.load()
    assert all(lib_scaled_size(lib, dim, denom) == K.scaled_size(dim, denom) for dim in DIMS + [65535] for denom in DENOMS)
    assert [lib_scaled_size(lib, 1920, d) for d in (8, 9, 16, 17, 18, 0)] == [1920, 1707, 960, 1440, 1920, 1920]
    assert [lib_scaled_size(lib, 20, 16), lib_scaled_size(lib, 12, 16)] == [16, 12]        # not below min(16, dim)


def test_scale_factors_are_the_references(ref):
    lib, n_invalid = abi.load(), 0
    pairs = list(size_pairs())
    for (ow, tw), (oh, th) in zip(pairs, pairs[7:] + pairs[:7]):
        want = RefScaleFactors(7, 7, 7, 7)
        ref.svt_av1_setup_scale_factors_for_frame(C.byref(want), ow, oh, tw, th)
        got, mine = lib_factors(lib, ow, oh, tw, th), K.scale_factors(ow, oh, tw, th)
        if want.x_scale_fp == abi.SCALE_INVALID:
            n_invalid += 1
            assert mine is None and (got.x_scale_fp, got.y_scale_fp, got.x_step_q4, got.y_step_q4) == (-1, -1, 7, 7) and want.y_scale_fp == -1
        else:
            assert (got.x_scale_fp, got.y_scale_fp, got.x_step_q4, got.y_step_q4) == (want.x_scale_fp, want.y_scale_fp, want.x_step_q4, want.y_step_q4) == mine
    assert 100 < n_invalid < len(pairs) - 1000


def test_scale_factors_are_the_restatement():
    lib = abi.load()
    for ow, oh, tw, th in ((1920, 1080, 1707, 960), (960, 540, 1920, 1080), (300, 200, 150, 100), (300, 200, 149, 100), (10, 10, 160, 160), (10, 10, 161, 160)):
        got, mine = lib_factors(lib, ow, oh, tw, th), K.scale_factors(ow, oh, tw, th)
        assert (got.x_scale_fp, got.y_scale_fp) == ((-1, -1) if mine is None else mine[:2]) and (mine is None or (got.x_step_q4, got.y_step_q4) == mine[2:])
    assert K.scale_factors(1920, 1080, 1920, 1080) == (1 << 14, 1 << 14, 1024, 1024)
    assert [K.scale_factors(ow, 100, tw, 100)[2] for ow, tw in ((2, 32), (100, 200), (9, 8), (4, 3), (200, 100))] == [64, 512, 1152, 1365, 2048]


def lib_position(lib, p):
    ow, oh, tw, th, sb, px, py, mvc, mvr, ssx, ssy = p
    sf, out = lib_factors(lib, ow, oh, tw, th), abi.ScaledPosition()
    lib.svt_hip_scaled_block_position(C.byref(sf), px, py, mvc, mvr, ssx, ssy, ow, oh, sb, C.byref(out))
    return (out.pos_x, out.pos_y, out.subpel_x, out.subpel_y, out.xs, out.ys)


def restated_position(p):
    ow, oh, tw, th, sb, px, py, mvc, mvr, ssx, ssy = p
    return K.scaled_block_position(K.scale_factors(ow, oh, tw, th), px, py, mvc, mvr, ssx, ssy, ow, oh, sb)


def test_block_position_is_the_references(pin):
    lib, sides = abi.load(), set()
    for p in K.position_probes():
        ow, oh, tw, th, sb, px, py, mvc, mvr, ssx, ssy = p
        out = (C.c_int32 * 6)()
        assert pin.pin_subpel_params(ow, oh, tw, th, sb, px, py, mvc, mvr, ssx, ssy, ow, oh, out) == 1
        assert tuple(out) == lib_position(lib, p) == restated_position(p), p
        border = sb * 2 + 32
        sides |= {("left", out[0] == -((border >> ssx) - 8)), ("top", out[1] == -((border >> ssy) - 8)), ("right", out[0] == (ow >> ssx) + 4),
                  ("bottom", out[1] == (oh >> ssy) + 4)}
    assert sides == {(s, hit) for s in ("left", "top", "right", "bottom") for hit in (False, True)}      # each side of the clamp, and inside


def test_block_position_is_the_restatement():
    lib = abi.load()
    assert all(lib_position(lib, p) == restated_position(p) for p in K.position_probes())


# ---- the cases are what the list asks for -----------------------------------------------------------------------------------------

def test_resize_cases_meet_their_conditions():
    """Asserted on the case lists and on traces of the restatement, which the fixture pins to the reference: not measurements of the code
    under test."""
    by = K.RESIZE_BY_NAME
    for d in range(9, 18):
        c = next(c for c in K.RESIZE if c.name.startswith(f"d{d}_131x37"))
        assert (c.dw, c.dh) == (K.scaled_size(131, d), K.scaled_size(37, d))
    wide = K.new_trace()                         # the rows of the width-131 cases, either way round
    for c in K.RESIZE:
        if 131 in (c.sw, c.dw):
            K.resize_line(K.resize_source(c)[:, :c.sw].astype(np.int64), c.dw, c.bd, wide)
    assert {b: len(p) for b, p in wide["phases"].items()} == {b: 64 for b in K.BANK_NAMES} and wide["halve"] == {"symodd"}
    total, per = K.new_trace(), {}
    for c in K.RESIZE:
        per[c.name] = K.new_trace()
        K.restate_resize(c, per[c.name])
        K.restate_resize(c, total)
    assert total["halve"] == {"symodd", "symeven", "symodd_short", "symeven_short"}
    assert per["d16_131x37_10bit"]["halve"] == {"symodd"} and not per["d16_131x37_10bit"]["phases"]           # 131 -> 66, 37 -> 19: halvings only
    assert per["d16_130x38_even"]["halve"] == {"symeven"} and not per["d16_130x38_even"]["phases"]
    assert list(per["up_66x19_to_131x37"]["phases"]) == [1000] and list(per["d17_131x37_12bit"]["phases"]) == [750]
    assert per["halve_then_875_100x9"]["halve"] == {"symeven"} and list(per["halve_then_875_100x9"]["phases"]) == [875]
    for n in ("tiny_5x3_to_4x3", "tiny_7x5_to_13x9"):
        assert per[n]["x1_above_x2"], n
    # 9 -> 7 is the three-part form at its smallest: x1 == x2 == 3, a middle part of one sample between three initial and three end ones
    assert K.interp_plan(9, 7)[2:] == (3, 3) and not per["tiny_9x2_to_7x2"]["x1_above_x2"]
    assert K.interp_plan(5, 4)[2:] == (3, 0) and K.interp_plan(7, 13)[2:] == (6, 5) and K.interp_plan(5, 9)[2:] == (6, 2)
    assert per["tiny_halve_6x5_to_3x3"]["halve"] == {"symeven_short", "symodd_short"}
    assert not any(per[n]["x1_above_x2"] for n in per if n.startswith("d1"))
    big = by["d12_322x98_10bit"]
    assert big.dw > 3 * 64 and big.sh > 4 * 4 * 4                                    # several workgroups in both passes
    assert {(c.bd, c.is16) for c in K.RESIZE} == {(8, 0), (8, 1), (10, 1), (12, 1)} and all(c.sstride > c.sw and c.dstride > c.dw for c in K.RESIZE)
    for bd in (8, 10, 12):                       # the clip acts at both ends: without it the output would leave the range
        assert any(c.kind == "stripes" and c.bd == bd and {0, (1 << bd) - 1} <= set(np.unique(K.restate_resize(c)).tolist()) and
                   _unclipped_range(c) for c in K.RESIZE), bd
    with pytest.raises(AssertionError, match="two halvings"):
        K.resize_line(np.zeros((1, 131), np.int64), 20, 8)
    assert len({(by[n].sw, by[n].sh) for n in K.RESIZE_MIXED}) >= 5 and {by[n].bd for n in K.RESIZE_MIXED} == {8, 10, 12}


def _unclipped_range(c):
    """True when the first pass of the case overshoots both ends of the sample range before the clip"""
    src = K.resize_source(c)[:, :c.sw].astype(np.int64)
    out = K.resize_line(src, c.dw, 30)           # a bit depth of 30: the upper clip cannot act; the lower one still does
    return out.max() > (1 << c.bd) - 1 and (K.resize_line((1 << c.bd) - 1 - src, c.dw, 30).max() > (1 << c.bd) - 1)


def test_superres_cases_meet_their_conditions():
    assert {c.denom for c in K.SUPERRES} == set(range(9, 17)) and {c.sub_x for c in K.SUPERRES} == {0, 1}
    assert {len(c.starts) - 1 for c in K.SUPERRES} == {1, 2, 3} and {(c.bd, c.is16) for c in K.SUPERRES} == {(8, 0), (10, 1)}
    assert all(c.rows == 8 for c in K.SUPERRES)
    below = []
    for c in K.SUPERRES:
        widths = np.diff(np.array(c.starts))
        assert len(widths) == 1 or len(set(widths.tolist())) == len(widths), c.name      # unequal tile columns
        down_w, up_w, end = K.sr_widths(c)
        assert down_w <= end <= c.sstride - 2 * K.SR_MARGIN and up_w < c.dstride
        t = {}
        K.restate_superres(c, t)
        below.append(t["last_below_width"])
    assert any(below) and not all(below)
    assert len({(K.SUPERRES_BY_NAME[n].bd, K.SUPERRES_BY_NAME[n].sub_x, len(K.SUPERRES_BY_NAME[n].starts)) for n in K.SUPERRES_MIXED}) >= 4


def test_scaled_cases_meet_their_conditions():
    cs = K.SCALED
    assert {(c.w, c.h) for c in cs} == set(K.BLOCKS) and {c.xs for c in cs} == {c.ys for c in cs} == set(K.STEPS)
    assert {c.compound for c in cs} == {0, 1, 2, 3} and {c.bd for c in cs} == {8, 10, 12}
    assert {(c.w, c.h, c.compound) for c in cs} >= {(w, h, k) for w, h in K.BLOCKS for k in range(4)}
    assert {t for c in cs for t in (c.tab_x, c.tab_y)} >= set(K.TABLES8) | {"sub_pel_filters_4", "sub_pel_filters_4smooth"}
    assert all((c.tab_x in K.TABLE4.values()) == (c.w <= 4) and (c.tab_y in K.TABLE4.values()) == (c.h <= 4) for c in cs)
    assert sum(c.sx % 64 != 0 and c.sy % 64 != 0 for c in cs) >= len(cs) - 1 and any(c.sx == c.sy == 0 for c in cs)
    assert any(c.xs != 1024 and c.ys == 1024 for c in cs) and not any(c.xs == c.ys == 1024 for c in cs)
    assert {c.taps for c in cs} == {(8, 8), (4, 4), (6, 8)}
    for c in cs:                                 # the rounds are those of get_conv_params for the depth
        assert K.sc_rounds(c) == {(8, False): (3, 11), (10, False): (3, 11), (12, False): (5, 9), (8, True): (3, 7), (10, True): (3, 7),
                                  (12, True): (5, 7)}[(c.bd, bool(c.compound))]
    traces = {}
    for c in cs:
        traces[c.name] = {}
        K.restate_scaled(c, trace=traces[c.name])
    assert traces["fractional_tile_row_128x128"]["second_tile_row_fraction"] != 0
    assert traces["largest_step_128x128"]["im_rows"] == 262 and max(t["im_rows"] for t in traces.values()) == 262
    for ch in K.CHAINS:
        assert ch.first.compound == 1 and ch.second.compound in (2, 3) and (ch.second.xs, ch.second.ys) == (1024, 1024)
        assert (ch.first.w, ch.first.h, ch.first.bd) == (ch.second.w, ch.second.h, ch.second.bd) and ch.second.sx % 64 == ch.second.sy % 64 == 0


# ---- the interface --------------------------------------------------------------------------------------------------------------

MIRRORS = [abi.ResizePlane, abi.SuperresPlane, abi.ConvolveScaleDesc, abi.ScaleFactors, abi.ScaledPosition]


@pytest.mark.parametrize("mirror", MIRRORS, ids=lambda m: m.__name__)
def test_mirror_has_no_implicit_padding(mirror):
    end = 0
    for f, _ in mirror._fields_:
        assert getattr(mirror, f).offset == end, f"implicit padding before {mirror.__name__}.{f}"
        end += getattr(mirror, f).size
    assert end == C.sizeof(mirror)


def test_records_and_constants_are_the_headers():
    want = header_values(["sizeof(SvtHipResizePlane)", "sizeof(SvtHipSuperresPlane)", "sizeof(SvtHipConvolveScaleDesc)", "sizeof(SvtHipScaleFactors)",
                          "sizeof(SvtHipScaledPosition)", "offsetof(SvtHipResizePlane, is_16bit)", "offsetof(SvtHipSuperresPlane, tile_col_start_mi)",
                          "offsetof(SvtHipConvolveScaleDesc, filter_x)", "offsetof(SvtHipConvolveScaleDesc, taps_x)", "offsetof(SvtHipConvolveScaleDesc, cbuf)",
                          "SVT_HIP_SCALE_MAX_PLANES", "SVT_HIP_SCALE_MAX_TILE_COLS", "SVT_HIP_SCALE_INVALID"], ["svt_hip_scale.h"])
    assert list(want.values()) == [48, 168, 96, 16, 24, 40, 38, 32, 64, 80, 24, 64, -1]
    assert [C.sizeof(m) for m in MIRRORS] == list(want.values())[:5]
    assert (abi.SCALE_MAX_PLANES, abi.SCALE_MAX_TILE_COLS, abi.SCALE_INVALID) == tuple(want.values())[10:]
    assert abi.CONVOLVE_SCALE_DESC_DTYPE.itemsize == 96 and abi.CONVOLVE_SCALE_DESC_DTYPE["filter_y"] == np.dtype("<u8")
    for field in ("compound", "fwd_offset", "bck_offset", "cbuf", "cbuf_stride", "dst", "dst_stride", "is_16bit", "bit_depth"):      # what the shared compound
        assert getattr(abi.ConvolveScaleDesc, field).size == getattr(abi.ConvolveDesc, field).size, field                                # epilogue reads
    codes = ("SVT_HIP_OK", "SVT_HIP_ERR_NO_DEVICE", "SVT_HIP_ERR_BAD_PARAMETER", "SVT_HIP_ERR_RUNTIME")
    status = header_values([f"SVT_HIP_SCALE_STATUS({s})" for s in codes] + ["sizeof(SVT_HIP_SCALE_STATUS(0))"])
    assert list(status.values()) == [getattr(abi, s) for s in codes] + [C.sizeof(C.c_ssize_t)]      # the SvtHipStatus whole, negative for an error


def test_new_names_are_exported_with_their_prototypes():
    lib = abi.load()
    for n in K.STATUS_NAMES + HELPERS:
        assert_not_rtcd_leaf(n)
        assert n in PROTOTYPES
    assert PROTOTYPES["svt_hip_resize_workspace_bytes"] == ("c_size_t", ("c_void_p", "c_uint32"))
    assert PROTOTYPES["svt_hip_resize_planes"] == ("c_ssize_t", ("c_void_p", "c_uint32", "c_void_p", "c_size_t", "c_void_p"))
    assert PROTOTYPES["svt_hip_superres_upscale_planes"] == PROTOTYPES["svt_hip_convolve_scale_batch"] == ("c_ssize_t", ("c_void_p", "c_uint32", "c_void_p"))
    assert PROTOTYPES["svt_hip_scale_factors"] == (None, ("c_int32",) * 4 + ("c_void_p",))
    assert PROTOTYPES["svt_hip_scaled_block_position"] == (None, ("c_void_p",) + ("c_int32",) * 4 + ("c_uint32",) * 5 + ("c_void_p",))
    assert PROTOTYPES["svt_hip_scaled_size"] == (None, ("c_void_p", "c_uint8"))
    assert all(getattr(lib, n).restype is C.c_ssize_t for n in K.STATUS_NAMES)
    assert not [n for n in PROTOTYPES if n.endswith("_hip") and ("scale" in n or "resize" in n or "upscale" in n)]        # no Tier A leaf


def test_workspace_query_is_layout_arithmetic():
    f = abi.load().svt_hip_resize_workspace_bytes
    one = lambda sw, sh, dw, dh, is16=0: abi.ResizePlane(1, 1, sw, dw, sw, sh, dw, dh, is16, 8)      # noqa: E731
    arr = lambda *p: (abi.ResizePlane * len(p))(*p)      # noqa: E731
    assert f(None, 3) == 0 and f(arr(one(131, 37, 116, 33)), 0) == 0
    assert f(arr(one(131, 37, 116, 33)), 1) == 116 * 37 // 256 * 256 + 256 and f(arr(one(131, 37, 116, 33, 1)), 1) == (2 * 116 * 37 + 255) // 256 * 256
    assert f(arr(one(131, 37, 116, 37)), 1) == f(arr(one(131, 37, 131, 33)), 1) == f(arr(one(21, 7, 21, 7)), 1) == 0      # one axis, or none
    three = arr(one(131, 37, 116, 33), one(100, 9, 45, 9), one(3840, 2160, 1920, 1080, 1))
    assert f(three, 3) == f(three, 1) + 2 * 1920 * 2160 and f(arr(*[one(16384, 16384, 8192, 8192, 1)] * 24), 24) > 2 ** 32


# ---- refusals -------------------------------------------------------------------------------------------------------------------

FAKE = 0x10000      # never followed: every call below is refused before the library asks for a device


def _resize(**kw):
    f = dict(src=FAKE, dst=2 * FAKE, src_stride=136, dst_stride=120, src_width=131, src_height=37, dst_width=116, dst_height=33, is_16bit=0, bit_depth=8)
    return abi.ResizePlane(**{**f, **kw})


def _superres(starts=(0, 16, 68), **kw):
    f = dict(src=FAKE, dst=2 * FAKE, src_stride=280, dst_stride=304, rows=8, frame_width=267, superres_upscaled_width=300, superres_denominator=9,
             sub_x=0, is_16bit=0, bit_depth=8, tile_cols=len(starts) - 1)
    p = abi.SuperresPlane(**{**f, **kw})
    for i, s in enumerate(starts):
        p.tile_col_start_mi[i] = s
    return p


def test_every_resize_refusal_comes_before_the_device():
    lib = abi.load()
    f, arr = lib.svt_hip_resize_planes, lambda *p: (abi.ResizePlane * len(p))(*p)      # noqa: E731
    need = lib.svt_hip_resize_workspace_bytes(arr(_resize()), 1)
    assert need == 116 * 37 // 256 * 256 + 256
    ws = 3 * FAKE
    calls = {
        "NULL planes": (None, 1, ws, need),
        "25 planes": (arr(*[_resize()] * 25), 25, ws, 25 * need),
        "NULL source": (arr(_resize(src=None)), 1, ws, need),
        "NULL destination": (arr(_resize(dst=None)), 1, ws, need),
        "no width": (arr(_resize(src_width=0)), 1, ws, need),
        "no height": (arr(_resize(src_height=0)), 1, ws, need),
        "no output width": (arr(_resize(dst_width=0)), 1, ws, need),
        "no output height": (arr(_resize(dst_height=0)), 1, ws, need),
        "too wide": (arr(_resize(src_width=16385, src_stride=16385)), 1, ws, 1 << 30),
        "source stride below the width": (arr(_resize(src_stride=130)), 1, ws, need),
        "destination stride below the width": (arr(_resize(dst_stride=115)), 1, ws, need),
        "9 bit": (arr(_resize(bit_depth=9, is_16bit=1)), 1, ws, 2 * need),
        "10 bit in uint8": (arr(_resize(bit_depth=10)), 1, ws, need),
        "is_16bit 2": (arr(_resize(is_16bit=2)), 1, ws, need),
        "two halvings across": (arr(_resize(dst_width=33)), 1, ws, need),
        "two halvings down": (arr(_resize(dst_height=10)), 1, ws, need),
        "second plane bad": (arr(_resize(), _resize(bit_depth=7)), 2, ws, 2 * need),
        "NULL workspace": (arr(_resize()), 1, None, need),
        "misaligned workspace": (arr(_resize()), 1, ws + 64, need),
        "workspace one byte short": (arr(_resize()), 1, ws, need - 1),
        "workspace for one plane of two": (arr(_resize(), _resize()), 2, ws, need),
    }
    for label, args in calls.items():
        assert f(*args, None) == K.BAD_PARAMETER, label
        assert lib.svt_hip_last_error().startswith(b"svt_hip_resize_planes:"), label
    assert f(arr(_resize()), 0, None, 0, None) == 0      # an empty call is fine and launches nothing
    assert f(arr(_resize(dst_width=66)), 1, ws, need, None) == f(arr(_resize(dst_height=37)), 1, None, 0, None) == K.NO_DEVICE      # one halving; no workspace needed


def test_every_superres_refusal_comes_before_the_device():
    lib = abi.load()
    f, arr = lib.svt_hip_superres_upscale_planes, lambda *p: (abi.SuperresPlane * len(p))(*p)      # noqa: E731
    calls = {
        "NULL planes": (None, 1),
        "25 planes": (arr(*[_superres()] * 25), 25),
        "NULL source": (arr(_superres(src=None)), 1),
        "NULL destination": (arr(_superres(dst=None)), 1),
        "no rows": (arr(_superres(rows=0)), 1),
        "no width": (arr(_superres(frame_width=0)), 1),
        "upscaled below the frame": (arr(_superres(superres_upscaled_width=266)), 1),
        "denominator 7": (arr(_superres(superres_denominator=7)), 1),
        "denominator 17": (arr(_superres(superres_denominator=17)), 1),
        "sub_x 2": (arr(_superres(sub_x=2)), 1),
        "9 bit": (arr(_superres(bit_depth=9, is_16bit=1)), 1),
        "12 bit in uint8": (arr(_superres(bit_depth=12)), 1),
        "no tile column": (arr(_superres(tile_cols=0)), 1),
        "65 tile columns": (arr(_superres(tile_cols=65)), 1),
        "first column not at 0": (arr(_superres(starts=(4, 16, 68))), 1),
        "columns not increasing": (arr(_superres(starts=(0, 32, 32, 68))), 1),
        "source stride below the last column's end": (arr(_superres(src_stride=271)), 1),
        "destination stride below the width": (arr(_superres(dst_stride=299)), 1),
        "second plane bad": (arr(_superres(), _superres(rows=0)), 2),
    }
    for label, args in calls.items():
        assert f(*args, None) == K.BAD_PARAMETER, label
        assert lib.svt_hip_last_error().startswith(b"svt_hip_superres_upscale_planes:"), label
    assert f(arr(_superres()), 0, None) == 0
    assert f(arr(_superres()), 1, None) == f(arr(_superres(starts=tuple(range(0, 64)) + (68,))), 1, None) == K.NO_DEVICE      # 2 and 64 columns


def test_descriptor_batch_refusals_and_the_empty_batch():
    lib = abi.load()
    assert lib.svt_hip_convolve_scale_batch(None, 1, None) == K.BAD_PARAMETER
    assert lib.svt_hip_last_error() == b"svt_hip_convolve_scale_batch: NULL argument"
    assert lib.svt_hip_convolve_scale_batch(FAKE, 0, None) == 0 and lib.svt_hip_convolve_scale_batch(FAKE, 1, None) == K.NO_DEVICE


def test_refusals_in_a_process_that_never_initialised_the_library():
    """What the list of the feature names, in a fresh interpreter: refused before any device is looked for; an empty batch is fine; good
    arguments get as far as SVT_HIP_ERR_NO_DEVICE."""
    got = fresh_process(
        "(lambda R, S, rz, sr: ("
        " lib.svt_hip_resize_planes(None, 1, 0x30000, 4352, None), lib.svt_hip_superres_upscale_planes(None, 1, None), lib.svt_hip_convolve_scale_batch(None, 1, None),"
        " lib.svt_hip_resize_planes(R(rz()), 25, 0x30000, 1 << 20, None), lib.svt_hip_superres_upscale_planes(S(sr()), 25, None),"
        " lib.svt_hip_resize_planes(R(rz(src_width=0)), 1, 0x30000, 4352, None), lib.svt_hip_superres_upscale_planes(S(sr(frame_width=0)), 1, None),"
        " lib.svt_hip_resize_planes(R(rz(src_stride=130)), 1, 0x30000, 4352, None), lib.svt_hip_superres_upscale_planes(S(sr(dst_stride=299)), 1, None),"
        " lib.svt_hip_resize_planes(R(rz(bit_depth=9, is_16bit=1)), 1, 0x30000, 8704, None), lib.svt_hip_superres_upscale_planes(S(sr(bit_depth=11, is_16bit=1)), 1, None),"
        " lib.svt_hip_resize_planes(R(rz(dst_width=33)), 1, 0x30000, 4352, None),"
        " lib.svt_hip_superres_upscale_planes(S(sr(tile_cols=0)), 1, None), lib.svt_hip_superres_upscale_planes(S(sr(tile_cols=65)), 1, None),"
        " lib.svt_hip_resize_planes(R(rz()), 1, 0x30000, 4351, None),"
        " lib.svt_hip_resize_planes(R(rz()), 0, None, 0, None), lib.svt_hip_superres_upscale_planes(S(sr()), 0, None), lib.svt_hip_convolve_scale_batch(p, 0, None),"
        " lib.svt_hip_resize_workspace_bytes(R(rz()), 1),"
        " lib.svt_hip_resize_planes(R(rz()), 1, 0x30000, 4352, None), lib.svt_hip_superres_upscale_planes(S(sr()), 1, None), lib.svt_hip_convolve_scale_batch(p, 1, None)))"
        "(lambda j: (abi.ResizePlane * 1)(j), lambda j: (abi.SuperresPlane * 1)(j),"
        " lambda **kw: abi.ResizePlane(**{**dict(src=0x10000, dst=0x20000, src_stride=136, dst_stride=120, src_width=131, src_height=37, dst_width=116,"
        " dst_height=33, is_16bit=0, bit_depth=8), **kw}),"
        " lambda **kw: abi.SuperresPlane(**{**dict(src=0x10000, dst=0x20000, src_stride=280, dst_stride=304, rows=8, frame_width=267, superres_upscaled_width=300,"
        " superres_denominator=9, sub_x=0, is_16bit=0, bit_depth=8, tile_cols=1, tile_col_start_mi=(C.c_uint16 * 65)(0, 68)), **kw}))")
    assert got == [K.BAD_PARAMETER] * 15 + [0, 0, 0, 4352] + [K.NO_DEVICE] * 3


def test_status_exports_returning_intptr_are_probed_here():
    """tests/test_tier_b_refusals.py takes its census from the exports that return int32_t, and the ABI tests of earlier features close
    the sets of the other fixed-width return types.  The three status exports here return intptr_t (SVT_HIP_SCALE_STATUS, the SvtHipStatus
    whole): every svt_hip_* export with that return type is listed with what the census's own child process (its three probes, its marking
    of the error text) records for it, and every probe that is refused names its function before a device is asked for."""
    import test_tier_b_refusals as T
    bad = K.BAD_PARAMETER
    want = {
        "svt_hip_convolve_scale_batch": [[bad, "svt_hip_convolve_scale_batch: NULL argument"], [0, None],
                                         [K.NO_DEVICE, "library not initialised: call svt_hip_init(device_ordinal) first"]],
        "svt_hip_resize_planes": [[bad, "svt_hip_resize_planes: NULL argument"], [0, None],
                                  [bad, "svt_hip_resize_planes: plane 0: NULL plane (0 x 0, stride 0 -> 0 x 0, stride 0, 0 bit)"]],
        "svt_hip_superres_upscale_planes": [[bad, "svt_hip_superres_upscale_planes: NULL argument"], [0, None],
                                            [bad, "svt_hip_superres_upscale_planes: plane 0: NULL plane (frame 0 -> 0, denominator 0, 0 rows, strides 0 and 0, "
                                                  "0 tile columns, 0 bit)"]],
    }
    assert {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_ssize_t"} == set(want) == set(K.STATUS_NAMES)
    assert not set(want) & set(T.census_names())
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(want)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == want
