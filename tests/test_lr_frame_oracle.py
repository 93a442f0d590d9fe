"""CPU: the oracle's frame-level loop restoration (oracle/src/orc_lr_frame.c) against the REAL
svt_av1_loop_restoration_filter_unit + svt_extend_frame run over the same planes (oracle/ref_harness_lr.c), and against the
committed fixture those produced (tests/golden/lr_frame.npz) where the reference build is absent."""
import ctypes as C
import os

import numpy as np
import pytest

import lr_cases as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_frame.npz")


def run(fn, case):
    arr, outs = R.lr_planes(case)
    assert fn(arr, C.c_uint32(len(case))) in (0, None)
    return [o[:c["h"], :c["w"]].copy() for o, c in zip(outs, case)]


@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_equals_reference(orc, ref, name):
    case = R.make_case(name)
    want = run(ref.ref_restoration_filter_frame, case)
    got = run(orc.orc_restoration_filter_frame, case)
    for p, (a, b, c) in enumerate(zip(want, got, case)):
        assert np.array_equal(a, b), (name, p, np.argwhere(a != b)[:5])
        types = set(int(u["restoration_type"]) for u in c["units"])
        assert (a != c["src"]).any() or types == {0}


def test_oracle_equals_golden(orc):
    g = np.load(GOLD)
    for name in R.CASES:
        got = run(orc.orc_restoration_filter_frame, R.make_case(name))
        for p, a in enumerate(got):
            assert np.array_equal(a, g[f"{name}_p{p}"]), (name, p)
    for name, (kind, dims) in R.GOLDEN_CONTENT.items():
        for p, a in enumerate(run(orc.orc_restoration_filter_frame, R.make_content_case(kind, dims))):
            assert np.array_equal(a, g[f"{name}_p{p}"]), (name, p)


# ---- harsh content, fixed unit table (lr_cases.make_content_case)
_content = {}


def content_case(name):
    """The case of one of R.CONTENT_CASES / R.GOLDEN_CONTENT, made once and left unchanged."""
    if name not in _content:
        kind, dims = {**R.CONTENT_CASES, **R.GOLDEN_CONTENT}[name]
        _content[name] = R.make_content_case(kind, dims)
    return _content[name]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_content_conditions(orc, bd):
    """Conditions on the INPUTS of test_frame_content (test_gpu_lr_frame.py), per bit depth, from the inputs and the oracle's
    outputs: the unit tables hold all 16 self-guided sets, Wiener and none, the four corners of xqd and Wiener taps at both
    ends of each range; in the luma plane of `noise` and of `ends` at least 100 samples that the filter changed end at 0 and
    at least 100 at the top value (what it clips there, as far as the output shows it)."""
    top = (1 << bd) - 1
    units = np.concatenate([c["units"] for name, (kind, dims) in R.CONTENT_CASES.items() if dims[2] == bd for c in content_case(name)])
    sgr, wiener = units[units["restoration_type"] == 2], units[units["restoration_type"] == 1]
    assert set(sgr["ep"].tolist()) == set(range(16)) and len(wiener) and (units["restoration_type"] == 0).any()
    both = sgr[sgr["ep"] < 10]
    assert {tuple(x) for x in both["xqd"].tolist()} == set(R.XQD_CORNERS)
    for f in ("hfilter", "vfilter"):
        for tap, (lo, hi) in enumerate(((-5, 10), (-23, 8), (-17, 46))):
            assert {lo, hi} <= set(wiener[f][:, tap].tolist()), (f, tap)
    for kind in ("noise", "ends"):
        for opt in (0, 1):
            case = content_case(f"{kind}_{bd}_opt{opt}")
            out = run(orc.orc_restoration_filter_frame, case)[0]
            ch = out != case[0]["src"]
            assert (ch & (out == 0)).sum() >= 100 and (ch & (out == top)).sum() >= 100, (kind, opt, (ch & (out == 0)).sum(), (ch & (out == top)).sum())


def test_content_conditions_need_the_content(orc):
    """The smooth_plane cases reach neither: no output of theirs is 0, and their tables miss self-guided sets."""
    outs, eps = [], set()
    for name in R.CASES:
        case = R.make_case(name)
        outs += run(orc.orc_restoration_filter_frame, case)
        eps |= {int(u["ep"]) for c in case for u in c["units"] if u["restoration_type"] == 2}
    assert not any((o == 0).any() for o in outs) and eps != set(range(16))


@pytest.mark.parametrize("name", list(R.CONTENT_CASES) + list(R.GOLDEN_CONTENT))
def test_oracle_equals_reference_content(orc, ref, name):
    """The oracle against the reference's svt_av1_loop_restoration_filter_unit on the harsh contents, 12 bit through the same
    frame harness (the reference takes the bit depth as an argument)."""
    case = content_case(name)
    want = run(ref.ref_restoration_filter_frame, case)
    got = run(orc.orc_restoration_filter_frame, case)
    for p, (a, b, c) in enumerate(zip(want, got, case)):
        assert np.array_equal(a, b), (name, p, np.argwhere(a != b)[:5])
        if name.split("_")[0] in ("noise", "ends"):
            assert (a != c["src"]).any()
