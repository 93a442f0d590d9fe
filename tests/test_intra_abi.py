"""CPU: the ctypes mirrors of include/svt_hip_intra.h have the compiler's layout, and the golden fixture of the intra search is what
the reference computes (when oracle/_ref/libsvtref.so is built)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from svtav1_hip import abi


def _c_layout(tmp_path, structs):
    """{struct: (sizeof, {field: offsetof})} as gcc lays out the header."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "svt_hip_intra.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        for f in fields:
            lines.append(f'    printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("    return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(abi.REPO_ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(line.rsplit(" ", 1) for line in out.splitlines())


def test_intra_structs_match_header(tmp_path):
    mirrors = {"SvtHipIntraCtrls": abi.IntraCtrls, "SvtHipIntraSearchJob": abi.IntraSearchJob, "SvtHipPlane8": abi.Plane8}
    got = _c_layout(tmp_path, {s: [f for f, _ in m._fields_] for s, m in mirrors.items()})
    for s, m in mirrors.items():
        assert int(got[s]) == C.sizeof(m), s
        for f, _ in m._fields_:
            assert int(got[f"{s}.{f}"]) == getattr(m, f).offset, (s, f)


def test_intra_golden_matches_reference(ref):
    """Every case of the golden fixture, recomputed by the reference's own functions."""
    import intra_cases as I
    gold = np.load(I.GOLD)
    orc = I.RefIntraSearch(ref)
    for i, case in enumerate(I.ALL_CASES):
        I.check_against_golden(gold, case[0], orc.run(I.case_plane(case, i), I.case_ctrls(case), all_modes=case in I.CASES))


def test_intra_golden_covers_every_mode_and_cost_form():
    """The cases reach every mode as a winner somewhere, both cost forms, every pf_shape and blocks that are not searched."""
    import intra_cases as I
    gold = np.load(I.GOLD)
    winners = set()
    for case in I.CASES:
        winners |= set(np.unique(gold[f"{case[0]}_best_mode"]).tolist())
    assert winners >= set(range(abi.INTRA_MODES)) | {I.NOT_SEARCHED}
    assert {c[5] for c in I.CASES} == {0, 1} and {c[6] for c in I.CASES if not c[5]} == {0, 1, 2}
    assert any(c[7] and (c[7], c[8]) != (c[2], c[3]) for c in I.CASES)


@pytest.mark.parametrize("name", ["svt_hip_intra_search_frames"])
def test_intra_export_is_not_an_rtcd_leaf(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf."""
    lib = abi.load()
    assert hasattr(lib, name) and not name.endswith("_hip")
