"""TEST INFRASTRUCTURE — writes tests/golden/fpel.npz from the reference (oracle/_ref/libsvtref.so + tests/fpel_pin_driver.c): per case
of fpel_cases.CASES the result of the chain of md_full_pel_search calls, and per entry of fpel_cases.WINDOW_CASES the three windows that
md_sq_motion_search derives.  A result is stored only once the restatement equals the reference on it: every stage the restatement
logs is replayed through md_full_pel_search itself (or, under the four cost types that svt_init_mv_cost_params cannot select, through
svt_pme_sad_loop_kernel_c and svt_aom_fp_mv_err_cost), and md_sq_motion_search / md_nsq_motion_search themselves are run wherever the
case's inputs are ones they can be given (see the driver's comment).  Before anything is written the cases are checked to reach what
they are meant to reach (coverage()), on the record of what the reference was asked and answered.  The archive is written with fixed time
stamps, so the same inputs give the same bytes.
    python tests/golden/make_golden_fpel.py"""
import collections
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import fpel_cases as F  # noqa: E402
from subpel_cases import SIZES  # noqa: E402


def coverage(searches):
    """Conditions on the inputs: what the cases must make the search do.  searches: one fpel_cases.Search per case."""
    ev = collections.Counter()
    for s in searches:
        ev.update(s.events)
    for dist in (F.SAD, F.VAR, F.SSD):
        assert {(k[3], k[4]) for k in ev if k[0] == "scan" and k[2] == dist} == set(SIZES) and len(set(SIZES)) == 22, dist
    assert {(k[3], k[4]) for k in ev if k[0] == "scan" and k[1] == "psad"} == set(SIZES)
    ran = [s for s in searches if any(k[0] == "scan" for k in s.events)]
    assert {s.c.cost_type for s in ran if any(k[0] == "scan" and k[1] == "psad" for k in s.events)} == set(range(6))
    assert {s.c.cost_type for s in ran if any(k[0] == "scan" and k[1] == "generic" for k in s.events) and s.c.mode != F.MVP} == set(range(6))
    assert {k[1] for k in ev if k[0] == "psad_width"} >= {7, 8, 9, 15, 16, 17}
    for side in ("left", "right", "top", "bottom"):
        assert ev[("clips", (side,))] > 0, side
    for mode in (F.SQ, F.NSQ, F.PME):
        assert ev[("empty_stage", mode, True)] > 0, mode
    assert ev[("non_full_pel_centre", F.NSQ)] > 0 and ev[("non_full_pel_centre", F.SQ)] > 0 and ev[("non_full_pel_centre", F.MVP)] > 0
    # the level-0 skip removes a position that would otherwise have won
    skipped = [s for s in searches if s.events["lev0_skip"]]
    assert skipped and any(F.Search(s.c, skip_rule=False).record() != s.record() for s in skipped)
    assert ev["gate_open"] > 0 and ev["gate_shut"] > 0 and ev["gate_equal"] > 0
    equal = [s for s in searches if s.events["gate_equal"]]
    assert all(not s.result[4] for s in equal) and any(s.c.sam for s in equal)
    assert {k[1] for k in ev if k[0] == "levels"} == {(bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(8)}
    assert ev["nsq_loses"] > 0 and ev["nsq_ties"] > 0 and ev["nsq_takes"] > 0 and ev["mvc_duplicates"] > 0
    assert max(len(s.c.mvs) for s in searches if s.c.mode == F.NSQ) == 6
    assert {len(s.c.mvs) for s in searches if s.c.mode == F.MVP} == {1, 2, 3, 4}
    assert ev["wrap"] > 0 and ev["table_clamp"] > 0
    for dist in (F.SAD, F.VAR, F.SSD):
        assert ev[("winner_beyond_first_tile", dist)] > 0, dist
    # the tie that tells the scans apart
    a, b = [s for s in searches if s.c.name == "scan_tie"]
    assert a.c.pic == b.c.pic and a.c.cost_type == F.NONE and (a.c.psad, b.c.psad) == (0, 1)
    (ay, ax, _), (by, bx, _) = a.c.pic[2]["at"]
    assert ax < bx and ay > by and a.result[2] == b.result[2] == 0
    assert a.result[:2] == (ay * 8, ax * 8) and b.result[:2] == (by * 8, bx * 8)
    # a tie across tiles, under both scans
    t = {(s.c.dist, s.c.psad): s for s in searches if s.c.name == "tiles" and s.c.mode == F.PME}
    assert len(t) == 4 and all(s.result[2] == 0 for s in t.values()) and t[(F.SAD, 0)].result[:2] != t[(F.SAD, 1)].result[:2]
    for s in t.values():
        assert any(st.span[0] >= 2 * F.TILE and st.span[1] >= 2 * F.TILE for st in s.stages)
    return ev


def archive(results, windows):
    """The bytes of the .npz: deflated .npy members with a fixed time stamp"""
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in (("results", results), ("windows", windows)):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(a), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, member.getvalue())
    return out.getvalue()


def pin_case(pin, c):
    """The restatement's Search of the case after every part of it that the reference can be asked about has agreed"""
    ms, mr, src, ref = F.pin_pictures(c)
    s = F.Search(c, src, ref)
    for k, st in enumerate(s.stages):
        if st.clip and c.cost_type in (F.ENTROPY, F.OPT):      # (not the MVP loop: pinned as a whole below)
            got = pin.stage(c, src, ref, st)
            assert got == st.after, (c.name, k, st, got)
    if c.cost_type not in (F.ENTROPY, F.OPT) and c.mode != F.MVP:
        pin_other_costs(pin, c, s, src, ref)
    whole = pin.function(c, src, ref)
    if whole is not None:
        if c.mode == F.MVP:
            assert whole == (s.result[0], s.result[1], s.result[2], s.result[5]), (c.name, whole, s.result)
        else:
            assert whole[:2] == s.result[:2], (c.name, whole, s.result)
            if c.mode == F.SQ and s.result[4] and s.levels[0].enabled:
                lv, me = s.levels[0], c.mvs[0]
                assert whole[2] == ((me[1] >> 3) + lv.start_x, (me[1] >> 3) + lv.end_x, (me[0] >> 3) + lv.start_y, (me[0] >> 3) + lv.end_y), (c.name, whole)
    return s, whole is not None


def pin_other_costs(pin, c, s, src, ref):
    """MV_COST_L1_* and MV_COST_NONE, which svt_init_mv_cost_params cannot select: the case's twin under MV_COST_ENTROPY is replayed stage
    by stage (clip, scan and distortion do not look at the cost type); every psad stage of the case itself goes through
    svt_pme_sad_loop_kernel_c with the window the restatement clipped; and the vector cost at every stage's corners, centre and winner
    goes through svt_aom_fp_mv_err_cost."""
    entropy = c._replace(cost_type=F.ENTROPY)
    for st in F.Search(entropy, src, ref).stages:
        if st.clip:
            assert pin.stage(entropy, src, ref, st) == st.after, (c.name, "entropy twin", st)
    probe = F.Search.__new__(F.Search)
    probe.c, probe.events = c, collections.Counter()
    probe.mvj, probe.mvrow, probe.mvcol = s.mvj, s.mvrow, s.mvcol
    for st in s.stages:
        dist, mvx, mvy, sx, ex, sy, ey, step, lev0, rng, best = st.args
        if st.psad:
            assert pin.psad(c, src, ref, mvx, mvy, *st.psad, step, best) == st.after, (c.name, "psad", st)
        for px, py in ((sx, sy), (ex, ey), (sx, ey), (0, 0)):
            row, col = F.i16(mvy + py * 8), F.i16(mvx + px * 8)
            assert pin.mv_cost(c, row, col) == probe.mv_cost(row, col), (c.name, row, col)
        assert pin.mv_cost(c, st.after[1], st.after[0]) == probe.mv_cost(st.after[1], st.after[0])


def build(pin):
    """The fixture's bytes from the reference, after the restatement has agreed with it on every case and the cases cover their list"""
    assert pin.pu_table() == F.pu_table()
    searches, rows, whole = [], [], 0
    for c in F.CASES:
        s, w = pin_case(pin, c)
        searches.append(s)
        rows.append(s.record())
        whole += w
    assert whole >= 30, whole
    coverage(searches)
    windows = []
    for level, sam, dist in F.WINDOW_CASES:
        ct = F.sq_level_ctrls(level)
        got = pin.windows(ct, sam, dist)
        want = [tuple(lv[2:]) for lv in F.sq_windows(ct, sam, F.scaled_distance(dist))]
        assert got == want, (level, sam, dist, got, want)
        windows.append(got)
    return archive(np.array(rows, np.int64), np.array(windows, np.int32))


def main():
    import pyorc
    with tempfile.TemporaryDirectory() as tmp:
        data = build(F.Pin(pyorc.ref(), tmp))
    with open(F.GOLD, "wb") as f:
        f.write(data)
    print(len(F.CASES), "cases ->", F.GOLD, len(data), "bytes")


if __name__ == "__main__":
    main()
