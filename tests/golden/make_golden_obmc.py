"""TEST INFRASTRUCTURE — writes tests/golden/obmc.npz from the reference (oracle/_ref/libsvtref.so + tests/obmc_pin_driver.c): per case of
obmc_cases.CASES the digests of the wsrc and mask arrays calc_target_weighted_pred leaves on the case's mode-info grid, and what
single_motion_search and the two stage functions it calls leave on those arrays: best_mv, the full-pel vector, the tree's return value,
dis, sse1, rate_mv and the full-pel rounds that moved; sadperbit16 per case; and the limits of obmc_cases.LIMIT_CASES before and after
svt_av1_set_mv_search_range.  No pictures.  A record is stored only once the restatement equals the reference on it, and where
single_motion_search's hard-wired controls are the case's, once the function itself agrees with the stage functions.  Before anything is
written the cases are checked to reach what they are meant to reach (coverage()).  The archive is written with fixed time stamps, so the
same inputs give the same bytes.
    python tests/golden/make_golden_obmc.py"""
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

import obmc_cases as O  # noqa: E402

INT_MIN = -2 ** 31


def coverage(restated):
    """Conditions on the inputs: what the cases must make the two entry points do.  restated: one obmc_cases.Restated per case."""
    events = collections.Counter(e for r in restated for e in r.events)
    for small in (True, False):      # the two kernel instantiations
        mine = [r for r in restated if (r.c.w * r.c.h <= 256) == small]
        assert {(r.c.w, r.c.h) for r in mine} == {s for s in O.SIZES if (s[0] * s[1] <= 256) == small}
        assert {(r.c.full, r.c.frac) for r in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {r.c.diag for r in mine if r.c.full} == {0, 1} and {r.c.approx for r in mine} == {0, 1}
        for rng in (8, 16):
            assert any(("fp_rounds", rng, rng) in r.events for r in mine), (small, rng)
        assert any(r.c.full and r.search.rounds == 0 for r in mine)
    assert len(set(O.SIZES)) == 22
    for side in (0, 1):
        counts = {len(r.segs[side]) for r in restated if (r.c.up, r.c.left)[side]}
        assert counts >= {0, 1, 2, 3, 4}, (side, counts)
    assert {(r.c.up, r.c.left) for r in restated} == {(0, 0), (0, 1), (1, 0), (1, 1)}

    def gaps(segs, n4):
        return sum(n for _, n in segs) < n4 and len(segs) > 0

    def tiles_under(c, side):      # the tiles that lie under the block's edge
        size, inter = O.edge_arrays(*((c.above_tiles, c.above_from, c.mi_cols) if side == 0 else (c.left_tiles, c.left_from, c.mi_rows)))
        pos, n4, limit = ((c.mi_col, c.w // 4, c.mi_cols) if side == 0 else (c.mi_row, c.h // 4, c.mi_rows))
        return size[pos:min(pos + n4, limit)], inter[pos:min(pos + n4, limit)], pos + n4 > limit

    for side in (0, 1):
        on = [r for r in restated if (r.c.up, r.c.left)[side]]
        assert any(gaps(r.segs[side], (r.c.w, r.c.h)[side] // 4) and not tiles_under(r.c, side)[2] for r in on), side      # an intra neighbour
        assert any(tiles_under(r.c, side)[2] for r in on), side                                                         # cut by the picture edge
        # nb_max reached: inter neighbours left over behind the last one visited
        assert any(len(r.segs[side]) == O.MAX_NEIGHBOR_OBMC[((r.c.w, r.c.h)[side] // 4).bit_length() - 1] and
                   sum(n for _, n in r.segs[side]) < (r.c.w, r.c.h)[side] // 4 and tiles_under(r.c, side)[1][-1] for r in on), side
        assert any((tiles_under(r.c, side)[0] == 1).any() and r.segs[side] for r in on), side                           # 4-wide pairs
        assert any(max(r.c.w, r.c.h) == 128 and (r.c.h, r.c.w)[side] == 128 and r.segs[side] for r in on), side         # overlap capped at 32
    ran_tree = [r for r in restated if r.c.frac]
    assert {r.c.hp for r in ran_tree} == {0, 1} and {r.c.stop for r in ran_tree} == {0, 1, 2, 3} and {r.c.iters for r in ran_tree} == {1, 2}
    assert {r.c.taps for r in ran_tree} == {1, 2, 3}
    for key in ([("refused",), ("clamp_moved",), ("second_comparison_fails",), ("beyond",), ("tie",)] + [("second", k) for k in ("kc", "kr", "diag", "third")] +
                [("tree_rounds", k) for k in range(4)] + [("site", j) for j in range(8)]):
        assert events[key] > 0, key
    for small in (True, False):      # the window: a full-pel vector 16 samples from the clamped start under both kernels
        assert any(("fp_reach", 16) in r.events for r in restated if (r.c.w * r.c.h <= 256) == small), small
    return events


def archive(arrays):
    """The bytes of the .npz: deflated .npy members with a fixed time stamp"""
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays:
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(a), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, member.getvalue())
    return out.getvalue()


def pin_case(pin, r):
    """(digests, RESULT_FIELDS, sadperbit16) of the reference on a restated case, after the checks a stored record has to pass"""
    c = r.c
    wsrc, mask = pin.target(c, r.src, r.above, r.left)
    assert (wsrc == r.wsrc).all() and (mask == r.mask).all(), ("target", c)
    out = pin.search(c, r.ref, wsrc, mask)
    got = tuple(out[:9])
    assert got == r.record(), ("search", c, got, r.record())
    if out[9] != INT_MIN:      # single_motion_search itself: x->best_mv and *rate_mv
        assert (out[9], out[10], out[11]) == (got[0], got[1], got[7]), ("single_motion_search", c, out)
    assert out[12] == O.SAD_PER_BIT[c.qindex] and (tuple(out[13:17]), tuple(out[17:21])) == O.case_limits(c), ("set-up", c, out)
    return (O.digest(wsrc), O.digest(mask)), got, out[12], out[9] != INT_MIN


def build(pin, restated=None):
    """The fixture's bytes from the reference, after the restatement has agreed with it on every case and the cases cover their list"""
    restated = restated or [O.Restated(c) for c in O.CASES]
    limits = np.array([sum(pin.limits(lc), ()) for lc in O.LIMIT_CASES], np.int32)
    rows = [pin_case(pin, r) for r in restated]
    coverage(restated)
    assert sum(row[3] for row in rows) * 2 > len(rows)      # most cases go through single_motion_search itself
    return archive((("digests", np.array([row[0] for row in rows], np.uint64)), ("results", np.array([row[1] for row in rows], np.int64)),
                    ("sad_per_bit", np.array([row[2] for row in rows], np.int32)), ("limits", limits)))


def main():
    import pyorc
    with tempfile.TemporaryDirectory() as tmp:
        data = build(O.Pin(pyorc.ref(), tmp))
    with open(O.GOLD, "wb") as f:
        f.write(data)
    print(len(O.CASES), "cases ->", O.GOLD, len(data), "bytes")


if __name__ == "__main__":
    main()
