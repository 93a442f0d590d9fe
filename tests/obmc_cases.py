"""TEST INFRASTRUCTURE — cases, picture generator, toy mode-info grid, Python restatement and descriptor builder for OBMC motion refinement
(svt_hip_obmc_target_batch, svt_hip_obmc_search_batch, svt_hip_obmc_mv_limits; include/svt_hip_inter.h).

One case is one block: its place in a picture of mode-info units, the blocks above and to its left (sizes and inter flags, from which the
restated foreach_overlappable_nb_above / _left derive the neighbour segments), seeded samples, and the controls of single_motion_search
(mode_decision.c:2425-2533).  Everything is generated here from integers, so tests/golden/obmc.npz (written by
tests/golden/make_golden_obmc.py from the reference through tests/obmc_pin_driver.c) holds only records: per case the digests of wsrc and
mask, the limits, sadperbit16 and the search's result.  tests/test_obmc_abi.py pins fixture and restatement to the reference wherever
oracle/_ref/libsvtref.so has been built."""
import collections
import ctypes as C
import hashlib
import os

import numpy as np

import md_search_cases
from md_search_cases import MAX_FULL_PEL_VAL, MV_LOW, MV_UPP, SIZES, i16, mv_cost_tables  # noqa: F401  (the tests read them from here)
from subpel_cases import FILTERS
from svtav1_hip import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "obmc.npz")
INT_MAX = 2 ** 31 - 1
BORDER = 40       # samples around the block in a generated reference picture: 16 (range) + 8 (window) + a start up to 12 samples away + slack
MAX_NEIGHBOR_OBMC = (0, 1, 2, 3, 4, 4)      # enc_inter_prediction.c:679, by log2 of the side in mode-info units
RESULT_FIELDS = ("best_row", "best_col", "fullpel_row", "fullpel_col", "besterr", "distortion", "sse", "rate_mv", "fullpel_rounds")
# svt_av1_get_obmc_mask (the AV1 specification's Obmc_Mask_*)
RAMPS = {1: (64,), 2: (45, 64), 4: (39, 50, 59, 64), 8: (36, 42, 48, 53, 57, 61, 64, 64),
         16: (34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64),
         32: (33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64)}
# svt_aom_get_sad_per_bit(qindex, 0) at the quantiser indices the cases use (the fixture holds what the reference returned)
SAD_PER_BIT = {20: 2, 100: 3, 180: 7, 255: 21}
SITES = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, 1), (1, 1), (1, -1), (-1, -1))      # obmc_refining_search_sad

Case = collections.namedtuple("Case", "group w h mi_row mi_col mi_rows mi_cols up left above_tiles above_from left_tiles left_from start ref_mv true_mv "
                                      "full frac fp_range diag qindex full_lambda approx hp taps stop iters kind noise seed")


# ---- the toy mode-info grid and the restated neighbour walk ----------------------------------------------------------------------
def edge_arrays(tiles, start, n):
    """Per mode-info position 0 .. n of a picture row (or column): the side of the block covering it, in mode-info units, and its inter flag.
    tiles: [(side, inter), ...] laid out from position `start`; everything else is a 4 x 4 intra block."""
    size, inter, p = np.ones(n, np.uint8), np.zeros(n, np.uint8), start
    for side, flag in tiles:
        size[max(p, 0):p + side], inter[max(p, 0):p + side] = side, flag
        p += side
    return size, inter


def overlappable(pos, n4, limit, size, inter):
    """foreach_overlappable_nb_above / _left (enc_inter_prediction.c:684-752) -> [(rel_mi, mi_len), ...]: the visitor's calls"""
    out, p, end = [], pos, min(pos + n4, limit)
    nb_max = MAX_NEIGHBOR_OBMC[n4.bit_length() - 1]
    while p < end and len(out) < nb_max:
        step, q = min(int(size[p]), 16), p
        if step == 1:            # half of a pair of 4-wide blocks: the pair's second block carries the information
            p &= ~1
            q, step = p + 1, 2
        if inter[q]:
            out.append((p - pos, min(n4, step)))
        p += step
    return out


def segments(c):
    """(above, left): the neighbour lists of a case as the walk gives them; [] on a side that is not available"""
    a_size, a_inter = edge_arrays(c.above_tiles, c.above_from, c.mi_cols)
    l_size, l_inter = edge_arrays(c.left_tiles, c.left_from, c.mi_rows)
    above = overlappable(c.mi_col, c.w // 4, c.mi_cols, a_size, a_inter) if c.up else []
    left = overlappable(c.mi_row, c.h // 4, c.mi_rows, l_size, l_inter) if c.left else []
    return above, left


# ---- generated inputs -----------------------------------------------------------------------------------------------------------
def pictures(c):
    """ref: uint8 [(h + 2 BORDER)][(w + 2 BORDER)] with the block at (BORDER, BORDER); src, above, left: uint8 [h][w].  A coarse random grid is
    interpolated in integers; ref samples it at the sample positions, src at the block's positions moved by true_mv (1/8 units), so that
    src(y, x) ~ ref(y + row / 8, x + col / 8); the neighbour predictions are the source with an error of their own."""
    rs = np.random.RandomState(c.seed)
    H, W, M = c.h + 2 * BORDER, c.w + 2 * BORDER, 40
    if c.kind == "flat":
        ref = np.full((H, W), 97, np.int64)
        src = np.full((c.h, c.w), 101, np.int64) + rs.randint(0, 4, (c.h, c.w))
    else:
        cell = {"smooth": 28, "busy": 7}[c.kind]
        step = cell * 8
        grid = rs.randint(16, 240, (((H + 2 * M) * 8) // step + 3, ((W + 2 * M) * 8) // step + 3)).astype(np.int64)

        def sample(ys, xs):
            a, u, b, v = ys // step, ys % step, xs // step, xs % step
            top = grid[a][:, b] * (step - v) + grid[a][:, b + 1] * v
            bot = grid[a + 1][:, b] * (step - v) + grid[a + 1][:, b + 1] * v
            return (top * (step - u)[:, None] + bot * u[:, None] + step * step // 2) // (step * step)

        ref = sample((np.arange(H) + M) * 8, (np.arange(W) + M) * 8)
        src = sample((np.arange(c.h) + M + BORDER) * 8 + c.true_mv[0], (np.arange(c.w) + M + BORDER) * 8 + c.true_mv[1])
        if c.noise:
            ref = ref + rs.randint(-c.noise, c.noise + 1, (H, W))
            src = src + rs.randint(-c.noise, c.noise + 1, (c.h, c.w))
    above = src + rs.randint(-14, 15, (c.h, c.w))
    left = src + rs.randint(-14, 15, (c.h, c.w))
    return tuple(np.clip(p, 0, 255).astype(np.uint8) for p in (ref, src, above, left))


def digest(a):
    """64 bits of an int32 array's content"""
    return int.from_bytes(hashlib.sha256(np.ascontiguousarray(a, "<i4").tobytes()).digest()[:8], "little")


# ---- restatement ----------------------------------------------------------------------------------------------------------------
def target(c, src, above, left, segs=None):
    """calc_target_weighted_pred (enc_inter_prediction.c:1767-1827) with its two visitors -> (wsrc, mask), int64 [h][w]"""
    seg_above, seg_left = segs if segs is not None else segments(c)
    src, above, left = src.astype(np.int64), above.astype(np.int64), left.astype(np.int64)
    wsrc, mask = np.zeros((c.h, c.w), np.int64), np.full((c.h, c.w), 64, np.int64)
    if c.up:
        ov = min(c.h, 64) >> 1
        m0 = np.array(RAMPS[ov], np.int64)[:, None]
        for rel, n in seg_above:
            cols = slice(rel * 4, (rel + n) * 4)
            wsrc[:ov, cols] = (64 - m0) * above[:ov, cols]
            mask[:ov, cols] = m0
    wsrc, mask = wsrc * 64, mask * 64
    if c.left:
        ov = min(c.w, 64) >> 1
        m0 = np.array(RAMPS[ov], np.int64)[None, :]
        for rel, n in seg_left:
            rows = slice(rel * 4, (rel + n) * 4)
            wsrc[rows, :ov] = (wsrc[rows, :ov] >> 6) * m0 + (left[rows, :ov] << 6) * (64 - m0)
            mask[rows, :ov] = (mask[rows, :ov] >> 6) * m0
    return src * 4096 - wsrc, mask


def mv_limits(mi_row, mi_col, mi_w, mi_h, mi_rows, mi_cols, ref_mv):
    """mode_decision.c:2459-2462 and svt_av1_set_mv_search_range -> (raw, fp): (col_min, col_max, row_min, row_max) each, full-pel"""
    raw = md_search_cases.block_mv_limits(mi_row, mi_col, mi_w, mi_h, mi_rows, mi_cols)
    return raw, md_search_cases.set_mv_search_range(raw, ref_mv)


def case_limits(c):
    return mv_limits(c.mi_row, c.mi_col, c.w // 4, c.h // 4, c.mi_rows, c.mi_cols, c.ref_mv)


class Search:
    """single_motion_search on a case.  After run(): best, fullpel (row, col), besterr, distortion, sse, rate_mv, rounds, and `events`, the set
    of things the coverage conditions of the golden script name."""

    def __init__(self, c, ref, wsrc, mask, tables=None):
        self.c, self.ref = c, ref.astype(np.int64)
        self.wsrc, self.mask = wsrc.astype(np.int64), mask.astype(np.int64)
        self.mvj, self.mvrow, self.mvcol = tables or mv_cost_tables()
        self.raw, self.fp = case_limits(c)
        self.sad_per_bit = SAD_PER_BIT[c.qindex]
        self.epb = max(c.full_lambda >> 6, 1)      # RD_EPB_SHIFT; errorperbit += (errorperbit == 0)
        self.events = set()
        self.run()

    def rate(self, dr, dc):
        """svt_mv_cost of a difference stored in an MV"""
        dr, dc = i16(dr), i16(dc)
        joint = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
        return int(self.mvj[joint]) + int(self.mvrow[min(max(dr, MV_LOW), MV_UPP) - MV_LOW]) + int(self.mvcol[min(max(dc, MV_LOW), MV_UPP) - MV_LOW])

    # mvsad_err_cost / mvsad_err_cost_light (av1me.c:237-261)
    def mvsad_cost(self, mv):
        dr, dc = mv[0] - (self.c.ref_mv[0] >> 3), mv[1] - (self.c.ref_mv[1] >> 3)
        if self.c.approx:
            return 1296 + 50 * (abs(dc) * 8 + abs(dr) * 8)
        return (((self.rate(dr * 8, dc * 8) & 0xFFFFFFFF) * self.sad_per_bit + 256) & 0xFFFFFFFF) >> 9

    # svt_aom_mv_err_cost / svt_aom_mv_err_cost_light (av1me.c:229-252)
    def mv_cost(self, mv):
        dr, dc = i16(mv[0]) - self.c.ref_mv[0], i16(mv[1]) - self.c.ref_mv[1]
        if self.c.approx:
            return 1296 + 50 * (abs(dc) + abs(dr))
        return (self.rate(dr, dc) * self.epb + (1 << 13)) >> 14

    # svt_aom_obmc_sad* (sad_av1.c:18-32)
    def sad(self, mv):
        c = self.c
        y, x = BORDER + mv[0], BORDER + mv[1]
        self.events.add(("fp_reach", max(abs(mv[0] - self.fp_start[0]), abs(mv[1] - self.fp_start[1]))))
        pre = self.ref[y:y + c.h, x:x + c.w]
        return int(((np.abs(self.wsrc - pre * self.mask) + 2048) >> 12).sum())

    # upsampled_obmc_pref_error: svt_aom_upsampled_pred_c, then svt_aom_obmc_variance* (variance.c:347-373)
    def variance(self, mv):
        c, table = self.c, c_table(self.c)
        y, x = BORDER + (mv[0] >> 3), BORDER + (mv[1] >> 3)
        fx, fy = FILTERS[table][mv[1] & 7], FILTERS[table][mv[0] & 7]
        r = self.ref[y - 3:y + c.h + 4, x - 3:x + c.w + 4]
        tmp = sum(int(fx[k]) * r[:, k:k + c.w] for k in range(8))
        tmp = np.clip((tmp + 64) >> 7, 0, 255)
        pred = sum(int(fy[k]) * tmp[k:k + c.h] for k in range(8))
        pred = np.clip((pred + 64) >> 7, 0, 255)
        v = self.wsrc - pred * self.mask
        diff = np.where(v < 0, -((-v + 2048) >> 12), (v + 2048) >> 12)
        s, sse = int(diff.sum()), int((diff * diff).sum()) & 0xFFFFFFFF
        return (sse - ((s * s) // (c.w * c.h) & 0xFFFFFFFF)) & 0xFFFFFFFF, sse

    def full_pel(self, mv):
        """svt_av1_obmc_full_pixel_search behind its set-up (av1me.c:721-776) -> (vector, rounds that moved)"""
        c, (lo_c, hi_c, lo_r, hi_r) = self.c, self.fp
        clamped = (min(max(mv[0], lo_r), hi_r), min(max(mv[1], lo_c), hi_c))
        if clamped != mv:
            self.events.add(("clamp_moved",))
        mv = self.fp_start = clamped
        best_sad = (self.sad(mv) + self.mvsad_cost(mv)) & 0xFFFFFFFF
        rounds = 0
        for _ in range(c.fp_range):
            best_site = -1
            for j in range(8 if c.diag else 4):
                cand = (mv[0] + SITES[j][0], mv[1] + SITES[j][1])
                if not (lo_c <= cand[1] <= hi_c and lo_r <= cand[0] <= hi_r):      # is_mv_in
                    self.events.add(("refused",))
                    continue
                sad = self.sad(cand)
                if sad < best_sad:
                    sad = (sad + self.mvsad_cost(cand)) & 0xFFFFFFFF
                    if sad < best_sad:
                        best_sad, best_site = sad, j
                    else:
                        self.events.add(("second_comparison_fails",))
                        if sad == best_sad:
                            self.events.add(("tie",))
                elif sad == best_sad:
                    self.events.add(("tie",))
            if best_site < 0:
                break
            mv, rounds = (mv[0] + SITES[best_site][0], mv[1] + SITES[best_site][1]), rounds + 1
            self.events.add(("site", best_site))
        self.events.add(("fp_rounds", c.fp_range, rounds))
        return mv, rounds

    def check(self, r, c):
        """The body of CHECK_BETTER1 and of the tree's own checks -> (cost, won)"""
        minc, maxc, minr, maxr = self.sub
        if not (minc <= c <= maxc and minr <= r <= maxr):
            self.events.add(("beyond",))
            return INT_MAX, False
        var, sse = self.variance((r, c))
        cost = (var + self.mv_cost((r, c))) & 0xFFFFFFFF
        if cost == self.besterr:
            self.events.add(("tie",))
        if cost < self.besterr:
            self.besterr, self.distortion, self.sse = cost, var, sse
            return cost, True
        return cost, False

    def tree(self, br, bc):
        """svt_av1_find_best_obmc_sub_pixel_tree_up (av1me.c:963-1132), accurate path -> (br, bc)"""
        c = self.c
        self.sub = md_search_cases.set_subpel_mv_search_range(self.raw, c.ref_mv)      # on the limits before the full-pel narrowing
        rounds = 3 - c.stop
        if not c.hp and rounds == 3:
            rounds = 2
        self.events.add(("tree_rounds", rounds))
        var, self.sse = self.variance((br, bc))
        self.distortion, self.besterr = var, (var + self.mv_cost((br, bc))) & 0xFFFFFFFF
        hstep = 4
        for _ in range(rounds):
            steps = ((0, -hstep), (0, hstep), (-hstep, 0), (hstep, 0))
            cost, best_idx = [], -1
            for idx, (dr, dc) in enumerate(steps):
                v, won = self.check(br + dr, bc + dc)
                cost.append(v)
                if won:
                    best_idx = idx
            kc, kr = (-hstep if cost[0] <= cost[1] else hstep), (-hstep if cost[2] <= cost[3] else hstep)
            tc, tr = bc + kc, br + kr
            if self.check(tr, tc)[1]:
                best_idx = 4
            if best_idx == 4:
                br, bc = tr, tc
            elif best_idx >= 0:
                br, bc = br + steps[best_idx][0], bc + steps[best_idx][1]
            if c.iters > 1 and best_idx != -1:      # SECOND_LEVEL_CHECKS_BEST
                br0, bc0 = br, bc
                assert tr == br or tc == bc
                if tr == br and tc != bc:
                    kc = bc - tc
                    self.events.add(("second", "kc"))
                elif tr != br and tc == bc:
                    kr = br - tr
                    self.events.add(("second", "kr"))
                else:
                    self.events.add(("second", "diag"))
                if self.check(br0 + kr, bc0)[1]:
                    br, bc = br0 + kr, bc0
                if self.check(br0, bc0 + kc)[1]:
                    br, bc = br0, bc0 + kc
                if (br0, bc0) != (br, bc):
                    self.events.add(("second", "third"))
                    if self.check(br0 + kr, bc0 + kc)[1]:
                        br, bc = br0 + kr, bc0 + kc
            hstep >>= 1
        return br, bc

    def run(self):
        c = self.c
        mv = self.fp_start = (c.start[0] >> 3, c.start[1] >> 3)
        self.rounds, self.besterr, self.distortion, self.sse = 0, 0, 0, 0
        if c.full:
            mv, self.rounds = self.full_pel(mv)
        self.fullpel = mv
        self.best = self.tree(mv[0] * 8, mv[1] * 8) if c.frac else (mv[0] * 8, mv[1] * 8)
        dr, dc = i16(self.best[0]) - c.ref_mv[0], i16(self.best[1]) - c.ref_mv[1]
        if c.approx:      # svt_av1_mv_bit_cost_light / svt_av1_mv_bit_cost with MV_COST_WEIGHT (rd_cost.c:67-87)
            self.rate_mv = 1296 + 50 * (abs(dc) + abs(dr))
        else:
            self.rate_mv = (self.rate(dr, dc) * 108 + 64) >> 7

    def record(self):
        """RESULT_FIELDS; besterr and distortion as the int the function returns / stores"""
        s32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v   # noqa: E731
        return (self.best[0], self.best[1], self.fullpel[0], self.fullpel[1], s32(self.besterr), s32(self.distortion), self.sse, self.rate_mv, self.rounds)


def c_table(c):
    return c.taps - abi.SUBPEL_USE_2_TAPS


class Restated:
    """Both entry points on a case, from its generated samples"""

    def __init__(self, c):
        self.c = c
        self.ref, self.src, self.above, self.left = pictures(c)
        self.segs = segments(c)
        self.wsrc, self.mask = target(c, self.src, self.above, self.left, self.segs)
        self.search = Search(c, self.ref, self.wsrc, self.mask)
        self.events = self.search.events

    def digests(self):
        return digest(self.wsrc), digest(self.mask)

    def record(self):
        return self.search.record()


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _tiles(n4, pattern):
    """(tiles, offset of the first tile from the block's edge position) along one side of a block of n4 mode-info units"""
    if pattern == "one":           # one neighbour as long as the block
        return [(n4, 1)], 0
    if pattern == "none":          # all intra
        return [(n4, 0)], 0
    if pattern == "twos":          # 8-sample neighbours: more than nb_max of them from 32 samples on
        return [(2, 1)] * max(n4 // 2, 1), 0
    if pattern == "gaps":          # inter, intra, inter, ... of a quarter of the side each
        q = max(n4 // 4, 1)
        return [(q, k % 2 == 0) for k in range(max(n4 // q, 1))], 0
    if pattern == "pairs":         # pairs of 4-wide blocks: the second of a pair decides
        return [(1, k % 4 in (1, 2)) for k in range(max(n4, 2))], 0
    if pattern == "larger":        # a neighbour larger than the block that starts before it
        return [(min(2 * n4, 32), 1)], -(n4 if 2 * n4 <= 32 else 0)
    if pattern == "halves":
        return [(max(n4 // 2, 1), 1)] * 2, 0
    if pattern == "three":         # three inter neighbours and an intra one
        q = max(n4 // 4, 1)
        return [(q, 1), (q, 0), (q, 1), (q, 1)], 0
    raise ValueError(pattern)


PATTERNS = ("one", "twos", "gaps", "pairs", "larger", "halves", "three", "none")


def _cases():
    out = []

    def add(group, w, h, ta="one", tl="one", **kw):      # ta, tl: the patterns of the tiles above and to the left
        i = len(out)
        d = dict(mi_row=32, mi_col=32, mi_rows=128, mi_cols=128, up=1, left=1, start=(8 * (i % 5 - 2), 8 * ((i // 5) % 5 - 2)), ref_mv=None, true_mv=None,
                 full=1, frac=1, fp_range=(8, 16)[i % 2], diag=(i // 2) % 2, qindex=(20, 100, 180, 255)[i % 4], full_lambda=(70, 5000, 90000, 31)[(i // 2) % 4],
                 approx=(i // 3) % 2, hp=1, taps=3, stop=0, iters=2, kind=("smooth", "busy")[(i // 4) % 2], noise=1 + i % 3, seed=3000 + i)
        d.update(kw)
        if d["ref_mv"] is None:
            d["ref_mv"] = (d["start"][0] + (5, -11, 0, 18)[i % 4], d["start"][1] + (-7, 3, 0, -20)[(i // 2) % 4])
        if d["true_mv"] is None:   # where the content really is: a few samples and a fraction from the start
            d["true_mv"] = (d["start"][0] + (i * 13) % 57 - 28, d["start"][1] + (i * 29 + 5) % 57 - 28)
        a_tiles, a_off = _tiles(w // 4, ta)
        l_tiles, l_off = _tiles(h // 4, tl)
        out.append(Case(group, w, h, above_tiles=tuple(a_tiles), above_from=d["mi_col"] + a_off, left_tiles=tuple(l_tiles), left_from=d["mi_row"] + l_off, **d))

    for k, (w, h) in enumerate(SIZES):
        add("size", w, h, ta=PATTERNS[k % 8], tl=PATTERNS[(k + 3) % 8])
        add("size", w, h, ta=PATTERNS[(k + 5) % 8], tl=PATTERNS[(k + 1) % 8], iters=1, hp=k % 2)
    # 0 .. 4 neighbours on each side of a 64 x 64 and of a 32 x 64 / 64 x 32
    counts = {0: [(16, 0)], 1: [(16, 1)], 2: [(8, 1), (8, 1)], 3: [(4, 1), (4, 0), (4, 1), (4, 1)], 4: [(4, 1)] * 4}
    for n in range(5):
        for w, h in ((64, 64), (64, 32), (32, 64)):
            add("count", w, h)
            t = tuple(counts[n]) if w == 64 else tuple((max(s // 2, 1), f) for s, f in counts[n])
            u = tuple(counts[4 - n]) if h == 64 else tuple((max(s // 2, 1), f) for s, f in counts[4 - n])
            out[-1] = out[-1]._replace(above_tiles=t, left_tiles=u)
    # availability
    for k, (w, h) in enumerate(((8, 8), (16, 16), (64, 16), (128, 128))):
        add("unavailable", w, h, up=0)
        add("unavailable", w, h, left=0, ta="twos")
        add("unavailable", w, h, up=0, left=0)
        add("unavailable", w, h, mi_row=0, up=0, tl="gaps")
        add("unavailable", w, h, mi_col=0, left=0, ta="gaps")
    # a block cut by the right and by the bottom picture edge: the walk stops at mi_cols / mi_rows
    add("edge", 32, 32, ta="twos", tl="one", mi_cols=36)
    add("edge", 64, 64, ta="gaps", tl="twos", mi_rows=40)
    add("edge", 64, 32, ta="twos", tl="twos", mi_cols=38, mi_rows=38)
    add("edge", 16, 16, ta="pairs", tl="pairs", mi_cols=34, mi_rows=34)
    # blocks of 128: the overlap is capped at 32, nb_max at 4
    for w, h in ((128, 128), (128, 64), (64, 128)):
        add("cap", w, h, ta="twos", tl="gaps", fp_range=16, diag=1)
        add("cap", w, h, ta="larger", tl="halves", fp_range=8, diag=0, iters=1)
    # the full-pel stage: long descents on smooth content (the truth further away than the range), a start that is the minimum
    for k, (w, h) in enumerate(((4, 4), (8, 8), (16, 16), (64, 16), (16, 64), (64, 64), (128, 128))):
        for rng, diag in ((8, 0), (16, 1), (16, 0), (8, 1)):
            far = ((rng + 6) * 8, (rng + 6) * 8 * (1 if k % 2 else -1)) if diag else ((0, (rng + 6) * 8) if k % 2 else (-(rng + 6) * 8, 0))
            add("descent", w, h, fp_range=rng, diag=diag, kind="smooth", noise=0, start=(0, 0), ref_mv=far, true_mv=far, approx=k % 2, qindex=20)
        add("stay", w, h, kind="busy", noise=0, start=(8, -8), true_mv=(8, -8), ref_mv=(8, -8))
    # the limits: svt_av1_set_mv_search_range around a far ref_mv moves the start and refuses neighbours; the tree's candidates leave the
    # limits the picture edge sets
    for k, (w, h) in enumerate(((8, 8), (16, 16), (32, 32), (64, 64))):
        add("limit", w, h, start=(0, 0), ref_mv=((MAX_FULL_PEL_VAL + 3) * 8, 0), true_mv=(-40, 9))
        add("limit", w, h, start=(0, 0), ref_mv=(2, -(MAX_FULL_PEL_VAL + 2) * 8 - 3), true_mv=(11, 50))
        add("limit", w, h, start=(-8, 8), ref_mv=(-(MAX_FULL_PEL_VAL - 1) * 8, (MAX_FULL_PEL_VAL - 1) * 8), true_mv=(-60, 60), iters=2)
        # at the picture's bottom right corner the raw limits are 4 + 4 samples away
        add("limit", w, h, mi_row=128 - h // 4, mi_col=128 - w // 4, start=(64, 64), true_mv=(90, 90), ref_mv=(60, 66), kind="smooth")
        add("limit", w, h, mi_row=128 - h // 4, mi_col=128 - w // 4, start=(64, 56), true_mv=(70, 61), ref_mv=(64, 64), full=0)
    # the controls of the tree
    for k, (w, h) in enumerate(((4, 16), (8, 8), (16, 16), (32, 8), (64, 64), (16, 64))):
        for stop in range(4):
            add("stop", w, h, stop=stop, iters=1 + stop % 2)
            add("stop", w, h, stop=stop, hp=0, iters=2 - stop % 2)
        for taps in (1, 2, 3):
            add("taps", w, h, taps=taps, full=k % 2)
        for full, frac in ((0, 0), (0, 1), (1, 0), (1, 1)):
            add("refine", w, h, full=full, frac=frac)
            add("refine", w, h, full=full, frac=frac, approx=1 - out[-1].approx)
        for t in ((-13, 3), (6, -13), (13, 13), (-5, -6), (3, 12), (-12, 1)):
            add("tree", w, h, full=0, kind="smooth", noise=0, start=(8, -16), true_mv=(8 + t[0], -16 + t[1]), ref_mv=(8 + t[0] // 2, -16), qindex=20,
                full_lambda=70)
        # equal costs: a flat reference gives every candidate the same variance, and the light vector cost is symmetric
        add("tie", w, h, kind="flat", approx=1, start=(0, 0), ref_mv=(2, 2), full=k % 2)
        add("tie", w, h, kind="flat", approx=1, start=(8, 8), ref_mv=(8, 8))
    return out


CASES = _cases()
# blocks at the four picture edges and in the middle, ref_mv near and far enough out for the MAX_FULL_PEL_VAL clamp and the MV_LOW / MV_UPP one:
# (mi_row, mi_col, mi_w, mi_h, mi_rows, mi_cols, ref_row, ref_col)
LIMIT_CASES = ((0, 0, 4, 4, 270, 480, 0, 0), (0, 476, 4, 4, 270, 480, 13, -7), (266, 0, 4, 4, 270, 480, -40, 55), (266, 476, 4, 4, 270, 480, 3, 3),
               (130, 240, 16, 16, 270, 480, 0, 0), (130, 240, 32, 16, 540, 960, 9000, -9000), (130, 240, 16, 32, 540, 960, -9001, 9003),
               (300, 500, 1, 4, 540, 960, 16383, -16383), (300, 500, 4, 1, 540, 960, -16384, 16384), (10, 950, 2, 2, 540, 960, 700, -650),
               (0, 0, 32, 32, 2000, 4000, -8192, 8191), (1968, 3968, 32, 32, 2000, 4000, 8185, -8185))


class Golden:
    def __init__(self, path=GOLD):
        z = np.load(path)
        self.digests, self.results, self.limits, self.sad_per_bit = z["digests"], z["results"], z["limits"], z["sad_per_bit"]
        assert len(self.digests) == len(self.results) == len(CASES) and len(self.limits) == len(LIMIT_CASES)

    def record(self, i):
        return tuple(int(v) for v in self.results[i])

    def digest(self, i):
        return tuple(int(v) for v in self.digests[i])


# ---- the reference's own functions ----------------------------------------------------------------------------------------------
class PinTarget(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("w", "h", "mi_row", "mi_col", "mi_rows", "mi_cols", "up_available", "left_available", "src_stride", "above_stride",
                                         "left_stride")]


class PinSearch(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("w", "h", "ref_stride", "start_row", "start_col", "ref_row", "ref_col", "mi_row", "mi_col", "mi_rows", "mi_cols",
                                         "do_full_refine", "do_frac_refine", "fpel_search_range", "fpel_search_diag", "qindex", "full_lambda",
                                         "approx_inter_rate", "allow_hp", "subpel_search_type", "forced_stop", "iters_per_step")]


class Pin:
    """tests/obmc_pin_driver.c built into `directory` against oracle/_ref/libsvtref.so (ref: the loaded pyorc.ref())"""

    def __init__(self, ref, directory):
        from support import build_pin
        self.ref, self.lib = ref, build_pin(directory, os.path.join(HERE, "obmc_pin_driver.c"))
        self.lib.pin_target.argtypes = [C.c_void_p] * 10
        self.lib.pin_search.argtypes = [C.c_void_p] * 8
        self.lib.pin_constants.argtypes = [C.c_void_p]
        self.mvj, self.mvrow, self.mvcol = mv_cost_tables()

    def target(self, c, src, above, left):
        """(wsrc, mask) int32 [h][w] of the reference's calc_target_weighted_pred on the case's mode-info grid"""
        src, above, left = (np.ascontiguousarray(p) for p in (src, above, left))
        a_size, a_inter = edge_arrays(c.above_tiles, c.above_from, c.mi_cols)
        l_size, l_inter = edge_arrays(c.left_tiles, c.left_from, c.mi_rows)
        a = PinTarget(c.w, c.h, c.mi_row, c.mi_col, c.mi_rows, c.mi_cols, c.up, c.left, c.w, c.w, c.w)
        wsrc, mask = np.full((c.h, c.w), -1, np.int32), np.full((c.h, c.w), -1, np.int32)
        self.lib.pin_target(C.addressof(a), src.ctypes.data, above.ctypes.data, left.ctypes.data, a_size.ctypes.data, a_inter.ctypes.data,
                            l_size.ctypes.data, l_inter.ctypes.data, wsrc.ctypes.data, mask.ctypes.data)
        return wsrc, mask

    def search(self, c, ref, wsrc, mask):
        """The 21 values of pin_search (see the driver)"""
        ref, wsrc, mask = np.ascontiguousarray(ref), np.ascontiguousarray(wsrc, np.int32), np.ascontiguousarray(mask, np.int32)
        a = PinSearch(c.w, c.h, ref.shape[1], c.start[0], c.start[1], c.ref_mv[0], c.ref_mv[1], c.mi_row, c.mi_col, c.mi_rows, c.mi_cols, c.full, c.frac,
                      c.fp_range, c.diag, c.qindex, c.full_lambda, c.approx, c.hp, c.taps, c.stop, c.iters)
        out = np.zeros(21, np.int64)
        self.lib.pin_search(C.addressof(a), wsrc.ctypes.data, mask.ctypes.data, ref.ctypes.data + BORDER * ref.shape[1] + BORDER, self.mvj.ctypes.data,
                            self.mvrow.ctypes.data - 4 * MV_LOW, self.mvcol.ctypes.data - 4 * MV_LOW, out.ctypes.data)
        return [int(v) for v in out]

    def limits(self, lc):
        """(raw, fp) of a LIMIT_CASES entry from single_motion_search's set-up lines and svt_av1_set_mv_search_range; the limits depend on the
        geometry alone, and with neither stage no sample is read"""
        w, h = lc[2] * 4, lc[3] * 4
        c = CASES[0]._replace(w=w, h=h, mi_row=lc[0], mi_col=lc[1], mi_rows=lc[4], mi_cols=lc[5], ref_mv=(lc[6], lc[7]), full=0, frac=0, start=(0, 0))
        out = self.search(c, np.zeros((h + 2 * BORDER, w + 2 * BORDER), np.uint8), np.zeros((h, w), np.int32), np.zeros((h, w), np.int32))
        return tuple(out[13:17]), tuple(out[17:21])

    def constants(self):
        out = np.zeros(12 + 63, np.int32)
        self.lib.pin_constants(C.c_void_p(out.ctypes.data))
        return [int(v) for v in out]


# ---- descriptors for the device -------------------------------------------------------------------------------------------------
class Arena(md_search_cases.Arena):
    """The samples of a list of cases, room for every case's wsrc and mask, and the cost tables in one host buffer.  The layout moves the
    uint8 planes; wsrc and mask stay 4-byte aligned."""

    def __init__(self, cases, layout=lambda i: (0, 0), restated=None):
        super().__init__(cases, layout)
        self.planes, self.outputs = [], []
        self.restated = restated or [Restated(c) for c in cases]
        for i, (c, r) in enumerate(zip(cases, self.restated)):
            entry = {}
            for name, plane in (("ref", r.ref), ("src", r.src), ("above", r.above), ("left", r.left)):
                at, stride, _ = self.place(i, name, plane)
                entry[name] = (at + (BORDER * stride + BORDER if name == "ref" else 0), stride)
            self.planes.append(entry)
            self.outputs.append(tuple(self.ab.add(f"{name} of case {i}", nbytes=4 * c.w * c.h, align=64, gap=64) for name in ("wsrc", "mask")))
        self.finish()

    def declared(self, picks=None):
        """(offset, bytes) of the wsrc and mask arrays of the cases `picks` (all by default)"""
        picks = range(len(self.cases)) if picks is None else picks
        return [(at, 4 * self.cases[i].w * self.cases[i].h) for i in picks for at in self.outputs[i]]

    def target_descs(self, base):
        d = np.zeros(len(self.cases), abi.OBMC_TARGET_DESC_DTYPE)
        for i, (c, r) in enumerate(zip(self.cases, self.restated)):
            p, (wsrc, mask) = self.planes[i], self.outputs[i]
            for f in ("src", "above", "left"):
                d[i][f], d[i][f + "_stride"] = base + p[f][0], p[f][1]
            d[i]["wsrc"], d[i]["mask"], d[i]["w"], d[i]["h"], d[i]["up_available"], d[i]["left_available"] = base + wsrc, base + mask, c.w, c.h, c.up, c.left
            for side, segs in zip(("above", "left"), r.segs):
                d[i]["n_" + side] = len(segs)
                for k, (rel, n) in enumerate(segs):
                    d[i][side + "_nb"][k]["rel_mi"], d[i][side + "_nb"][k]["mi_len"] = rel, n
        return d

    def search_descs(self, base):
        d = np.zeros(len(self.cases), abi.OBMC_SEARCH_DESC_DTYPE)
        for i, c in enumerate(self.cases):
            (ref, ref_stride), (wsrc, mask) = self.planes[i]["ref"], self.outputs[i]
            d[i] = fill_search_desc(c, base + wsrc, base + mask, base + ref, ref_stride)
        return d

    descs = search_descs


def fill_search_desc(c, wsrc, mask, ref, ref_stride):
    d = np.zeros((), abi.OBMC_SEARCH_DESC_DTYPE)
    d["wsrc"], d["mask"], d["ref"], d["ref_stride"], d["w"], d["h"] = wsrc, mask, ref, ref_stride, c.w, c.h
    d["start_mv"]["row"], d["start_mv"]["col"] = c.start
    d["ref_mv"]["row"], d["ref_mv"]["col"] = c.ref_mv
    d["raw_limits"], d["fp_limits"] = case_limits(c)
    for f, v in (("sad_per_bit", SAD_PER_BIT[c.qindex]), ("error_per_bit", max(c.full_lambda >> 6, 1)), ("iters_per_step", c.iters), ("do_full_refine", c.full),
                 ("do_frac_refine", c.frac), ("fpel_search_range", c.fp_range), ("fpel_search_diag", c.diag), ("approx_inter_rate", c.approx),
                 ("allow_hp", c.hp), ("subpel_search_type", c.taps), ("forced_stop", c.stop)):
        d[f] = v
    return d


def result_tuple(r):
    """A record of abi.OBMC_SEARCH_RESULT_DTYPE as RESULT_FIELDS"""
    return (int(r["best_mv"]["row"]), int(r["best_mv"]["col"]), int(r["fullpel_mv"]["row"]), int(r["fullpel_mv"]["col"]), int(r["besterr"]),
            int(r["distortion"]), int(r["sse"]), int(r["rate_mv"]), int(r["fullpel_rounds"]))
