"""TEST INFRASTRUCTURE — cases, picture generator, Python restatement and descriptor builder for the sub-pel motion search of mode
decision (svt_hip_subpel_search_batch, include/svt_hip_inter.h).

The search is svt_av1_find_best_sub_pixel_tree / svt_av1_find_best_sub_pixel_tree_pruned (mcomp.c:609-775) as md_subpel_search
(product_coding_loop.c:2502-2614) calls them.  Pictures and motion-vector cost tables are generated here (integers only, seeded), so
tests/golden/subpel.npz (written by tests/golden/make_golden_subpel.py) holds only the limits of LIMIT_CASES and every case's result.
tests/test_subpel_abi.py pins fixture and restatement to the reference's own functions through tests/subpel_pin_driver.c wherever
oracle/_ref/libsvtref.so has been built."""
import collections
import ctypes as C
import os

import numpy as np

import md_search_cases
from md_search_cases import MAX_FULL_PEL_VAL, MV_LOW, MV_UPP, SIZES, i16, mv_cost_tables  # noqa: F401  (re-exported)
from svtav1_hip import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "subpel.npz")

TREE, PRUNED = abi.SUBPEL_TREE, abi.SUBPEL_TREE_PRUNED
ENTROPY, L1_LOWRES, L1_MIDRES, L1_HDRES, OPT, NONE = range(6)     # MV_COST_TYPE (mcomp.h:29-36)
INT_MAX = 2 ** 31 - 1
BORDER = 24                                                        # samples around the block in a generated picture
RESULT_FIELDS = ("best_row", "best_col", "besterr", "distortion", "sse", "fullpel_err", "exit")

# av1_bilinear_filters, av1_sub_pel_filters_4, av1_sub_pel_filters_8 (variance.c:73-140) at the rows subpel_q3 << 1
FILTERS = np.array([
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, 0, 112, 16, 0, 0, 0], [0, 0, 0, 96, 32, 0, 0, 0], [0, 0, 0, 80, 48, 0, 0, 0],
     [0, 0, 0, 64, 64, 0, 0, 0], [0, 0, 0, 48, 80, 0, 0, 0], [0, 0, 0, 32, 96, 0, 0, 0], [0, 0, 0, 16, 112, 0, 0, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, -8, 122, 18, -4, 0, 0], [0, 0, -12, 110, 38, -8, 0, 0], [0, 0, -14, 94, 58, -10, 0, 0],
     [0, 0, -12, 76, 76, -12, 0, 0], [0, 0, -10, 58, 94, -14, 0, 0], [0, 0, -8, 38, 110, -12, 0, 0], [0, 0, -4, 18, 122, -8, 0, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0], [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -16, 94, 58, -12, 2, 0],
     [0, 2, -14, 76, 76, -14, 2, 0], [0, 2, -12, 58, 94, -16, 2, 0], [0, 2, -10, 38, 110, -14, 2, 0], [0, 0, -4, 18, 122, -10, 2, 0]]], np.int32)

Case = collections.namedtuple("Case", "group w h method taps iters forced_stop allow_hp bias_fp skip_diag pred_var_th abs_th_mult round_dev_th qp "
                                      "cost_type epb early_exit_th early_exit mvp_th hp_mv_th mvp_dist mvp start ref_mv true_mv limits kind noise seed")
LimitCase = collections.namedtuple("LimitCase", "mi_row mi_col mi_w mi_h mi_rows mi_cols ref_row ref_col")


# ---- generated inputs -----------------------------------------------------------------------------------------------------------
def pictures(c):
    """(src, ref): two uint8 planes of (h + 2 BORDER) x (w + 2 BORDER) with the block at (BORDER, BORDER).  A coarse random grid is
    interpolated, in integers, to eight times the picture's resolution; ref samples it at the sample positions, src at the positions
    moved by true_mv (1/8 units), so that src(y, x) ~ ref(y + row / 8, x + col / 8); then noise is added to both."""
    rs = np.random.RandomState(c.seed)
    H, W = c.h + 2 * BORDER, c.w + 2 * BORDER
    if c.kind == "flat":
        ref = np.full((H, W), 90, np.int64) + rs.randint(0, 2, (H, W))
        src = np.full((H, W), 93, np.int64) + rs.randint(0, 3, (H, W))
        return src.astype(np.uint8), ref.astype(np.uint8)
    if c.kind == "contrast":   # a poor match of full contrast: the cost of a 64x128 / 128x128 block times 110 passes 2^32
        ref = rs.randint(0, 2, (H, W)) * 255
        src = 255 - ref
        flip = rs.randint(0, 100, (H, W)) < 3
        src = np.where(flip, 255 - src, src)
        return src.astype(np.uint8), ref.astype(np.uint8)
    cell = 6 if c.kind == "busy" else 12
    gh, gw = (H + 10) // cell + 3, (W + 10) // cell + 3
    grid = rs.randint(16, 240, (gh, gw)).astype(np.int64)
    step = cell * 8
    yy, xx = np.arange((H + 10) * 8), np.arange((W + 10) * 8)
    a, u = yy // step, yy % step
    b, v = xx // step, xx % step
    top = grid[a][:, b] * (step - v) + grid[a][:, b + 1] * v
    bot = grid[a + 1][:, b] * (step - v) + grid[a + 1][:, b + 1] * v
    hi = (top * (step - u)[:, None] + bot * u[:, None] + step * step // 2) // (step * step)   # [(H + 10) * 8][(W + 10) * 8]
    ys, xs = (np.arange(H) + 5) * 8, (np.arange(W) + 5) * 8   # |true_mv| < 40
    ref = hi[ys][:, xs]
    src = hi[ys + c.true_mv[0]][:, xs + c.true_mv[1]]
    if c.noise:
        ref = ref + rs.randint(-c.noise, c.noise + 1, (H, W))
        src = src + rs.randint(-c.noise, c.noise + 1, (H, W))
    return np.clip(src, 0, 255).astype(np.uint8), np.clip(ref, 0, 255).astype(np.uint8)


# ---- restatement ----------------------------------------------------------------------------------------------------------------
def c_div(a, b):
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def mv_limits(lc):
    """product_coding_loop.c:2527-2537: MvLimits, svt_av1_set_mv_search_range, svt_av1_set_subpel_mv_search_range -> (col_min, col_max,
    row_min, row_max)"""
    ref_mv = (lc.ref_row, lc.ref_col)
    fp = md_search_cases.set_mv_search_range(md_search_cases.block_mv_limits(*lc[:6]), ref_mv)
    return md_search_cases.set_subpel_mv_search_range(fp, ref_mv)


def case_limits(c):
    """The limits of a case: those of a 4K picture's middle around ref_mv, or the case's own"""
    if c.limits is not None:
        return c.limits
    return mv_limits(LimitCase(270, 480, c.w // 4, c.h // 4, 540, 960, c.ref_mv[0], c.ref_mv[1]))


class Search:
    """One search on a case's pictures.  After run(): best (row, col), besterr, distortion, sse, fullpel_err, exit, and `events`, the
    set of things the coverage conditions of the golden script name."""

    def __init__(self, c, src=None, ref=None, tables=None):
        self.c = c
        if src is None:
            src, ref = pictures(c)
        self.ref = ref.astype(np.int32)
        self.src = src[BORDER:BORDER + c.h, BORDER:BORDER + c.w].astype(np.int64)
        self.mvj, self.mvrow, self.mvcol = tables or mv_cost_tables()
        self.limits = case_limits(c)
        self.table = 0 if c.method == PRUNED else c.taps - abi.SUBPEL_USE_2_TAPS
        self.events = set()
        self.sse = 0
        self.run()

    # svt_aom_upsampled_pred_c + vf, and the bilinear svf: the identity kernel of a direction without an offset is exact
    def error(self, mv, against_128=False):
        c = self.c
        y, x = BORDER + (mv[0] >> 3), BORDER + (mv[1] >> 3)
        self.events.add(("reach", (mv[0] >> 3) - (c.start[0] >> 3), (mv[1] >> 3) - (c.start[1] >> 3)))
        fx, fy = FILTERS[self.table][mv[1] & 7], FILTERS[self.table][mv[0] & 7]
        r = self.ref[y - 3:y + c.h + 4, x - 3:x + c.w + 4]
        tmp = sum(int(fx[k]) * r[:, k:k + c.w] for k in range(8))
        tmp = np.clip((tmp + 64) >> 7, 0, 255)
        pred = sum(int(fy[k]) * tmp[k:k + c.h] for k in range(8))
        pred = np.clip((pred + 64) >> 7, 0, 255).astype(np.int64)
        diff = pred - (128 if against_128 else self.src)
        s, sse = int(diff.sum()), int((diff * diff).sum())
        assert sse < 1 << 32
        return (sse - ((s * s) // (c.w * c.h) & 0xFFFFFFFF)) & 0xFFFFFFFF, sse

    # svt_mv_err_cost (mcomp.c:44-68)
    def mv_cost(self, mv):
        c = self.c
        dr, dc = i16(mv[0] - c.ref_mv[0]), i16(mv[1] - c.ref_mv[1])
        l1 = i16(abs(dr)) + i16(abs(dc))
        if c.cost_type == ENTROPY:
            joint = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
            rate = int(self.mvj[joint]) + int(self.mvrow[min(max(dr, MV_LOW), MV_UPP) - MV_LOW]) + int(self.mvcol[min(max(dc, MV_LOW), MV_UPP) - MV_LOW])
            return (rate * c.epb + (1 << 13)) >> 14
        if c.cost_type == OPT:
            return ((l1 << 8) * c.epb + (1 << 13)) >> 14
        return {L1_LOWRES: (2 * l1) >> 3, L1_MIDRES: 0, L1_HDRES: l1 >> 3, NONE: 0}[c.cost_type]

    def in_range(self, mv):
        lo_c, hi_c, lo_r, hi_r = self.limits
        for beyond, name in ((mv[1] < lo_c, "col_min"), (mv[1] > hi_c, "col_max"), (mv[0] < lo_r, "row_min"), (mv[0] > hi_r, "row_max")):
            if beyond:
                self.events.add(("beyond", name))
        return lo_c <= mv[1] <= hi_c and lo_r <= mv[0] <= hi_r

    def take_if_better(self, mv, cost, thismse, sse):
        # best_mv.col % 8 on a signed value: zero exactly when the low three bits are
        at_fp = self.c.bias_fp and self.best[0] % 8 == 0 and self.best[1] % 8 == 0
        weight = 110 if at_fp else 100
        if cost * weight >= 1 << 32:
            self.events.add(("wrap", weight))
        won = ((cost * weight) & 0xFFFFFFFF) // 100 < self.besterr
        if at_fp and won != (cost < self.besterr):
            self.events.add(("bias_changes_winner",))
        if won:
            self.besterr, self.best, self.distortion, self.sse = cost, mv, thismse, sse
        return won

    # svt_check_better
    def check(self, mv):
        mv = (i16(mv[0]), i16(mv[1]))
        if not self.in_range(mv):
            return INT_MAX, False
        thismse, sse = self.error(mv)
        thismse = thismse - (1 << 32) if thismse >= 1 << 31 else thismse      # int
        cost = (self.mv_cost(mv) + thismse) & 0xFFFFFFFF
        return cost, self.take_if_better(mv, cost, thismse, sse)

    # svt_check_better_fast; the second value is what the cost would have been without the MV_COST_OPT return
    def check_fast(self, mv):
        mv = (i16(mv[0]), i16(mv[1]))
        if not self.in_range(mv):
            return INT_MAX, INT_MAX
        cost = self.mv_cost(mv) & 0xFFFFFFFF
        if self.c.cost_type == OPT:
            bestcost = (self.distortion + cost) & 0xFFFFFFFF
            if bestcost > c_div(self.besterr * self.c.early_exit_th, 1000):
                self.events.add(("opt_return",))
                return bestcost, (cost + self.error(mv)[0]) & 0xFFFFFFFF
        thismse, sse = self.error(mv)
        thismse = thismse - (1 << 32) if thismse >= 1 << 31 else thismse
        cost = (cost + thismse) & 0xFFFFFFFF
        self.take_if_better(mv, cost, thismse, sse)
        return cost, cost

    def tree_rounds(self, rounds):
        hstep = 4
        for _ in range(rounds):
            cr, cc = self.best
            left, right = self.check((cr, cc - hstep))[0], self.check((cr, cc + hstep))[0]
            up, down = self.check((cr - hstep, cc))[0], self.check((cr + hstep, cc))[0]
            sr, sc = (-hstep if up <= down else hstep), (-hstep if left <= right else hstep)
            self.check((cr + sr, cc + sc))
            if (cr, cc) != self.best and self.c.iters > 1:      # svt_second_level_check_v2
                if cr == self.best[0]:
                    sr = -sr
                    self.events.add(("v2", "row"))
                elif cc == self.best[1]:
                    sc = -sc
                    self.events.add(("v2", "col"))
                else:
                    self.events.add(("v2", "diag"))
                mr, mc = self.best
                better = self.check((mr + sr, mc))[1]
                better = self.check((mr, mc + sc))[1] or better
                if better:
                    self.events.add(("v2", "third"))
                    self.check((mr + sr, mc + sc))
            hstep >>= 1

    def two_level_checks_fast(self, t, hstep, orgerr):
        tr, tc = t
        (left, left_full), (right, right_full) = self.check_fast((tr, tc - hstep)), self.check_fast((tr, tc + hstep))
        (up, up_full), (down, down_full) = self.check_fast((tr - hstep, tc)), self.check_fast((tr + hstep, tc))
        sr, sc = (-hstep if up <= down else hstep), (-hstep if left <= right else hstep)
        if (sr, sc) != ((-hstep if up_full <= down_full else hstep), (-hstep if left_full <= right_full else hstep)):
            self.events.add(("opt_return_alters_diag",))
        if self.besterr >= orgerr:
            self.events.add(("fast", "no_diag"))
            return
        self.check_fast((tr + sr, tc + sc))
        if self.besterr >= orgerr or self.c.iters <= 1:
            return
        br, bc = self.best
        if tr != br and tc != bc:
            self.events.add(("second_fast", "diag"))
            self.check_fast((br, bc + sc))
            self.check_fast((br + sr, bc))
        elif tr == br and tc != bc:
            self.events.add(("second_fast", "row"))
            self.check_fast((br + hstep, bc + sc))
            self.check_fast((br - hstep, bc + sc))
            self.check_fast((br - sr, bc))
        elif tr != br and tc == bc:
            self.events.add(("second_fast", "col"))
            self.check_fast((br + sr, bc + hstep))
            self.check_fast((br + sr, bc - hstep))
            self.check_fast((br, bc - sc))

    def search(self):
        c = self.c
        pruned = c.method == PRUNED
        rounds = min(3 - c.forced_stop, 3 - (not c.allow_hp))
        if not pruned and c.mvp_th > 0:
            mvp_err, me_err = c.mvp_dist + 1, self.besterr + 1
            assert abs((me_err - mvp_err) * 100) < 1 << 31     # the reference's int would overflow
            if c_div((me_err - mvp_err) * 100, me_err) >= c.mvp_th:
                rounds = 1
                self.events.add(("mvp", "deviation"))
            elif abs(self.best[1] - c.mvp[1]) > c.hp_mv_th or abs(self.best[0] - c.mvp[0]) > c.hp_mv_th:
                rounds = min(rounds, 2)
                self.events.add(("mvp", "hp"))
            else:
                self.events.add(("mvp", "neither"))
        self.events.add(("rounds", rounds))
        if c.early_exit:
            return abi.SUBPEL_EXIT_EARLY
        th_normalizer = ((c.w * c.h) >> (3 if pruned else 2)) * c.abs_th_mult * (c.qp >> 1)
        if pruned:
            if self.besterr < th_normalizer:
                return abi.SUBPEL_EXIT_ABS_TH
            if not rounds:
                return abi.SUBPEL_EXIT_NO_ROUND
        n = (c.w * c.h).bit_length() - 1
        var = self.error(self.best, against_128=True)[0]
        if (var + ((1 << n) >> 1)) >> n < c.pred_var_th:
            return abi.SUBPEL_EXIT_VARIANCE
        if not pruned:
            if self.besterr < th_normalizer:
                return abi.SUBPEL_EXIT_ABS_TH
            if not rounds:
                return abi.SUBPEL_EXIT_NO_ROUND
            self.tree_rounds(rounds)
            return abi.SUBPEL_EXIT_END
        if c.skip_diag >= 4:
            org_error = 0
        else:
            demo = 2 if c.skip_diag >= 2 and (c.w >= 64 or c.h >= 64) else 1
            org_error = self.besterr // demo if c.skip_diag else INT_MAX
        start, hstep = self.best, 4
        for it in range(rounds):
            prev = self.besterr
            self.two_level_checks_fast(start, hstep, org_error)
            hstep >>= 1
            start = self.best
            if c.skip_diag and it < 1:
                org_error = min(org_error, self.besterr)
            if c_div((max(self.besterr, 1) - max(prev, 1)) * 100, max(prev, 1)) >= c.round_dev_th:
                return abi.SUBPEL_EXIT_ROUND_DEV
        return abi.SUBPEL_EXIT_END

    def run(self):
        c = self.c
        self.best = tuple(c.start)
        self.distortion = self.error(self.best)[0]          # svt_upsampled_setup_center_error: the variance; *sse1 is not written
        self.besterr = (self.distortion + self.mv_cost(self.best)) & 0xFFFFFFFF
        self.fullpel_err = self.besterr
        self.exit = self.search()
        frac = (self.best[0] | self.best[1]) & 7
        self.events.add(("winner", "centre" if self.best == tuple(c.start) else "full" if not frac else "eighth" if frac & 1 else "quarter" if frac & 2 else "half"))

    def record(self):
        """RESULT_FIELDS; besterr and distortion as the int the function returns / stores"""
        s32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v   # noqa: E731
        return (self.best[0], self.best[1], s32(self.besterr), s32(self.distortion), self.sse, self.fullpel_err, self.exit)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []

    def add(group, w, h, method, **kw):
        i = len(out)
        d = dict(taps=(3, 1, 2)[i % 3], iters=1 + i % 2, forced_stop=0, allow_hp=1, bias_fp=(i // 2) % 2, skip_diag=0, pred_var_th=0, abs_th_mult=0,
                 round_dev_th=INT_MAX, qp=40, cost_type=(i // 3) % 6, epb=(60, 350, 2400)[i % 3], early_exit_th=(1500, 1100, 1030)[(i // 2) % 3], early_exit=0,
                 mvp_th=0, hp_mv_th=0, mvp_dist=0, mvp=(0, 0), start=(8 * (i % 5 - 2), 8 * ((i // 5) % 5 - 2)), ref_mv=None, true_mv=None, limits=None,
                 kind=("smooth", "busy")[(i // 4) % 2], noise=2 + i % 3, seed=1000 + i)
        d.update(kw)
        if d["ref_mv"] is None:
            d["ref_mv"] = (d["start"][0] + (5, -11, 0, 18)[i % 4], d["start"][1] + (-7, 3, 0, -20)[(i // 2) % 4])
        if d["true_mv"] is None:   # where the content really is: a sub-pel offset within 7/8 of the start, every eighth in turn
            d["true_mv"] = (d["start"][0] + (i * 3) % 15 - 7, d["start"][1] + (i * 5 + 2) % 15 - 7)
        out.append(Case(group, w, h, method, **d))

    for w, h in SIZES:
        for method in (TREE, PRUNED):
            add("size", w, h, method)
    # the controls, on sizes of both kernels
    for k, (w, h) in enumerate(((8, 8), (16, 16), (32, 16), (64, 64), (16, 64), (4, 16))):
        for taps in (1, 2, 3):
            add("taps", w, h, TREE, taps=taps, iters=2)
        for cost_type in range(6):
            add("cost", w, h, (TREE, PRUNED)[(k + cost_type) % 2], cost_type=cost_type, epb=(90, 700, 5000)[(k + cost_type) % 3])
        for skip in range(5):
            add("skip_diag", w, h, PRUNED, skip_diag=skip, iters=2, round_dev_th=(INT_MAX, -3)[skip % 2])
        for forced_stop in range(4):
            add("stop", w, h, (TREE, PRUNED)[forced_stop % 2], forced_stop=forced_stop)
            add("stop", w, h, (PRUNED, TREE)[forced_stop % 2], forced_stop=forced_stop, iters=2)
        add("no_hp", w, h, TREE, allow_hp=0, iters=2)
        add("no_hp", w, h, PRUNED, allow_hp=0, iters=2)
        for method in (TREE, PRUNED):
            add("exit_early", w, h, method, early_exit=1)
            add("exit_variance", w, h, method, kind="flat", pred_var_th=50)
            add("variance_passes", w, h, method, pred_var_th=50)
            add("exit_abs_th", w, h, method, abs_th_mult=200, qp=63, noise=0, true_mv=(0, 0), start=(0, 0))
            add("abs_th_passes", w, h, method, abs_th_mult=1, qp=20)
        add("exit_round_dev", w, h, PRUNED, round_dev_th=-8, iters=2)
        add("exit_round_dev", w, h, PRUNED, round_dev_th=0, skip_diag=1)
        # the mvp rule: ME far worse than the MVP; the ME vector far from the MVP; neither
        add("mvp", w, h, TREE, mvp_th=20, mvp_dist=0, hp_mv_th=1000, iters=2)
        add("mvp", w, h, TREE, mvp_th=100, mvp_dist=0, hp_mv_th=4, mvp=(200, -90), iters=2)
        add("mvp", w, h, TREE, mvp_th=100, mvp_dist=10 ** 6, hp_mv_th=300, mvp=(8, 8), iters=2)
        # MV_COST_OPT: thresholds just above 1000 make the early return frequent
        for th in (1001, 1010, 1060):
            add("opt", w, h, PRUNED, cost_type=OPT, early_exit_th=th, iters=2, epb=(400, 3000, 12000)[k % 3], skip_diag=k % 2)
        # the limits one candidate step from the start, on each side, and a start on a limit
        for side in range(4):
            s = (8 * (k - 2), 8 * (2 - k))
            lim = [s[1] - 100, s[1] + 100, s[0] - 100, s[0] + 100]
            lim[side] = (s[1] - 3, s[1] + 3, s[0] - 3, s[0] + 3)[side]
            add("limit", w, h, (TREE, PRUNED)[(side + k) % 2], start=s, limits=tuple(lim), iters=2)
        add("limit", w, h, TREE, start=(16, -8), limits=(-8, -8, 16, 16), iters=2)
        # two iterations per step carry a search up to 14 / 8 from its start
        for t in ((-14, -14), (14, 14), (-14, 13), (12, -14)):
            add("reach", w, h, (TREE, PRUNED)[k % 2], iters=2, true_mv=t, start=(0, 0), noise=1, cost_type=NONE, kind="smooth")
        add("bias", w, h, TREE, bias_fp=1, noise=6, iters=2)
        add("bias", w, h, PRUNED, bias_fp=1, noise=6, iters=2)
        add("bias", w, h, TREE, bias_fp=0, noise=6, iters=2)
    # a poor match of full contrast: cost * 110 wraps mod 2^32
    for w, h in ((128, 128), (64, 128), (128, 64)):
        for method in (TREE, PRUNED):
            add("wrap", w, h, method, kind="contrast", bias_fp=1, iters=2, cost_type=NONE)
            add("wrap", w, h, method, kind="contrast", bias_fp=0, iters=2, cost_type=L1_LOWRES)
    # cost tables addressed at their clamped ends: ref_mv far from the vector
    add("far_ref", 16, 16, TREE, cost_type=ENTROPY, ref_mv=(16000, -16200), start=(-16, 8), limits=(-200, 200, -200, 200))
    add("far_ref", 32, 32, PRUNED, cost_type=ENTROPY, ref_mv=(-16300, 16100), start=(8, 16), limits=(-200, 200, -200, 200))
    return out


CASES = _cases()
# blocks at the four picture edges and in the middle, ref_mv near and far enough out for the MAX_FULL_PEL_VAL clamp and the MV_LOW / MV_UPP one
LIMIT_CASES = [LimitCase(*v) for v in (
    (0, 0, 4, 4, 270, 480, 0, 0), (0, 476, 4, 4, 270, 480, 13, -7), (266, 0, 4, 4, 270, 480, -40, 55), (266, 476, 4, 4, 270, 480, 3, 3),
    (130, 240, 16, 16, 270, 480, 0, 0), (130, 240, 32, 16, 540, 960, 9000, -9000), (130, 240, 16, 32, 540, 960, -9001, 9003),
    (300, 500, 1, 4, 540, 960, 16383, -16383), (300, 500, 4, 1, 540, 960, -16384, 16384), (10, 950, 2, 2, 540, 960, 700, -650),
    (0, 0, 32, 32, 2000, 4000, -8192, 8191), (1968, 3968, 32, 32, 2000, 4000, 8185, -8185))]


class Golden:
    def __init__(self, path=GOLD):
        z = np.load(path)
        self.limits, self.results = z["limits"], z["results"]     # [LIMIT_CASES][4], [CASES][RESULT_FIELDS]
        assert len(self.limits) == len(LIMIT_CASES) and len(self.results) == len(CASES)

    def record(self, i):
        return tuple(int(v) for v in self.results[i])


# ---- the reference's own functions ----------------------------------------------------------------------------------------------
class PinArgs(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("w", "h", "src_stride", "ref_stride", "start_row", "start_col", "ref_row", "ref_col", "col_min", "col_max", "row_min",
                                         "row_max", "method", "search_type", "iters_per_step", "forced_stop", "allow_hp", "bias_fp", "skip_diag_refinement",
                                         "pred_variance_th", "abs_th_mult", "round_dev_th", "qp", "mv_cost_type", "error_per_bit", "early_exit_th", "early_exit",
                                         "mvp_th", "hp_mv_th", "best_mvp_dist", "best_mvp_row", "best_mvp_col")]


class Pin:
    """tests/subpel_pin_driver.c built into `directory` against oracle/_ref/libsvtref.so (ref: the loaded pyorc.ref(), whose ref_init has
    set the RTCD pointers the variance functions go through)"""

    def __init__(self, ref, directory):
        from support import build_pin
        self.ref, self.lib = ref, build_pin(directory, os.path.join(HERE, "subpel_pin_driver.c"))
        self.lib.pin_subpel.argtypes = [C.c_void_p] * 7
        self.lib.pin_limits.argtypes = [C.c_int32] * 8 + [C.c_void_p]
        self.mvj, self.mvrow, self.mvcol = mv_cost_tables()

    def run(self, c, src=None, ref=None):
        """RESULT_FIELDS without `exit` of the reference's function on the case"""
        if src is None:
            src, ref = pictures(c)
        src, ref = np.ascontiguousarray(src), np.ascontiguousarray(ref)
        lim = case_limits(c)
        a = PinArgs(c.w, c.h, src.shape[1], ref.shape[1], c.start[0], c.start[1], c.ref_mv[0], c.ref_mv[1], lim[0], lim[1], lim[2], lim[3], c.method, c.taps,
                    c.iters, c.forced_stop, c.allow_hp, c.bias_fp, c.skip_diag, c.pred_var_th, c.abs_th_mult, c.round_dev_th, c.qp, c.cost_type, c.epb,
                    c.early_exit_th, c.early_exit, c.mvp_th, c.hp_mv_th, c.mvp_dist, c.mvp[0], c.mvp[1])
        out = np.zeros(6, np.int64)
        at = BORDER * src.shape[1] + BORDER
        self.lib.pin_subpel(C.addressof(a), src.ctypes.data + at, ref.ctypes.data + BORDER * ref.shape[1] + BORDER, self.mvj.ctypes.data,
                            self.mvrow.ctypes.data - 4 * MV_LOW, self.mvcol.ctypes.data - 4 * MV_LOW, out.ctypes.data)
        return tuple(int(v) for v in out)

    def limits(self, lc):
        out = np.zeros(4, np.int32)
        self.lib.pin_limits(*lc, out.ctypes.data)
        return tuple(int(v) for v in out)

    def constants(self):
        out = np.zeros(16, np.int32)
        self.lib.pin_constants(C.c_void_p(out.ctypes.data))
        return [int(v) for v in out]


# ---- descriptors for the device -------------------------------------------------------------------------------------------------
class Arena(md_search_cases.Arena):
    """The pictures of a list of cases and the cost tables in one host buffer"""

    def __init__(self, cases, layout=lambda i: (0, 0)):
        super().__init__(cases, layout, fill=0)
        self.planes = []
        for i, c in enumerate(cases):
            placed = [self.place(i, name, plane) for name, plane in zip(("src", "ref"), pictures(c))]
            self.planes.append([(at + BORDER * stride + BORDER, stride) for at, stride, _ in placed])
        self.finish()

    def descs(self, base):
        d = np.zeros(len(self.cases), abi.SUBPEL_DESC_DTYPE)
        for i, c in enumerate(self.cases):
            (src, src_stride), (ref, ref_stride) = self.planes[i]
            lim = case_limits(c)
            d[i] = fill_desc(c, base + src, base + ref, src_stride, ref_stride, lim)
        return d


def fill_desc(c, src, ref, src_stride, ref_stride, lim):
    d = np.zeros((), abi.SUBPEL_DESC_DTYPE)
    d["src"], d["ref"], d["src_stride"], d["ref_stride"], d["w"], d["h"] = src, ref, src_stride, ref_stride, c.w, c.h
    for f, v in (("start_mv", c.start), ("ref_mv", c.ref_mv), ("best_mvp", c.mvp)):
        d[f]["row"], d[f]["col"] = v
    d["col_min"], d["col_max"], d["row_min"], d["row_max"] = lim
    for f, v in (("iters_per_step", c.iters), ("pred_variance_th", c.pred_var_th), ("round_dev_th", c.round_dev_th), ("error_per_bit", c.epb),
                 ("early_exit_th", c.early_exit_th), ("hp_mv_th", c.hp_mv_th), ("best_mvp_dist", c.mvp_dist), ("method", c.method),
                 ("subpel_search_type", c.taps), ("forced_stop", c.forced_stop), ("allow_hp", c.allow_hp), ("bias_fp", c.bias_fp),
                 ("skip_diag_refinement", c.skip_diag), ("abs_th_mult", c.abs_th_mult), ("qp", c.qp), ("mv_cost_type", c.cost_type),
                 ("early_exit", c.early_exit), ("mvp_th", c.mvp_th)):
        d[f] = v
    return d


def result_tuple(r):
    """A record of abi.SUBPEL_RESULT_DTYPE as RESULT_FIELDS"""
    return (int(r["best_mv"]["row"]), int(r["best_mv"]["col"]), int(r["besterr"]), int(r["distortion"]), int(r["sse"]), int(r["fullpel_err"]), int(r["exit"]))
