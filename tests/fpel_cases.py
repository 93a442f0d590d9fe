"""TEST INFRASTRUCTURE — cases, picture generators, Python restatement and descriptor builder for the full-pel motion search of mode
decision (svt_hip_fpel_search_batch, include/svt_hip_inter.h).

The search is md_full_pel_search (product_coding_loop.c:1918-2046) with md_full_pel_search_large_lbd / svt_pme_sad_loop_kernel_c behind
it, chained as md_sq_motion_search (:2314-2498), md_nsq_motion_search (:2075-2241), the full-pel call of pme_search (:3263) and the MVP
scoring of :3087-3108 chain it.  Pictures and motion-vector cost tables are generated here (integers only, seeded), so
tests/golden/fpel.npz (written by tests/golden/make_golden_fpel.py) holds only every case's result and the windows of WINDOW_CASES.
tests/test_fpel_abi.py pins fixture and restatement to the reference's own functions through tests/fpel_pin_driver.c wherever
oracle/_ref/libsvtref.so has been built."""
import collections
import ctypes as C
import os

import numpy as np

import arena
import md_search_cases
from md_search_cases import MV_LOW, MV_UPP, SIZES, i16, mv_cost_tables
from svtav1_hip import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fpel.npz")

MVP, SQ, NSQ, PME = abi.FPEL_MVP, abi.FPEL_SQ, abi.FPEL_NSQ, abi.FPEL_PME
SAD, VAR, SSD = abi.FPEL_SAD, abi.FPEL_VAR, abi.FPEL_SSD
ENTROPY, L1_LOWRES, L1_MIDRES, L1_HDRES, OPT, NONE = range(6)     # MV_COST_TYPE (mcomp.h:29-36)
TILE = abi.FPEL_TILE
TAIL = 64                                                          # bytes behind a picture that the psad overshoot of its last rows may read
RESULT_FIELDS = ("best_row", "best_col", "best_cost", "aux_cost", "expanded", "mvp_idx")
M1 = 0xFFFFFFFF

Geo = collections.namedtuple("Geo", "pic_w pic_h org_x org_y blk_x blk_y")          # max_width, max_height, padding, ctx->blk_org_x / _y
Level = collections.namedtuple("Level", "enabled step start_x end_x start_y end_y")
Ctrls = collections.namedtuple("Ctrls", "enabled step w h max_w max_h multiplier")  # MdSqMotionSearchCtrls, a triple per field
StageLog = collections.namedtuple("StageLog", "args clip cost after visited span psad")   # psad: (start_x, start_y, width, height) after the clip, or None
Case = collections.namedtuple("Case", "name mode w h dist psad cost_type epb ref_mv geo mvs levels ctrls sam pocd th sq_size nsq sub geom_org pic")
# pic: (kind, seed, parameters).  mvs: (row, col) pairs.  SQ: levels come from ctrls, sam and pocd when ctrls is given (then md_sq_motion_search
# itself can be driven); th is pame_distortion_th.  NSQ: sub = {PU index: (x, y) full-pel ME vector} and geom_org = blk_geom->org_x / _y make the
# MVC list of :2079-2140 (then md_nsq_motion_search itself can be driven).


def c_rem(a, b):
    """C's a % b (the sign of a)"""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def scaled_distance(dist):
    """svt_aom_get_scaled_picture_distance (motion_estimation.c:1239-1243)"""
    return ((dist * 5) // 8 + (0 if dist % 8 == 0 else 1)) & 0xFFFF


def sq_windows(ct, sam, dist):
    """product_coding_loop.c:2379-2393, 2423-2446, 2480-2487 -> three Levels (what svt_hip_fpel_sq_windows gives)"""
    out = []
    for l in range(3):
        step = ct.step[l]
        if not step:
            out.append(Level(ct.enabled[l], 0, 0, 0, 0, 0))
            continue
        if l == 2:
            sw, sh = ct.w[l], ct.h[l]
        else:
            sw = int(ct.multiplier[l] * min(ct.w[l] * sam * dist, ct.max_w[l]) / 100) & 0xFFFF     # int arithmetic into uint16_t
            sh = int(ct.multiplier[l] * min(ct.h[l] * sam * dist, ct.max_h[l]) / 100) & 0xFFFF
        x, y = ((sw >> 1) // step) * step, ((sh >> 1) // step) * step
        sx, ex, sy, ey = -x, x, -y, y
        if l == 1:
            sx, ex = (sx - 2 if c_rem(sx, 4) == 0 else sx), (ex + 2 if c_rem(ex, 4) == 0 else ex)
            sy, ey = (sy - 2 if c_rem(sy, 4) == 0 else sy), (ey + 2 if c_rem(ey, 4) == 0 else ey)
        out.append(Level(ct.enabled[l], step, i16(sx), i16(ex), i16(sy), i16(ey)))
    return out


def sq_level_ctrls(level):
    """md_sq_motion_search_controls (enc_mode_config.c:3185-3301), levels 1 .. 4: they differ in the two multipliers"""
    m = {1: 500, 2: 400, 3: 300, 4: 100}[level]
    return Ctrls((1, 1, 1), (4, 2, 1), (15, 4, 3), (15, 4, 3), (150, 50, 0), (150, 50, 0), (m, m, 0))


def pu_table():
    """(x, y, width, height) of the 85 square PUs: pu_search_index_map, partition_width / _height (motion_estimation.h:117-150)"""
    out = []
    for size in (64, 32, 16, 8):
        n = 64 // size
        out += [(x * size, y * size, size, size) for y in range(n) for x in range(n)]
    return out


def nsq_mvcs(me_mv, w, h, sq_size, geom_org, sub):
    """The MVC list of md_nsq_motion_search (:2079-2140), (row, col) pairs in 1/8 units, not yet rounded"""
    mvc = [(me_mv[1], me_mv[0])]                                    # (x, y)
    if w != 4 and h != 4 and sq_size >= 16:
        m = min(w, h)
        for i, (px, py, pw, ph) in enumerate(pu_table()):
            if (m == pw or m == ph) and geom_org[0] <= px < w + geom_org[0] and geom_org[1] <= py < h + geom_org[1] and i in sub:
                cand = (i16(sub[i][0] << 3), i16(sub[i][1] << 3))
                if cand not in mvc:
                    mvc.append(cand)
    if (0, 0) not in mvc:
        mvc.append((0, 0))
    return [(y, x) for x, y in mvc]


# ---- generated inputs -----------------------------------------------------------------------------------------------------------
def pictures(c):
    """(src, ref): two uint8 planes of (pic_h + 2 org_y) x (pic_w + 2 org_x), the padded pictures, sample (0, 0) at (org_y, org_x)."""
    g = c.geo
    H, W = g.pic_h + 2 * g.org_y, g.pic_w + 2 * g.org_x
    kind, seed, prm = c.pic
    rs = np.random.RandomState(seed)
    by, bx = g.org_y + g.blk_y, g.org_x + g.blk_x
    if kind == "tex":          # a smooth texture; the source is the reference moved by prm["shift"] (dy, dx) plus noise
        cell = prm.get("cell", 6)
        gh, gw = H // cell + 3, W // cell + 3
        grid = rs.randint(8, 248, (gh, gw)).astype(np.int64)
        yy, xx = np.arange(H), np.arange(W)
        a, u, b, v = yy // cell, yy % cell, xx // cell, xx % cell
        top = grid[a][:, b] * (cell - v) + grid[a][:, b + 1] * v
        bot = grid[a + 1][:, b] * (cell - v) + grid[a + 1][:, b + 1] * v
        ref = (top * (cell - u)[:, None] + bot * u[:, None] + cell * cell // 2) // (cell * cell)
        n = prm.get("noise", 2)
        ref = np.clip(ref + rs.randint(-n, n + 1, (H, W)), 0, 255)
        dy, dx = prm.get("shift", (0, 0))
        src = np.clip(np.roll(ref, (-dy, -dx), (0, 1)) + rs.randint(-n, n + 1, (H, W)), 0, 255)
        return src.astype(np.uint8), ref.astype(np.uint8)
    if kind == "paste":        # noise everywhere; the source block copied into the reference at prm["at"] = [(dy, dx, noise), ..] from the block
        ref = rs.randint(0, 256, (H, W))
        src = rs.randint(0, 256, (H, W))
        blk = src[by:by + c.h, bx:bx + c.w]
        for dy, dx, noise in prm["at"]:
            ref[by + dy:by + dy + c.h, bx + dx:bx + dx + c.w] = np.clip(blk + (rs.randint(-noise, noise + 1, blk.shape) if noise else 0), 0, 255)
        return src.astype(np.uint8), ref.astype(np.uint8)
    if kind == "flat":         # source and reference blocks that differ by prm["delta"] everywhere: every position costs the same
        ref = np.full((H, W), 100, np.int64)
        src = np.full((H, W), 100 + prm["delta"], np.int64)
        return src.astype(np.uint8), ref.astype(np.uint8)
    raise ValueError(kind)


def memory(plane):
    """A picture as the flat bytes a kernel addresses, TAIL bytes of filler behind it"""
    return np.concatenate([plane.reshape(-1), arena.pattern(TAIL)])


# ---- restatement ----------------------------------------------------------------------------------------------------------------
def s32(v):
    v &= M1
    return v - (1 << 32) if v >= 1 << 31 else v


class Search:
    """One descriptor's search on a case's pictures.  After run(): result (RESULT_FIELDS), `stages` (the arguments and the outcome of
    every md_full_pel_search call, for the stage-by-stage pin) and `events`, what the coverage conditions of the golden script name."""

    def __init__(self, c, src=None, ref=None, tables=None, skip_rule=True):
        self.c, g = c, c.geo
        if src is None:
            src, ref = pictures(c)
        self.stride = ref.shape[1]
        self.mem = memory(ref).astype(np.int64)
        by, bx = g.org_y + g.blk_y, g.org_x + g.blk_x
        self.src = src[by:by + c.h, bx:bx + c.w].astype(np.int64)
        self.at0 = by * self.stride + bx                         # the co-located first sample
        self.idx = (np.arange(c.h)[:, None] * self.stride + np.arange(c.w)[None, :]).reshape(-1)
        self.src_flat = self.src.reshape(-1)
        self.mvj, self.mvrow, self.mvcol = tables or mv_cost_tables()
        self.levels = case_levels(c)
        self.skip_rule = skip_rule
        self.events, self.stages = collections.Counter(), []
        self.run()

    def distortion(self, dist, px, py):
        """at the full-pel offset (px, py) from the co-located block"""
        r = self.mem[self.at0 + py * self.stride + px + self.idx]
        d = r - self.src_flat
        if dist == SAD:
            return int(np.abs(d).sum())
        sse = int((d * d).sum())
        if dist == SSD:
            return sse & M1
        s = int(d.sum())
        return (sse - ((s * s) // (self.c.w * self.c.h) & M1)) & M1

    # svt_mv_err_cost (mcomp.c:44-68) as an int
    def mv_cost(self, row, col):
        c = self.c
        dr, dc = i16(row - c.ref_mv[0]), i16(col - c.ref_mv[1])
        l1 = i16(abs(dr)) + i16(abs(dc))
        if c.cost_type == ENTROPY:
            joint = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
            lo, hi = min(max(dr, MV_LOW), MV_UPP), min(max(dc, MV_LOW), MV_UPP)
            if lo != dr or hi != dc:
                self.events["table_clamp"] += 1
            rate = int(self.mvj[joint]) + int(self.mvrow[lo - MV_LOW]) + int(self.mvcol[hi - MV_LOW])
            return s32((rate * c.epb + (1 << 13)) >> 14)
        if c.cost_type == OPT:
            return s32((s32(l1 << 8) * c.epb + (1 << 13)) >> 14)
        return {L1_LOWRES: (2 * l1) >> 3, L1_MIDRES: 0, L1_HDRES: l1 >> 3, NONE: 0}[c.cost_type]

    def full_pel_search(self, dist, mvx, mvy, sx, ex, sy, ey, step, lev0, lev0_range, best, clip=True, cost=True):
        """md_full_pel_search; best = (mvx, mvy, cost) in, the same out"""
        c, g = self.c, self.c.geo
        cx, cy = mvx >> 3, mvy >> 3
        args = (dist, mvx, mvy, sx, ex, sy, ey, step, int(lev0), tuple(lev0_range), best)
        clips = []
        if clip:
            bx, by = g.blk_x + cx, g.blk_y + cy
            if bx + sx < -g.org_x + 1:
                sx = i16((-g.org_x + 1) - bx)
                clips.append("left")
            if bx + c.w + ex > g.org_x + g.pic_w - 1:
                ex = i16((g.org_x + g.pic_w - 1) - (bx + c.w))
                clips.append("right")
            if by + sy < -g.org_y + 1:
                sy = i16((-g.org_y + 1) - by)
                clips.append("top")
            if by + c.h + ey > g.org_y + g.pic_h - 1:
                ey = i16((g.org_y + g.pic_h - 1) - (by + c.h))
                clips.append("bottom")
        visited = []
        psad = dist == SAD and c.psad and ex - sx >= 7
        if psad:      # md_full_pel_search_large_lbd -> svt_pme_sad_loop_kernel_c: row-major
            remain = 8 - c_rem(ex - sx, 8)
            width = i16(max(ex, ex + (0 if remain == 8 else remain))) - sx
            self.events[("psad_width", ex - sx)] += 1
            col_num, step_x = 0, 1
            ys = 0
            while ys < i16(ey - sy + 1):
                xs = 0
                while xs < width:
                    if width - xs < 8 and col_num == 0:
                        xs += step_x
                        continue
                    if col_num == 7:
                        col_num, nxt = 0, step
                    else:
                        col_num, nxt = col_num + 1, 1
                    step_x = nxt
                    visited.append((sx + xs, sy + ys))
                    xs += step_x
                ys += step
        else:         # column-major
            px = sx
            while px <= ex:
                py = sy
                while py <= ey:
                    if step == 2 and lev0 and (lev0_range[0] <= px + cx <= lev0_range[1] and lev0_range[2] <= py + cy <= lev0_range[3] and
                                               c_rem(px, 4) == 0 and c_rem(py, 4) == 0):
                        self.events["lev0_skip"] += 1
                        if self.skip_rule:
                            py += step
                            continue
                    visited.append((px, py))
                    py += step
                px += step
        if visited:
            self.events[("scan", "psad" if psad else "generic", dist, c.w, c.h)] += 1
            self.events[("clips", tuple(clips))] += 1
            if (mvx | mvy) & 7:
                self.events[("non_full_pel_centre", c.mode)] += 1
        else:
            self.events[("empty_stage", c.mode, bool(clips))] += 1
        span = (max(p[0] for p in visited) - min(p[0] for p in visited), max(p[1] for p in visited) - min(p[1] for p in visited)) if visited else (0, 0)
        first_tile = None
        for px, py in visited:
            d = self.distortion(SAD if psad else dist, cx + px, cy + py)
            row, col = i16(mvy + py * 8), i16(mvx + px * 8)
            total = d + (self.mv_cost(row, col) if cost else 0)
            if total < 0 or total > M1:
                self.events["wrap"] += 1
            total &= M1
            if first_tile is None:
                first_tile = (px, py)
            if total < best[2]:
                best = (col, row, total)
                if (px - first_tile[0]) // TILE or (py - first_tile[1]) // TILE:
                    self.events[("winner_beyond_first_tile", SAD if psad else dist)] += 1
        self.stages.append(StageLog(args, clip, cost, best, len(visited), span, (sx, sy, width, i16(ey - sy + 1)) if psad else None))
        return best

    def run(self):
        c = self.c
        none = (i16(M1), i16(M1), M1)
        stage = lambda mv, lv, step, best, lev0=False, rng=(0, 0, 0, 0): self.full_pel_search(  # noqa: E731
            c.dist, mv[0], mv[1], lv[0], lv[1], lv[2], lv[3], step, lev0, rng, best)
        if c.mode == MVP:
            best, idx = (0, 0, M1), 0
            for i, (row, col) in enumerate(c.mvs):
                new = self.full_pel_search(VAR, col, row, 0, 0, 0, 0, 1, False, (0, 0, 0, 0), best, clip=False, cost=False)
                if new[2] < best[2]:
                    idx = i
                best = new
            mv = c.mvs[idx] if best[2] != M1 else (0, 0)
            self.result = (mv[0], mv[1], best[2], 0, 0, idx)
        elif c.mode == SQ:
            me = (c.mvs[0][1], c.mvs[0][0])            # (x, y)
            pa = stage(me, (0, 0, 0, 0), 1, none)
            th = c.th * c.w * c.h
            sam = c.sam if c.sq_size <= 64 and pa[2] > th else 0
            self.events["gate_equal" if pa[2] == th else "gate_open" if pa[2] > th else "gate_shut"] += 1
            best, rng = none, (0, 0, 0, 0)
            if sam:
                self.events[("levels", tuple(bool(lv.enabled) for lv in self.levels))] += 1
                for l, lv in enumerate(self.levels):
                    if not lv.enabled:
                        continue
                    if l == 0:
                        rng = (i16((me[0] >> 3) + lv.start_x), i16((me[0] >> 3) + lv.end_x), i16((me[1] >> 3) + lv.start_y), i16((me[1] >> 3) + lv.end_y))
                    lev0 = l == 1 and self.levels[0].enabled and self.levels[0].step == 4
                    best = stage(me, lv[2:], lv.step, best, lev0, rng)
                    me = (best[0], best[1])
            self.result = (me[1], me[0], best[2], pa[2], int(sam != 0), 0)
        elif c.mode == NSQ:
            centre = (c.mvs[0][1], c.mvs[0][0], M1)
            rounded = [(i16((col + 4) & ~7), i16((row + 4) & ~7)) for row, col in c.mvs]
            if len(set(rounded)) < len(rounded):
                self.events["mvc_duplicates"] += 1
            for mv in rounded:
                centre = stage(mv, (0, 0, 0, 0), 1, centre)
            hw, hh = c.nsq[0] >> 1, c.nsq[1] >> 1
            best = stage(centre[:2], (-hw, hw, -hh, hh), 4, none)
            best = stage(best[:2], (-2, 2, -2, 2), 2, best)
            best = stage(best[:2], (-1, 1, -1, 1), 1, best)
            take = best[2] < centre[2]
            self.events["nsq_takes" if take else "nsq_ties" if best[2] == centre[2] else "nsq_loses"] += 1
            mv = best if take else centre
            self.result = (mv[1], mv[0], best[2], centre[2], 0, 0)
        else:
            lv = self.levels[0]
            best = stage((c.mvs[0][1], c.mvs[0][0]), lv[2:], 1, none)
            self.result = (best[1], best[0], best[2], 0, 0, 0)

    def record(self):
        return tuple(int(v) for v in self.result)


def case_levels(c):
    if c.mode == SQ and c.ctrls is not None:
        return sq_windows(c.ctrls, c.sam, scaled_distance(c.pocd))
    return list(c.levels) if c.levels else [Level(0, 0, 0, 0, 0, 0)] * 3


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _window(r, step=1, enabled=1):
    return Level(enabled, step, -r, r, -r, r)


def _cases():
    out = []
    off = Level(0, 1, 0, 0, 0, 0)

    def add(name, mode, w, h, **kw):
        i = len(out)
        room = kw.pop("room", 24)         # picture samples around the block
        d = dict(dist=i % 3, psad=0, cost_type=(i // 2) % 6, epb=(60, 350, 2400)[i % 3], ref_mv=((5, -11, 0, 18)[i % 4], (-7, 3, 0, -20)[(i // 2) % 4]),
                 geo=Geo(w + 2 * room, h + 2 * room, 16, 16, room, room), mvs=[(0, 0)], levels=None, ctrls=None, sam=1, pocd=1, th=0, sq_size=max(w, h), nsq=(0, 0),
                 sub=None, geom_org=(0, 0), pic=("tex", 3000 + i, {"shift": ((i * 3) % 7 - 3, (i * 5) % 7 - 3)}))
        d.update(kw)
        out.append(Case(name, mode, w, h, **d))

    # every size under every distortion type: a 9 x 9 PME window (13 x 13 with psad for SAD: both scans on every size)
    for w, h in SIZES:
        for dist in (SAD, VAR, SSD):
            big = w * h > 4096
            r = 1 if w * h > 8192 else 2 if big else 4
            add("size", PME, w, h, dist=dist, levels=[_window(r), off, off], mvs=[(8, -8)])
        add("size_psad", PME, w, h, dist=SAD, psad=1, levels=[Level(1, 1, -4, 4, -1, 1), off, off], mvs=[(-8, 8)])
    # all six cost types, generic and psad
    for ct in range(6):
        for psad in (0, 1):
            add("cost", PME, 8, 8, dist=SAD, psad=psad, cost_type=ct, epb=(90, 700, 5000)[ct % 3], levels=[_window(5), off, off])
            add("cost", NSQ, 16, 4, dist=VAR, psad=psad, cost_type=ct, nsq=(15, 15), mvs=[(16, 8), (0, 0)], sq_size=16, sub={})
    # windows: a single position, +-1, +-2 at step 2, 9 x 9
    for w, h in ((4, 4), (16, 16), (64, 16)):
        for dist in (SAD, VAR, SSD):
            add("single", PME, w, h, dist=dist, levels=[_window(0), off, off], mvs=[(16, -24)])
            add("pm1", PME, w, h, dist=dist, levels=[_window(1), off, off])
            add("pm2", SQ, w, h, dist=dist, levels=[off, _window(2, 2), off], th=0)
            add("nine", PME, w, h, dist=dist, psad=1, levels=[_window(4), off, off])
    # psad widths: end_x - start_x in 7, 8, 9, 15, 16, 17, steps 1, 2 and 4 (PME has step 1; SQ levels carry the steps)
    for width in (7, 8, 9, 15, 16, 17):
        for step in (1, 2, 4):
            lv = Level(1, step, -(width // 2), width - width // 2, -4, 4)
            add("psad_width", SQ, (4, 8, 16)[step % 3], (4, 8, 16)[step % 3], dist=SAD, psad=1, levels=[off, off, lv] if step == 1 else [lv, off, off], room=32)
    # each of the four clips binding alone, and clips that empty a window
    edge = {"left": (2, 30), "right": (58, 30), "top": (30, 2), "bottom": (30, 58)}
    for side, (bx, by) in edge.items():
        for psad in (0, 1):
            add("clip_" + side, PME, 8, 8, dist=(SAD, VAR)[psad ^ 1] if psad == 0 else SAD, psad=psad, geo=Geo(68, 68, 8, 8, bx, by), levels=[_window(12), off, off])
        add("clip_" + side, SQ, 8, 8, dist=SSD, geo=Geo(68, 68, 8, 8, bx, by), levels=[_window(12, 4), _window(6, 2), _window(1)])
    add("clip_empty", PME, 8, 8, dist=SAD, geo=Geo(68, 68, 8, 8, 58, 30), levels=[_window(3), off, off], mvs=[(0, 112)])      # mv 14 samples right: end < start
    add("clip_empty", SQ, 8, 8, dist=VAR, geo=Geo(68, 68, 8, 8, 30, 2), levels=[_window(8, 4), _window(2, 2), _window(1)], mvs=[(-160, 0)])
    add("clip_empty", NSQ, 8, 4, dist=SAD, geo=Geo(68, 68, 8, 8, 58, 30), nsq=(15, 15), mvs=[(0, 160), (0, 152)], sq_size=8)   # item 7: (-1, -1) centres
    add("clip_empty", NSQ, 16, 8, dist=SSD, geo=Geo(68, 68, 8, 8, 30, 2), nsq=(7, 7), mvs=[(-88, 0)], sq_size=16)
    # the SQ gate: open, shut, equal (shut); sq_size above 64; multiplier 0 with the gate open
    flat = ("flat", 1, {"delta": 3})
    for name, th in (("gate_open", 2), ("gate_equal", 3), ("gate_shut", 4)):      # MV_COST_OPT at ref_mv costs nothing: pa_me_cost is the SAD, 3 * 64
        add(name, SQ, 8, 8, dist=SAD, pic=flat, th=th, ctrls=sq_level_ctrls(4), sam=2, cost_type=OPT, ref_mv=(0, 0))
    add("gate_128", SQ, 128, 128, dist=SAD, th=0, ctrls=sq_level_ctrls(4), sam=3, sq_size=128)
    add("gate_sam0", SQ, 16, 16, dist=VAR, th=0, ctrls=sq_level_ctrls(4), sam=0)
    # md_sq_motion_search under the four levels' controls, both scans, 4 x 4 so that the level-0 window may be large
    for level in (1, 2, 3, 4):
        for psad in (0, 1):
            add("sq_level", SQ, 4, 4, dist=SAD, psad=psad, th=0, ctrls=sq_level_ctrls(level), sam=1, pocd=1, room=48, cost_type=(ENTROPY, OPT)[psad])
    add("sq_level", SQ, 16, 16, dist=VAR, th=1, ctrls=sq_level_ctrls(3), sam=1, pocd=2, room=56, cost_type=ENTROPY)
    add("sq_level", SQ, 8, 8, dist=SSD, th=1, ctrls=sq_level_ctrls(4), sam=3, pocd=8, room=56, cost_type=OPT)
    # every subset of the three sparse levels
    for mask in range(8):
        ct = sq_level_ctrls(4)._replace(enabled=(mask & 1, mask >> 1 & 1, mask >> 2 & 1), w=(33, 13, 3), h=(33, 13, 3))
        add("subset", SQ, 8, 8, dist=(SAD, VAR, SSD)[mask % 3], psad=mask & 1, th=0, ctrls=ct, sam=1, room=40, cost_type=(ENTROPY, OPT)[mask % 2])
    # the level-0 skip: level 0 on the psad path leaves columns 8 .. 10 of every 11 unvisited; the source sits in one of them, four columns
    # left of the level-0 winner, where the generic level 1 (narrow) would find it but for the skip
    add("lev0_skip", SQ, 4, 4, dist=SAD, psad=1, cost_type=NONE, th=0, room=40,
        levels=[Level(1, 4, -12, 12, -12, 12), Level(1, 2, -4, 0, 0, 0), off], pic=("paste", 77, {"at": [(0, 0, 9), (0, -4, 0)]}))
    add("lev0_skip", SQ, 16, 16, dist=VAR, psad=0, th=0, room=40, levels=[_window(8, 4), _window(6, 2), _window(1)])
    # NSQ: a result that loses to the centre, one that ties it, one that wins; MVC duplicates after rounding; six MVCs from sub-blocks
    add("nsq_loses", NSQ, 16, 8, dist=SAD, cost_type=NONE, nsq=(15, 15), mvs=[(0, 0)], sq_size=16, pic=("paste", 5, {"at": [(0, 0, 0)]}))
    add("nsq_ties", NSQ, 16, 8, dist=SAD, cost_type=NONE, nsq=(15, 15), mvs=[(0, 0)], sq_size=16, pic=("tex", 6, {"shift": (0, 0), "cell": 12, "noise": 1}))
    add("nsq_wins", NSQ, 16, 8, dist=SAD, cost_type=NONE, nsq=(15, 15), mvs=[(8, 8)], sq_size=16, pic=("paste", 7, {"at": [(5, -3, 0)]}))
    add("nsq_dup", NSQ, 8, 16, dist=VAR, nsq=(7, 7), mvs=[(9, 3), (11, 5), (8, 0), (0, 0)], sq_size=16)
    sub = {i: (x, y) for i, (x, y) in zip(range(21, 25), ((3, -2), (4, -2), (-5, 1), (2, 6)))}
    add("nsq_sub", NSQ, 32, 8, dist=SAD, psad=1, nsq=(15, 15), sq_size=32, sub=sub, mvs=nsq_mvcs((10, -6), 32, 8, 32, (0, 0), sub), cost_type=ENTROPY)
    sub = {i: (x, y) for i, (x, y) in zip((5, 6, 9, 10, 21), ((1, 1), (-2, 0), (1, 1), (0, 3), (7, 7)))}
    add("nsq_sub", NSQ, 32, 16, dist=SSD, nsq=(7, 15), sq_size=32, sub=sub, mvs=nsq_mvcs((-13, 22), 32, 16, 32, (0, 0), sub), cost_type=OPT)
    for k, (w, h) in enumerate(((4, 16), (16, 4), (64, 16), (8, 8))):
        add("nsq", NSQ, w, h, dist=k % 3, psad=k & 1, nsq=((15, 15), (7, 15), (15, 7), (31, 31))[k], sq_size=max(w, h), sub={},
            mvs=nsq_mvcs(((-20, 12), (7, 0), (0, 0), (12, 12))[k], w, h, max(w, h), (0, 0), {}), cost_type=(ENTROPY, OPT)[k % 2], room=32)
    # MVP scoring: 1 .. 4 vectors, ties in index order, vectors that are not full-pel
    for k, (w, h) in enumerate(((4, 4), (16, 16), (32, 8), (64, 64), (128, 128))):
        add("mvp", MVP, w, h, mvs=[(8 * (k - 2), -16), (5, 13), (-17, 9), (24, 8 * k)][:1 + (k + 3) % 4])
    add("mvp_tie", MVP, 8, 8, mvs=[(16, 16), (0, -8), (0, -5), (-8, 0)], pic=("paste", 8, {"at": [(0, -1, 0), (-1, 0, 0)]}))
    # a uint32_t wrap of the cost: MV_COST_OPT far from ref_mv under a large error_per_bit; a vector difference beyond the tables' ends
    add("wrap", PME, 16, 16, dist=SSD, cost_type=OPT, epb=1 << 25, ref_mv=(-8000, 8000), levels=[_window(4), off, off])
    add("wrap", SQ, 8, 8, dist=SAD, psad=1, cost_type=OPT, epb=1 << 25, ref_mv=(9000, -7000), th=0, levels=[_window(8, 4), _window(6, 2), _window(1)])
    add("far_ref", PME, 16, 16, dist=VAR, cost_type=ENTROPY, ref_mv=(16380, -16383), levels=[_window(4), off, off], mvs=[(-16, 24)])
    add("far_ref", NSQ, 8, 8, dist=SAD, psad=1, cost_type=ENTROPY, ref_mv=(-16384, 16384), nsq=(15, 15), mvs=[(8, -8), (0, 0)], sq_size=8)
    # the tie that tells the scans apart: the source at (x, y) = (-6, 5) and (4, -5): the generic loop finds (-6, 5) first, the psad scan (4, -5)
    two = ("paste", 9, {"at": [(5, -6, 0), (-5, 4, 0)]})
    add("scan_tie", PME, 8, 8, dist=SAD, psad=0, cost_type=NONE, levels=[_window(8), off, off], pic=two)
    add("scan_tie", PME, 8, 8, dist=SAD, psad=1, cost_type=NONE, levels=[_window(8), off, off], pic=two)
    # windows larger than the tile, per distortion type: the winner beyond the first tile, and a tie across tiles
    far = ("paste", 10, {"at": [(30, -25, 0), (-28, 33, 0)]})
    for dist, psad in ((SAD, 0), (SAD, 1), (VAR, 0), (SSD, 0)):
        add("tiles", PME, 4, 4, dist=dist, psad=psad, cost_type=NONE, levels=[_window(40), off, off], pic=far, room=48)
    add("tiles", SQ, 4, 4, dist=SAD, psad=1, cost_type=ENTROPY, th=0, levels=[_window(44, 4), _window(6, 2), _window(1)], room=56,
        pic=("paste", 11, {"at": [(36, -40, 0)]}))
    add("tiles", SQ, 8, 8, dist=VAR, cost_type=OPT, th=0, levels=[_window(44, 4), _window(6, 2), _window(1)], room=56, pic=("paste", 12, {"at": [(-40, 39, 3)]}))
    add("tiles", NSQ, 4, 16, dist=SSD, cost_type=NONE, nsq=(95, 95), mvs=[(0, 0)], sq_size=16, room=56, pic=("paste", 13, {"at": [(41, 37, 0), (-43, -39, 0)]}))
    return out


CASES = _cases()
# the windows of md_sq_motion_search: the four md_sq_mv_search_levels x search_area_multiplier 1 .. 3 x picture distances 1, 2, 8, 16
WINDOW_CASES = [(level, sam, dist) for level in (1, 2, 3, 4) for sam in (1, 2, 3) for dist in (1, 2, 8, 16)]


class Golden:
    def __init__(self, path=GOLD):
        z = np.load(path)
        self.results, self.windows = z["results"], z["windows"]     # [CASES][RESULT_FIELDS], [WINDOW_CASES][3 levels][start_x, end_x, start_y, end_y]
        assert len(self.results) == len(CASES) and len(self.windows) == len(WINDOW_CASES)

    def record(self, i):
        return tuple(int(v) for v in self.results[i])


# ---- the reference's own functions ----------------------------------------------------------------------------------------------
PIN_MVP, PIN_SQ, PIN_NSQ, PIN_STAGE = range(4)


class PinArgs(C.Structure):
    _fields_ = ([(f, C.c_int32) for f in ("mode", "w", "h", "sq_size", "stride", "pic_width", "blk_org_x", "blk_org_y", "org_x", "org_y", "max_width",
                                          "max_height", "ref_row", "ref_col", "cost_opt", "error_per_bit", "dist_type", "enable_psad", "n_mv")] +
                [("mv", C.c_int32 * 12)] + [(f, C.c_int32) for f in ("pame_distortion_th", "multiplier_dial", "poc_distance")] +
                [(f, C.c_int32 * 3) for f in ("lev_enabled", "lev_step", "lev_w", "lev_h", "lev_max_w", "lev_max_h", "lev_multiplier")] +
                [(f, C.c_int32) for f in ("nsq_width", "nsq_height", "blk_geom_org_x", "blk_geom_org_y")] + [("sub_mv", C.c_int32 * 170)] +
                [(f, C.c_int32) for f in ("start_x", "end_x", "start_y", "end_y", "step", "lev0_performed")] + [("lev0", C.c_int32 * 4)] +
                [("best_mvx", C.c_int32), ("best_mvy", C.c_int32), ("best_cost", C.c_uint32)])


class Pin:
    """tests/fpel_pin_driver.c built into `directory` against oracle/_ref/libsvtref.so"""

    def __init__(self, ref, directory):
        from support import build_pin
        self.ref, self.lib = ref, build_pin(directory, os.path.join(HERE, "fpel_pin_driver.c"))
        V = C.c_void_p
        self.lib.pin_fpel.argtypes = [V] * 7
        self.lib.pin_psad.argtypes = [C.c_int32] * 4 + [V] * 4 + [C.c_uint32, V, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_int32] * 7 + [V]
        self.lib.pin_mv_cost.argtypes = [C.c_int32] * 6 + [V] * 3
        self.lib.pin_pu_tables.argtypes = self.lib.pin_constants.argtypes = [V]
        self.lib.pin_scaled_distance.argtypes, self.lib.pin_scaled_distance.restype = [C.c_uint16], C.c_uint16
        self.mvj, self.mvrow, self.mvcol = mv_cost_tables()
        self.tables = (self.mvj.ctypes.data, self.mvrow.ctypes.data - 4 * MV_LOW, self.mvcol.ctypes.data - 4 * MV_LOW)

    def base(self, c, src, ref):
        g = c.geo
        a = PinArgs()
        a.w, a.h, a.sq_size, a.stride, a.pic_width = c.w, c.h, c.sq_size, ref.shape[1], g.pic_w
        a.blk_org_x, a.blk_org_y, a.org_x, a.org_y, a.max_width, a.max_height = g.blk_x, g.blk_y, g.org_x, g.org_y, g.pic_w, g.pic_h
        a.ref_row, a.ref_col, a.cost_opt, a.error_per_bit, a.dist_type, a.enable_psad = c.ref_mv[0], c.ref_mv[1], int(c.cost_type == OPT), c.epb, c.dist, c.psad
        a.n_mv = len(c.mvs)
        for i, (row, col) in enumerate(c.mvs):
            a.mv[2 * i], a.mv[2 * i + 1] = row, col
        return a

    def call(self, a, src, ref, tables=None):
        out = np.zeros(9, np.int64)
        self.lib.pin_fpel(C.addressof(a), src.ctypes.data, ref.ctypes.data, *(tables or self.tables), out.ctypes.data)
        return [int(v) for v in out]

    def windows(self, ct, sam, pocd):
        """The three windows of md_sq_motion_search before the clip, observed on the function itself: one level enabled at a time, no
        vector cost, a 16 x 16 source of 255 on a reference that brightens (then darkens) by 1 every 8 samples along x + y, so that every
        step right or down lowers (raises) the SAD by 32: the winner is the window's far (near) corner.  Level 0 also through
        ctx->sprs_lev0_*."""
        n, org, at = 1100, 16, 542
        yy, xx = np.mgrid[0:n + 2 * org, 0:n + 2 * org]
        up = ((xx + yy) // 8).astype(np.uint8)
        refs = [np.ascontiguousarray(up), np.ascontiguousarray(250 - up)]
        src = np.full_like(up, 255)
        zero = np.zeros(2 * MV_UPP + 1, np.int32)
        tables = (zero.ctypes.data, zero.ctypes.data - 4 * MV_LOW, zero.ctypes.data - 4 * MV_LOW)
        c = Case("windows", SQ, 16, 16, SAD, 0, ENTROPY, 1, (0, 0), Geo(n, n, org, org, at, at), [(0, 0)], None, ct, sam, pocd, 0, 16, (0, 0), None, (0, 0), None)
        out = []
        for l in range(3):
            corners = []
            for ref in refs:
                a = self.base(c, src, ref)
                a.mode, a.pame_distortion_th, a.multiplier_dial, a.poc_distance = PIN_SQ, 0, sam, pocd
                for f, v in zip(("lev_enabled", "lev_step", "lev_w", "lev_h", "lev_max_w", "lev_max_h", "lev_multiplier"), ct):
                    for k in range(3):
                        getattr(a, f)[k] = v[k] if f != "lev_enabled" else int(k == l)
                o = self.call(a, src, ref, tables)
                assert o[0] % 8 == 0 and o[1] % 8 == 0
                corners.append((o[0] // 8, o[1] // 8))
                if l == 0:
                    lev0 = tuple(o[5:9])
            win = (corners[1][0], corners[0][0], corners[1][1], corners[0][1])
            assert l or win == lev0, (win, lev0)
            out.append(win)
        return out

    def function(self, c, src, ref):
        """What the reference's own function leaves for the case, or None where only its stages can be pinned: MVP (row, col, dist, idx);
        SQ with controls (row, col) of *me_mv and ctx->sprs_lev0_*; NSQ (row, col) of *me_mv"""
        a = self.base(c, src, ref)
        if c.mode == MVP:
            a.mode = PIN_MVP
            o = self.call(a, src, ref)
            return (o[1], o[0], o[2], o[3])
        if c.mode == SQ and c.ctrls is not None and c.cost_type in (ENTROPY, OPT):
            a.mode, a.pame_distortion_th, a.multiplier_dial, a.poc_distance = PIN_SQ, c.th, c.sam, c.pocd
            for l in range(3):
                for f, v in zip(("lev_enabled", "lev_step", "lev_w", "lev_h", "lev_max_w", "lev_max_h", "lev_multiplier"), c.ctrls):
                    getattr(a, f)[l] = v[l]
            o = self.call(a, src, ref)
            return (o[1], o[0], tuple(o[5:9]))
        if c.mode == NSQ and c.cost_type in (ENTROPY, OPT) and c.sub is not None:
            a.mode, a.nsq_width, a.nsq_height, a.blk_geom_org_x, a.blk_geom_org_y = PIN_NSQ, c.nsq[0], c.nsq[1], c.geom_org[0], c.geom_org[1]
            for i in range(85):
                a.sub_mv[2 * i] = 0x7FFF
            for i, (x, y) in (c.sub or {}).items():
                a.sub_mv[2 * i], a.sub_mv[2 * i + 1] = x, y
            o = self.call(a, src, ref)
            return (o[1], o[0])
        return None

    def stage(self, c, src, ref, st):
        """One logged stage of a Search through md_full_pel_search (MV_COST_ENTROPY / _OPT and the MVP stage apart: those go through
        psad() / mv_cost() and the MVP loop)"""
        dist, mvx, mvy, sx, ex, sy, ey, step, lev0, rng, best = st.args
        a = self.base(c, src, ref)
        a.mode, a.dist_type = PIN_STAGE, dist
        a.mv[0], a.mv[1] = mvy, mvx
        a.start_x, a.end_x, a.start_y, a.end_y, a.step, a.lev0_performed = sx, ex, sy, ey, step, lev0
        for k in range(4):
            a.lev0[k] = rng[k]
        a.best_mvx, a.best_mvy, a.best_cost = best
        o = self.call(a, src, ref)
        return (o[0], o[1], o[2])

    def mv_cost(self, c, row, col):
        return self.lib.pin_mv_cost(c.cost_type, c.epb, c.ref_mv[0], c.ref_mv[1], row, col, *self.tables)

    def psad(self, c, src, ref, mvx, mvy, sx, sy, width, height, step, best):
        """svt_pme_sad_loop_kernel_c as md_full_pel_search_large_lbd calls it, under the case's cost type"""
        g = c.geo
        stride = ref.shape[1]
        s_at = (g.org_y + g.blk_y) * stride + g.org_x + g.blk_x
        r_at = s_at + ((mvy >> 3) + sy) * stride + (mvx >> 3) + sx
        out = np.array(best, np.int64)
        self.lib.pin_psad(c.cost_type, c.epb, c.ref_mv[0], c.ref_mv[1], *self.tables, src.ctypes.data + s_at, stride, ref.ctypes.data + r_at, stride, c.h, c.w,
                          sx, sy, width, height, step, mvx, mvy, out.ctypes.data)
        return tuple(int(v) for v in out)

    def constants(self):
        out = np.zeros(16, np.int32)
        self.lib.pin_constants(out.ctypes.data)
        return [int(v) for v in out]

    def pu_table(self):
        out = np.zeros(85 * 4, np.int32)
        self.lib.pin_pu_tables(out.ctypes.data)
        return [tuple(int(v) for v in r) for r in out.reshape(85, 4)]


def pin_pictures(c):
    """The case's pictures as contiguous memory with TAIL bytes behind each, shaped as pictures: (src, ref, src view, ref view)"""
    src, ref = pictures(c)
    ms, mr = memory(src), memory(ref)
    return ms, mr, ms[:src.size].reshape(src.shape), mr[:ref.size].reshape(ref.shape)


# ---- descriptors for the device -------------------------------------------------------------------------------------------------
class Arena(md_search_cases.Arena):
    """The pictures of a list of cases and the cost tables in one host buffer.  `views`: the planes as widened by the layout, on which the
    restatement is then run (the psad overshoot reads the stride padding)."""

    def __init__(self, cases, layout=lambda i: (0, 0)):
        super().__init__(cases, layout)
        self.planes, self.views = [], []
        for i, c in enumerate(cases):
            placed = [self.place(i, name, plane, memory) for name, plane in zip(("src", "ref"), pictures(c))]
            self.planes.append([(at + (c.geo.org_y + c.geo.blk_y) * stride + c.geo.org_x + c.geo.blk_x, stride) for at, stride, _ in placed])
            self.views.append([buf for _, _, buf in placed])
        self.finish()

    def descs(self, base):
        d = np.zeros(len(self.cases), abi.FPEL_DESC_DTYPE)
        for i, c in enumerate(self.cases):
            (src, src_stride), (ref, ref_stride) = self.planes[i]
            d[i] = fill_desc(c, base + src, base + ref, src_stride, ref_stride)
        return d


def fill_desc(c, src, ref, src_stride, ref_stride):
    d = np.zeros((), abi.FPEL_DESC_DTYPE)
    g = c.geo
    d["src"], d["ref"], d["src_stride"], d["ref_stride"], d["w"], d["h"] = src, ref, src_stride, ref_stride, c.w, c.h
    d["blk_org_x"], d["blk_org_y"], d["ref_org_x"], d["ref_org_y"], d["ref_max_width"], d["ref_max_height"] = g.blk_x, g.blk_y, g.org_x, g.org_y, g.pic_w, g.pic_h
    d["ref_mv"]["row"], d["ref_mv"]["col"] = c.ref_mv
    d["error_per_bit"], d["gate_th"] = c.epb, c.th * c.w * c.h
    for i, (row, col) in enumerate(c.mvs):
        d["mv"][i]["row"], d["mv"][i]["col"] = row, col
    for l, lv in enumerate(case_levels(c)):
        for f in Level._fields:
            d["level"][l][f] = getattr(lv, f)
    for f, v in (("mode", c.mode), ("dist_type", c.dist), ("enable_psad", c.psad), ("mv_cost_type", c.cost_type), ("n_mv", len(c.mvs)),
                 ("gate_enabled", int(c.sq_size <= 64)), ("search_area_multiplier", c.sam), ("nsq_search_width", c.nsq[0]), ("nsq_search_height", c.nsq[1])):
        d[f] = v
    return d


def result_tuple(r):
    """A record of abi.FPEL_RESULT_DTYPE as RESULT_FIELDS"""
    return (int(r["best_mv"]["row"]), int(r["best_mv"]["col"]), int(r["best_cost"]), int(r["aux_cost"]), int(r["expanded"]), int(r["mvp_idx"]))
