"""Cases of the luma palette entry points (svt_hip_palette_search_batch, svt_hip_palette_predict_batch, svt_hip_sc_classify), a plain
Python / numpy restatement of what they stand for -- search_palette_luma (palette.c:309-434) over svt_av1_k_means_dim1_c and palette_rd_y,
the palette terms of av1_intra_fast_cost (rd_cost.c:691-704), the palette branch of svt_av1_predict_intra_block and
svt_aom_is_screen_content -- and the calls into the reference's own functions through tests/palette_pin_driver.c.
tests/golden/palette.npz (tests/golden/make_golden_palette.py) holds the rate table and what the reference gave for every case; the
inputs are regenerated from the seeds here.  The restatement works on the pixels, one by one, as the reference does: it shares nothing
with the device's (value, count) formulation."""
import ctypes as C
import os
from collections import Counter, namedtuple

import numpy as np

from svtav1_hip import abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "palette.npz")
DRIVER = os.path.join(HERE, "palette_pin_driver.c")
BAD_PARAMETER, NO_DEVICE = abi.palette_status(abi.SVT_HIP_ERR_BAD_PARAMETER), abi.palette_status(abi.SVT_HIP_ERR_NO_DEVICE)
NAMES = ("svt_hip_palette_search_batch", "svt_hip_palette_predict_batch", "svt_hip_sc_classify")
MAX_SIZE, MAX_CANDS, RECORD_BYTES, COST_SHIFT = abi.PALETTE_MAX_SIZE, abi.PALETTE_MAX_CANDS, C.sizeof(abi.PaletteRecord), 9
# the block sizes svt_aom_allow_palette admits with both sides of 8 .. 64
SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (8, 32), (32, 8), (16, 64), (64, 16)]

# kind: ("levels", n, cell)  n distinct values, cells of cell x cell pixels drawn with skewed odds, every value present
#       ("counts", values, counts)  exactly counts[i] pixels of values[i] (they sum to rows * cols), shuffled; first: data[0] when given
Case = namedtuple("Case", "name w h rows cols bd step max_itr kind seed above left first")


def _c(name, w, h, kind, seed=0, rows=None, cols=None, bd=8, step=1, max_itr=50, above=(), left=(), first=None):
    return Case(name, w, h, rows or h, cols or w, bd, step, max_itr, kind, seed, tuple(above), tuple(left), first)


def _sizes():
    levels = [3, 5, 8, 12, 20, 33, 64, 4, 9, 16, 6, 40, 7, 10]
    out = []
    for bd in (8, 10):
        for i, (w, h) in enumerate(SIZES):
            short = {(16, 32): (27, 16), (64, 32): (32, 50), (8, 32): (31, 8)}.get((w, h), (h, w)) if bd == 10 else (h, w)
            cache = ((40, 90, 200), (90, 131)) if i % 3 == 1 else ((), ())
            out.append(_c(f"s{w}x{h}_{bd}", w, h, ("levels", levels[(i + (bd == 10) * 3) % 14], max(1, min(w, h) // 8)), 100 + i, rows=short[0], cols=short[1],
                          bd=bd, step=1 + (i + bd // 10) % 2, above=cache[0], left=cache[1]))
    return out


CASES = _sizes() + [
    # the colour counts around the search's limits
    _c("colors_1", 16, 16, ("levels", 1, 1), 1),
    _c("colors_2", 16, 16, ("levels", 2, 1), 2),
    _c("colors_3", 16, 16, ("levels", 3, 1), 3),
    _c("colors_8", 16, 16, ("levels", 8, 1), 4, step=2),
    _c("colors_9", 16, 16, ("levels", 9, 1), 5, step=2),
    _c("colors_64", 16, 16, ("levels", 64, 1), 6),
    _c("colors_65", 16, 16, ("levels", 65, 1), 7),
    _c("colors_64_10", 32, 32, ("levels", 64, 2), 8, bd=10),
    _c("colors_65_10", 32, 32, ("levels", 65, 2), 9, bd=10),
    # rows and cols short of the block
    _c("short_9x13", 16, 16, ("levels", 6, 1), 10, rows=9, cols=13),
    _c("short_3x5", 8, 8, ("levels", 4, 1), 11, rows=3, cols=5, step=2),
    _c("short_cols", 32, 32, ("levels", 10, 2), 12, cols=20),
    _c("short_rows", 64, 64, ("levels", 7, 4), 13, rows=40),
    _c("short_1x1", 8, 8, ("levels", 1, 1), 14, rows=1, cols=1),
    # caches: 1 and 16 entries; a snap at difference 1, none at difference 2
    _c("cache_1", 16, 16, ("counts", (20, 60, 120, 200), (100, 80, 50, 26)), 20, left=(61,)),
    _c("cache_16", 16, 16, ("counts", (20, 60, 120, 200, 250), (90, 70, 50, 26, 20)), 21, above=(1, 22, 30, 59, 77, 100, 150, 251), left=(5, 18, 40, 62, 90, 122, 180, 230)),
    _c("cache_dup", 16, 16, ("counts", (20, 60, 120, 200), (100, 80, 50, 26)), 22, above=(19, 60, 130), left=(19, 60, 201)),
    _c("cache_snap_merge", 16, 16, ("counts", (10, 11, 200), (120, 100, 36)), 23, above=(10,), step=2),
    _c("cache_10", 16, 16, ("counts", (100, 500, 1023), (120, 100, 36)), 24, bd=10, above=(101, 498), left=(1023,)),
    # ties
    _c("tie_top", 16, 16, ("counts", (200, 50, 90, 10, 130), (64, 64, 64, 32, 32)), 30),
    _c("tie_nearest", 16, 16, ("counts", (10, 20, 30, 100), (100, 6, 100, 50)), 31),
    # empty clusters: two in one update (the LCG advances), and a 10-bit first pixel
    _c("empties", 16, 16, ("counts", (0, 1, 2, 255), (100, 80, 50, 26)), 40, first=255),
    _c("empties_10", 16, 16, ("counts", (0, 1, 2, 1023), (100, 80, 50, 26)), 41, bd=10, first=1023),
    _c("empties_wide", 32, 32, ("counts", (3, 4, 5, 6, 7, 900, 1000), (300, 200, 200, 100, 100, 100, 24)), 42, bd=10, first=1000),
    # duplicates that shrink k; 12 survivors (n = 2 never survives, so 6 + 6 is the most there can be)
    _c("dups", 16, 16, ("counts", (0, 1, 254, 255), (100, 80, 50, 26)), 50),
    _c("one_cand", 16, 16, ("counts", (0, 1, 255), (30, 200, 26)), 53, step=2),      # k-means ends on 1, 1, 255
    _c("full_12", 32, 32, ("levels", 24, 2), 51),
    _c("full_12_10", 16, 16, ("levels", 30, 1), 52, bd=10),
    # the iteration cap
    _c("itr_1", 32, 32, ("levels", 40, 1), 60, max_itr=1),
    _c("itr_2", 32, 32, ("levels", 40, 1), 60, max_itr=2),
    _c("itr_50", 32, 32, ("levels", 40, 1), 60),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def make_block(c):
    """The (h, w) samples of a case; what lies beyond rows x cols is a pattern that is no part of the block."""
    rng, top = np.random.RandomState(7000 + c.seed), (1 << c.bd) - 1
    blk = ((np.arange(c.h * c.w).reshape(c.h, c.w) * 37 + 11) % (top + 1)).astype(np.int64)
    if c.kind[0] == "levels":
        _, n, cell = c.kind
        values = np.sort(rng.choice(top + 1, n, replace=False))
        odds = rng.rand(n) ** 3 + 0.02
        g = rng.choice(n, (-(-c.rows // cell), -(-c.cols // cell)), p=odds / odds.sum())
        idx = np.ascontiguousarray(np.kron(g, np.ones((cell, cell), np.int64))[:c.rows, :c.cols])
        flat = idx.reshape(-1)
        if n <= flat.size:      # every value at least once, at scattered places
            flat[rng.choice(flat.size, n, replace=False)] = np.arange(n)
        blk[:c.rows, :c.cols] = values[idx]
    else:
        _, values, counts = c.kind
        assert sum(counts) == c.rows * c.cols, c.name
        flat = np.repeat(np.array(values, np.int64), counts)
        rng.shuffle(flat)
        if c.first is not None:
            k = int(np.flatnonzero(flat == c.first)[0])
            flat[0], flat[k] = flat[k], flat[0]
        blk[:c.rows, :c.cols] = flat.reshape(c.rows, c.cols)
    return blk.astype(np.uint8 if c.bd == 8 else np.uint16)


# ---- the fixture --------------------------------------------------------------------------------------------------------------

_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLD) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


def golden_rates():
    return gold()["ysize"].astype(np.int32).reshape(7, 7), gold()["ycolor"].astype(np.int32).reshape(7, 5, 8)


def golden_record(name):
    """The 496 bytes of the record and the maps [n_cands, h, w]"""
    c = CASE[name]
    return gold()["rec_" + name], gold()["maps_" + name].reshape(-1, c.h, c.w)


def rates_struct(ysize, ycolor):
    r = abi.PaletteRates()
    C.memmove(C.addressof(r), np.concatenate([ysize.reshape(-1), ycolor.reshape(-1)]).astype(np.int32).tobytes(), C.sizeof(r))
    return r


# ---- the restatement: search ------------------------------------------------------------------------------------------------------

def merge_cache(above, left):
    """svt_get_palette_cache_y"""
    a, b, out = list(above), list(left), []

    def add(v):
        if not (out and out[-1] == v):
            out.append(v)
    while a and b:
        if b[0] < a[0]:
            add(b.pop(0))
        else:
            v = a.pop(0)
            add(v)
            if b[0] == v:
                b.pop(0)
    for v in a + b:
        add(v)
    return out


def _assign(data, cen, log):
    d = (data[:, None] - np.array(cen, np.int64)[None, :]) ** 2
    if log is not None and len(cen) > 1:
        s = np.sort(d, axis=1)
        log["tie_nearest"] += int((s[:, 0] == s[:, 1]).sum())
    return d.argmin(axis=1), d        # argmin: the first minimum


def k_means(data, cen, max_itr, log):
    """svt_av1_k_means_dim1_c: (centroids, indices)"""
    data, cen, n, k = data.astype(np.int64), list(cen), len(data), len(cen)
    idx, d = _assign(data, cen, None)
    dist = int(d[np.arange(n), idx].sum())
    for it in range(max_itr):
        pre_dist, pre_cen, pre_idx = dist, list(cen), idx
        count = np.bincount(idx, minlength=k)
        total = np.bincount(idx, weights=data, minlength=k).astype(np.int64)
        state, empties = int(data[0]), 0
        for j in range(k):
            if count[j] == 0:
                full = state * 1103515245 + 12345
                log["wrap"] += full >= 1 << 32
                state = full & 0xFFFFFFFF
                cen[j] = int(data[(state // 65536 % 32768) % n])
                empties += 1
            else:
                cen[j] = int((total[j] + (count[j] >> 1)) // count[j])
        log["empty"] += empties
        log["two_empties"] += empties >= 2
        idx, d = _assign(data, cen, None)
        dist = int(d[np.arange(n), idx].sum())
        if dist > pre_dist:
            cen, idx = pre_cen, pre_idx
            log["exit_worse"] += 1
            break
        if cen == pre_cen:
            log["exit_same"] += 1
            log["itr_max"] = max(log["itr_max"], it + 1)
            break
    else:
        log["exit_cap"] += 1
    return cen, idx


def uniform_cost(n, v):
    """svt_aom_write_uniform_cost"""
    bits = n.bit_length()
    m = (1 << bits) - n
    return ((bits - 1) if v < m else bits) << COST_SHIFT


def _ceil_log2(n):
    return 0 if n < 2 else (n - 1).bit_length()


def color_cost_y(colors, cache, bd):
    """svt_av1_palette_color_cost_y"""
    k = len(colors)
    if cache:
        found, n_in = [False] * k, 0
        for v in cache:
            if n_in >= k:
                break
            for j in range(k):
                if colors[j] == v:
                    found[j], n_in = True, n_in + 1
                    break
        out = [colors[j] for j in range(k) if not found[j]]
    else:
        out = list(colors)
    bits = 0
    if out:
        bits = bd
        if len(out) > 1:
            bits += 2
            deltas = [out[i] - out[i - 1] for i in range(1, len(out))]
            per, rng = max(_ceil_log2(max(deltas + [0]) + 1 - 1), bd - 3), (1 << bd) - out[0] - 1
            for dlt in deltas:
                bits += per
                rng -= dlt
                per = min(per, _ceil_log2(rng))
    return (len(cache) + bits) << COST_SHIFT


def color_contexts(m):
    """svt_aom_get_palette_color_index_context_optimized at every position of the map m: (ctx, re-ordered index); (0, 0) is not meant"""
    m = m.astype(np.int64)
    n = np.full((3,) + m.shape, -1, np.int64)       # left, top, top-left
    n[0][:, 1:], n[1][1:, :], n[2][1:, 1:] = m[:, :-1], m[:-1, :], m[:-1, :-1]
    s = np.stack([np.full(m.shape, 2), np.full(m.shape, 2), np.full(m.shape, 1)])
    a, b, c = n[0] == n[1], n[0] == n[2], n[1] == n[2]
    ab, b_only, c_only = a & b, ~a & b, ~a & ~b & c
    s[0] = s[0] + 2 * a + ab + b_only
    s[1] = s[1] + c_only
    n[1] = np.where(a, -1, n[1])
    n[2] = np.where(ab | b_only | c_only, -1, n[2])
    valid = n != -1
    pos = np.cumsum(valid, axis=0) - valid
    col, scr = np.full(n.shape, -1, np.int64), np.zeros(n.shape, np.int64)
    for i in range(3):
        for k in range(3):
            sel = valid[i] & (pos[i] == k)
            col[k][sel], scr[k][sel] = n[i][sel], s[i][sel]

    def swap(i, j, cond):
        for arr in (col, scr):
            arr[i], arr[j] = np.where(cond, arr[j], arr[i]), np.where(cond, arr[i], arr[j])
    swap(0, 1, (scr[0] < scr[1]) | ((scr[0] == scr[1]) & (col[0] > col[1])))
    swap(0, 2, scr[0] < scr[2])
    swap(1, 2, scr[1] < scr[2])
    idx = m + (col > m).sum(axis=0)
    for i in range(3):
        idx = np.where(col[i] == m, i, idx)      # the last that equals wins, as in the reference's loop
    hashed = scr[0] + 2 * scr[1] + 2 * scr[2]
    lookup = np.array([-1, -1, 0, -1, -1, 4, 3, 2, 1])
    return lookup[np.clip(hashed, 0, 8)], idx


Result = namedtuple("Result", "colors cache cands maps")      # cands: (origin, n, k, colors, size_bits, color_bits, map_bits)


def search(c, blk, ysize, ycolor, log=None):
    """search_palette_luma with the rate terms, on the block of make_block(c)"""
    log = log if log is not None else Counter()
    px = blk[:c.rows, :c.cols].astype(np.int64)
    data = px.reshape(-1)
    values, counts = np.unique(data, return_counts=True)
    colors, cache = len(values), merge_cache(c.above, c.left)
    if c.bd > 8 and data.max() >= 1 << c.bd:
        colors = 0
    if not 1 < colors <= 64:
        return Result(colors, cache, [], [])
    left_counts, top = counts.copy(), []
    for _ in range(min(colors, MAX_SIZE)):
        i = int(np.argmax(left_counts))               # the first of the largest: the lowest value
        log["tie_top"] += int((left_counts == left_counts[i]).sum() > 1)
        top.append(int(values[i]))
        left_counts[i] = 0
    lb, ub, n_max = int(values[0]), int(values[-1]), min(colors, MAX_SIZE)
    tries = [(abi.PALETTE_DOMINANT, n) for n in range(n_max, 1, -c.step)] + [(abi.PALETTE_KMEANS, n) for n in range(n_max, 1, -1)]
    cands, maps, rejected_before = [], [], False
    for origin, n in tries:
        if origin == abi.PALETTE_DOMINANT:
            cen = top[:n]
        elif colors == 2:
            cen = [lb, ub]
        else:
            cen, _ = k_means(data, [lb + (2 * i + 1) * (ub - lb) // n // 2 for i in range(n)], c.max_itr, log)
        # palette_rd_y
        if cache:
            for i in range(n):
                diffs = [abs(cen[i] - v) for v in cache]
                at = diffs.index(min(diffs))
                if diffs[at] <= 1:
                    log["snap"] += cen[i] != cache[at]
                    cen[i] = cache[at]
                elif diffs[at] == 2:
                    log["no_snap_at_2"] += 1
        uniq = sorted(set(cen))
        k = len(uniq)
        log["dup"] += k < n
        if k <= 2:
            log["rejected"] += 1
            rejected_before = True
            continue
        log["slot_reuse"] += rejected_before
        rejected_before = False
        pal = [min(max(v, 0), (1 << c.bd) - 1) for v in uniq]
        idx, _ = _assign(data, uniq, log)
        m = np.zeros((c.h, c.w), np.uint8)
        m[:c.rows, :c.cols] = idx.reshape(c.rows, c.cols)
        m[:c.rows, c.cols:] = m[:c.rows, c.cols - 1:c.cols]
        m[c.rows:, :] = m[c.rows - 1:c.rows, :]
        ctx, new = color_contexts(m[:c.rows, :c.cols])
        cost = ycolor[k - 2][ctx, new]
        bsize_ctx = (c.w * c.h).bit_length() - 1 - 6
        cands.append((origin, n, k, pal, int(ysize[bsize_ctx][k - 2]) + uniform_cost(k, int(m[0, 0])), color_cost_y(pal, cache, c.bd),
                      int(cost.sum() - cost[0, 0])))
        maps.append(m)
    log["max_cands"] = max(log["max_cands"], len(cands))
    return Result(colors, cache, cands, maps)


def record_bytes(res):
    """The device record of a result, as bytes"""
    rec = np.zeros(1, abi.PALETTE_RECORD_DTYPE)
    rec["colors"], rec["n_cands"], rec["n_cache"] = res.colors, len(res.cands), len(res.cache)
    rec["cache"][0, :len(res.cache)] = res.cache
    for i, (origin, n, k, pal, size_bits, color_bits, map_bits) in enumerate(res.cands):
        cand = rec["cand"][0, i]
        cand["origin"], cand["n"], cand["palette_size"] = origin, n, k
        cand["palette_colors"][:k] = pal
        cand["size_bits"], cand["color_bits"], cand["map_bits"] = size_bits, color_bits, map_bits
    return rec.view(np.uint8).reshape(-1).copy()


def maps_array(c, res):
    return np.stack(res.maps).astype(np.uint8) if res.maps else np.zeros((0, c.h, c.w), np.uint8)


# ---- prediction ---------------------------------------------------------------------------------------------------------------

Pred = namedtuple("Pred", "name case cand x y w h is_16bit bd")
PREDS = [
    Pred("p8_whole", "s64x64_8", 0, 0, 0, 64, 64, 0, 8),
    Pred("p8_sub", "s64x64_8", 1, 16, 32, 16, 16, 0, 8),
    Pred("p8_tall", "s64x64_8", 2, 60, 4, 4, 16, 0, 8),
    Pred("p8_last", "s64x64_8", 0, 32, 48, 32, 16, 0, 8),
    Pred("p10_sub", "s64x64_10", 0, 48, 16, 16, 64 - 16, 1, 10),
    Pred("p10_clamp", "cache_10", 0, 8, 4, 8, 8, 1, 10),      # its palette holds 1023, the clamp's own value
    Pred("p16_of_8", "s64x64_8", 0, 8, 8, 8, 8, 1, 8),        # 8-bit colours into uint16 samples
    Pred("p10_small", "s8x8_10", 0, 4, 0, 4, 8, 1, 10),
]


def predict(p, pal, m):
    """dst[r][c] = palette[map[(r + y) * wpx + c + x]], clamped to the bit depth"""
    out = np.minimum(np.array(pal, np.int64), (1 << p.bd) - 1)[m[p.y:p.y + p.h, p.x:p.x + p.w]]
    return out.astype(np.uint16 if p.is_16bit else np.uint8)


def golden_pred(p):
    """The prediction from the fixture's own record and map"""
    rec, maps = golden_record(p.case)
    cand = rec.view(abi.PALETTE_RECORD_DTYPE)[0]["cand"][p.cand]
    return predict(p, cand["palette_colors"], maps[p.cand])


# ---- the screen-content decision ------------------------------------------------------------------------------------------------

ScPlane = namedtuple("ScPlane", "name kind w h stride seed")
SC_PLANES = [
    ScPlane("noise", "noise", 128, 96, 128, 1),
    ScPlane("text", "text", 128, 96, 136, 2),
    ScPlane("between", "between", 160, 96, 160, 3),       # above the sc_class0 threshold, below that of sc_class1
    ScPlane("ragged", "text", 141, 75, 150, 4),           # neither side a multiple of 16
    ScPlane("tiny", "text", 15, 40, 15, 5),               # no whole block
    ScPlane("flat_pairs", "pairs", 64, 64, 64, 6),        # two colours one level apart: counted, variance rounds to 0 against 128
]
SC_PLANE = {p.name: p for p in SC_PLANES}


def make_sc_plane(p):
    rng = np.random.RandomState(9000 + p.seed)
    buf = ((np.arange(p.h * p.stride, dtype=np.uint32) * 29 + 7) & 0xFF).astype(np.uint8).reshape(p.h, p.stride)
    if p.kind == "noise":
        img = rng.randint(0, 256, (p.h, p.w))
    elif p.kind == "text":          # dark strokes on a light page
        img = np.full((p.h, p.w), 235)
        img[rng.rand(p.h, p.w) < 0.18] = 20
        img[rng.rand(p.h, p.w) < 0.04] = 120
    elif p.kind == "pairs":
        img = np.full((p.h, p.w), 128)
        img[::3, ::5] = 129
    else:                           # "between": text in a fifth of the blocks, the rest noise; the text blocks are nearly flat at 128
        img = rng.randint(0, 256, (p.h, p.w))
        for by in range(p.h // 16):
            for bx in range(p.w // 16):
                if (bx + by * (p.w // 16)) % 5 == 0:
                    blk = np.full((16, 16), 128)
                    blk[3, 4] = 129
                    if (bx + by) % 8 == 0:
                        blk[5:9, 2:14] = 30
                    img[16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = blk
    buf[:, :p.w] = img
    return buf


def sc_classify(buf, w, h):
    """svt_aom_is_screen_content: (counts_1, counts_2, blocks, [sc_class0 .. 3])"""
    c1 = c2 = blocks = 0
    for r in range(0, h - 15, 16):
        for c in range(0, w - 15, 16):
            blk = buf[r:r + 16, c:c + 16].astype(np.int64)
            blocks += 1
            if 1 < len(np.unique(blk)) <= 4:
                c1 += 1
                d = blk - 128
                var = int((d * d).sum()) - int(d.sum()) ** 2 // 256
                c2 += (var + 128) >> 8 > 0
    area = w * h
    cls0 = c1 * 256 * 10 > area
    cls1 = cls0 and c2 * 256 * 12 > area
    cls2 = cls1 or (c1 * 256 * 10 > area * 4 and c2 * 256 * 30 > area)
    cls3 = cls1 or (c1 * 256 * 8 > area and c2 * 256 * 50 > area)
    return c1, c2, blocks, [int(cls0), int(cls1), int(cls2), int(cls3)]


def sc_record_bytes(c1, c2, blocks, cls):
    rec = np.zeros(1, abi.SC_CLASS_DTYPE)
    rec["counts_1"], rec["counts_2"], rec["blocks"], rec["sc_class"] = c1, c2, blocks, cls
    return rec.view(np.uint8).reshape(-1).copy()


# ---- the reference's own functions ----------------------------------------------------------------------------------------------

class PinPalette(C.Structure):
    _fields_ = [(n, C.c_int32) for n in "width height rows cols bit_depth step stride org_x org_y above_n left_n".split()] + \
               [("above", C.c_uint16 * 8), ("left", C.c_uint16 * 8)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_rates(pin):
    ysize, ycolor = np.zeros(49, np.int32), np.zeros(280, np.int32)
    pin.pin_tables(_p(ysize), _p(ycolor))
    return ysize.reshape(7, 7), ycolor.reshape(7, 5, 8)


def ref_search(pin, c, blk):
    """What the reference's search_palette_luma and rate functions give for the block inside a plane of its own, at an offset:
    (colors, cache, [(k, colors, size_bits, color_bits, map_bits)], maps).  max_itr is the reference's 50."""
    org_x, org_y, stride = 5, 3, c.w + 11
    plane = np.zeros((c.h + 4, stride), blk.dtype)
    plane[org_y:org_y + c.h, org_x:org_x + c.w] = blk
    a = PinPalette(c.w, c.h, c.rows, c.cols, c.bd, c.step, stride, org_x, org_y, len(c.above), len(c.left))
    a.above[:len(c.above)], a.left[:len(c.left)] = c.above, c.left
    hdr, cache, sizes = np.zeros(2, np.int32), np.zeros(16, np.uint16), np.zeros(14, np.uint8)
    colors, maps, bits = np.zeros(14 * 8, np.uint16), np.zeros(14 * 4096, np.uint8), np.zeros(14 * 3, np.int32)
    assert pin.pin_palette_search(C.byref(a), _p(plane), _p(hdr), _p(cache), _p(sizes), _p(colors), _p(maps), _p(bits)) == 0, c.name
    first = plane[org_y:, org_x:]
    count = pin.pin_count_colors(_p(np.ascontiguousarray(first)), first.shape[1], c.rows, c.cols, c.bd)
    cands = [(int(sizes[i]), [int(v) for v in colors[8 * i:8 * i + sizes[i]]], *[int(v) for v in bits[3 * i:3 * i + 3]]) for i in range(hdr[0])]
    return count, [int(v) for v in cache[:hdr[1]]], cands, [maps[4096 * i:4096 * i + c.w * c.h].reshape(c.h, c.w).copy() for i in range(hdr[0])]


def same_as_reference(res, ref):
    """Every field the reference lets one observe"""
    count, cache, cands, maps = ref
    return (res.colors == count and res.cache == cache and [tuple(x[2:]) for x in res.cands] == [(k, pal, s, cb, mb) for k, pal, s, cb, mb in cands]
            and len(maps) == len(res.maps) and all(np.array_equal(a, b) for a, b in zip(maps, res.maps)))


def ref_k_means(pin, data, cen, max_itr):
    data, cen = np.ascontiguousarray(data, np.int32), np.array(cen, np.int32)
    idx = np.zeros(len(data), np.uint8)
    pin.pin_k_means(_p(data), _p(cen), _p(idx), len(data), len(cen), max_itr)
    return [int(v) for v in cen], idx


def ref_sc_classes(pin, buf, w, h):
    out, buf = np.zeros(4, np.int32), np.ascontiguousarray(buf)
    pin.pin_sc_classify(_p(buf), w, h, buf.shape[1], _p(out))
    return [int(v) for v in out]


# ---- building the calls -----------------------------------------------------------------------------------------------------

def groups(names):
    """The cases of `names` by what one call shares: {(bd, step, max_itr): [case, ...]}"""
    out = {}
    for n in names:
        c = CASE[n]
        out.setdefault((c.bd, c.step, c.max_itr), []).append(c)
    return out


def desc(c, src, stride, org_x, org_y, record, maps):
    d = abi.PaletteDesc(src, record, maps, stride, org_x, org_y, c.w, c.h, c.rows, c.cols, len(c.above), len(c.left))
    d.above[:len(c.above)], d.left[:len(c.left)] = c.above, c.left
    return d
