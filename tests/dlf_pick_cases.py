"""Seeded cases for svt_hip_dlf_pick_levels / svt_hip_dlf_apply_picked and a plain Python driver of search_filter_level
(deblocking_filter.c:886-991), once per searched plane (test infrastructure).  The driver does the loop in Python integers wrapped to
int64_t where the reference's types would wrap; the two things under it are functions it is GIVEN: a frame filter (the reference's own
svt_av1_loop_filter_frame or the oracle's) that it calls on a copy of the planes, and an SSE.  Pictures are regenerated from the seeds;
tests/golden/dlf_pick.npz stores results only."""
import ctypes as C
from collections import namedtuple

import numpy as np

import lf_cases as L
from lf_cases import BH, BW, INTER_MODES_WITH_DELTA, TX, P, flat_mode_info, max_depth_of, split_tx  # noqa: F401
from svtav1_hip import abi

MAX_LEVEL = abi.DLF_MAX_LEVEL
RESULT_DTYPE = np.dtype(abi.DLF_PICK_RESULT_DTYPE)
PAD = L.PAD

# w x h: unpadded luma size; pitch: mi_stride - mi_cols; amp: amplitude of the per-block steps of the reconstruction (8-bit units);
# noise: amplitude of its per-sample noise; seg: segment deltas on; conv: early_exit_convergence; mask: plane_mask; start: the three
# start levels; area: "aligned" = the mi-aligned plane is measured, "cropped" = w x h (chroma (w + 1) >> 1 x (h + 1) >> 1)
Case = namedtuple("Case", "name w h bd is16 sb pitch amp noise seg only4 conv mask start area seed")
CASES = [
    Case("small_8bit_flat", 40, 24, 8, 0, 64, 0, 0, 3, 0, 0, 0, 7, (15, 16, 0), "aligned", 21),
    Case("small_10bit_seg", 40, 24, 10, 1, 64, 3, 10, 1, 1, 1, 2, 7, (40, 63, 15), "aligned", 20),
    Case("tiles_8bit_blocky", 200, 136, 8, 0, 64, 3, 12, 1, 0, 0, 0, 7, (16, 0, 40), "aligned", 3),
    Case("tiles_10bit_cropped", 196, 134, 10, 1, 64, 0, 7, 2, 0, 0, 1, 7, (0, 15, 16), "cropped", 4),
    Case("tiles_8in16_sb128", 200, 136, 8, 1, 128, 1, 5, 2, 1, 0, 2, 7, (63, 40, 0), "aligned", 5),
    Case("tiles_8bit_luma_only", 198, 130, 8, 0, 64, 0, 3, 2, 0, 1, 0, 1, (40, 0, 0), "cropped", 6),
    Case("tiles_10bit_chroma_only", 200, 136, 10, 1, 128, 3, 9, 1, 1, 0, 0, 6, (0, 16, 63), "aligned", 7),
    Case("tiles_8bit_clean", 260, 196, 8, 0, 64, 0, 0, 2, 1, 0, 1, 7, (16, 15, 40), "cropped", 8),
    Case("tiles_8bit_harsh", 200, 136, 8, 0, 64, 2, 24, 0, 0, 1, 0, 7, (15, 40, 16), "aligned", 9),
]
CASE = {c.name: c for c in CASES}


class Inputs:
    """One case's picture: recon / src (three padded planes each, lf_cases.PAD samples on every side), the partition (minfo, flat),
    geometry, the measured areas and the segment features."""


def make_inputs(case):
    rng = np.random.default_rng(9100 + case.seed)
    x = Inputs()
    x.case = case
    x.mi_cols, x.mi_rows = (case.w + 7) // 8 * 2, (case.h + 7) // 8 * 2
    x.mi_stride = x.mi_cols + case.pitch
    x.minfo = L.random_mode_info(rng, x.mi_rows, x.mi_cols, x.mi_stride, sb=case.sb)
    x.flat = flat_mode_info(x.minfo, x.mi_rows, x.mi_stride)
    wa, ha = x.mi_cols * 4, x.mi_rows * 4
    x.src = L.lf_planes(rng, wa, ha, case.bd, case.is16)
    # the reconstruction: the source, one step per coding block (every record of a block is the same, so a hash of it is), noise
    key = (x.minfo["bsize"].astype(np.int64) * 131 + x.minfo["tx_depth"] * 31 + x.minfo["skip"] * 17 + x.minfo["ref_frame0"] * 7
           + x.minfo["mode"] * 3 + x.minfo["segment_id"]) % 997
    table = rng.integers(-case.amp, case.amp + 1, size=997)
    sc, top = 1 << (case.bd - 8), (1 << case.bd) - 1
    x.recon = []
    for p, s in enumerate(x.src):
        ss = int(p > 0)
        pw, ph = wa >> ss, ha >> ss
        steps = table[key[ss::1 + ss, ss:x.mi_cols:1 + ss][:x.mi_rows >> ss]].repeat(4, 0).repeat(4, 1)[:ph, :pw]
        r = s.astype(np.int64)
        r[PAD:PAD + ph, PAD:PAD + pw] += sc * steps
        r += sc * rng.integers(-case.noise, case.noise + 1, size=r.shape)
        x.recon.append(np.clip(r, 0, top).astype(s.dtype))
    if case.area == "aligned":
        x.sse_w, x.sse_h = [wa, wa >> 1, wa >> 1], [ha, ha >> 1, ha >> 1]
    else:
        x.sse_w, x.sse_h = [case.w] + [(case.w + 1) >> 1] * 2, [case.h] + [(case.h + 1) >> 1] * 2
    x.seg_enabled, x.seg_data = np.zeros((8, 4), np.uint8), np.zeros((8, 4), np.int16)
    if case.seg:
        x.seg_enabled[:] = rng.random((8, 4)) < 0.6
        x.seg_data[:] = rng.integers(-20, 21, size=(8, 4))
    return x


def level_table(x, levels):
    """svt_av1_loop_filter_frame_init (deblocking_common.c:76-138) without mode_ref_delta: lvl[3][8][2][8][2] from the frame header's
    filter_level[0], [1], _u, _v."""
    lvl = np.zeros((3, 8, 2, 8, 2), np.uint8)
    for p in range(3):
        for d in range(2):
            base, feat = levels[d] if p == 0 else levels[p + 1], d if p == 0 else p + 1
            for s in range(8):
                v = base
                if x.case.seg and x.seg_enabled[s, feat]:
                    v = min(max(base + int(x.seg_data[s, feat]), 0), MAX_LEVEL)
                lvl[p, s, d] = v
    return lvl.reshape(-1)


class Hdr:
    """The header fields lf_cases.lf_frame reads."""

    def __init__(self, levels, sharpness=0):
        self.filter_level, self.filter_level_u, self.filter_level_v, self.sharpness_level = list(levels[:2]), levels[2], levels[3], sharpness


def frame(x, planes, levels, mi_ptr, plane_start=0, plane_end=3, with_table=True):
    """SvtHipLfFrame over `planes` (padded arrays, or (address of the top-left picture sample, stride) pairs)."""
    c = x.case
    return L.lf_frame(planes, c.w, c.h, mi_ptr, x.mi_stride, x.mi_rows, x.mi_cols, Hdr(levels), c.bd, c.is16, plane_start, plane_end,
                      level_table(x, levels) if with_table else None)


def orc_filter(orc, x):
    """filter_frame(planes, plane_start, plane_end, levels) over the oracle's orc_loop_filter_frame."""
    def run(planes, plane_start, plane_end, levels):
        f = frame(x, planes, levels, x.flat.ctypes.data, plane_start, plane_end)
        orc.orc_loop_filter_frame(C.byref(f), x.case.sb)
    return run


def ref_filter(ref, x):
    """The same over the REAL svt_av1_loop_filter_frame (oracle/ref_harness_lf.c): it derives the level table itself."""
    m = L.RefLfModeInfo(*[x.minfo[k].ctypes.data for k in ("bsize", "tx_depth", "skip", "ref_frame0", "mode", "segment_id")])

    def run(planes, plane_start, plane_end, levels):
        h = L.RefLfHeader()
        h.filter_level[0], h.filter_level[1], h.filter_level_u, h.filter_level_v = levels
        h.segmentation_enabled = x.case.seg
        for s in range(8):
            for k in range(4):
                h.seg_lf_enabled[s][k], h.seg_lf_data[s][k] = int(x.seg_enabled[s, k]), int(x.seg_data[s, k])
        f = frame(x, planes, levels, None, plane_start, plane_end, with_table=False)
        assert ref.ref_loop_filter_frame(C.byref(f), C.byref(m), C.byref(h), x.case.sb) == 0
    return run


def numpy_sse(x):
    def run(plane, src, p):
        a, b = (v[PAD:PAD + x.sse_h[p], PAD:PAD + x.sse_w[p]].astype(np.int64) for v in (plane, src))
        return int(((a - b) ** 2).sum())
    return run


def ref_sse(ref, x):
    """The reference's full-distortion leaves as picture_sse_calculations (:716-834) calls them: svt_spatial_full_distortion_kernel on
    8-bit samples, svt_full_distortion_kernel16_bits on 16-bit ones, through the dispatch pointers."""
    V = C.c_void_p
    sig = (C.c_uint64, V, C.c_uint32, C.c_uint32, V, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
    fn = L.rtcd(ref, "svt_full_distortion_kernel16_bits" if x.case.is16 else "svt_spatial_full_distortion_kernel", *sig)

    def run(plane, src, p):
        at = lambda a: V(a.ctypes.data + (PAD * a.shape[1] + PAD) * a.itemsize)     # noqa: E731
        return int(fn(at(src), 0, src.shape[1], at(plane), 0, plane.shape[1], x.sse_w[p], x.sse_h[p]))
    return run


def w64(v):
    """A Python integer as int64_t arithmetic leaves it."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


FIELDS = ("record", "path", "conv_exit", "both", "none")
HOST_LEVELS = (9, 21, 5, 30)      # frame.filter_level[0], [1], _u, _v of every case: what a plane that is not searched is filtered with


def drive(x, filter_frame, sse, max_rounds=63):
    """search_filter_level for every plane of the case's mask.  Returns `record` (one RESULT_DTYPE record, as the device leaves it:
    a round is an iteration, or the first trial, that measured at least one new level) and what only the case checks read:
    `path` [3][64] the successive filt_mid (-1 padded), `conv_exit` [3] the loop ended by early_exit_convergence, `both` / `none` [3]
    iterations that needed two trials / none."""
    case = x.case
    rec = np.zeros((), RESULT_DTYPE)
    rec["ss_err"][:] = -1
    path, conv_exit, both, none = np.full((3, 64), -1, np.int8), np.zeros(3, np.uint8), np.zeros(3, np.int32), np.zeros(3, np.int32)
    for p in range(3):
        if not (case.mask >> p) & 1:
            continue
        ss_err = [-1] * (MAX_LEVEL + 1)
        rounds = trials = 0

        def trial(level):
            planes = [a.copy() for a in x.recon]
            levels = [level, level, 0, 0] if p == 0 else [0, 0, level if p == 1 else 0, level if p == 2 else 0]   # try_filter_frame :852-870
            filter_frame(planes, p, p + 1, levels)
            for q in range(3):
                assert q == p or np.array_equal(planes[q], x.recon[q])
            return sse(planes[p], x.src[p], p)

        filt_mid = min(max(case.start[p], 0), MAX_LEVEL)
        filter_step = 4 if filt_mid < 16 else filt_mid // 4
        filt_direction = tot_convergence = 0
        best_err = ss_err[filt_mid] = trial(filt_mid)
        filt_best, rounds, trials = filt_mid, 1, 1
        path[p, 0], n_path, out_of_rounds = filt_mid, 1, False
        while filter_step > 0:
            filt_high, filt_low = min(filt_mid + filter_step, MAX_LEVEL), max(filt_mid - filter_step, 0)
            look_low, look_high = filt_direction <= 0 and filt_low != filt_mid, filt_direction >= 0 and filt_high != filt_mid
            need = [lv for look, lv in ((look_low, filt_low), (look_high, filt_high)) if look and ss_err[lv] < 0]
            if need and rounds == max_rounds:
                out_of_rounds = True
                break
            for lv in need:
                ss_err[lv] = trial(lv)
            rounds, trials = rounds + bool(need), trials + len(need)
            both[p], none[p] = both[p] + (len(need) == 2), none[p] + (not need)
            bias = w64(w64(best_err >> (15 - filt_mid // 8)) * filter_step)
            if not case.only4:
                bias >>= 1
            if look_low and ss_err[filt_low] < w64(best_err + bias):
                if ss_err[filt_low] < best_err:
                    best_err = ss_err[filt_low]
                filt_best = filt_low
            if look_high and ss_err[filt_high] < w64(best_err - bias):
                best_err, filt_best = ss_err[filt_high], filt_high
            if filt_best == filt_mid:
                tot_convergence += 1
                if tot_convergence == case.conv:
                    filter_step, conv_exit[p] = 0, 1
                else:
                    filter_step //= 2
                filt_direction = 0
            else:
                filt_direction = -1 if filt_best < filt_mid else 1
                filt_mid = filt_best
                path[p, n_path], n_path = filt_mid, n_path + 1
        if not out_of_rounds:
            best_err = ss_err[filt_best]
            rec["finished"] |= 1 << p
        rec["level"][p], rec["best_err"][p], rec["rounds"][p], rec["trials"][p], rec["ss_err"][p] = filt_best, best_err, rounds, trials, ss_err
    lv = [int(rec["level"][q]) if (case.mask >> q) & 1 else None for q in range(3)]
    rec["hdr_level"][:] = [HOST_LEVELS[0] if lv[0] is None else lv[0], HOST_LEVELS[1] if lv[0] is None else lv[0],
                           HOST_LEVELS[2] if lv[1] is None else lv[1], HOST_LEVELS[3] if lv[2] is None else lv[2]]
    return {"record": rec, "path": path, "conv_exit": conv_exit, "both": both, "none": none}


def same(a, b, fields=FIELDS):
    """The names of the fields in which two driver / fixture outputs differ."""
    return [f for f in fields if not (a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes())]


_golden = {}


def golden(case):
    """The recorded results of one case (tests/golden/dlf_pick.npz, written by tests/golden/make_golden_dlf_pick.py)."""
    import os
    if not _golden:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dlf_pick.npz")) as g:
            _golden.update({k: g[k] for k in g.files})
    out = {f: _golden[f"{case.name}_{f}"] for f in FIELDS if f != "record"}
    rec = np.zeros((), RESULT_DTYPE)
    for f in ("level", "finished", "rounds", "trials", "hdr_level", "best_err", "ss_err"):
        rec[f] = _golden[f"{case.name}_{f}"]
    out["record"] = rec
    return out


def params(x, planes, srcs, mi_ptr, max_rounds=abi.DLF_PICK_DEFAULT_ROUNDS, plane_start=0, plane_end=3):
    """SvtHipDlfPickParams of the case; planes / srcs: padded arrays, or (address of the top-left picture sample, stride) pairs."""
    case = x.case
    prm = abi.DlfPickParams()
    prm.frame = frame(x, planes, HOST_LEVELS, mi_ptr, plane_start, plane_end, with_table=False)
    for p, s in enumerate(srcs):
        if isinstance(s, np.ndarray):
            prm.src[p], prm.src_stride[p] = s.ctypes.data + (PAD * s.shape[1] + PAD) * s.itemsize, s.shape[1]
        else:
            prm.src[p], prm.src_stride[p] = s
        prm.sse_width[p], prm.sse_height[p], prm.start_level[p] = x.sse_w[p], x.sse_h[p], case.start[p]
    prm.plane_mask, prm.only_4x4, prm.early_exit_convergence, prm.max_rounds = case.mask, case.only4, case.conv, max_rounds
    prm.segmentation_enabled = case.seg
    for s in range(8):
        for k in range(4):
            prm.seg_lf_enabled[s][k], prm.seg_lf_data[s][k] = int(x.seg_enabled[s, k]), int(x.seg_data[s, k])
    return prm


ARGS = ("prm", "d_result", "d_workspace")


def rejections(x):
    """(label, function that spoils the parameters, argument to pass as NULL, bytes to take off the workspace size, whether
    svt_hip_dlf_apply_picked reads what is spoilt): every call svt_hip_dlf_pick_levels must refuse with SVT_HIP_ERR_BAD_PARAMETER, and
    svt_hip_dlf_apply_picked too where the last entry says so."""
    def setf(path, v):
        def change(prm):
            obj, names = prm, path.split(".")
            for n in names[:-1]:
                obj = getattr(obj, n)
            if isinstance(v, tuple):
                getattr(obj, names[-1])[v[0]] = v[1]
            else:
                setattr(obj, names[-1], v)
        return change
    wa, ha = x.mi_cols * 4, x.mi_rows * 4
    for a in ARGS:
        yield f"NULL {a}", None, a, 0, a != "d_workspace"
    for p in range(3):
        yield f"start_level[{p}] 64", setf("start_level", (p, 64)), None, 0, False
    yield "filter_level[1] 64", setf("frame.filter_level", (1, 64)), None, 0, True
    yield "filter_level_v 200", setf("frame.filter_level_v", 200), None, 0, True
    yield "empty mask", setf("plane_mask", 0), None, 0, True
    yield "mask 8", setf("plane_mask", 8), None, 0, True
    for v in (0, -1, 64):
        yield f"max_rounds {v}", setf("max_rounds", v), None, 0, False
    yield "luma area too wide", setf("sse_width", (0, wa + 1)), None, 0, False
    yield "luma area of no width", setf("sse_width", (0, 0)), None, 0, False
    yield "chroma area of no height", setf("sse_height", (1, 0)), None, 0, False
    yield "chroma area too tall", setf("sse_height", (2, (ha >> 1) + 1)), None, 0, False
    yield "workspace short", None, None, 1, False
    yield "no source", setf("src", (1, None)), None, 0, False
    yield "no source stride", setf("src_stride", (0, 0)), None, 0, False
    # everything svt_hip_loop_filter_frame refuses
    yield "no mode info", setf("frame.mi", None), None, 0, True
    yield "no width", setf("frame.width", 0), None, 0, True
    yield "no height", setf("frame.height", 0), None, 0, True
    yield "planes reversed", setf("frame.plane_start", 4), None, 0, True
    yield "plane_end 4", setf("frame.plane_end", 4), None, 0, True
    yield "mi_stride short", setf("frame.mi_stride", x.mi_cols - 1), None, 0, True
    yield "bit depth 9", setf("frame.bit_depth", 9), None, 0, True
    yield "wider than the grid", setf("frame.width", wa + 1), None, 0, True
    yield "taller than the grid", setf("frame.height", ha + 1), None, 0, True
    yield "odd mi_cols", setf("frame.mi_cols", x.mi_cols + 1), None, 0, True
    yield "odd mi_rows", setf("frame.mi_rows", x.mi_rows + 1), None, 0, True
    yield "sharpness 8", setf("frame.sharpness_level", 8), None, 0, True
    yield "missing plane", setf("frame.plane", (2, None)), None, 0, True
    yield "missing stride", setf("frame.stride", (0, 0)), None, 0, True
    if x.case.bd > 8:
        yield "deep samples in bytes", setf("frame.is_16bit", 0), None, 0, True


STATUS_NAMES = ("svt_hip_dlf_apply_picked", "svt_hip_dlf_pick_levels")
BAD_PARAMETER = abi.SVT_HIP_ERR_BAD_PARAMETER & 0xFFFFFFFF      # the status as these two return it: uint32_t


def refusal_probes():
    """{export: [[return code, error text or None] per probe]} of the two status exports for the three probes of
    tests/test_tier_b_refusals.py (all NULL / zero, an empty buffer and zeros, that buffer and ones), made like its census in one fresh
    interpreter that never calls svt_hip_init.  They return the status as uint32_t, so that census (every int32_t export) does not
    list them; tests/golden/dlf_pick_refusals.json holds their rows instead."""
    import json
    import subprocess
    import sys

    import test_tier_b_refusals as T
    r = subprocess.run([sys.executable, "-c", T._CHILD, abi.PKG_ROOT, json.dumps(sorted(STATUS_NAMES)), "[]"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout)
