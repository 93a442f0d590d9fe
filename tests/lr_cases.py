"""Shared inputs of the frame-level loop-restoration tests (test infrastructure): CDEF-output planes, the saved stripe
boundary rows, a random restoration-unit table (RESTORE_NONE / WIENER / SGRPROJ) and the flat SvtHipLrPlane records."""
import ctypes as C

import numpy as np

import lf_cases as L
import sgr_cases as G
from svtav1_hip import abi

# name: width, height (luma), bit depth, is16, luma restoration-unit size, optimized_lr, seed
CASES = {
    "a_8bit": (200, 136, 8, 0, 64, 0, 1),
    "b_10bit": (328, 200, 10, 1, 128, 0, 2),
    "c_opt_10bit": (264, 152, 10, 1, 64, 1, 3),
    "d_8in16": (136, 264, 8, 1, 64, 0, 4),
    "e_one_unit": (72, 40, 10, 1, 256, 0, 5),
    "f_opt_h57": (136, 121, 8, 0, 64, 1, 6),    # H = 64 + 57: the rows below the second stripe run past the picture
}


DST_EXTRA = 40


def units_in(size, unit):
    return max((size + (unit >> 1)) // unit, 1)             # count_units_in_tile (restoration.c:124-126)


def make_case(name, planes=(0, 1, 2), dims=None):
    w, h, bd, is16, us, opt, seed = dims if dims else CASES[name]
    rng = np.random.default_rng(1000 + seed)
    dt = np.uint16 if is16 else np.uint8
    out = []
    for p in planes:
        ss = int(p > 0)
        pw, ph, unit = w >> ss, h >> ss, max(us >> ss, 32)
        src = np.clip(L.smooth_plane(rng, pw, ph, bd) + rng.integers(-3, 4, size=(ph, pw)) * (1 << (bd - 8)), 0, (1 << bd) - 1).astype(dt)
        n_stripes = (ph + (8 >> ss) + (64 >> ss) - 1) // (64 >> ss)
        bstride = pw + 2 * abi.LR_EXTRA_HORZ + 8
        above = rng.integers(0, 1 << bd, size=(2 * n_stripes, bstride)).astype(dt)
        below = rng.integers(0, 1 << bd, size=(2 * n_stripes, bstride)).astype(dt)
        hu, vu = units_in(pw, unit), units_in(ph, unit)
        units = np.zeros(vu * hu, abi.LR_UNIT_DTYPE)
        for u in units:
            u["restoration_type"] = int(rng.integers(0, 3))
            u["ep"] = int(rng.integers(0, 16))
            r0, r1 = abi.SGR_PARAMS[int(u["ep"])][:2]
            u["xqd"] = (int(rng.integers(-96, 32)) if r0 else 0, int(rng.integers(-32, 96)) if r1 else 0)
            if r0 == 0:                                        # encode_xq keeps xqd[0] = 0 / clamps xqd[1] (restoration_pick.c)
                u["xqd"] = (0, int(np.clip(128 - 0 - int(rng.integers(33, 128)), -32, 95)))
            u["hfilter"] = G.wiener_filter(rng)[0]
            u["vfilter"] = G.wiener_filter(rng)[0]
        out.append(dict(src=src, above=above, below=below, units=units, w=pw, h=ph, ss=ss, bd=bd, is16=is16, unit=unit, hu=hu, vu=vu,
                        opt=opt, bstride=bstride))
    return out


def lr_planes(case, ptr_of=lambda a: a.ctypes.data, dsts=None, units_ptr=None):
    """-> (ctypes array of SvtHipLrPlane, list of dst arrays).  ptr_of maps a host array to the address to put in the record."""
    arr = (abi.LrPlane * len(case))()
    outs = []
    for i, c in enumerate(case):
        dst = np.zeros((c["h"] + 2, c["w"] + DST_EXTRA), c["src"].dtype) if dsts is None else dsts[i]   # the reference's Wiener stripe filter rounds the width of a unit's last column of processing units up to 16 (restoration.c:444): room to the right
        outs.append(dst)
        arr[i] = abi.LrPlane(ptr_of(c["src"]), ptr_of(dst) if dsts is None else dsts[i], c["w"], c["w"] + DST_EXTRA, c["w"], c["h"], c["ss"], c["ss"], c["is16"],
                             c["bd"], c["unit"], c["hu"], c["vu"], ptr_of(c["units"]) if units_ptr is None else units_ptr[i],
                             0 if c["opt"] else ptr_of(c["above"]), 0 if c["opt"] else ptr_of(c["below"]), c["bstride"], c["opt"])
    return arr, outs


# ---- harsh content with a fixed unit table.  smooth_plane keeps every sample above 35 and the random table leaves out
# self-guided sets; here the source is one of lf_cases.content_plane's kinds and the table walks everything a unit can hold.
CONTENT_KINDS = ("noise", "ends", "checker", "saturated", "stripes")
XQD_CORNERS = ((-96, -32), (31, 95), (-96, 95), (31, -32))                 # the corners of the coded range of xqd
WIENER_ENDS = ((-5, -23, -17), (10, 8, 46), (10, -23, 46), (-5, 8, -17))   # taps 0..2 at the ends of sgr_cases.wiener_filter's ranges
TYPE_CYCLE = (2, 2, 1, 2, 0, 2)                                            # two thirds self-guided, a sixth Wiener, a sixth none
# name: kind, (width, height, bit depth, is16, luma unit size, optimized_lr); 185 = 64 * 2 + 57 rows, like f_opt_h57
CONTENT_CASES = {f"{kind}_{bd}_opt{opt}": (kind, (264, 200, bd, int(bd > 8), 64, opt))
                 for kind in CONTENT_KINDS for bd in (8, 10, 12) for opt in (0, 1)}
CONTENT_CASES.update({"noise_10_h57": ("noise", (136, 185, 10, 1, 64, 1)), "ends_8_h57": ("ends", (136, 185, 8, 0, 64, 1))})
GOLDEN_CONTENT = {"g_noise_8": ("noise", (136, 72, 8, 0, 64, 0)), "g_ends_10": ("ends", (136, 72, 10, 1, 64, 1))}


def make_content_case(kind, dims, seed=0):
    """Like make_case, with the source from lf_cases.content_plane(kind) and a unit table that is fixed, not drawn: the types
    cycle through TYPE_CYCLE, `ep` of the self-guided units walks all 16 sets over the three planes, xqd the corners of its
    range (for the sets with one radius 0 the pairs encode_xq leaves, as in make_case), and every third Wiener unit has its
    taps at the ends of their ranges, both filters, the others seeded ones."""
    w, h, bd, is16, us, opt = dims
    rng = np.random.default_rng(2000 + seed)
    dt = np.uint16 if is16 else np.uint8
    out, n, n_sgr, n_wiener = [], 0, 0, 0
    for p in range(3):
        ss = int(p > 0)
        pw, ph, unit = w >> ss, h >> ss, max(us >> ss, 32)
        src = L.content_plane(kind, rng, pw, ph, bd)[0].astype(dt)
        n_stripes = (ph + (8 >> ss) + (64 >> ss) - 1) // (64 >> ss)
        bstride = pw + 2 * abi.LR_EXTRA_HORZ + 8
        above = rng.integers(0, 1 << bd, size=(2 * n_stripes, bstride)).astype(dt)
        below = rng.integers(0, 1 << bd, size=(2 * n_stripes, bstride)).astype(dt)
        hu, vu = units_in(pw, unit), units_in(ph, unit)
        units = np.zeros(vu * hu, abi.LR_UNIT_DTYPE)
        for u in units:
            u["restoration_type"] = TYPE_CYCLE[n % len(TYPE_CYCLE)]
            n += 1
            u["ep"] = n_sgr % 16
            r0, r1 = abi.SGR_PARAMS[int(u["ep"])][:2]
            x0, x1 = XQD_CORNERS[(n_sgr // 16 + n_sgr) % 4]
            u["xqd"] = (x0, x1) if r0 and r1 else (0, x1) if r1 else (x0, 0)
            fx, fy = G.wiener_filter(rng)[0], G.wiener_filter(rng)[0]
            if u["restoration_type"] == 2:
                n_sgr += 1
            if u["restoration_type"] == 1:
                if n_wiener % 3 == 0:
                    for f, (t0, t1, t2) in ((fx, WIENER_ENDS[n_wiener // 3 % 4]), (fy, WIENER_ENDS[(n_wiener // 3 + 2) % 4])):
                        f[:] = [t0, t1, t2, -2 * (t0 + t1 + t2), t2, t1, t0, 0]
                n_wiener += 1
            u["hfilter"], u["vfilter"] = fx, fy
        out.append(dict(src=src, above=above, below=below, units=units, w=pw, h=ph, ss=ss, bd=bd, is16=is16, unit=unit, hu=hu, vu=vu,
                        opt=opt, bstride=bstride))
    return out
