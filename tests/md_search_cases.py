"""TEST INFRASTRUCTURE — what the cases of the three motion searches of mode decision share (subpel_cases.py, fpel_cases.py, obmc_cases.py,
and the GPU tests on them): the constants and made-up cost tables, the restatement of svt_av1_set_mv_search_range, the host image of a list
of cases, and that image on the device with the checks every search's test makes of a call."""
import ctypes as C

import numpy as np

import arena
from svtav1_hip import abi

# init_fn_ptr (av1me.c:31-170)
SIZES = ((4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64),
         (64, 128), (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16))
MV_LOW, MV_UPP, MAX_FULL_PEL_VAL = -(1 << 14), 1 << 14, 1023


def i16(v):
    return ((int(v) + 0x8000) & 0xFFFF) - 0x8000


def mv_cost_tables():
    """(mvjcost[4], the row and the column table over MV_LOW .. MV_UPP): made up, shaped like the reference's (a cost per magnitude
    class plus a little for the fractional bits), different for rows and columns."""
    v = np.abs(np.arange(MV_LOW, MV_UPP + 1, dtype=np.int64))
    bits = np.zeros_like(v)
    for k in range(15):
        bits += (v >> k) > 0
    row = 300 + 410 * bits + 35 * (v & 7) + 17 * ((v >> 3) & 3)
    col = 260 + 450 * bits + 29 * (v & 7) + 11 * ((v >> 3) & 5)
    return np.array([130, 640, 580, 910], np.int32), row.astype(np.int32), col.astype(np.int32)


def block_mv_limits(mi_row, mi_col, mi_w, mi_h, mi_rows, mi_cols):
    """x->mv_limits of product_coding_loop.c:2532-2535 and mode_decision.c:2459-2462 (MI_SIZE 4, AOM_INTERP_EXTEND 4): (col_min, col_max,
    row_min, row_max), full-pel"""
    return -(((mi_col + mi_w) * 4) + 4), (mi_cols - mi_col) * 4 + 4, -(((mi_row + mi_h) * 4) + 4), (mi_rows - mi_row) * 4 + 4


def set_mv_search_range(lim, ref_mv):
    """svt_av1_set_mv_search_range (av1me.c:205-226) on the full-pel limits (col_min, col_max, row_min, row_max) around ref_mv (row, col)"""
    r, c = ref_mv
    return (max(lim[0], (c >> 3) - MAX_FULL_PEL_VAL + int(c & 7 != 0), (MV_LOW >> 3) + 1), min(lim[1], (c >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1),
            max(lim[2], (r >> 3) - MAX_FULL_PEL_VAL + int(r & 7 != 0), (MV_LOW >> 3) + 1), min(lim[3], (r >> 3) + MAX_FULL_PEL_VAL, (MV_UPP >> 3) - 1))


def set_subpel_mv_search_range(lim, ref_mv):
    """svt_av1_set_subpel_mv_search_range (mcomp.h:113-125), set_subpel_mv_search_range (av1me.c:778-790): the limits in 1/8 units from the
    full-pel ones"""
    (r, c), m = ref_mv, MAX_FULL_PEL_VAL * 8
    return (max(MV_LOW + 1, lim[0] * 8, c - m), min(MV_UPP - 1, lim[1] * 8, c + m), max(MV_LOW + 1, lim[2] * 8, r - m), min(MV_UPP - 1, lim[3] * 8, r + m))


class Arena:
    """The planes of a list of cases in one host buffer, each at its own byte offset with its own stride, and the two cost tables behind
    them.  layout(i) -> (offset shift in bytes, extra stride) lets a test ask for unaligned pointers and odd strides.  A subclass places
    its planes (and outputs) case by case and then calls finish()."""

    def __init__(self, cases, layout, fill=arena.GUARD):
        self.cases, self.layout, self.ab = cases, layout, arena.Arena(fill=fill, tail=64)

    def place(self, i, name, plane, memory=lambda buf: buf):
        """(offset, stride, the widened plane) of a uint8 plane of case i; memory(widened plane) is what goes into the buffer"""
        shift, extra = self.layout(i)
        stride = plane.shape[1] + extra
        buf = np.full((plane.shape[0], stride), 0x5A, np.uint8)
        buf[:, :plane.shape[1]] = plane
        return self.ab.add(f"{name} of case {i}", memory(buf), align=64, gap=0, skew=shift), stride, buf

    def finish(self):
        self.mvj, row, col = mv_cost_tables()
        self.table_at = [self.ab.add(name, t, align=64, gap=0) - 4 * MV_LOW for name, t in (("mvcost row", row), ("mvcost col", col))]     # the centres
        self.regions, self.host = self.ab.regions, self.ab.build()      # regions: for arena.check_containment

    def job(self, base):
        j = abi.SubpelJob()
        j.mvjcost[:] = [int(v) for v in self.mvj]
        j.mvcost[0], j.mvcost[1] = base + self.table_at[0], base + self.table_at[1]
        return j


# ---- the GPU tests' plumbing ----------------------------------------------------------------------------------------------------
def guarded(result):
    """(records, whether the guard bytes around them kept their fill) of a device.*_batch(.., fill=GUARD)"""
    out, guards = result
    return out, bool((guards == arena.GUARD).all())


class Loaded:
    """An Arena on the device: its job, its descriptors, and `search` (device.*_search_batch) on them"""

    def __init__(self, lib, host, search):
        from svtav1_hip import device
        self.lib, self.arena, self.search_batch = lib, host, search
        self.buf = device.DeviceBuffer(lib, host.host.nbytes)
        self.buf.upload(host.host)
        self.job, self.descs = host.job(self.buf.ptr), host.descs(self.buf.ptr)

    def run(self, descs, job=None):
        """(records, whether the guard bytes around them kept their fill)"""
        return guarded(self.search_batch(self.lib, job or self.job, descs, fill=arena.GUARD))

    def image(self):
        return self.buf.download(np.uint8, (self.arena.host.nbytes,))

    def assert_untouched(self, what):
        """Pictures, tables and everything between them are what was uploaded: the search writes its records and nothing else"""
        arena.check_containment(self.arena.host, self.image(), self.arena.regions, [], what)


def one_by_one_fixture(before=None):
    """The module's `one_by_one` fixture over its `loaded`: every case in a call of its own, the records, computed once.  With
    before(loaded, i), called ahead of case i's search: (what it returned per case, the records)."""
    import pytest      # here, so that the tools and golden scripts that read the constants above need none

    @pytest.fixture(scope="module")
    def one_by_one(loaded):
        first, records = [], []
        for i in range(len(loaded.descs)):
            if before:
                first.append(before(loaded, i))
            rec, clean = loaded.run(loaded.descs[i:i + 1])
            assert clean, i
            records.append(rec[:1])
        records = np.concatenate(records)
        return (first, records) if before else records
    return one_by_one


def assert_call_level_errors(hip, export, bad, args):
    """export(*args, result pointer, n, stream) with each pointer NULL in turn, and all of them with n == 0, returns `bad` and names itself in
    svt_hip_last_error(); an empty batch with good pointers returns 0; and nothing was written"""
    from svtav1_hip import device
    res = device.DeviceBuffer(hip, 256)
    res.fill(arena.GUARD)
    f, args = getattr(hip, export), list(args) + [C.c_void_p(res.ptr)]
    for k in range(len(args)):
        assert f(*[None if j == k else a for j, a in enumerate(args)], 1, None) == bad, k
        assert k or export.encode() in hip.svt_hip_last_error()
    assert f(*[None] * len(args), 0, None) == bad
    assert f(*args, 0, None) == 0
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    assert (res.download(np.uint8, (256,)) == arena.GUARD).all()
