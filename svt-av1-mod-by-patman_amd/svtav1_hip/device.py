"""Device-side plumbing over the C-ABI (no compute here): device buffers, picture upload, job building.

Everything goes through libsvtav1_hip's own allocator / copy entry points (include/svt_hip.h), so this
module works without torch; bench.py may instead hand in torch-owned device pointers.
"""
import ctypes as C

import numpy as np

from . import abi, frames


class HipError(RuntimeError):
    pass


def check(lib, rc, what):
    if rc != 0:
        raise HipError(f"{what} failed (0x{rc & 0xffffffff:08x}): {lib.svt_hip_last_error().decode()}")


def _call(lib, name, *args, stream=None, sync=False):
    """The export `name` with `stream` as its last argument (abi.load declared the argument types: plain ints, None and byref(..) do),
    its return code checked under its own name, then svt_hip_stream_sync if asked for."""
    check(lib, getattr(lib, name)(*args, stream), name)
    if sync:
        check(lib, lib.svt_hip_stream_sync(stream), "svt_hip_stream_sync")


class DeviceBuffer:
    def __init__(self, lib, nbytes):
        self.lib, self.nbytes = lib, int(nbytes)
        p = C.c_void_p()
        check(lib, lib.svt_hip_malloc(C.byref(p), self.nbytes), "svt_hip_malloc")
        self.ptr = p.value

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _call(self.lib, "svt_hip_upload", self.ptr, arr.ctypes.data, arr.nbytes, stream=stream, sync=True)

    def download(self, dtype, shape, stream=None, offset=0):
        """The array of `shape` that starts `offset` bytes into the buffer"""
        out = np.empty(shape, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        _call(self.lib, "svt_hip_download", out.ctypes.data, self.ptr + offset, out.nbytes, stream=stream, sync=True)
        return out

    def fill(self, value, stream=None):
        _call(self.lib, "svt_hip_memset", self.ptr, int(value), self.nbytes, stream=stream)

    def free(self):
        if self.ptr:
            self.lib.svt_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Guarded:
    """A device buffer of nbytes between two runs of `guard` bytes, all of it `fill`; ptr is the payload's address."""

    def __init__(self, lib, nbytes, guard, fill, stream=None):
        self.buf, self.guard, self.stream = DeviceBuffer(lib, 2 * guard + nbytes), guard, stream
        self.buf.fill(fill, stream)
        self.ptr = self.buf.ptr + guard

    def read(self, dtype):
        """(the records between the guards, the guard bytes before and after them: still the fill if untouched)"""
        raw, end = self.buf.download(np.uint8, (self.buf.nbytes,), self.stream), self.buf.nbytes - self.guard
        return raw[self.guard:end].view(np.dtype(dtype)).copy(), np.concatenate([raw[:self.guard], raw[end:]])


class DevicePlane:
    """Device mirror of a HostPlane (same geometry)."""

    def __init__(self, lib, host_plane, upload=True):
        self.lib, self.h = lib, host_plane
        self.buf = DeviceBuffer(lib, host_plane.nbytes)
        if upload:
            self.buf.upload(host_plane.buf)

    def desc(self):
        return self.h.desc(self.buf.ptr)

    def download(self):
        return self.buf.download(np.uint8, self.h.buf.shape)


class DevicePyramid:
    def __init__(self, lib, host_pyr, upload=True):
        self.full = DevicePlane(lib, host_pyr.full, upload)
        self.quarter = DevicePlane(lib, host_pyr.quarter, upload)
        self.sixteenth = DevicePlane(lib, host_pyr.sixteenth, upload)

    def desc(self):
        return abi.Pyramid8(self.full.desc(), self.quarter.desc(), self.sixteenth.desc())


class DeviceMeOut:
    """Device output arrays of one picture, pre-filled with `fill` (as frames.alloc_me_out_host)."""

    def __init__(self, lib, prm, n_b64, fill=0xA5):
        self.lib, self.shapes, self.bufs = lib, frames.me_out_shapes(prm, n_b64), {}
        for name, (dt, shape) in self.shapes.items():
            b = DeviceBuffer(lib, int(np.prod(shape)) * np.dtype(dt).itemsize)
            b.fill(fill)
            self.bufs[name] = b

    def desc(self):
        return abi.MeFrameOut(**{k: v.ptr for k, v in self.bufs.items()})

    def download(self):
        return {k: self.bufs[k].download(dt, shape) for k, (dt, shape) in self.shapes.items()}


class DeviceIntraOut:
    """Device output arrays of one picture's intra search (include/svt_hip_intra.h), pre-filled with `fill`; the per-mode costs and
    predictions only with `all_modes`."""

    def __init__(self, lib, width, height, all_modes=False, fill=0xA5):
        cells = ((width + 15) // 16, (height + 15) // 16)
        self.shape = (cells[1], cells[0])
        self.shapes = {"best_mode": (np.uint8, self.shape), "best_cost": (np.int64, self.shape)}
        if all_modes:
            self.shapes["mode_cost"] = (np.int64, self.shape + (abi.INTRA_MODES,))
            self.shapes["pred"] = (np.uint8, self.shape + (abi.INTRA_MODES, 16, 16))
        self.bufs = {}
        for name, (dt, shape) in self.shapes.items():
            b = DeviceBuffer(lib, int(np.prod(shape)) * np.dtype(dt).itemsize)
            b.fill(fill)
            self.bufs[name] = b

    def fill_job(self, job):
        for name in ("best_mode", "best_cost", "mode_cost", "pred"):
            setattr(job, name, self.bufs[name].ptr if name in self.bufs else None)
        return job

    def download(self):
        return {k: self.bufs[k].download(dt, shape) for k, (dt, shape) in self.shapes.items()}


def _tables(lib, tables, stream):
    """Rate tables as one contiguous record array, and its device copy"""
    tables = np.ascontiguousarray(tables, np.dtype(abi.RATE_TABLES_DTYPE)).reshape(-1)
    d_tab = DeviceBuffer(lib, tables.nbytes)
    d_tab.upload(tables, stream)
    return tables, d_tab


def intra_search_frames(lib, jobs, stream=None, sync=True):
    """svt_hip_intra_search_frames over a list of abi.IntraSearchJob (one launch)."""
    _call(lib, "svt_hip_intra_search_frames", (abi.IntraSearchJob * len(jobs))(*jobs), len(jobs), stream=stream, sync=sync)


def intra_predict_batch(lib, descs, stream=None, sync=True, waves_per_workgroup=None):
    """svt_hip_intra_predict_batch over a list of abi.IntraPredDesc or a record array of abi.INTRA_PRED_DESC_DTYPE (one launch); with waves_per_workgroup (1, 2 or 4) the
    same through svt_hip_intra_predict_batch_packed.  Returns the device copy of the descriptors: keep it until the stream has been synchronised."""
    d_desc = upload_descriptors(lib, descs, stream)
    if waves_per_workgroup is None:
        _call(lib, "svt_hip_intra_predict_batch", d_desc.ptr, len(descs), stream=stream, sync=sync)
    else:
        _call(lib, "svt_hip_intra_predict_batch_packed", d_desc.ptr, len(descs), waves_per_workgroup, stream=stream, sync=sync)
    return d_desc


def cfl_predict_batch(lib, descs, stream=None, sync=True):
    """svt_hip_cfl_predict_batch over a list of abi.CflDesc or a record array of abi.CFL_DESC_DTYPE (one launch)."""
    d_desc = upload_descriptors(lib, descs, stream)
    _call(lib, "svt_hip_cfl_predict_batch", d_desc.ptr, len(descs), stream=stream, sync=sync)
    return d_desc


def me_frames(lib, jobs, stream=None, sync=True):
    _call(lib, "svt_hip_me_frames", (abi.MeFrameJob * len(jobs))(*jobs), len(jobs), stream=stream, sync=sync)


def upload_descriptors(lib, descs, stream=None):
    """A list of ctypes structures of one type, or a numpy record array, as a device array (the Tier B entry points of
    include/svt_hip_inter.h and svt_hip_intra.h read their descriptors from device memory).  Keep the returned buffer alive until the
    launch that reads it has finished."""
    if isinstance(descs, np.ndarray):
        raw = np.ascontiguousarray(descs).view(np.uint8).reshape(-1)
    else:
        raw = np.frombuffer((type(descs[0]) * len(descs))(*descs), np.uint8)
    buf = DeviceBuffer(lib, raw.nbytes)
    buf.upload(raw, stream)
    return buf


def convolve_batch(lib, descs, stream=None, sync=True):
    """svt_hip_convolve_batch over a list of abi.ConvolveDesc (one launch)."""
    d_desc = upload_descriptors(lib, descs, stream)
    _call(lib, "svt_hip_convolve_batch", d_desc.ptr, len(descs), stream=stream, sync=sync)
    return d_desc


def blend_batch(lib, descs, stream=None, sync=True):
    """svt_hip_blend_batch over a list of abi.BlendDesc (one launch)."""
    d_desc = upload_descriptors(lib, descs, stream)
    _call(lib, "svt_hip_blend_batch", d_desc.ptr, len(descs), stream=stream, sync=sync)
    return d_desc


def compound_mask_search_batch(lib, descs, stream=None, fill=0xA5):
    """svt_hip_compound_mask_search_batch over a list of abi.MaskSearchDesc (one launch); the results as a numpy record array
    (abi.MASK_SEARCH_RESULT_DTYPE).  The result buffer is pre-filled with `fill`."""
    d_desc = upload_descriptors(lib, descs, stream)
    d_res = DeviceBuffer(lib, C.sizeof(abi.MaskSearchResult) * len(descs))
    d_res.fill(fill, stream)
    _call(lib, "svt_hip_compound_mask_search_batch", d_desc.ptr, d_res.ptr, len(descs), stream=stream)
    return d_res.download(np.dtype(abi.MASK_SEARCH_RESULT_DTYPE), (len(descs),), stream)


def _search_batch(lib, export, result_ctype, result_dtype, job, descs, stream, guard, fill):
    """One call of a motion-search export under the abi.SubpelJob `job`: (results as a record array of result_dtype, the `guard` bytes before
    and after them)"""
    n = len(descs)
    d_desc = upload_descriptors(lib, descs, stream)
    d_out = Guarded(lib, C.sizeof(result_ctype) * n, guard, fill, stream)
    _call(lib, export, C.byref(job), d_desc.ptr, d_out.ptr, n, stream=stream)
    return d_out.read(result_dtype)


def subpel_search_batch(lib, job, descs, stream=None, guard=64, fill=0xA5):
    """svt_hip_subpel_search_batch over a record array of abi.SUBPEL_DESC_DTYPE (or a list of abi.SubpelDesc) under the abi.SubpelJob `job`
    (one call).  Returns (results as a record array of abi.SUBPEL_RESULT_DTYPE, the `guard` bytes before and after them: still `fill` if
    untouched)."""
    return _search_batch(lib, "svt_hip_subpel_search_batch", abi.SubpelResult, abi.SUBPEL_RESULT_DTYPE, job, descs, stream, guard, fill)


def ifs_search_batch(lib, job, descs, trace=True, stream=None, guard=64, fill=0xA5):
    """svt_hip_ifs_search_batch over a record array of abi.IFS_DESC_DTYPE (or a list of abi.IfsDesc) under the abi.IfsJob `job` (one call).
    Returns (results as a record array of abi.IFS_RESULT_DTYPE, the trace as one of abi.IFS_TRACE_DTYPE or None, the `guard` bytes before
    and after the results and the trace: still `fill` if untouched)."""
    n = len(descs)
    d_desc = upload_descriptors(lib, descs, stream)
    d_out = Guarded(lib, C.sizeof(abi.IfsResult) * n, guard, fill, stream)
    d_trace = Guarded(lib, C.sizeof(abi.IfsTrace) * n, guard, fill, stream) if trace else None
    check(lib, lib.svt_hip_ifs_search_batch(C.byref(job), d_desc.ptr, d_out.ptr, d_trace.ptr if trace else None, n, stream), "svt_hip_ifs_search_batch")
    out, guards = d_out.read(abi.IFS_RESULT_DTYPE)
    if not trace:
        return out, None, guards
    tr, tr_guards = d_trace.read(abi.IFS_TRACE_DTYPE)
    return out, tr, np.concatenate([guards, tr_guards])


def fpel_search_batch(lib, job, descs, stream=None, guard=64, fill=0xA5):
    """svt_hip_fpel_search_batch over a record array of abi.FPEL_DESC_DTYPE (or a list of abi.FpelDesc) under the abi.SubpelJob `job`
    (one call).  Returns (results as a record array of abi.FPEL_RESULT_DTYPE, the `guard` bytes before and after them: still `fill` if
    untouched)."""
    return _search_batch(lib, "svt_hip_fpel_search_batch", abi.FpelResult, abi.FPEL_RESULT_DTYPE, job, descs, stream, guard, fill)


def obmc_target_batch(lib, descs, stream=None, guard=64, fill=0xA5):
    """svt_hip_obmc_target_batch over a record array of abi.OBMC_TARGET_DESC_DTYPE (or a list of abi.ObmcTargetDesc), one call.  Returns
    (the status words, the `guard` bytes before and after them: still `fill` if untouched); wsrc and mask land where the descriptors say."""
    n = len(descs)
    d_desc = upload_descriptors(lib, descs, stream)
    d_out = Guarded(lib, 4 * n, guard, fill, stream)
    _call(lib, "svt_hip_obmc_target_batch", d_desc.ptr, d_out.ptr, n, stream=stream)
    return d_out.read(np.uint32)


def obmc_search_batch(lib, job, descs, stream=None, guard=64, fill=0xA5):
    """svt_hip_obmc_search_batch over a record array of abi.OBMC_SEARCH_DESC_DTYPE (or a list of abi.ObmcSearchDesc) under the abi.SubpelJob
    `job` (one call).  Returns (results as a record array of abi.OBMC_SEARCH_RESULT_DTYPE, the `guard` bytes before and after them: still
    `fill` if untouched)."""
    return _search_batch(lib, "svt_hip_obmc_search_batch", abi.ObmcSearchResult, abi.OBMC_SEARCH_RESULT_DTYPE, job, descs, stream, guard, fill)


def txb_cost_batch(lib, d_base, descs, tables, w, h, d_txfm_result=None, d_distortion=None, stream=None, tables_in_lds=None, guard=64, fill=0xA5):
    """svt_hip_txb_cost_batch for blocks of one size w x h (one launch).  d_base: device address of the arena the descriptors' offsets
    refer to; descs: a record array of abi.TXB_COST_DESC_DTYPE (or a list of abi.TxbCostDesc); tables: a record array of
    abi.RATE_TABLES_DTYPE, one record per table set; d_txfm_result / d_distortion: device addresses of what the transform batch and
    svt_hip_txfm_distortion_batch wrote, or None.  With tables_in_lds (0 or 1) the same through svt_hip_txb_cost_batch_placed.
    Returns (results as a record array of abi.TXB_COST_DTYPE, the `guard` bytes before and after them: still `fill` if untouched)."""
    n = len(descs)
    d_desc, (tables, d_tab) = upload_descriptors(lib, descs, stream), _tables(lib, tables, stream)
    d_out = Guarded(lib, C.sizeof(abi.TxbCost) * n, guard, fill, stream)
    args = (d_base, d_desc.ptr, d_tab.ptr, len(tables), d_txfm_result, d_distortion, d_out.ptr, n, w, h)
    if tables_in_lds is None:
        _call(lib, "svt_hip_txb_cost_batch", *args, stream=stream)
    else:
        _call(lib, "svt_hip_txb_cost_batch_placed", *args, tables_in_lds, stream=stream)
    return d_out.read(abi.TXB_COST_DTYPE)


def rdoq_batch(lib, d_base, d_txfm_desc, descs, tables, d_txfm_result, w, h, stream=None, mapping=None, guard=64, fill=0xA5):
    """svt_hip_rdoq_batch for blocks of one size w x h (one launch), behind svt_hip_txfm_quant_batch.  d_base: device address of the
    arena; d_txfm_desc / d_txfm_result: device addresses of the transform batch's descriptors and results (eob is updated in place);
    descs: a record array of abi.RDOQ_DESC_DTYPE (or a list of abi.RdoqDesc); tables: a record array of abi.RATE_TABLES_DTYPE.
    With mapping (0, 1 or 2) the same through svt_hip_rdoq_batch_mapped.
    Returns (results as a record array of abi.RDOQ_RESULT_DTYPE, the `guard` bytes before and after them: still `fill` if untouched)."""
    n = len(descs)
    d_desc, (tables, d_tab) = upload_descriptors(lib, descs, stream), _tables(lib, tables, stream)
    d_out = Guarded(lib, C.sizeof(abi.RdoqResult) * n, guard, fill, stream)
    args = (d_base, d_txfm_desc, d_desc.ptr, d_tab.ptr, len(tables), d_txfm_result, d_out.ptr, n, w, h)
    if mapping is None:
        _call(lib, "svt_hip_rdoq_batch", *args, stream=stream)
    else:
        _call(lib, "svt_hip_rdoq_batch_mapped", *args, mapping, stream=stream)
    return d_out.read(abi.RDOQ_RESULT_DTYPE)


def spatial_distortion_batch(lib, d_base, d_txfm_desc, srcs, w, h, stream=None, guard=64, fill=0xA5):
    """svt_hip_txfm_spatial_distortion_batch for candidates of one size w x h (one launch).  d_txfm_desc: device address of the
    candidates' transform descriptors (pred_off, recon_off, strides, TX_PIXEL16); srcs: a record array of abi.SPATIAL_SRC_DTYPE.
    Returns (uint64 [n][2] = {residual, prediction}, the guard bytes around them)."""
    n = len(srcs)
    d_src = upload_descriptors(lib, srcs, stream)
    d_out = Guarded(lib, 16 * n, guard, fill, stream)
    _call(lib, "svt_hip_txfm_spatial_distortion_batch", d_base, d_txfm_desc, d_src.ptr, d_out.ptr, n, w, h, stream=stream)
    out, guards = d_out.read(np.uint64)
    return out.reshape(n, 2), guards


def txt_select_batch(lib, d_base, descs, d_txfm_desc, cost_descs, tables, d_txfm_result, d_rdoq_result, d_distortion, d_cost, n_cand, w, h,
                     stream=None, mapping=None, guard=64, fill=0xA5):
    """svt_hip_txt_select_batch for blocks of one size w x h over the records of n_cand candidates.  descs: a record array of
    abi.TXT_DESC_DTYPE; cost_descs: one of abi.TXB_COST_DESC_DTYPE; tables: one of abi.RATE_TABLES_DTYPE; the d_* are device addresses
    (d_rdoq_result may be None).  With mapping (0 or 1) the same through svt_hip_txt_select_batch_mapped.
    Returns (results as a record array of abi.TXT_RESULT_DTYPE, the guard bytes around them)."""
    n = len(descs)
    d_desc, d_cdesc, (tables, d_tab) = upload_descriptors(lib, descs, stream), upload_descriptors(lib, cost_descs, stream), _tables(lib, tables, stream)
    d_out = Guarded(lib, C.sizeof(abi.TxtResult) * n, guard, fill, stream)
    args = (d_base, d_desc.ptr, d_txfm_desc, d_cdesc.ptr, d_tab.ptr, len(tables), d_txfm_result, d_rdoq_result, d_distortion, d_cost, d_out.ptr,
            n_cand, n, w, h)
    if mapping is None:
        _call(lib, "svt_hip_txt_select_batch", *args, stream=stream)
    else:
        _call(lib, "svt_hip_txt_select_batch_mapped", *args, mapping, stream=stream)
    return d_out.read(abi.TXT_RESULT_DTYPE)


def txt_search_batch(lib, d_base, txfm_descs, rdoq_descs, cost_descs, tables, descs, w, h, inverse=False, stream=None, guard=64, fill=0xA5):
    """svt_hip_txt_search_batch: the whole transform-type search of the blocks `descs` (abi.TXT_DESC_DTYPE) of one size w x h over their
    candidates (txfm_descs: abi.TXFM_DESC_DTYPE, rdoq_descs: abi.RDOQ_DESC_DTYPE or None, cost_descs: abi.TXB_COST_DESC_DTYPE, one record per
    candidate each), with a scratch of exactly svt_hip_txt_search_scratch_bytes between guards.  inverse: SVT_HIP_TXT_SEARCH_INVERSE; without
    it no block measures spatial SSE or gets a reconstruction, whatever its descriptor says.
    Returns (results as a record array of abi.TXT_RESULT_DTYPE, the guard bytes around results and scratch)."""
    n, n_cand = len(descs), len(txfm_descs)
    d_tdesc, d_cdesc, d_desc = upload_descriptors(lib, txfm_descs, stream), upload_descriptors(lib, cost_descs, stream), upload_descriptors(lib, descs, stream)
    d_rdesc = upload_descriptors(lib, rdoq_descs, stream) if rdoq_descs is not None else None
    tables, d_tab = _tables(lib, tables, stream)
    need = lib.svt_hip_txt_search_scratch_bytes(n_cand, n)
    d_scratch = Guarded(lib, need, 256, fill, stream)
    d_out = Guarded(lib, C.sizeof(abi.TxtResult) * n, guard, fill, stream)
    _call(lib, "svt_hip_txt_search_batch", d_base, d_tdesc.ptr, d_rdesc.ptr if d_rdesc else None, d_cdesc.ptr, d_tab.ptr, len(tables), d_desc.ptr,
          d_scratch.ptr, need, d_out.ptr, n_cand, n, w, h, abi.TXT_SEARCH_INVERSE if inverse else 0, stream=stream)
    out, guards = d_out.read(abi.TXT_RESULT_DTYPE)
    return out, np.concatenate([guards, d_scratch.read(np.uint8)[1]])


class DeviceCdefPick:
    """Result record, per-block outputs and workspace of svt_hip_cdef_pick_strengths for a grid of n_fb filter blocks, pre-filled
    with `fill`.  run() only enqueues; download() waits for the stream."""

    def __init__(self, lib, n_fb, n_strengths, fill=0xA5):
        self.lib, self.n_fb = lib, n_fb
        self.result = DeviceBuffer(lib, C.sizeof(abi.CdefPickResult))
        self.fb_gi, self.fb_strength = DeviceBuffer(lib, n_fb), DeviceBuffer(lib, 2 * n_fb)
        self.workspace = DeviceBuffer(lib, lib.svt_hip_cdef_pick_workspace_bytes(n_fb, n_strengths))
        for b in (self.result, self.fb_gi, self.fb_strength, self.workspace):
            b.fill(fill)
        _call(lib, "svt_hip_stream_sync")

    def run(self, prm, d_mse, d_filt8x8, stream=None):
        return self.lib.svt_hip_cdef_pick_strengths(C.byref(prm), d_mse, d_filt8x8, self.result.ptr, self.fb_gi.ptr, self.fb_strength.ptr,
                                                    self.workspace.ptr, self.workspace.nbytes, stream)

    def download(self, stream=None):
        return {"result": self.result.download(np.dtype(abi.CDEF_PICK_RESULT_DTYPE), (), stream),
                "fb_gi": self.fb_gi.download(np.uint8, (self.n_fb,), stream),
                "fb_strength": self.fb_strength.download(np.uint8, (2, self.n_fb), stream)}


class DeviceDlfPick:
    """Result record and workspace of svt_hip_dlf_pick_levels / svt_hip_dlf_apply_picked for a picture of width x height luma samples,
    pre-filled with `fill`; pass `result` / `workspace` (device addresses) to use memory of the caller's instead.  run() and apply() only
    enqueue; download() waits for the stream."""

    def __init__(self, lib, width, height, is_16bit, fill=0xA5, result=None, workspace=None):
        self.lib = lib
        self.workspace_bytes = lib.svt_hip_dlf_pick_workspace_bytes(width, height, is_16bit)
        self.bufs = []
        if result is None:
            self.bufs.append(DeviceBuffer(lib, C.sizeof(abi.DlfPickResult)))
            result = self.bufs[-1].ptr
        if workspace is None:
            self.bufs.append(DeviceBuffer(lib, self.workspace_bytes))
            workspace = self.bufs[-1].ptr
        self.result, self.workspace = result, workspace
        for b in self.bufs:
            b.fill(fill)
        _call(lib, "svt_hip_stream_sync")

    def run(self, prm, stream=None):
        return self.lib.svt_hip_dlf_pick_levels(C.byref(prm), self.result, self.workspace, self.workspace_bytes, stream)

    def apply(self, prm, stream=None):
        return self.lib.svt_hip_dlf_apply_picked(C.byref(prm), self.result, stream)

    def download(self, stream=None):
        out = np.empty((), abi.DLF_PICK_RESULT_DTYPE)
        _call(self.lib, "svt_hip_download", out.ctypes.data, self.result, out.nbytes, stream=stream, sync=True)
        return out


class DeviceWienerPick:
    """Unit records, result record, the units for svt_hip_restoration_filter_frame and the workspace of svt_hip_wiener_pick_plane
    for a plane of n_units restoration units, pre-filled with `fill`.  run() only enqueues; download() waits for the stream."""

    def __init__(self, lib, n_units, fill=0xA5):
        self.lib, self.n_units = lib, n_units
        self.units = DeviceBuffer(lib, n_units * C.sizeof(abi.WienerPickUnit))
        self.result = DeviceBuffer(lib, C.sizeof(abi.WienerPickResult))
        self.lr_units = DeviceBuffer(lib, n_units * C.sizeof(abi.LrUnit))
        self.workspace = DeviceBuffer(lib, lib.svt_hip_wiener_pick_workspace_bytes(n_units))
        for b in (self.units, self.result, self.lr_units, self.workspace):
            b.fill(fill)
        _call(lib, "svt_hip_stream_sync")

    def run(self, prm, units, d_M, d_H, d_prev_units=None, stream=None):
        """units: the host array of abi.WienerUnit that svt_hip_wiener_stats took"""
        return self.lib.svt_hip_wiener_pick_plane(C.byref(prm), units, self.n_units, d_M, d_H, d_prev_units, self.units.ptr, self.result.ptr,
                                                  self.lr_units.ptr, self.workspace.ptr, self.workspace.nbytes, stream)

    def download(self, stream=None):
        return {"units": self.units.download(abi.WIENER_PICK_UNIT_DTYPE, (self.n_units,), stream),
                "result": self.result.download(abi.WIENER_PICK_RESULT_DTYPE, (), stream),
                "lr_units": self.lr_units.download(abi.LR_UNIT_DTYPE, (self.n_units,), stream)}


class DeviceRestPick:
    """Unit records, result record, the units for svt_hip_restoration_filter_frame and the workspace of svt_hip_rest_pick_plane for a
    plane of n_units restoration units and n_ep candidates, pre-filled with `fill`.  run() only enqueues and returns the call's
    int64 (launches, or a negative status); download() waits for the stream."""

    def __init__(self, lib, n_units, plane_width, plane_height, n_ep, fill=0xA5):
        self.lib, self.n_units = lib, n_units
        self.units = DeviceBuffer(lib, n_units * C.sizeof(abi.RestPickUnit))
        self.result = DeviceBuffer(lib, C.sizeof(abi.RestPickResult))
        self.lr_units = DeviceBuffer(lib, n_units * C.sizeof(abi.LrUnit))
        self.workspace = DeviceBuffer(lib, lib.svt_hip_rest_pick_workspace_bytes(n_units, plane_width, plane_height, n_ep))
        for b in (self.units, self.result, self.lr_units, self.workspace):
            b.fill(fill)
        _call(lib, "svt_hip_stream_sync")

    def run(self, prm, units, d_wiener_records=None, stream=None):
        """units: the host array of abi.WienerUnit that svt_hip_wiener_stats took"""
        return self.lib.svt_hip_rest_pick_plane(C.byref(prm), units, self.n_units, d_wiener_records, self.units.ptr, self.result.ptr,
                                                self.lr_units.ptr, self.workspace.ptr, self.workspace.nbytes, stream)

    def download(self, stream=None):
        return {"units": self.units.download(abi.REST_PICK_UNIT_DTYPE, (self.n_units,), stream),
                "result": self.result.download(abi.REST_PICK_RESULT_DTYPE, (), stream),
                "lr_units": self.lr_units.download(abi.LR_UNIT_DTYPE, (self.n_units,), stream)}


def warp_batch(lib, descs, d_filter, stream=None, sync=True):
    """svt_hip_warp_batch over a list of abi.WarpDesc (one launch); d_filter: device address of the [193][8] int16 filter table."""
    d_desc = upload_descriptors(lib, descs, stream)
    _call(lib, "svt_hip_warp_batch", d_desc.ptr, len(descs), d_filter, stream=stream, sync=sync)
    return d_desc


def warp_error_workspace(lib, job, n=1):
    """Allocates job.workspace for n candidates; keep the returned buffer alive as long as the job is used."""
    ws = DeviceBuffer(lib, lib.svt_hip_warp_error_workspace_bytes(job.cur_width, job.cur_height, n))
    job.workspace, job.workspace_bytes = ws.ptr, ws.nbytes
    return ws


def warp_error_batch(lib, job, candidates, stream=None, fill=0xA5):
    """svt_hip_warp_error_batch: candidates is a numpy record array (abi.WARP_CANDIDATE_DTYPE); the results come back as one of
    abi.WARP_ERROR_RESULT_DTYPE.  The result buffer is pre-filled with `fill`."""
    cand = np.ascontiguousarray(candidates, np.dtype(abi.WARP_CANDIDATE_DTYPE))
    d_cand, d_res = DeviceBuffer(lib, cand.nbytes), DeviceBuffer(lib, C.sizeof(abi.WarpErrorResult) * len(cand))
    d_cand.upload(cand, stream)
    d_res.fill(fill, stream)
    _call(lib, "svt_hip_warp_error_batch", C.byref(job), d_cand.ptr, d_res.ptr, len(cand), stream=stream)
    return d_res.download(np.dtype(abi.WARP_ERROR_RESULT_DTYPE), (len(cand),), stream)


def gm_refine(lib, job, wmmat, wmtype, n_refinements, best_frame_error, stream=None):
    """svt_hip_gm_refine: (wmmat[8] as a list, wmtype, error) after the hill climb."""
    mat, wt, err = (C.c_int32 * 8)(*wmmat), C.c_int32(wmtype), C.c_int64(0)
    _call(lib, "svt_hip_gm_refine", C.byref(job), mat, C.byref(wt), n_refinements, best_frame_error, C.byref(err), stream=stream)
    return list(mat), wt.value, err.value


class DeviceMap:
    """Uploads host arrays on first use and hands out their device addresses (keyed by the host address)."""

    def __init__(self, lib):
        self.lib, self.m = lib, {}

    def __call__(self, arr):
        key = arr.ctypes.data
        if key not in self.m:
            b = DeviceBuffer(self.lib, arr.nbytes)
            b.upload(arr)
            self.m[key] = (b, arr)
        return self.m[key][0].ptr

    def download(self, arr):
        b, a = self.m[arr.ctypes.data]
        return b.download(a.dtype, a.shape)


def tpl_workspace(lib, job):
    """A workspace of the size svt_hip_tpl_dispenser_frame needs for the picture of `job` (an abi.TplFrameJob)."""
    return DeviceBuffer(lib, lib.svt_hip_tpl_workspace_bytes(job.src.width, job.src.height))


def tpl_dispenser_frame(lib, job, workspace=None, stream=None, sync=True):
    """svt_hip_tpl_dispenser_frame on one abi.TplFrameJob with the caller's workspace or a new one; returns the workspace."""
    if workspace is None:
        workspace = tpl_workspace(lib, job)
    job.workspace, job.workspace_bytes = workspace.ptr, workspace.nbytes
    _call(lib, "svt_hip_tpl_dispenser_frame", C.byref(job), stream=stream, sync=sync)
    return workspace


def tpl_status(lib, job, workspace):
    """The status word a finished svt_hip_tpl_dispenser_frame left in its workspace: 0 unless a dependency wait ran into its bound."""
    off = lib.svt_hip_tpl_status_offset(job.src.width, job.src.height)
    return int(workspace.download(np.uint8, (workspace.nbytes,))[off:off + 4].view(np.uint32)[0])


def tf_workspace(lib, job):
    """A workspace of the size svt_hip_tf_filter_picture needs for the window of `job` (an abi.TfPictureJob)."""
    full = job.centre.pyr.full
    return DeviceBuffer(lib, lib.svt_hip_tf_workspace_bytes(full.width, full.height, job.n_refs))


def tf_filter_picture(lib, job, workspace=None, tot_blks=None, stream=None, sync=True):
    """svt_hip_tf_filter_picture on one abi.TfPictureJob with the caller's workspace and counters (8 bytes, zeroed) or new ones;
    returns (workspace, tot_blks)."""
    if workspace is None:
        workspace = tf_workspace(lib, job)
    if tot_blks is None:
        tot_blks = DeviceBuffer(lib, 8)
        tot_blks.fill(0, stream)
    job.workspace, job.workspace_bytes, job.tot_blks = workspace.ptr, workspace.nbytes, tot_blks.ptr
    _call(lib, "svt_hip_tf_filter_picture", C.byref(job), stream=stream, sync=sync)
    return workspace, tot_blks


def tf_read_back(lib, job, workspace, tot_blks):
    """What a finished svt_hip_tf_filter_picture left behind: the abi.TfB64State of every (reference, b64) as the rows of a uint8 array,
    and the two tot_blks counters."""
    full = job.centre.pyr.full
    nb = frames.b64_count(full.width, full.height)
    raw = workspace.download(np.uint8, (workspace.nbytes,))
    states = []
    for r in range(job.n_refs):
        off = lib.svt_hip_tf_workspace_state_offset(full.width, full.height, job.n_refs, r)
        states.append(raw[off:off + nb * C.sizeof(abi.TfB64State)].reshape(nb, -1))
    return np.concatenate(states), tuple(int(x) for x in tot_blks.download(np.uint32, (2,)))
