"""ctypes mirror of include/*.h (the C-ABI of libsvtav1_hip): the structs here, the function prototypes in prototypes.py.

This module only describes the binary interface; it contains no compute and no CPU fallback.
`load()` raises if the HIP library has not been built (product path must fail loudly).
"""
import ctypes as C
import os

import numpy as np

from .prototypes import PROTOTYPES

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.path.join(PKG_ROOT, "csrc", "libsvtav1_hip.so")


def record_dtype(mirror):
    """The numpy record of a ctypes.Structure, from the mirror's own fields, offsets and size: arrays keep their whole shape,
    nested structures are records, pointers are addresses (<u8).  The *_DTYPE views below are this, so tests/test_abi.py, which
    compares every mirror with the compiler's layout of its header struct, covers them."""
    def fmt(t):
        shape = ()
        while issubclass(t, C.Array):
            shape, t = shape + (t._length_,), t._type_
        if issubclass(t, C.Structure):
            base = record_dtype(t)
        else:
            base = np.dtype("<u8" if issubclass(t, (C.c_void_p, C._Pointer)) else t)
        return np.dtype((base, shape)) if shape else base
    names = [n for n, _ in mirror._fields_]
    return np.dtype({"names": names, "formats": [fmt(t) for _, t in mirror._fields_],
                     "offsets": [getattr(mirror, n).offset for n in names], "itemsize": C.sizeof(mirror)})

ME_MAX_LIST, ME_MAX_REF, ME_SQUARE_PUS = 2, 4, 85


class Plane8(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("stride", C.c_uint32), ("org_x", C.c_uint16), ("org_y", C.c_uint16),
                ("width", C.c_uint16), ("height", C.c_uint16)]


class SearchArea(C.Structure):
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16)]


class MeParams(C.Structure):
    _fields_ = [
        ("hme_search_method", C.c_uint8), ("me_search_method", C.c_uint8),
        ("enable_hme_flag", C.c_uint8), ("enable_hme_level0_flag", C.c_uint8),
        ("enable_hme_level1_flag", C.c_uint8), ("enable_hme_level2_flag", C.c_uint8),
        ("num_hme_sa_w", C.c_uint8), ("num_hme_sa_h", C.c_uint8),
        ("hme_l0_sa_min", SearchArea), ("hme_l0_sa_max", SearchArea), ("hme_l1_sa", SearchArea),
        ("hme_l2_sa", SearchArea), ("me_sa_min", SearchArea), ("me_sa_max", SearchArea),
        ("prehme_enable", C.c_uint8), ("prehme_skip_search_line", C.c_uint8),
        ("prehme_l1_early_exit", C.c_uint8), ("me_mctf", C.c_uint8),
        ("prehme_sa_min", SearchArea * 2), ("prehme_sa_max", SearchArea * 2),
        ("enable_me_hme_ref_pruning", C.c_uint8), ("pad1_", C.c_uint8),
        ("prune_ref_if_hme_sad_dev_bigger_than_th", C.c_uint16),
        ("prune_ref_if_me_sad_dev_bigger_than_th", C.c_uint16),
        ("zz_sad_pct", C.c_uint16), ("phme_sad_pct", C.c_uint16), ("tf_me_exit_th", C.c_uint16),
        ("zz_sad_th", C.c_uint32), ("phme_sad_th", C.c_uint32),
        ("enable_me_sr_adjustment", C.c_uint8), ("distance_based_hme_resizing", C.c_uint8),
        ("reduce_me_sr_based_on_mv_length_th", C.c_uint16), ("stationary_hme_sad_abs_th", C.c_uint16),
        ("stationary_me_sr_divisor", C.c_uint16), ("reduce_me_sr_based_on_hme_sad_abs_th", C.c_uint16),
        ("me_sr_divisor_for_low_hme_sad", C.c_uint16),
        ("me_8x8_var_enabled", C.c_uint8), ("pad3_", C.c_uint8 * 3),
        ("me_sr_div4_th", C.c_uint32), ("me_sr_div2_th", C.c_uint32), ("me_sr_mult2_th", C.c_uint32),
        ("mv_sa_adj_enabled", C.c_uint8), ("mv_sa_adj_nearest_ref_only", C.c_uint8),
        ("mv_sa_adj_mv_size_th", C.c_uint16), ("mv_sa_adj_sa_multiplier", C.c_uint16),
        ("reduce_hme_l0_sr_th_min", C.c_uint8), ("reduce_hme_l0_sr_th_max", C.c_uint8),
        ("me_early_exit_th", C.c_uint32), ("me_safe_limit_zz_th", C.c_uint32),
        ("prev_me_stage_based_exit_th", C.c_uint32), ("prune_me_candidates_th", C.c_int32),
        ("use_best_unipred_cand_only", C.c_uint8),
        ("num_of_list_to_search", C.c_uint8), ("num_of_ref_pic_to_search", C.c_uint8 * 2),
        ("temporal_layer_index", C.c_uint8), ("is_ref", C.c_uint8), ("hierarchical_levels", C.c_uint8),
        ("similar_brightness_refs", C.c_uint8),
        ("enable_me_8x8", C.c_uint8), ("enable_me_16x16", C.c_uint8), ("max_number_of_pus_per_sb", C.c_uint8),
        ("max_cand", C.c_uint8), ("max_refs", C.c_uint8), ("max_l0", C.c_uint8),
        ("only_l_bwd", C.c_uint8), ("input_resolution_le_480p", C.c_uint8), ("pad4_", C.c_uint8 * 2),
        ("picture_number", C.c_uint64), ("ref_picture_number", (C.c_uint64 * 4) * 2),
    ]

    def stored_pus(self):
        return (85 if self.enable_me_8x8 else 21) if self.enable_me_16x16 else 5

    def to_dict(self):
        def conv(v):
            if isinstance(v, SearchArea):
                return [v.width, v.height]
            if hasattr(v, "__len__"):
                return [conv(x) for x in v]
            return int(v)
        return {n: conv(getattr(self, n)) for n, _ in self._fields_ if not n.startswith("pad")}

    @classmethod
    def from_dict(cls, d):
        p = cls()
        for n, t in cls._fields_:
            if n.startswith("pad") or n not in d:
                continue
            v = d[n]
            if t is SearchArea:
                setattr(p, n, SearchArea(*v))
            elif n in ("prehme_sa_min", "prehme_sa_max"):
                for i in range(2):
                    getattr(p, n)[i] = SearchArea(*v[i])
            elif n == "ref_picture_number":
                for l in range(2):
                    for r in range(4):
                        p.ref_picture_number[l][r] = v[l][r]
            elif n == "num_of_ref_pic_to_search":
                p.num_of_ref_pic_to_search[0], p.num_of_ref_pic_to_search[1] = v
            else:
                setattr(p, n, v)
        return p


class Pyramid8(C.Structure):
    _fields_ = [("full", Plane8), ("quarter", Plane8), ("sixteenth", Plane8)]


class MeSearchResult(C.Structure):
    _fields_ = [("hme_sad", C.c_uint64), ("hme_sc_x", C.c_int16), ("hme_sc_y", C.c_int16),
                ("do_ref", C.c_uint8), ("pad_", C.c_uint8 * 3)]


class MeFrameOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "best_sad", "best_mv", "search_results", "me_mv_array", "me_candidate_array",
        "total_me_candidate_index", "me_64x64_distortion", "me_32x32_distortion", "me_16x16_distortion",
        "me_8x8_distortion", "me_8x8_cost_variance", "rc_me_distortion")]


class MeFrameJob(C.Structure):
    _fields_ = [("prm", MeParams), ("src", Pyramid8), ("ref", (Pyramid8 * 4) * 2), ("out", MeFrameOut)]


class SadLoopDesc(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("ref_off", C.c_uint64), ("src_stride", C.c_uint32),
                ("ref_stride", C.c_uint32), ("src_stride_raw", C.c_uint32), ("block_width", C.c_uint16),
                ("block_height", C.c_uint16), ("search_area_width", C.c_int16),
                ("search_area_height", C.c_int16), ("skip_search_line", C.c_uint8), ("pad_", C.c_uint8 * 7)]


class SadLoopResult(C.Structure):
    _fields_ = [("best_sad", C.c_uint64), ("x", C.c_int16), ("y", C.c_int16), ("pad_", C.c_uint32)]


_lib = None


def load():
    """Load libsvtav1_hip.so (built by __graft_entry__.build()).  No fallback."""
    global _lib
    if _lib is None:
        # tuning aid: SVTAV1_HIP_LIB names another build of the SAME library (kernel variants side by side in one GPU call)
        global LIB_PATH
        LIB_PATH = os.environ.get("SVTAV1_HIP_LIB", LIB_PATH)
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP path has no CPU fallback)")
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():   # every function of include/*.h; one the library lacks fails here
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype and getattr(C, restype), [getattr(C, t) for t in argtypes]
        _lib = lib
    return _lib


NO_OFFSET = 0xFFFFFFFFFFFFFFFF
# SvtHipStatus (include/svt_hip.h:34-39), as the signed int32 values a ctypes call returns
SVT_HIP_OK = 0
SVT_HIP_ERR_NO_DEVICE = 0x80001000 - (1 << 32)
SVT_HIP_ERR_BAD_PARAMETER = 0x80001005 - (1 << 32)
SVT_HIP_ERR_RUNTIME = 0x80001001 - (1 << 32)
QUANT_NONE, QUANT_B, QUANT_B_HBD, QUANT_FP, QUANT_FP_HBD = range(5)
TX_FWD, TX_INV, TX_PIXEL16, TX_FULLCOEFF, TX_SRC_PRED, TX_SATD = 1, 2, 4, 8, 16, 32
TXFM_RESULT_BYTES = 16


class TxfmDesc(C.Structure):
    _fields_ = [("residual_off", C.c_uint64), ("coeff_off", C.c_uint64), ("qcoeff_off", C.c_uint64),
                ("dqcoeff_off", C.c_uint64), ("pred_off", C.c_uint64), ("recon_off", C.c_uint64),
                ("iscan_off", C.c_uint64), ("qm_off", C.c_uint64), ("iqm_off", C.c_uint64),
                ("residual_stride", C.c_uint32), ("pred_stride", C.c_uint32), ("recon_stride", C.c_uint32),
                ("zbin", C.c_int16 * 2), ("round", C.c_int16 * 2), ("quant", C.c_int16 * 2),
                ("quant_shift", C.c_int16 * 2), ("dequant", C.c_int16 * 2),
                ("tx_type", C.c_uint8), ("shape", C.c_uint8), ("bit_depth", C.c_uint8), ("quant_mode", C.c_uint8),
                ("log_scale", C.c_uint8), ("flags", C.c_uint8), ("dist_w", C.c_uint8), ("dist_h", C.c_uint8)]


class TxfmResult(C.Structure):
    _fields_ = [("three_quad_energy", C.c_uint64), ("eob", C.c_uint16), ("pad_", C.c_uint16), ("satd", C.c_uint32)]


class CoeffCost(C.Structure):          # SvtHipCoeffCost == LvMapCoeffCost (md_rate_estimation.h:41-49)
    _fields_ = [("txb_skip", (C.c_int32 * 2) * 13), ("base_eob", (C.c_int32 * 3) * 4), ("base", (C.c_int32 * 8) * 42),
                ("eob_extra", (C.c_int32 * 2) * 9), ("dc_sign", (C.c_int32 * 2) * 3), ("lps", (C.c_int32 * 26) * 21)]


class RateTables(C.Structure):         # SvtHipRateTables: one set of rate tables
    _fields_ = [("coeff", (CoeffCost * 2) * 5), ("eob", (((C.c_int32 * 11) * 2) * 2) * 7),
                ("intra_tx_type", (((C.c_int32 * 17) * 13) * 4) * 3), ("inter_tx_type", ((C.c_int32 * 17) * 4) * 4)]


TXB_COST_EXACT, TXB_COST_SHORT_SMALL, TXB_COST_SHORT_ALL = range(3)   # SvtHipTxbCostDesc::est_mode
TXB_COST_NO_SHIFT = 1                                                  # SvtHipTxbCostDesc::flags


class TxbCostDesc(C.Structure):        # SvtHipTxbCostDesc
    _fields_ = [("qcoeff_off", C.c_uint64), ("iscan_off", C.c_uint64), ("table", C.c_uint32), ("lambda", C.c_uint32), ("eob", C.c_uint16),
                ("tx_type", C.c_uint8), ("plane_type", C.c_uint8), ("txb_skip_ctx", C.c_uint8), ("dc_sign_ctx", C.c_uint8),
                ("pred_mode", C.c_uint8), ("filter_intra_mode", C.c_uint8), ("reduced_tx_set", C.c_uint8),
                ("fast_coeff_est_level", C.c_uint8), ("subres_step", C.c_uint8), ("est_mode", C.c_uint8), ("flags", C.c_uint8),
                ("pad_", C.c_uint8 * 3)]


class TxbCost(C.Structure):            # SvtHipTxbCost
    _fields_ = [("bits", C.c_uint64), ("rd_cost", C.c_uint64)]


# numpy views of SvtHipRateTables and of arrays of SvtHipTxbCostDesc / SvtHipTxbCost
COEFF_COST_DTYPE, RATE_TABLES_DTYPE = record_dtype(CoeffCost), record_dtype(RateTables)
TXB_COST_DESC_DTYPE, TXB_COST_DTYPE = record_dtype(TxbCostDesc), record_dtype(TxbCost)

RDOQ_PERFORM, RDOQ_FAST_MODE, RDOQ_SHARPNESS = 1, 2, 4                # SvtHipRdoqDesc::flags
# SvtHipRdoqResult::path: the way a block went (path & RDOQ_PATH_MASK) and what happened on the way
(RDOQ_PATH_NOT_FLAGGED, RDOQ_PATH_EOB_ZERO, RDOQ_PATH_REQUANT_SATD, RDOQ_PATH_REQUANT_EOB, RDOQ_PATH_EARLY_EXIT,
 RDOQ_PATH_TRELLIS) = range(6)
RDOQ_PATH_MASK, RDOQ_PATH_FAST_TRIM, RDOQ_PATH_SKIP, RDOQ_PATH_BAD_EOB = 7, 8, 16, 32


class RdoqDesc(C.Structure):           # SvtHipRdoqDesc
    _fields_ = [("table", C.c_uint32), ("lambda", C.c_uint32), ("zbin", C.c_int16 * 2), ("round", C.c_int16 * 2), ("quant", C.c_int16 * 2),
                ("quant_shift", C.c_int16 * 2), ("early_exit_limit", C.c_uint32), ("plane_type", C.c_uint8), ("txb_skip_ctx", C.c_uint8),
                ("dc_sign_ctx", C.c_uint8), ("is_inter", C.c_uint8), ("eob_th", C.c_uint8), ("eob_fast_th", C.c_uint8),
                ("satd_factor", C.c_uint8), ("dequant_shift", C.c_uint8), ("flags", C.c_uint8), ("pic_bit_depth", C.c_uint8), ("pad_", C.c_uint8 * 2)]


class RdoqResult(C.Structure):         # SvtHipRdoqResult
    _fields_ = [("eob", C.c_uint16), ("cul_level", C.c_uint8), ("path", C.c_uint8)]


TXFM_DESC_DTYPE, TXFM_RESULT_DTYPE = record_dtype(TxfmDesc), record_dtype(TxfmResult)
RDOQ_DESC_DTYPE, RDOQ_RESULT_DTYPE = record_dtype(RdoqDesc), record_dtype(RdoqResult)

TXT_MAX_CAND = 16                                                     # SVT_HIP_TXT_MAX_CAND
TXT_EARLY_EXIT, TXT_SPATIAL_SSE = 1, 2                                # SvtHipTxtDesc::flags
TXT_SEARCH_INVERSE = 1                                                # flags of svt_hip_txt_search_batch
TXT_NO_CAND = 0xFF                                                    # SvtHipTxtResult::cand where no candidate reached the comparison


class SpatialSrc(C.Structure):         # SvtHipSpatialSrc
    _fields_ = [("src_off", C.c_uint64), ("src_stride", C.c_uint32), ("crop_w", C.c_uint8), ("crop_h", C.c_uint8), ("pad_", C.c_uint8 * 2)]


class TxtDesc(C.Structure):            # SvtHipTxtDesc
    _fields_ = [("src_off", C.c_uint64), ("dst_qcoeff_off", C.c_uint64), ("dst_dqcoeff_off", C.c_uint64), ("dst_recon_off", C.c_uint64),
                ("first_cand", C.c_uint32), ("src_stride", C.c_uint32), ("dst_recon_stride", C.c_uint32), ("full_lambda", C.c_uint32),
                ("early_exit_coeff_th", C.c_uint32), ("early_exit_dist_th", C.c_uint32), ("tx_pixels", C.c_uint32),
                ("satd_early_exit_th", C.c_uint16), ("txt_rate_cost_th", C.c_uint16), ("group_start", C.c_uint16), ("n_cand", C.c_uint8),
                ("flags", C.c_uint8), ("crop_w", C.c_uint8), ("crop_h", C.c_uint8), ("pad_", C.c_uint8 * 2)]


class TxtResult(C.Structure):          # SvtHipTxtResult
    _fields_ = [("bits", C.c_uint64), ("distortion", C.c_uint64 * 2), ("cost", C.c_uint64), ("eob", C.c_uint16), ("quant_mask", C.c_uint16),
                ("cost_mask", C.c_uint16), ("tx_type", C.c_uint8), ("cand", C.c_uint8), ("cul_level", C.c_uint8), ("pad_", C.c_uint8 * 7)]


SPATIAL_SRC_DTYPE, TXT_DESC_DTYPE, TXT_RESULT_DTYPE = record_dtype(SpatialSrc), record_dtype(TxtDesc), record_dtype(TxtResult)


class CdefList(C.Structure):
    _fields_ = [("by", C.c_uint8), ("bx", C.c_uint8)]


class CdefPlane(C.Structure):
    _fields_ = [("recon", C.c_void_p), ("source", C.c_void_p), ("recon_stride", C.c_uint32), ("source_stride", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("is_16bit", C.c_uint8), ("xdec", C.c_uint8),
                ("ydec", C.c_uint8), ("pli", C.c_uint8)]


class CdefSearchParams(C.Structure):
    _fields_ = [("n_strengths", C.c_int32), ("strengths", C.c_int8 * 64), ("pri_damping", C.c_int32),
                ("sec_damping", C.c_int32), ("coeff_shift", C.c_int32), ("subsampling_factor", C.c_int32)]


CDEF_MAX_STRENGTHS = 64           # SVT_HIP_CDEF_MAX_STRENGTHS
CDEF_PICK_WIDTHS, CDEF_PICK_MAX_LEVELS = 4, 8   # signalling widths cdef_bits 0..3; CDEF_MAX_STRENGTHS of the reference


class CdefPickParams(C.Structure):   # SvtHipCdefPickParams
    _fields_ = [("n_strengths", C.c_int32), ("fb_cols", C.c_uint32), ("fb_rows", C.c_uint32), ("w8", C.c_uint32), ("h8", C.c_uint32),
                ("zero_fs_cost_bias", C.c_uint16), ("pad_", C.c_uint16), ("lambda", C.c_uint64),
                ("strengths", C.c_int8 * CDEF_MAX_STRENGTHS), ("strengths_uv", C.c_int8 * CDEF_MAX_STRENGTHS)]


class CdefPickResult(C.Structure):   # SvtHipCdefPickResult
    _fields_ = [("cdef_bits", C.c_int32), ("nb_strengths", C.c_int32), ("sb_count", C.c_int32), ("pad_", C.c_int32),
                ("y_index", C.c_int32 * 8), ("uv_index", C.c_int32 * 8), ("y_strength", C.c_uint8 * 8), ("uv_strength", C.c_uint8 * 8),
                ("best_cost", C.c_uint64), ("joint_mse", C.c_uint64 * 4), ("rd_cost", C.c_uint64 * 4),
                ("lev0", (C.c_int32 * 8) * 4), ("lev1", (C.c_int32 * 8) * 4)]


# numpy view of SvtHipCdefPickResult
CDEF_PICK_RESULT_DTYPE = record_dtype(CdefPickResult)


class LfMi(C.Structure):          # SvtHipLfMi (include/svt_hip_lf.h)
    _fields_ = [(n, C.c_uint8) for n in ("bsize", "tx_size_y", "tx_size_uv", "skip_inter", "segment_id", "ref_frame0", "mode_lf",
                                         "reserved")]


class LfFrame(C.Structure):       # SvtHipLfFrame
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_uint32 * 3), ("width", C.c_uint32), ("height", C.c_uint32),
                ("mi", C.c_void_p), ("mi_stride", C.c_uint32), ("mi_rows", C.c_uint32), ("mi_cols", C.c_uint32),
                ("lvl", C.c_uint8 * 768), ("filter_level", C.c_uint8 * 2), ("filter_level_u", C.c_uint8),
                ("filter_level_v", C.c_uint8), ("sharpness_level", C.c_uint8), ("bit_depth", C.c_uint8), ("is_16bit", C.c_uint8),
                ("plane_start", C.c_uint8), ("plane_end", C.c_uint8), ("reserved", C.c_uint8 * 3)]


LF_MI_DTYPE = record_dtype(LfMi)   # numpy view of the mode-info grid

DLF_MAX_LEVEL, DLF_PICK_DEFAULT_ROUNDS, DLF_PICK_RESULT_BYTES = 63, 16, 1608


class DlfPickParams(C.Structure):   # SvtHipDlfPickParams
    _fields_ = [("frame", LfFrame), ("src", C.c_void_p * 3), ("src_stride", C.c_uint32 * 3), ("sse_width", C.c_uint32 * 3),
                ("sse_height", C.c_uint32 * 3), ("plane_mask", C.c_uint32), ("start_level", C.c_uint8 * 3), ("only_4x4", C.c_uint8),
                ("early_exit_convergence", C.c_int32), ("max_rounds", C.c_int32), ("segmentation_enabled", C.c_uint8),
                ("seg_lf_enabled", (C.c_uint8 * 4) * 8), ("pad_", C.c_uint8 * 3), ("seg_lf_data", (C.c_int16 * 4) * 8)]


class DlfPickResult(C.Structure):   # SvtHipDlfPickResult
    _fields_ = [("level", C.c_int32 * 3), ("finished", C.c_uint32), ("rounds", C.c_int32 * 3), ("trials", C.c_int32 * 3),
                ("hdr_level", C.c_uint8 * 4), ("pad_", C.c_int32), ("best_err", C.c_int64 * 3), ("ss_err", (C.c_int64 * 64) * 3)]


DLF_PICK_RESULT_DTYPE = record_dtype(DlfPickResult)   # numpy view of SvtHipDlfPickResult


class SgrParams(C.Structure):     # SvtHipSgrParams == SgrParamsType
    _fields_ = [("r", C.c_int32 * 2), ("s", C.c_int32 * 2)]


class SgrUnit(C.Structure):       # SvtHipSgrUnit
    _fields_ = [("dat", C.c_void_p), ("src", C.c_void_p), ("dat_stride", C.c_uint32), ("src_stride", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("is_16bit", C.c_uint8), ("bit_depth", C.c_uint8),
                ("pu_w", C.c_uint8), ("pu_h", C.c_uint8)]


SGR_PARAMS = [(2, 1, 140, 3236), (2, 1, 112, 2158), (2, 1, 93, 1618), (2, 1, 80, 1438), (2, 1, 70, 1295), (2, 1, 58, 1177),
              (2, 1, 47, 1079), (2, 1, 37, 996), (2, 1, 30, 925), (2, 1, 25, 863), (0, 1, -1, 2589), (0, 1, -1, 1618),
              (0, 1, -1, 1177), (0, 1, -1, 925), (2, 0, 56, -1), (2, 0, 22, -1)]   # r0, r1, s0, s1 (AV1 Sgr_Params)


class AnalysisJob(C.Structure):   # SvtHipAnalysisJob
    _fields_ = [("pyr", Pyramid8), ("variance", C.c_void_p), ("mean", C.c_void_p)]


class WienerUnit(C.Structure):    # SvtHipWienerUnit
    _fields_ = [("dgd", C.c_void_p), ("src", C.c_void_p), ("dgd_stride", C.c_uint32), ("src_stride", C.c_uint32),
                ("h_start", C.c_int32), ("h_end", C.c_int32), ("v_start", C.c_int32), ("v_end", C.c_int32)]


LR_EXTRA_HORZ = 4                   # SVT_HIP_LR_EXTRA_HORZ


class LrUnit(C.Structure):          # SvtHipLrUnit
    _fields_ = [("restoration_type", C.c_uint8), ("ep", C.c_uint8), ("pad_", C.c_int16), ("xqd", C.c_int32 * 2),
                ("hfilter", C.c_int16 * 8), ("vfilter", C.c_int16 * 8)]


LR_UNIT_DTYPE = record_dtype(LrUnit)


class LrPlane(C.Structure):         # SvtHipLrPlane
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_stride", C.c_uint32), ("dst_stride", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("is_16bit", C.c_uint8),
                ("bit_depth", C.c_uint8), ("unit_size", C.c_uint32), ("horz_units", C.c_uint32), ("vert_units", C.c_uint32),
                ("units", C.c_void_p), ("boundary_above", C.c_void_p), ("boundary_below", C.c_void_p),
                ("boundary_stride", C.c_uint32), ("optimized_lr", C.c_uint32)]


class WienerPickParams(C.Structure):   # SvtHipWienerPickParams
    _fields_ = [("wiener_win", C.c_int32), ("is_16bit", C.c_int32), ("bit_depth", C.c_int32), ("plane_width", C.c_uint32),
                ("plane_height", C.c_uint32), ("use_refinement", C.c_int32), ("max_one_refinement_step", C.c_int32), ("rdmult", C.c_int32),
                ("wiener_restore_cost", C.c_int32 * 2)]


WIENER_PICK_UNIT_BYTES = 64         # SVT_HIP_WIENER_PICK_UNIT_BYTES


class WienerPickUnit(C.Structure):     # SvtHipWienerPickUnit
    _fields_ = [("sse", C.c_int64 * 2), ("hfilter", C.c_int16 * 8), ("vfilter", C.c_int16 * 8), ("bits", C.c_int64),
                ("best_rtype", C.c_int32), ("trials", C.c_int32)]


class WienerPickResult(C.Structure):   # SvtHipWienerPickResult
    _fields_ = [("frame_restoration_type", C.c_int32), ("n_wiener", C.c_int32), ("sse", C.c_int64 * 2), ("bits", C.c_int64 * 2),
                ("cost", C.c_double * 2)]


WIENER_PICK_UNIT_DTYPE, WIENER_PICK_RESULT_DTYPE = record_dtype(WienerPickUnit), record_dtype(WienerPickResult)


class RestPickParams(C.Structure):     # SvtHipRestPickParams
    _fields_ = [("is_16bit", C.c_int32), ("bit_depth", C.c_int32), ("plane_width", C.c_uint32), ("plane_height", C.c_uint32),
                ("ss_x", C.c_int32), ("ss_y", C.c_int32), ("wiener_win", C.c_int32), ("sg_start_ep", C.c_int32), ("sg_end_ep", C.c_int32),
                ("sg_ep_inc", C.c_int32), ("sg_refine", C.c_int32), ("rdmult", C.c_int32), ("wiener_restore_cost", C.c_int32 * 2),
                ("sgrproj_restore_cost", C.c_int32 * 2), ("switchable_restore_cost", C.c_int32 * 3)]


REST_PICK_UNIT_BYTES, REST_PICK_RESULT_BYTES = 64, 184      # SVT_HIP_REST_PICK_UNIT_BYTES, SVT_HIP_REST_PICK_RESULT_BYTES


class RestPickUnit(C.Structure):       # SvtHipRestPickUnit
    _fields_ = [("sse", C.c_int64 * 3), ("search_err", C.c_int64), ("ep", C.c_int32), ("xqd", C.c_int32 * 2), ("best_rtype", C.c_int32 * 3),
                ("trials", C.c_int32), ("pad_", C.c_int32)]


class RestPickResult(C.Structure):     # SvtHipRestPickResult
    _fields_ = [("frame_restoration_type", C.c_int32), ("tested", C.c_int32), ("sse", C.c_int64 * 4), ("bits", C.c_int64 * 4),
                ("cost", C.c_double * 4), ("n_units_of_type", C.c_int32 * 3), ("pad_", C.c_int32), ("sg_frame_ep_cnt", C.c_int32 * 16)]


REST_PICK_UNIT_DTYPE, REST_PICK_RESULT_DTYPE = record_dtype(RestPickUnit), record_dtype(RestPickResult)


class ConvolveParams(C.Structure):   # SvtHipConvolveParams == ConvolveParams (definitions.h:580-593)
    _fields_ = [("ref", C.c_int32), ("do_average", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_int32), ("round_0", C.c_int32),
                ("round_1", C.c_int32), ("plane", C.c_int32), ("is_compound", C.c_int32), ("use_jnt_comp_avg", C.c_int32),
                ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32), ("use_dist_wtd_comp_avg", C.c_int32)]


class InterpFilterParams(C.Structure):   # SvtHipInterpFilterParams == InterpFilterParams (definitions.h:750-755)
    _fields_ = [("filter_ptr", C.c_void_p), ("taps", C.c_uint16), ("subpel_shifts", C.c_uint16), ("interp_filter", C.c_int32)]


class ConvolveDesc(C.Structure):         # SvtHipConvolveDesc (include/svt_hip_inter.h)
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("w", C.c_uint16),
                ("h", C.c_uint16), ("filter_x", C.c_int16 * 8), ("filter_y", C.c_int16 * 8), ("taps_x", C.c_uint8), ("taps_y", C.c_uint8),
                ("round_0", C.c_uint8), ("round_1", C.c_uint8), ("bit_depth", C.c_uint8), ("is_16bit", C.c_uint8), ("compound", C.c_uint8),
                ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8), ("pad_", C.c_uint8 * 3), ("cbuf", C.c_void_p),
                ("cbuf_stride", C.c_uint32), ("pad2_", C.c_uint32)]


BLEND_D16, BLEND_D16_DIFFWTD, BLEND_MASK, BLEND_VMASK, BLEND_HMASK = range(5)   # SVT_HIP_BLEND_*
WEDGE_TYPES = 16
MASK_SEARCH_OK, MASK_SEARCH_BAD_WEDGE_SIZE, MASK_SEARCH_BAD_DESC = range(3)     # SVT_HIP_MASK_SEARCH_*


class BlendDesc(C.Structure):            # SvtHipBlendDesc (include/svt_hip_inter.h)
    _fields_ = [("src0", C.c_void_p), ("src1", C.c_void_p), ("dst", C.c_void_p), ("mask", C.c_void_p), ("src0_stride", C.c_uint32),
                ("src1_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("mask_stride", C.c_uint32), ("w", C.c_uint16), ("h", C.c_uint16),
                ("kind", C.c_uint8), ("subw", C.c_uint8), ("subh", C.c_uint8), ("mask_type", C.c_uint8), ("round_0", C.c_uint8),
                ("round_1", C.c_uint8), ("bit_depth", C.c_uint8), ("is_16bit", C.c_uint8), ("pad_", C.c_uint32)]


class MaskSearchDesc(C.Structure):       # SvtHipMaskSearchDesc
    _fields_ = [("src", C.c_void_p), ("pred0", C.c_void_p), ("pred1", C.c_void_p), ("wedge_masks", C.c_void_p),
                ("src_stride", C.c_uint32), ("pred0_stride", C.c_uint32), ("pred1_stride", C.c_uint32), ("w", C.c_uint16),
                ("h", C.c_uint16), ("bit_depth", C.c_uint8), ("is_16bit", C.c_uint8), ("pad_", C.c_uint8 * 6)]


class MaskSearchResult(C.Structure):     # SvtHipMaskSearchResult
    _fields_ = [("wedge_sse", C.c_uint64 * WEDGE_TYPES), ("diffwtd_sse", C.c_uint64 * 2), ("pred0_to_pred1_dist", C.c_uint32),
                ("wedge_sign", C.c_uint8 * WEDGE_TYPES), ("best_wedge_index", C.c_int8), ("best_wedge_sign", C.c_int8),
                ("best_diffwtd_type", C.c_uint8), ("status", C.c_uint8)]


# numpy view of an array of SvtHipMaskSearchResult
MASK_SEARCH_RESULT_DTYPE = record_dtype(MaskSearchResult)


WARP_FILTER_ROWS, WARP_FILTER_BYTES = 193, 193 * 8 * 2                          # SVT_HIP_WARP_FILTER_*
WARP_ERROR_BLOCK = 32
WARP_ERROR_OK, WARP_ERROR_BAD_SHEAR = range(2)                                  # SVT_HIP_WARP_ERROR_*


class WarpDesc(C.Structure):             # SvtHipWarpDesc (include/svt_hip_inter.h)
    _fields_ = [("ref", C.c_void_p), ("dst", C.c_void_p), ("cbuf", C.c_void_p), ("ref_stride", C.c_uint32), ("dst_stride", C.c_uint32),
                ("cbuf_stride", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("p_col", C.c_int32), ("p_row", C.c_int32),
                ("p_width", C.c_uint16), ("p_height", C.c_uint16), ("mat", C.c_int32 * 6), ("alpha", C.c_int16), ("beta", C.c_int16),
                ("gamma", C.c_int16), ("delta", C.c_int16), ("subsampling_x", C.c_uint8), ("subsampling_y", C.c_uint8),
                ("round_0", C.c_uint8), ("round_1", C.c_uint8), ("bit_depth", C.c_uint8), ("is_16bit", C.c_uint8), ("compound", C.c_uint8),
                ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8), ("pad_", C.c_uint8 * 7)]


class WarpErrorJob(C.Structure):         # SvtHipWarpErrorJob
    _fields_ = [("ref", C.c_void_p), ("cur", C.c_void_p), ("filter", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64),
                ("ref_stride", C.c_uint32), ("ref_width", C.c_uint32), ("ref_height", C.c_uint32), ("cur_stride", C.c_uint32),
                ("cur_width", C.c_uint32), ("cur_height", C.c_uint32), ("chess_refn", C.c_uint8), ("pad_", C.c_uint8 * 7)]


class WarpCandidate(C.Structure):        # SvtHipWarpCandidate
    _fields_ = [("mat", C.c_int32 * 6), ("alpha", C.c_int16), ("beta", C.c_int16), ("gamma", C.c_int16), ("delta", C.c_int16),
                ("best_error", C.c_int64)]


class WarpErrorResult(C.Structure):      # SvtHipWarpErrorResult
    _fields_ = [("error", C.c_int64), ("blocks_summed", C.c_uint32), ("status", C.c_uint8), ("pad_", C.c_uint8 * 3)]


# numpy views of arrays of SvtHipWarpCandidate / SvtHipWarpErrorResult
WARP_CANDIDATE_DTYPE, WARP_ERROR_RESULT_DTYPE = record_dtype(WarpCandidate), record_dtype(WarpErrorResult)


GM_MAX_CORNERS, GM_MAX_PLANES, GM_MAX_MATCH_SZ = 4096, 8, 13     # SVT_HIP_GM_* (include/svt_hip_inter.h)


def gm_status(status):
    """SVT_HIP_GM_STATUS: a SvtHipStatus as the uint16_t that svt_hip_gm_detect_corners and svt_hip_gm_match_corners return"""
    return status & 0xFFFF


class GmPlane(C.Structure):              # SvtHipGmPlane
    _fields_ = [("luma", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32), ("pad_", C.c_uint32)]


class GmCorners(C.Structure):            # SvtHipGmCorners
    _fields_ = [("count", C.c_uint32), ("found", C.c_uint32), ("xy", C.c_int32 * (2 * GM_MAX_CORNERS))]


class GmMatchJob(C.Structure):           # SvtHipGmMatchJob
    _fields_ = [("frm", GmPlane), ("ref", GmPlane), ("frm_corners", C.c_void_p), ("ref_corners", C.c_void_p), ("frm_quarters", C.c_uint8),
                ("ref_quarters", C.c_uint8), ("match_sz", C.c_uint8), ("pad_", C.c_uint8 * 5)]


class GmMatches(C.Structure):            # SvtHipGmMatches
    _fields_ = [("count", C.c_uint32), ("pad_", C.c_uint32), ("pts", C.c_int32 * (4 * GM_MAX_CORNERS))]


GM_CORNERS_DTYPE, GM_MATCHES_DTYPE = record_dtype(GmCorners), record_dtype(GmMatches)   # numpy views of the two device records


SCALE_MAX_PLANES, SCALE_MAX_TILE_COLS, SCALE_INVALID = 24, 64, -1     # SVT_HIP_SCALE_* (include/svt_hip_scale.h)


class ResizePlane(C.Structure):          # SvtHipResizePlane
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("src_width", C.c_uint32),
                ("src_height", C.c_uint32), ("dst_width", C.c_uint32), ("dst_height", C.c_uint32), ("is_16bit", C.c_uint8),
                ("bit_depth", C.c_uint8), ("pad_", C.c_uint8 * 6)]


class SuperresPlane(C.Structure):        # SvtHipSuperresPlane
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("rows", C.c_uint32),
                ("frame_width", C.c_uint16), ("superres_upscaled_width", C.c_uint16), ("superres_denominator", C.c_uint8),
                ("sub_x", C.c_uint8), ("is_16bit", C.c_uint8), ("bit_depth", C.c_uint8), ("tile_cols", C.c_uint16),
                ("tile_col_start_mi", C.c_uint16 * (SCALE_MAX_TILE_COLS + 1))]


class ConvolveScaleDesc(C.Structure):    # SvtHipConvolveScaleDesc
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("w", C.c_uint16),
                ("h", C.c_uint16), ("pad0_", C.c_uint32), ("filter_x", C.c_void_p), ("filter_y", C.c_void_p), ("subpel_x_qn", C.c_int32),
                ("x_step_qn", C.c_int32), ("subpel_y_qn", C.c_int32), ("y_step_qn", C.c_int32), ("taps_x", C.c_uint8), ("taps_y", C.c_uint8),
                ("round_0", C.c_uint8), ("round_1", C.c_uint8), ("bit_depth", C.c_uint8), ("is_16bit", C.c_uint8), ("compound", C.c_uint8),
                ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8), ("pad_", C.c_uint8 * 7), ("cbuf", C.c_void_p),
                ("cbuf_stride", C.c_uint32), ("pad2_", C.c_uint32)]


class ScaleFactors(C.Structure):         # SvtHipScaleFactors
    _fields_ = [("x_scale_fp", C.c_int32), ("y_scale_fp", C.c_int32), ("x_step_q4", C.c_int32), ("y_step_q4", C.c_int32)]


class ScaledPosition(C.Structure):       # SvtHipScaledPosition
    _fields_ = [("pos_x", C.c_int32), ("pos_y", C.c_int32), ("subpel_x", C.c_int32), ("subpel_y", C.c_int32), ("xs", C.c_int32),
                ("ys", C.c_int32)]


CONVOLVE_SCALE_DESC_DTYPE = record_dtype(ConvolveScaleDesc)   # numpy view of an array of descriptors


class TfBlock(C.Structure):              # SvtHipTfBlock (include/svt_hip_tf.h)
    _fields_ = [("src", C.c_void_p * 3), ("pred", C.c_void_p * 3), ("accum", C.c_void_p * 3), ("count", C.c_void_p * 3),
                ("src_stride", C.c_uint32 * 3), ("pred_stride", C.c_uint32 * 3), ("decay_factor_fp16", C.c_uint32 * 3),
                ("block_error", C.c_uint64 * 4), ("mv_x", C.c_int16 * 4), ("mv_y", C.c_int16 * 4), ("mv_dist_th", C.c_uint16),
                ("split", C.c_uint8), ("chroma", C.c_uint8), ("ss_x", C.c_uint8), ("ss_y", C.c_uint8), ("is_16bit", C.c_uint8),
                ("bit_depth", C.c_uint8), ("zz_based", C.c_uint8), ("pad_", C.c_uint8 * 7)]


class TfOut(C.Structure):                # SvtHipTfOut
    _fields_ = [("dst", C.c_void_p * 3), ("dst_stride", C.c_uint32 * 3), ("pad_", C.c_uint32)]


TF_MAX_REFS = 32


class TfCtrls(C.Structure):              # SvtHipTfCtrls
    _fields_ = [("half_pel_mode", C.c_uint8), ("quarter_pel_mode", C.c_uint8), ("eight_pel_mode", C.c_uint8), ("use_2tap", C.c_uint8),
                ("sub_sampling_shift", C.c_uint8), ("use_pred_64x64_only_th", C.c_uint8), ("subpel_early_exit_th", C.c_uint8),
                ("use_8bit_subpel", C.c_uint8), ("use_zz_based_filter", C.c_uint8), ("enable_8x8_pred", C.c_uint8), ("low_delay", C.c_uint8),
                ("pad_", C.c_uint8 * 5),
                ("pred_error_32x32_th", C.c_uint64)]


class TfPic(C.Structure):                # SvtHipTfPic
    _fields_ = [("pyr", Pyramid8), ("chroma8", C.c_void_p * 2), ("chroma8_stride", C.c_uint32), ("pad_", C.c_uint32), ("hbd", C.c_void_p * 3),
                ("picture_number", C.c_uint64)]


class TfPictureJob(C.Structure):         # SvtHipTfPictureJob
    _fields_ = [("me", MeParams), ("ctrls", TfCtrls), ("decay_factor_fp16", C.c_uint32 * 3), ("mv_dist_th", C.c_uint16), ("chroma", C.c_uint8),
                ("bit_depth", C.c_uint8), ("mi_rows", C.c_uint32), ("mi_cols", C.c_uint32), ("n_refs", C.c_uint32), ("centre", TfPic),
                ("ref", TfPic * TF_MAX_REFS), ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64), ("tot_blks", C.c_void_p)]


class TfB64State(C.Structure):           # SvtHipTfB64State
    _fields_ = [("err64", C.c_uint64), ("err32", C.c_uint64 * 4), ("err16", C.c_uint64 * 16), ("mv64_x", C.c_int16), ("mv64_y", C.c_int16),
                ("mv32_x", C.c_int16 * 4), ("mv32_y", C.c_int16 * 4), ("mv16_x", C.c_int16 * 16), ("mv16_y", C.c_int16 * 16),
                ("split32", C.c_uint8 * 4), ("use_64x64", C.c_uint8), ("pad_", C.c_uint8 * 3), ("err8", C.c_uint64 * 64),
                ("mv8_x", C.c_int16 * 64), ("mv8_y", C.c_int16 * 64), ("split16", C.c_uint8 * 16)]


class TplStats(C.Structure):             # SvtHipTplStats (include/svt_hip_tpl.h)
    _fields_ = [("srcrf_dist", C.c_int64), ("recrf_dist", C.c_int64), ("srcrf_rate", C.c_int64), ("recrf_rate", C.c_int64),
                ("mc_dep_rate", C.c_int64), ("mc_dep_dist", C.c_int64), ("mv_row", C.c_int16), ("mv_col", C.c_int16), ("pad_", C.c_uint32),
                ("ref_frame_poc", C.c_uint64)]


class TplSrcStats(C.Structure):          # SvtHipTplSrcStats
    _fields_ = [("srcrf_dist", C.c_int64), ("srcrf_rate", C.c_int64), ("ref_frame_poc", C.c_uint64), ("mv_row", C.c_int16), ("mv_col", C.c_int16),
                ("best_rf_idx", C.c_int32), ("best_mode", C.c_uint8), ("best_intra_mode", C.c_uint8), ("pad_", C.c_uint8 * 6)]


class TplRef(C.Structure):               # SvtHipTplRef
    _fields_ = [("src", C.c_void_p), ("recon", C.c_void_p), ("src_stride", C.c_uint32), ("recon_stride", C.c_uint32), ("picture_number", C.c_uint64),
                ("max_width", C.c_uint16), ("max_height", C.c_uint16), ("usable", C.c_uint8), ("pad_", C.c_uint8 * 3)]


class TplFrameJob(C.Structure):          # SvtHipTplFrameJob
    _fields_ = [("src", Plane8), ("recon", Plane8), ("ref", (TplRef * 4) * 2), ("me_mv_array", C.c_void_p), ("me_candidate_array", C.c_void_p),
                ("total_me_candidate_index", C.c_void_p), ("max_cand", C.c_uint8), ("max_refs", C.c_uint8), ("max_l0", C.c_uint8),
                ("enable_me_16x16", C.c_uint8), ("stored_pus", C.c_uint8), ("pf_shape", C.c_uint8), ("disable_intra_pred", C.c_uint8),
                ("is_ref", C.c_uint8), ("i_slice", C.c_uint8), ("tpl_i_slice", C.c_uint8), ("src_data_ready", C.c_uint8),
                ("store_src_stats", C.c_uint8), ("synth_blk_size", C.c_uint8), ("blk_size", C.c_uint8), ("subsample_tx", C.c_uint8), ("publish_fence", C.c_uint8),
                ("round_fp", C.c_int16 * 2),
                ("quant_fp", C.c_int16 * 2), ("dequant", C.c_int16 * 2), ("quarter_pel", C.c_uint8), ("pad2_", C.c_uint8), ("stats", C.c_void_p), ("src_stats", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64)]


class Mv(C.Structure):                   # SvtHipMv == MV (block_structures.h:26-29)
    _fields_ = [("row", C.c_int16), ("col", C.c_int16)]


class MvCostParam(C.Structure):          # SvtHipMvCostParam == struct svt_mv_cost_param (mcomp.h:37-49)
    _fields_ = [("ref_mv", C.POINTER(Mv)), ("full_ref_mv", Mv), ("mv_cost_type", C.c_uint8), ("mvjcost", C.c_void_p),
                ("mvcost", C.c_void_p * 2), ("error_per_bit", C.c_int), ("early_exit_th", C.c_int), ("sad_per_bit", C.c_int)]


SUBPEL_TREE, SUBPEL_TREE_PRUNED = range(2)                                       # SVT_HIP_SUBPEL_* (include/svt_hip_inter.h)
SUBPEL_USE_2_TAPS, SUBPEL_USE_4_TAPS, SUBPEL_USE_8_TAPS = 1, 2, 3
(SUBPEL_EXIT_NONE, SUBPEL_EXIT_EARLY, SUBPEL_EXIT_VARIANCE, SUBPEL_EXIT_ABS_TH, SUBPEL_EXIT_NO_ROUND, SUBPEL_EXIT_ROUND_DEV,
 SUBPEL_EXIT_END) = range(7)
(SUBPEL_OK, SUBPEL_BAD_SIZE, SUBPEL_BAD_POINTER, SUBPEL_BAD_START_MV, SUBPEL_BAD_METHOD, SUBPEL_BAD_FILTER,
 SUBPEL_BAD_COST) = range(7)


class SubpelJob(C.Structure):            # SvtHipSubpelJob (include/svt_hip_inter.h)
    _fields_ = [("mvjcost", C.c_int32 * 4), ("mvcost", C.c_void_p * 2)]


class SubpelDesc(C.Structure):           # SvtHipSubpelDesc
    _fields_ = [("src", C.c_void_p), ("ref", C.c_void_p), ("src_stride", C.c_uint32), ("ref_stride", C.c_uint32), ("w", C.c_uint16),
                ("h", C.c_uint16), ("start_mv", Mv), ("ref_mv", Mv), ("best_mvp", Mv), ("col_min", C.c_int32), ("col_max", C.c_int32),
                ("row_min", C.c_int32), ("row_max", C.c_int32), ("iters_per_step", C.c_int32), ("pred_variance_th", C.c_int32),
                ("round_dev_th", C.c_int32), ("error_per_bit", C.c_int32), ("early_exit_th", C.c_int32), ("hp_mv_th", C.c_int32),
                ("best_mvp_dist", C.c_uint32), ("method", C.c_uint8), ("subpel_search_type", C.c_uint8), ("forced_stop", C.c_uint8),
                ("allow_hp", C.c_uint8), ("bias_fp", C.c_uint8), ("skip_diag_refinement", C.c_uint8), ("abs_th_mult", C.c_uint8),
                ("qp", C.c_uint8), ("mv_cost_type", C.c_uint8), ("early_exit", C.c_uint8), ("mvp_th", C.c_uint8), ("pad_", C.c_uint8)]


class SubpelResult(C.Structure):         # SvtHipSubpelResult
    _fields_ = [("best_mv", Mv), ("besterr", C.c_int32), ("distortion", C.c_int32), ("sse", C.c_uint32), ("fullpel_err", C.c_uint32),
                ("exit", C.c_uint8), ("status", C.c_uint8), ("pad_", C.c_uint8 * 2)]


SUBPEL_DESC_DTYPE = record_dtype(SubpelDesc)       # numpy views of arrays of them
SUBPEL_RESULT_DTYPE = record_dtype(SubpelResult)


IFS_COMBOS, IFS_FILTER_BANKS, IFS_CONTEXTS = 9, 5, 16                            # SVT_HIP_IFS_* (include/svt_hip_inter.h)
IFS_OK, IFS_BAD_SIZE, IFS_BAD_POINTER, IFS_BAD_PHASE, IFS_BAD_CTX, IFS_BAD_COMPOUND, IFS_BAD_WEIGHT = range(7)


def ifs_status(status):
    """SVT_HIP_IFS_STATUS: a SvtHipStatus as the size_t that svt_hip_ifs_search_batch returns"""
    return status & 0xFFFFFFFF


class IfsJob(C.Structure):               # SvtHipIfsJob
    _fields_ = [("d_switchable_rate", C.c_void_p), ("d_filters", C.c_void_p), ("full_lambda", C.c_uint32), ("quantizer", C.c_int16),
                ("bit_depth", C.c_uint8), ("enable_dual_filter", C.c_uint8), ("subsampled_distortion", C.c_uint8),
                ("skip_sse_rd_model", C.c_uint8), ("smooth_bias_pct", C.c_uint16), ("pad_", C.c_uint8 * 4)]


class IfsDesc(C.Structure):              # SvtHipIfsDesc
    _fields_ = [("src", C.c_void_p), ("ref0", C.c_void_p), ("ref1", C.c_void_p), ("dst", C.c_void_p), ("src_stride", C.c_uint32),
                ("ref0_stride", C.c_uint32), ("ref1_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("w", C.c_uint16), ("h", C.c_uint16),
                ("subpel_x0", C.c_uint8), ("subpel_y0", C.c_uint8), ("subpel_x1", C.c_uint8), ("subpel_y1", C.c_uint8),
                ("compound", C.c_uint8), ("fwd_offset", C.c_uint8), ("bck_offset", C.c_uint8), ("ctx", C.c_uint8 * 2), ("pad_", C.c_uint8 * 3)]


class IfsResult(C.Structure):            # SvtHipIfsResult
    _fields_ = [("rd", C.c_uint64), ("sse", C.c_uint64), ("interp_filters", C.c_uint32), ("switchable_rate", C.c_int32), ("best", C.c_uint8),
                ("status", C.c_uint8), ("pad_", C.c_uint8 * 6)]


class IfsTrace(C.Structure):             # SvtHipIfsTrace
    _fields_ = [("sse", C.c_uint64 * 9), ("rd", C.c_uint64 * 9)]


IFS_DESC_DTYPE = record_dtype(IfsDesc)
IFS_RESULT_DTYPE = record_dtype(IfsResult)
IFS_TRACE_DTYPE = record_dtype(IfsTrace)


FPEL_MVP, FPEL_SQ, FPEL_NSQ, FPEL_PME = range(4)                                 # SVT_HIP_FPEL_* (include/svt_hip_inter.h)
FPEL_SAD, FPEL_VAR, FPEL_SSD = range(3)
FPEL_MAX_MV, FPEL_MAX_MVP, FPEL_TILE, FPEL_MAX_EXTENT = 6, 4, 32, 4095
(FPEL_OK, FPEL_BAD_SIZE, FPEL_BAD_POINTER, FPEL_BAD_MODE, FPEL_BAD_DIST, FPEL_BAD_COST, FPEL_BAD_COUNT, FPEL_BAD_STEP,
 FPEL_BAD_WINDOW) = range(9)


def fpel_status(status):
    """SVT_HIP_FPEL_STATUS: a SvtHipStatus as the int16_t that svt_hip_fpel_search_batch returns"""
    return 0 if status == 0 else ((0x8000 | (status & 0x7FFF)) ^ 0x8000) - 0x8000


class FpelLevel(C.Structure):            # SvtHipFpelLevel
    _fields_ = [("start_x", C.c_int16), ("end_x", C.c_int16), ("start_y", C.c_int16), ("end_y", C.c_int16), ("enabled", C.c_uint8),
                ("step", C.c_uint8), ("pad_", C.c_uint8 * 2)]


class FpelDesc(C.Structure):             # SvtHipFpelDesc
    _fields_ = [("src", C.c_void_p), ("ref", C.c_void_p), ("src_stride", C.c_uint32), ("ref_stride", C.c_uint32), ("w", C.c_uint16),
                ("h", C.c_uint16), ("blk_org_x", C.c_uint16), ("blk_org_y", C.c_uint16), ("ref_org_x", C.c_uint16), ("ref_org_y", C.c_uint16),
                ("ref_max_width", C.c_uint16), ("ref_max_height", C.c_uint16), ("ref_mv", Mv), ("error_per_bit", C.c_int32),
                ("gate_th", C.c_uint32), ("mv", Mv * FPEL_MAX_MV), ("level", FpelLevel * 3), ("mode", C.c_uint8), ("dist_type", C.c_uint8),
                ("enable_psad", C.c_uint8), ("mv_cost_type", C.c_uint8), ("n_mv", C.c_uint8), ("gate_enabled", C.c_uint8),
                ("search_area_multiplier", C.c_uint8), ("nsq_search_width", C.c_uint8), ("nsq_search_height", C.c_uint8),
                ("pad_", C.c_uint8 * 7)]


class FpelResult(C.Structure):           # SvtHipFpelResult
    _fields_ = [("best_mv", Mv), ("best_cost", C.c_uint32), ("aux_cost", C.c_uint32), ("expanded", C.c_uint8), ("mvp_idx", C.c_uint8),
                ("status", C.c_uint8), ("pad_", C.c_uint8)]


class FpelSqCtrls(C.Structure):          # SvtHipFpelSqCtrls
    _fields_ = [("w", C.c_uint16 * 3), ("h", C.c_uint16 * 3), ("max_w", C.c_uint16 * 3), ("max_h", C.c_uint16 * 3),
                ("multiplier", C.c_int16 * 3), ("enabled", C.c_uint8 * 3), ("step", C.c_uint8 * 3)]


FPEL_DESC_DTYPE = record_dtype(FpelDesc)
FPEL_RESULT_DTYPE = record_dtype(FpelResult)


OBMC_MAX_NEIGHBOURS = 4                                                          # SVT_HIP_OBMC_* (include/svt_hip_inter.h)
(OBMC_OK, OBMC_BAD_SIZE, OBMC_BAD_POINTER, OBMC_BAD_SEGMENT, OBMC_BAD_RANGE, OBMC_BAD_START_MV, OBMC_BAD_LIMITS, OBMC_BAD_FILTER,
 OBMC_BAD_COST) = range(9)


class ObmcNeighbour(C.Structure):        # SvtHipObmcNeighbour
    _fields_ = [("rel_mi", C.c_uint8), ("mi_len", C.c_uint8)]


class ObmcTargetDesc(C.Structure):       # SvtHipObmcTargetDesc
    _fields_ = [("src", C.c_void_p), ("above", C.c_void_p), ("left", C.c_void_p), ("wsrc", C.c_void_p), ("mask", C.c_void_p),
                ("src_stride", C.c_uint32), ("above_stride", C.c_uint32), ("left_stride", C.c_uint32), ("w", C.c_uint16), ("h", C.c_uint16),
                ("up_available", C.c_uint8), ("left_available", C.c_uint8), ("n_above", C.c_uint8), ("n_left", C.c_uint8),
                ("above_nb", ObmcNeighbour * OBMC_MAX_NEIGHBOURS), ("left_nb", ObmcNeighbour * OBMC_MAX_NEIGHBOURS), ("pad_", C.c_uint32)]


class ObmcSearchDesc(C.Structure):       # SvtHipObmcSearchDesc
    _fields_ = [("wsrc", C.c_void_p), ("mask", C.c_void_p), ("ref", C.c_void_p), ("ref_stride", C.c_uint32), ("w", C.c_uint16),
                ("h", C.c_uint16), ("start_mv", Mv), ("ref_mv", Mv), ("raw_limits", C.c_int32 * 4), ("fp_limits", C.c_int32 * 4),
                ("sad_per_bit", C.c_int32), ("error_per_bit", C.c_int32), ("iters_per_step", C.c_int32), ("do_full_refine", C.c_uint8),
                ("do_frac_refine", C.c_uint8), ("fpel_search_range", C.c_uint8), ("fpel_search_diag", C.c_uint8),
                ("approx_inter_rate", C.c_uint8), ("allow_hp", C.c_uint8), ("subpel_search_type", C.c_uint8), ("forced_stop", C.c_uint8),
                ("pad_", C.c_uint32)]


class ObmcSearchResult(C.Structure):     # SvtHipObmcSearchResult
    _fields_ = [("best_mv", Mv), ("fullpel_mv", Mv), ("besterr", C.c_int32), ("distortion", C.c_int32), ("sse", C.c_uint32),
                ("rate_mv", C.c_int32), ("fullpel_rounds", C.c_uint8), ("status", C.c_uint8), ("pad_", C.c_uint8 * 2)]


OBMC_TARGET_DESC_DTYPE = record_dtype(ObmcTargetDesc)
OBMC_SEARCH_DESC_DTYPE = record_dtype(ObmcSearchDesc)
OBMC_SEARCH_RESULT_DTYPE = record_dtype(ObmcSearchResult)


class TxfmParam(C.Structure):            # SvtHipTxfmParam == TxfmParam (definitions.h:1051-1063)
    _fields_ = [("tx_type", C.c_uint8), ("tx_size", C.c_uint8), ("lossless", C.c_int32), ("bd", C.c_int32), ("is_hbd", C.c_int32),
                ("tx_set_type", C.c_uint8), ("eob", C.c_int32)]


# include/svt_hip_intra.h: PredictionMode DC_PRED .. PAETH_PRED, EB_TRANS_COEFF_SHAPE
INTRA_MODES = 13
DC_PRED, V_PRED, H_PRED, D45_PRED, D135_PRED, D113_PRED, D157_PRED, D203_PRED, D67_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, \
    PAETH_PRED = range(INTRA_MODES)
DEFAULT_SHAPE, N2_SHAPE, N4_SHAPE = 0, 1, 2


class IntraCtrls(C.Structure):           # SvtHipIntraCtrls
    _fields_ = [("intra_mode_end", C.c_uint8), ("use_sad", C.c_uint8), ("pf_shape", C.c_uint8), ("subsample_tx", C.c_uint8),
                ("max_input_luma_width", C.c_uint16), ("max_input_luma_height", C.c_uint16)]


class IntraSearchJob(C.Structure):       # SvtHipIntraSearchJob
    _fields_ = [("src", Plane8), ("ctrls", IntraCtrls), ("best_mode", C.c_void_p), ("best_cost", C.c_void_p),
                ("mode_cost", C.c_void_p), ("pred", C.c_void_p)]


FILTER_INTRA_NONE = 5                    # SVT_HIP_FILTER_INTRA_NONE (FILTER_INTRA_MODES)
II_DC_PRED, II_V_PRED, II_H_PRED, II_SMOOTH_PRED = range(4)   # InterIntraMode
CFL_BUF_LINE = 32                        # SVT_HIP_CFL_BUF_LINE


class IntraPredDesc(C.Structure):        # SvtHipIntraPredDesc
    _fields_ = [("above", C.c_void_p), ("left", C.c_void_p), ("dst", C.c_void_p), ("inter", C.c_void_p), ("left_stride", C.c_uint32),
                ("dst_stride", C.c_uint32), ("inter_stride", C.c_uint32), ("w", C.c_uint8), ("h", C.c_uint8), ("mode", C.c_uint8),
                ("angle_delta", C.c_int8), ("filter_intra_mode", C.c_uint8), ("disable_edge_filter", C.c_uint8), ("filt_type", C.c_uint8),
                ("ii_mode", C.c_uint8), ("n_top_px", C.c_uint8), ("n_topright_px", C.c_uint8), ("n_left_px", C.c_uint8),
                ("n_bottomleft_px", C.c_uint8), ("is_16bit", C.c_uint8), ("bit_depth", C.c_uint8), ("pad_", C.c_uint8 * 6)]


class CflDesc(C.Structure):              # SvtHipCflDesc
    _fields_ = [("luma", C.c_void_p), ("pred", C.c_void_p), ("dst", C.c_void_p), ("ac_out", C.c_void_p), ("luma_stride", C.c_uint32),
                ("pred_stride", C.c_uint32), ("dst_stride", C.c_uint32), ("alpha_q3", C.c_int8), ("w", C.c_uint8), ("h", C.c_uint8),
                ("is_16bit", C.c_uint8), ("bit_depth", C.c_uint8), ("pad_", C.c_uint8 * 7)]


# numpy views of arrays of SvtHipIntraPredDesc / SvtHipCflDesc (pointers as addresses)
INTRA_PRED_DESC_DTYPE, CFL_DESC_DTYPE = record_dtype(IntraPredDesc), record_dtype(CflDesc)

PALETTE_MAX_SIZE, PALETTE_MAX_CANDS, PALETTE_DOMINANT, PALETTE_KMEANS = 8, 14, 0, 1   # SVT_HIP_PALETTE_*


def palette_status(status):
    """SVT_HIP_PALETTE_STATUS: a SvtHipStatus as the uint64_t that svt_hip_palette_search_batch, svt_hip_palette_predict_batch and
    svt_hip_sc_classify return"""
    return status & 0xFFFFFFFF


class PaletteRates(C.Structure):         # SvtHipPaletteRates
    _fields_ = [("palette_ysize_fac_bits", C.c_int32 * 7 * 7), ("palette_ycolor_fac_bitss", C.c_int32 * 8 * 5 * 7)]


class PaletteCtrls(C.Structure):         # SvtHipPaletteCtrls
    _fields_ = [("d_rates", C.c_void_p), ("dominant_color_step", C.c_uint8), ("bit_depth", C.c_uint8), ("max_itr", C.c_uint8),
                ("pad_", C.c_uint8 * 5)]


class PaletteCand(C.Structure):          # SvtHipPaletteCand
    _fields_ = [("origin", C.c_uint8), ("n", C.c_uint8), ("palette_size", C.c_uint8), ("pad_", C.c_uint8),
                ("palette_colors", C.c_uint16 * PALETTE_MAX_SIZE), ("size_bits", C.c_int32), ("color_bits", C.c_int32), ("map_bits", C.c_int32)]


class PaletteRecord(C.Structure):        # SvtHipPaletteRecord
    _fields_ = [("colors", C.c_uint16), ("n_cands", C.c_uint8), ("n_cache", C.c_uint8), ("cache", C.c_uint16 * (2 * PALETTE_MAX_SIZE)),
                ("pad_", C.c_uint8 * 12), ("cand", PaletteCand * PALETTE_MAX_CANDS)]


class PaletteDesc(C.Structure):          # SvtHipPaletteDesc
    _fields_ = [("src", C.c_void_p), ("record", C.c_void_p), ("maps", C.c_void_p), ("stride", C.c_uint32), ("org_x", C.c_uint32),
                ("org_y", C.c_uint32), ("width", C.c_uint8), ("height", C.c_uint8), ("rows", C.c_uint8), ("cols", C.c_uint8),
                ("above_n", C.c_uint8), ("left_n", C.c_uint8), ("pad_", C.c_uint8 * 6), ("above", C.c_uint16 * PALETTE_MAX_SIZE),
                ("left", C.c_uint16 * PALETTE_MAX_SIZE)]


class PalettePredDesc(C.Structure):      # SvtHipPalettePredDesc
    _fields_ = [("map", C.c_void_p), ("colors", C.c_void_p), ("dst", C.c_void_p), ("dst_stride", C.c_uint32), ("map_width", C.c_uint16),
                ("x", C.c_uint8), ("y", C.c_uint8), ("w", C.c_uint8), ("h", C.c_uint8), ("is_16bit", C.c_uint8), ("bit_depth", C.c_uint8),
                ("pad_", C.c_uint8 * 4)]


class ScClass(C.Structure):              # SvtHipScClass
    _fields_ = [("counts_1", C.c_uint32), ("counts_2", C.c_uint32), ("blocks", C.c_uint32), ("sc_class", C.c_uint8 * 4), ("pad_", C.c_uint32 * 2)]


# numpy views of the device records and of an array of SvtHipPalettePredDesc
PALETTE_RECORD_DTYPE, PALETTE_PRED_DESC_DTYPE, SC_CLASS_DTYPE = record_dtype(PaletteRecord), record_dtype(PalettePredDesc), record_dtype(ScClass)
