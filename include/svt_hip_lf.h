/*
 * svt_hip_lf.h — C-ABI for the in-loop filters: CDEF, deblocking, self-guided restoration
 * (SURVEY.md §8 rows a9–a11).
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   Source/Lib/Codec/common_dsp_rtcd.c:796-804   svt_aom_cdef_find_dir, svt_aom_cdef_find_dir_dual,
 *                                                svt_cdef_filter_block, svt_aom_copy_rect8_8bit_to_16bit
 *   Source/Lib/Codec/aom_dsp_rtcd.c:207-208      svt_compute_cdef_dist_16bit, svt_compute_cdef_dist_8bit
 *   Source/Lib/Codec/cdef_process.c:106-349      cdef_seg_search            (Tier B: svt_hip_cdef_search_plane)
 *   Source/Lib/Codec/enc_cdef.c:284-610          svt_av1_cdef_frame         (Tier B: svt_hip_cdef_apply_plane)
 *   Source/Lib/Codec/enc_cdef.c:697-727, 728-926 joint_strength_search_dual, finish_cdef_search
 *                                                                           (Tier B: svt_hip_cdef_pick_strengths)
 *   Source/Lib/Codec/restoration_pick.c:1296-1431, 1555-1625  search_wiener_seg, search_wiener_finish, rest_finish_search
 *                                                                           (Tier B: svt_hip_wiener_pick_plane)
 *   Source/Lib/Codec/restoration_pick.c:1148-1293, 1380-1431, 1555-1625  search_sgrproj_seg, the finish visitors, rest_finish_search,
 *                                                                           copy_unit_info (Tier B: svt_hip_rest_pick_plane)
 *   Source/Lib/Codec/deblocking_filter.c:841-991, 1129-1252  try_filter_frame, search_filter_level, svt_av1_pick_filter_level
 *                                                                           (Tier B: svt_hip_dlf_pick_levels, svt_hip_dlf_apply_picked)
 */
#ifndef SVT_HIP_LF_H
#define SVT_HIP_LF_H

#include <stddef.h>

#include "svt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_CDEF_BSTRIDE 144      /* CDEF_BSTRIDE, cdef.h:35 */
#define SVT_HIP_CDEF_VERY_LARGE 0x7F7F /* CDEF_VERY_LARGE, cdef.h:38 */

typedef struct SvtHipCdefList { /* CdefList, definitions.h:255-259 */
    uint8_t by, bx;
} SvtHipCdefList;

/* ---------------------------------------------------------------------------------------------
 * Tier A (host pointers, RTCD signatures; BlockSize values: BLOCK_4X4=0, 4X8=1, 8X4=2, 8X8=3)
 * ------------------------------------------------------------------------------------------- */
SVT_HIP_API uint8_t svt_aom_cdef_find_dir_hip(const uint16_t *img, int32_t stride, int32_t *var, int32_t coeff_shift);
SVT_HIP_API void    svt_aom_cdef_find_dir_dual_hip(const uint16_t *img1, const uint16_t *img2, int stride, int32_t *var1,
                                                   int32_t *var2, int32_t coeff_shift, uint8_t *out1, uint8_t *out2);
SVT_HIP_API void    svt_cdef_filter_block_hip(uint8_t *dst8, uint16_t *dst16, int32_t dstride, const uint16_t *in,
                                              int32_t pri_strength, int32_t sec_strength, int32_t dir, int32_t pri_damping,
                                              int32_t sec_damping, int32_t bsize, int32_t coeff_shift,
                                              uint8_t subsampling_factor);
SVT_HIP_API void    svt_aom_copy_rect8_8bit_to_16bit_hip(uint16_t *dst, int32_t dstride, const uint8_t *src, int32_t sstride,
                                                         int32_t v, int32_t h);
SVT_HIP_API uint64_t svt_compute_cdef_dist_16bit_hip(const uint16_t *dst, int32_t dstride, const uint16_t *src,
                                                     const SvtHipCdefList *dlist, int32_t cdef_count, int32_t bsize,
                                                     int32_t coeff_shift, int32_t pli, uint8_t subsampling_factor);
SVT_HIP_API uint64_t svt_compute_cdef_dist_8bit_hip(const uint8_t *dst8, int32_t dstride, const uint8_t *src8,
                                                    const SvtHipCdefList *dlist, int32_t cdef_count, int32_t bsize,
                                                    int32_t coeff_shift, int32_t pli, uint8_t subsampling_factor);

/* svt_search_one_dual (aom_dsp_rtcd.h:239; enc_cdef.c:627-686): one greedy step of the joint luma / chroma strength
 * search over the per-filter-block tables mse[0][i][strength], mse[1][i][strength]. */
SVT_HIP_API uint64_t svt_search_one_dual_hip(int *lev0, int *lev1, int nb_strengths, uint64_t **mse[2], int sb_count,
                                             int start_gi, int end_gi);

/* ---------------------------------------------------------------------------------------------
 * Tier B — one picture plane per call, device pointers.
 *   recon / source : top-left sample of the picture area (no padding needed; samples outside the
 *                    8-aligned picture are CDEF_VERY_LARGE as in the reference)
 *   filt8x8        : uint8 [ceil(h8)][ceil(w8)] in units of 8x8 LUMA blocks, non-zero = block is filtered
 *                    (what svt_sb_compute_cdef_list derives from the skip flags, enc_cdef.c:238-276)
 * ------------------------------------------------------------------------------------------- */
typedef struct SvtHipCdefPlane {
    void    *recon;       /* uint8 or uint16 samples */
    void    *source;      /* search: the original picture; apply: the OUTPUT plane (must not alias recon) */
    uint32_t recon_stride, source_stride; /* in samples */
    uint32_t width, height;               /* plane size in samples (luma: 8-aligned picture size; chroma: half) */
    uint8_t  is_16bit, xdec, ydec, pli;   /* pli: 0 luma, 1/2 chroma; xdec == ydec (4:2:0 or 4:4:4) — the reference
                                           * encoder accepts 4:2:0 only (enc_settings.c:447); others: BAD_PARAMETER */
} SvtHipCdefPlane;

#define SVT_HIP_CDEF_MAX_STRENGTHS 64
typedef struct SvtHipCdefSearchParams {
    int32_t n_strengths;
    int8_t  strengths[SVT_HIP_CDEF_MAX_STRENGTHS]; /* pri*4+sec as in default_first/second_pass_fs; -1 = not tested */
    int32_t pri_damping, sec_damping;              /* 3 + (base_q_idx >> 6), cdef_process.c:139-140 */
    int32_t coeff_shift;                           /* bit_depth - 8 */
    int32_t subsampling_factor;                    /* cdef_ctrls->subsampling_factor (capped per block size inside) */
} SvtHipCdefSearchParams;

/* mse[fb][gi] (uint64, fb raster over 64x64 filter blocks) = curr_mse * subsampling_factor of
 * cdef_process.c:283-286 for this plane; dir / var: [fb][8][8] luma direction / variance (uint8 / int32),
 * written when pli == 0 and read when pli != 0 (run the luma plane first). */
SVT_HIP_API int32_t svt_hip_cdef_search_plane(const SvtHipCdefPlane *plane, const uint8_t *d_filt8x8,
                                              const SvtHipCdefSearchParams *prm, uint64_t *d_mse, uint8_t *d_dir,
                                              int32_t *d_var, void *stream);

/* Apply: strength per filter block (uint8 [n_fb], pri*4+sec with sec already in {0,1,2,3}->{0,1,2,4} mapping
 * applied inside); blocks that are not filtered are copied through. */
SVT_HIP_API int32_t svt_hip_cdef_apply_plane(const SvtHipCdefPlane *plane, const uint8_t *d_filt8x8,
                                             const uint8_t *d_fb_strength, int32_t damping, int32_t coeff_shift,
                                             const uint8_t *d_dir, const int32_t *d_var, void *stream);

/* The same for up to three planes of one picture in ONE launch (svt_av1_cdef_frame, enc_cdef.c:284-610, walks the planes
 * of a filter block together): planes[p] / fb_strength_dptrs[p] per plane (luma strength index for plane 0, chroma for 1, 2);
 * all planes must cover the same 64x64 (luma) filter-block grid.  `planes` and `fb_strength_dptrs` are HOST arrays of
 * n_planes entries (the latter holds DEVICE pointers, one strength array per plane); everything else is device memory. */
SVT_HIP_API int32_t svt_hip_cdef_apply_frame(const SvtHipCdefPlane *planes, uint32_t n_planes, const uint8_t *d_filt8x8,
                                             const uint8_t *const *fb_strength_dptrs, int32_t damping, int32_t coeff_shift,
                                             const uint8_t *d_dir, const int32_t *d_var, void *stream);

/* finish_cdef_search (enc_cdef.c:728-926) between the two: the picture's strength decision taken on the device from the
 * tables svt_hip_cdef_search_plane wrote, for use_reference_cdef_fs == 0 and 64x64 superblocks.  Not covered (the caller
 * keeps such pictures on the host): use_reference_cdef_fs (:744-795) and 128x128 superblocks, whose odd filter blocks
 * are left out of the search (:824-827).
 *   takes part   a filter block with at least one non-zero 8x8 in its filt8x8 tile (!skip_cdef_seg)
 *   costs        luma = plane 0; chroma = U + V, or 1040400 * 64 where strengths_uv[gi] == -1 (cdef_process.c:251);
 *                zero_fs_cost_bias scales entry 0 of both (:845-851)
 *   search       joint_strength_search_dual (:697-727) per signalling width i = 0..3, start_gi = 0, end_gi = n_strengths;
 *                ties between (luma, chroma) pairs go to the first in luma-major order as in svt_search_one_dual
 *   choice       RDCOST(lambda, (sb_count * i + (1 << i) * 6 * 2) << 9, joint_mse * 16), first strictly smaller wins;
 *                every block then takes the first gi with the strictly smallest cost0[y_index[gi]] + cost1[uv_index[gi]]
 * All arithmetic is the reference's, modulo 2^64; with no block taking part the same arithmetic gives width 0, index 0. */
typedef struct SvtHipCdefPickParams {
    int32_t  n_strengths;      /* first_pass_fs_num + default_second_pass_fs_num = end_gi of the reference, 1..64 */
    uint32_t fb_cols, fb_rows; /* 64x64 filter-block grid */
    uint32_t w8, h8;           /* dimensions of filt8x8 (row stride w8); must reach into every filter block */
    uint16_t zero_fs_cost_bias;/* 0 = off; else cost[.][fb][0] = (bias * cost) >> 6 for both tables */
    uint16_t pad_;
    uint64_t lambda;           /* full_lambda of the picture (svt_aom_av1_lambda_assignment_function_table, :808-815) */
    int8_t   strengths[SVT_HIP_CDEF_MAX_STRENGTHS];    /* luma list given to the search (pri*4+sec), 0..63: the reference's
                                                        * filter_map (:911-919), used for BOTH planes' output */
    int8_t   strengths_uv[SVT_HIP_CDEF_MAX_STRENGTHS]; /* chroma list given to the search; -1 = not tested */
} SvtHipCdefPickParams;

typedef struct SvtHipCdefPickResult { /* ONE record in device memory */
    int32_t  cdef_bits, nb_strengths, sb_count, pad_;
    int32_t  y_index[8], uv_index[8];       /* winner: indices into the searched list (before filter_map); unused slots 0 */
    uint8_t  y_strength[8], uv_strength[8]; /* winner after filter_map = frm_hdr->cdef_params.cdef_y/uv_strength */
    uint64_t best_cost;                     /* RDCOST of the winner */
    uint64_t joint_mse[4], rd_cost[4];      /* per signalling width: joint_strength_search_dual's return, and its RDCOST */
    int32_t  lev0[4][8], lev1[4][8];        /* per width: the final best_lev0 / best_lev1 (entries >= 1 << i are 0) */
} SvtHipCdefPickResult;

/* Bytes of d_workspace for a grid of n_fb filter blocks: layout arithmetic, no device; 0 for an empty grid or list. */
SVT_HIP_API uint64_t svt_hip_cdef_pick_workspace_bytes(uint32_t n_fb, int32_t n_strengths);
/* prm is read on the host; everything else is device memory, n_fb = fb_cols * fb_rows:
 *   d_mse          uint64 [3][n_fb][n_strengths], the three planes as svt_hip_cdef_search_plane wrote them; not modified
 *   d_fb_gi        uint8 [n_fb]: mbmi.cdef_strength of each filter block, 0xFF where the block takes no part
 *   d_fb_strength  uint8 [2][n_fb]: luma, then chroma strength value per block, what svt_hip_cdef_apply_frame takes;
 *                  0 where the block takes no part
 * The call enqueues its launches on `stream` and returns; it neither synchronises nor reads anything back. */
SVT_HIP_API int32_t svt_hip_cdef_pick_strengths(const SvtHipCdefPickParams *prm, const uint64_t *d_mse, const uint8_t *d_filt8x8,
                                                SvtHipCdefPickResult *d_result, uint8_t *d_fb_gi, uint8_t *d_fb_strength,
                                                void *d_workspace, uint64_t workspace_bytes, void *stream);

/* =============================================================================================
 * Deblocking
 *   Source/Lib/Codec/common_dsp_rtcd.h:1043-1074  svt_aom_lpf_{horizontal,vertical}_{4,6,8,14} and the highbd set
 *   Source/Lib/Codec/deblocking_filter.c:162-282  set_lpf_parameters
 *   Source/Lib/Codec/deblocking_filter.c:287-653  svt_av1_filter_block_plane_vert/horz, svt_aom_loop_filter_sb,
 *                                                 svt_av1_loop_filter_frame   (Tier B: svt_hip_loop_filter_frame)
 *   Source/Lib/Codec/deblocking_common.c:582-600  svt_aom_update_sharpness (lim / mblim; hev_thr = level >> 4,
 *                                                 deblocking_filter.c:47)
 * ============================================================================================= */

/* Tier A: RTCD signatures, host pointers.  `s` points at the first q0 sample of a 4-sample edge segment;
 * the call reads/writes up to 7 samples on either side of the edge (what the reference touches). */
#define SVT_HIP_DECL_LPF(dir, n)                                                                                              \
    SVT_HIP_API void svt_aom_lpf_##dir##_##n##_hip(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,    \
                                                   const uint8_t *thresh);                                                    \
    SVT_HIP_API void svt_aom_highbd_lpf_##dir##_##n##_hip(uint16_t *s, int32_t pitch, const uint8_t *blimit,                  \
                                                          const uint8_t *limit, const uint8_t *thresh, int32_t bd);
SVT_HIP_DECL_LPF(horizontal, 4)
SVT_HIP_DECL_LPF(horizontal, 6)
SVT_HIP_DECL_LPF(horizontal, 8)
SVT_HIP_DECL_LPF(horizontal, 14)
SVT_HIP_DECL_LPF(vertical, 4)
SVT_HIP_DECL_LPF(vertical, 6)
SVT_HIP_DECL_LPF(vertical, 8)
SVT_HIP_DECL_LPF(vertical, 14)
#undef SVT_HIP_DECL_LPF

/* One record per 4x4 luma mode-info unit: the fields set_lpf_parameters reads through pcs->mi_grid_base,
 * gathered into a flat array (INTEGRATION.md shows the gather loop).  Enum values are the reference's
 * BlockSize / TxSize (definitions.h). */
typedef struct SvtHipLfMi {
    uint8_t bsize;      /* mbmi->block_mi.bsize */
    uint8_t tx_size_y;  /* tx_depth_to_tx_size[skip_inter ? 0 : tx_depth][bsize]   (get_transform_size, :145-150) */
    uint8_t tx_size_uv; /* av1_get_max_uv_txsize(bsize, 1, 1) */
    uint8_t skip_inter; /* block_mi.skip && is_inter_block_no_intrabc(ref_frame[0]) */
    uint8_t segment_id; /* block_mi.segment_id */
    uint8_t ref_frame0; /* block_mi.ref_frame[0] (INTRA_FRAME = 0) */
    uint8_t mode_lf;    /* mode_lf_lut[block_mi.mode] (deblocking_common.h:33-37) */
    uint8_t reserved;
} SvtHipLfMi;

typedef struct SvtHipLfFrame {
    void             *plane[3];  /* device; top-left picture sample of Y, Cb, Cr (4:2:0).  Filtered IN PLACE.  The buffer
                                  * must be padded like the reference's recon pictures: whole 4x4 units are filtered and
                                  * taps reach 7 samples past an edge, also below / right of the picture. */
    uint32_t          stride[3]; /* in samples */
    uint32_t          width, height; /* unpadded luma size (plane_ptr->dst.width/height, :90-96); chroma is >> 1 */
    const SvtHipLfMi *mi;        /* device; [mi_rows][mi_stride] */
    uint32_t          mi_stride, mi_rows, mi_cols; /* mi_cols = aligned_width >> 2, mi_rows = aligned_height >> 2 */
    uint8_t           lvl[3][8][2][8][2]; /* LoopFilterInfoN.lvl after svt_av1_loop_filter_frame_init */
    uint8_t           filter_level[2], filter_level_u, filter_level_v; /* frm_hdr.loop_filter_params: plane on/off */
    uint8_t           sharpness_level;
    uint8_t           bit_depth; /* static_config.encoder_bit_depth: 8 / 10 */
    uint8_t           is_16bit;  /* samples are uint16 (is_16bit_pipeline or bit_depth > 8) */
    uint8_t           plane_start, plane_end; /* as svt_av1_loop_filter_frame(.., plane_start, plane_end) */
    uint8_t           reserved[3];
} SvtHipLfFrame;

/* Whole-frame deblocking: all vertical edges, then all horizontal edges, per plane (the order
 * svt_aom_loop_filter_sb's combine_vert_horz_lf schedule is equivalent to).  delta_lf is not supported —
 * the reference never enables it (resource_coordination_process.c:410-412). */
SVT_HIP_API int32_t svt_hip_loop_filter_frame(const SvtHipLfFrame *frame, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The deblocking levels of a picture, searched on the device: svt_av1_pick_filter_level (deblocking_filter.c:1129) for the
 * searched methods (LPF_PICK_FROM_FULL_IMAGE; the reference ignores partial_frame) = search_filter_level (:886-991) once per
 * plane, every trial of it try_filter_frame (:841-881) = svt_av1_loop_filter_frame of that plane at the trial level, the SSE
 * against the source (picture_sse_calculations, :716-834), and the unfiltered plane put back.
 *   svt_hip_dlf_pick_levels   the whole search of up to three planes; the levels and the measured errors stay in a device record
 *   svt_hip_dlf_apply_picked  svt_av1_loop_filter_frame with the levels read from that record
 * Both only enqueue on `stream` and return the 32 bits of an SvtHipStatus as uint32_t: 0 = SVT_HIP_OK, else (uint32_t)SVT_HIP_ERR_*,
 * the value EbErrorType has.  Neither synchronises nor reads anything back, and the host never learns a level.
 *
 * The chain is fixed: max_rounds times {plan, trial}, then one plan step.  The plan step (one wave; a lane per plane) takes the
 * sums of the trials before it, advances each plane's loop through every iteration that needs no new error and stops at the
 * first one that does: its filt_low and filt_high are both known before either is tried (:943-970), so a round carries up to two
 * trials per plane, six in all; the first round is the trial at filt_mid.  The trial kernel filters one tile of one trial in LDS
 * (all vertical edges, then all horizontal ones) and adds the tile's squared error to the trial's sum; the filtered samples are
 * never written to memory.  A plane whose search has ended makes its trials inactive, and the workgroups of an inactive trial
 * return at once.  Every round that runs measures at least one new level, so 63 rounds always finish; a plane that runs out of
 * rounds gets its `finished` bit clear and the caller falls back (to the host loop, or to the record's best level so far).
 *
 * Not covered: mode_ref_delta_enabled (the reference never sets it, resource_coordination_process.c:367), delta_lf, several
 * tiles, superres / resize pictures (their scaling itself is svt_hip_scale.h: svt_hip_resize_planes, svt_hip_superres_upscale_planes),
 * formats other than 4:2:0, the LPF_PICK_FROM_Q family (scalar host work).
 * ------------------------------------------------------------------------------------------------------------------- */
#define SVT_HIP_DLF_MAX_LEVEL 63            /* MAX_LOOP_FILTER */
/* Recommended max_rounds: the largest `rounds` of tests/golden/dlf_pick.npz (12), plus 4.  A search CAN need more (a replay of the loop
 * over synthetic error tables needed up to 20): after every call check that `finished` has the bit of every searched plane, and fall
 * back where it has not, or ask for up to 63 rounds, which always finish. */
#define SVT_HIP_DLF_PICK_DEFAULT_ROUNDS 16

typedef struct SvtHipDlfPickParams { /* read on the host */
    SvtHipLfFrame frame;         /* plane[]: the UNFILTERED reconstruction (pick: read only; apply: filtered in place); mi, geometry,
                                  * sharpness_level, bit_depth, is_16bit, plane_start / plane_end as in svt_hip_loop_filter_frame;
                                  * lvl[] is ignored; filter_level[2] / _u / _v: the levels of planes that are not searched */
    const void   *src[3];        /* device: top-left sample of the source picture's planes (sample type of the reconstruction) */
    uint32_t      src_stride[3]; /* in samples */
    uint32_t      sse_width[3], sse_height[3]; /* measured area per plane, not empty, at most the mi-aligned plane ((mi_cols * 4) >> ss): the
                                  * reference measures aligned_width x aligned_height in the 8-bit pipeline and input_pic->width x
                                  * height ((w + ss) >> ss for chroma) in the 16-bit one */
    uint32_t      plane_mask;    /* bit p: plane p is searched (the reference skips chroma under dlf_avg_uv && temporal layer > 0) */
    uint8_t       start_level[3];/* where each plane's search starts (`lvl`, :901-912), 0..63.  Luma is searched with dir == 2, so
                                  * without dlf_avg the reference starts it from last_frame_filter_level[2], the previous U level */
    uint8_t       only_4x4;      /* tx_mode == ONLY_4X4: the bias is not halved (:940) */
    int32_t       early_exit_convergence; /* dlf_ctrls.early_exit_convergence; 0 = never */
    int32_t       max_rounds;    /* 1..63 rounds of {plan, trial} to enqueue; SVT_HIP_DLF_PICK_DEFAULT_ROUNDS */
    uint8_t       segmentation_enabled;
    uint8_t       seg_lf_enabled[8][4]; /* [segment][SEG_LVL_ALT_LF_Y_V, _Y_H, _U, _V]: a segment's level is clamp(level + data, 0, 63) */
    uint8_t       pad_[3];
    int16_t       seg_lf_data[8][4];    /* where the feature is active (deblocking_common.c:107-115) */
} SvtHipDlfPickParams;

#define SVT_HIP_DLF_PICK_RESULT_BYTES 1608
typedef struct SvtHipDlfPickResult { /* ONE record in device memory, no implicit padding; a plane that is not searched keeps level 0,
                                      * rounds 0, trials 0, best_err 0, ss_err -1 and a clear `finished` bit */
    int32_t  level[3];      /*    0: filt_best; of a plane that ran out of rounds, the best of what was measured */
    uint32_t finished;      /*   12: bit p: the search of plane p ran to its end */
    int32_t  rounds[3];     /*   16: rounds in which the plane measured something */
    int32_t  trials[3];     /*   28: try_filter_frame calls = measured entries of ss_err */
    uint8_t  hdr_level[4];  /*   40: loop_filter_params.filter_level[0], [1] (both level[0], :1211), filter_level_u, _v: searched planes
                             *       from level[], the others from frame.filter_level*: the 4 bytes the frame header needs */
    int32_t  pad_;          /*   44: zero */
    int64_t  best_err[3];   /*   48: ss_err[filt_best] (:986) */
    int64_t  ss_err[3][64]; /*   72: the reference's ss_err array (:920-923): -1 where the level was never tried */
} SvtHipDlfPickResult;

/* Bytes of d_workspace for a picture of width x height luma samples: layout arithmetic, no device; 0 for an empty picture.  The
 * workspace holds the state of the three loops and the six trial sums; nothing in it depends on the picture's size today. */
SVT_HIP_API uint64_t svt_hip_dlf_pick_workspace_bytes(uint32_t width, uint32_t height, int32_t is_16bit);
/* Reads frame.plane[] and src[] of the searched planes and the mode info; writes d_result and d_workspace, nothing else.  Of the
 * planes it reads nothing left of column 0 or above row 0 and nothing more than 8 samples past the mi-aligned size.  A trial at
 * level 0 is the unfiltered plane's error whatever the segment features say (the reference leaves the frame call before it
 * builds the table).  Refused with SVT_HIP_ERR_BAD_PARAMETER and a message, before the library asks for a device:
 *   - a NULL prm, d_result or d_workspace; either of the last two not 8-byte aligned;
 *   - everything svt_hip_loop_filter_frame refuses of `frame`; a searched plane without plane, stride, src or src_stride;
 *   - a start_level of a searched plane or a frame.filter_level* above 63; plane_mask 0 or above 7; max_rounds outside 1..63;
 *   - an empty measured area of a searched plane, or one larger than the mi-aligned plane; workspace_bytes below svt_hip_dlf_pick_workspace_bytes(). */
SVT_HIP_API uint32_t svt_hip_dlf_pick_levels(const SvtHipDlfPickParams *prm, SvtHipDlfPickResult *d_result, void *d_workspace,
                                             uint64_t workspace_bytes, void *stream);
/* Filters frame.plane[plane_start .. plane_end) in place as svt_hip_loop_filter_frame does, with the level table of
 * svt_av1_loop_filter_frame_init (deblocking_common.c:76-138) derived on the device: a searched plane (plane_mask) takes
 * d_result->level[], luma in both directions; any other plane takes frame.filter_level[2] / _u / _v.  Luma levels 0 and 0 with
 * plane_start == 0 filter nothing at all, a chroma level of 0 skips that plane (:99-105, deblocking_filter.c:570-572).  src, the
 * measured areas, the start levels and max_rounds are not read.  Refused like svt_hip_dlf_pick_levels: a NULL prm or d_result,
 * a d_result not 8-byte aligned, what the frame call refuses, a frame.filter_level* above 63, plane_mask 0 or above 7. */
SVT_HIP_API uint32_t svt_hip_dlf_apply_picked(const SvtHipDlfPickParams *prm, const SvtHipDlfPickResult *d_result, void *stream);

/* =============================================================================================
 * Self-guided restoration
 *   Source/Lib/Codec/common_dsp_rtcd.h:181,185   svt_apply_selfguided_restoration, svt_av1_selfguided_restoration
 *   Source/Lib/Codec/aom_dsp_rtcd.h:79,81,212    svt_av1_{lowbd,highbd}_pixel_proj_error, svt_get_proj_subspace
 *   Source/Lib/Codec/restoration_pick.c:523-652  apply_sgr, search_selfguided_restoration (Tier B: svt_hip_sgr_*)
 * ============================================================================================= */
typedef struct SvtHipSgrParams { /* SgrParamsType, definitions.h:1758-1761 */
    int32_t r[2], s[2];
} SvtHipSgrParams;

/* Tier A: RTCD signatures.  For highbd != 0 the uint8_t pointers carry the reference's CONVERT_TO_BYTEPTR encoding
 * (address >> 1 of a uint16 buffer, definitions.h:953-954), exactly as the callers pass them. */
SVT_HIP_API void    svt_av1_selfguided_restoration_hip(const uint8_t *dgd8, int32_t width, int32_t height, int32_t dgd_stride,
                                                       int32_t *flt0, int32_t *flt1, int32_t flt_stride, int32_t sgr_params_idx,
                                                       int32_t bit_depth, int32_t highbd);
SVT_HIP_API void    svt_apply_selfguided_restoration_hip(const uint8_t *dat, int32_t width, int32_t height, int32_t stride, int32_t eps,
                                                         const int32_t *xqd, uint8_t *dst, int32_t dst_stride, int32_t *tmpbuf,
                                                         int32_t bit_depth, int32_t highbd);
SVT_HIP_API int64_t svt_av1_lowbd_pixel_proj_error_hip(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride,
                                                       const uint8_t *dat8, int32_t dat_stride, int32_t *flt0, int32_t flt0_stride,
                                                       int32_t *flt1, int32_t flt1_stride, int32_t xq[2],
                                                       const SvtHipSgrParams *params);
SVT_HIP_API int64_t svt_av1_highbd_pixel_proj_error_hip(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride,
                                                        const uint8_t *dat8, int32_t dat_stride, int32_t *flt0, int32_t flt0_stride,
                                                        int32_t *flt1, int32_t flt1_stride, int32_t xq[2],
                                                        const SvtHipSgrParams *params);
SVT_HIP_API void    svt_get_proj_subspace_hip(const uint8_t *src8, int width, int height, int src_stride, const uint8_t *dat8,
                                              int dat_stride, int use_highbitdepth, int32_t *flt0, int flt0_stride, int32_t *flt1,
                                              int flt1_stride, int *xq, const SvtHipSgrParams *params);

/* Tier B: one restoration unit (<= 384 x 384 samples for the search; filter / apply take any region up to a whole
 * plane whose origin lies on the processing-unit grid), device pointers.  `dat` = the degraded picture (after
 * deblocking + CDEF) at the unit's top-left sample, readable 3 samples beyond the unit on every side (the extended
 * frame the reference searches on); `src` = the original. */
typedef struct SvtHipSgrUnit {
    const void *dat, *src;
    uint32_t    dat_stride, src_stride; /* in samples */
    uint32_t    width, height;
    uint8_t     is_16bit, bit_depth;
    uint8_t     pu_w, pu_h; /* processing-unit size: 64 (luma) or 32 (4:2:0 chroma), restoration_pick.c:561-562 */
} SvtHipSgrUnit;

/* apply_sgr (restoration_pick.c:523-548): flt0 / flt1 = int32 [height][flt_stride] */
SVT_HIP_API int32_t svt_hip_sgr_filter_unit(const SvtHipSgrUnit *unit, int32_t ep, int32_t *d_flt0, int32_t *d_flt1,
                                            uint32_t flt_stride, void *stream);
/* svt_apply_selfguided_restoration over the unit, filter and projection fused (no flt arrays); d_dst has the
 * sample type of `dat`.  Stripe-boundary handling of the final loop-restoration pass stays with the caller. */
SVT_HIP_API int32_t svt_hip_sgr_apply_unit(const SvtHipSgrUnit *unit, int32_t ep, const int32_t xqd[2], void *d_dst,
                                           uint32_t dst_stride, void *stream);
/* search_selfguided_restoration (restoration_pick.c:550-652) for ep = start_ep, start_ep + ep_inc, ... < end_ep:
 * filter, projection (get_proj_subspace + encode_xq) and the finer search all run on the device; the call returns
 * after reading back out = {ep, xqd[0], xqd[1]} and the winning error.  d_work: svt_hip_sgr_search_work_bytes(). */
SVT_HIP_API size_t  svt_hip_sgr_search_work_bytes(uint32_t width, uint32_t height, int32_t n_ep);
SVT_HIP_API int32_t svt_hip_sgr_search_unit(const SvtHipSgrUnit *unit, int32_t start_ep, int32_t end_ep, int32_t ep_inc,
                                            int32_t do_refine, void *d_work, int32_t out[3], int64_t *best_err, void *stream);

/* =============================================================================================
 * Wiener restoration (what runs at presets M4-M8)
 *   Source/Lib/Codec/aom_dsp_rtcd.h:66,68        svt_av1_compute_stats, svt_av1_compute_stats_highbd
 *   Source/Lib/Codec/common_dsp_rtcd.h:177,179   svt_av1_wiener_convolve_add_src, svt_av1_highbd_wiener_convolve_add_src
 *   callers: search_wiener (restoration_pick.c:1296-1430), wiener_filter_stripe (restoration.c:432-458)
 * ============================================================================================= */
typedef struct SvtHipConvolveParams { /* ConvolveParams, definitions.h:580-593 (only round_0 / round_1 are read) */
    int32_t ref, do_average;
    void   *dst;
    int32_t dst_stride, round_0, round_1, plane, is_compound, use_jnt_comp_avg, fwd_offset, bck_offset, use_dist_wtd_comp_avg;
} SvtHipConvolveParams;

/* Tier A: RTCD signatures (highbd: CONVERT_TO_BYTEPTR-encoded pointers; bit_depth = EbBitDepth value 8 / 10 / 12). */
SVT_HIP_API void svt_av1_compute_stats_hip(int32_t wiener_win, const uint8_t *dgd8, const uint8_t *src8, int32_t h_start, int32_t h_end,
                                           int32_t v_start, int32_t v_end, int32_t dgd_stride, int32_t src_stride, int64_t *M, int64_t *H);
SVT_HIP_API void svt_av1_compute_stats_highbd_hip(int32_t wiener_win, const uint8_t *dgd8, const uint8_t *src8, int32_t h_start,
                                                  int32_t h_end, int32_t v_start, int32_t v_end, int32_t dgd_stride, int32_t src_stride,
                                                  int64_t *M, int64_t *H, int32_t bit_depth);
SVT_HIP_API void svt_av1_wiener_convolve_add_src_hip(const uint8_t *src, ptrdiff_t src_stride, uint8_t *dst, ptrdiff_t dst_stride,
                                                     const int16_t *filter_x, const int16_t *filter_y, int32_t w, int32_t h,
                                                     const SvtHipConvolveParams *conv_params);
SVT_HIP_API void svt_av1_highbd_wiener_convolve_add_src_hip(const uint8_t *src, ptrdiff_t src_stride, uint8_t *dst,
                                                            ptrdiff_t dst_stride, const int16_t *filter_x, const int16_t *filter_y,
                                                            int32_t w, int32_t h, const SvtHipConvolveParams *conv_params, int32_t bd);

/* Tier B: statistics of many restoration units in one launch chain.  dgd / src point at sample (0,0) of the planes the
 * limits refer to (device memory; dgd readable wiener_win/2 samples beyond every limit); M = int64 [n][49],
 * H = int64 [n][49*49] (device), laid out as the reference's (only the first win^2 rows / columns are used). */
typedef struct SvtHipWienerUnit {
    const void *dgd, *src;
    uint32_t    dgd_stride, src_stride; /* in samples */
    int32_t     h_start, h_end, v_start, v_end; /* RestorationTileLimits */
} SvtHipWienerUnit;
SVT_HIP_API int32_t svt_hip_wiener_stats(const SvtHipWienerUnit *units /* host */, uint32_t n_units, int32_t wiener_win, int32_t is_16bit,
                                         int32_t bit_depth, int64_t *d_M, int64_t *d_H, void *stream);
/* The separable filter over a w x h region (any size; the reference's callers tile it in <= 64 x 64 processing units,
 * which gives the same samples).  Output must not alias the input. */
SVT_HIP_API int32_t svt_hip_wiener_convolve(const void *d_src, uint32_t src_stride, void *d_dst, uint32_t dst_stride, uint32_t w,
                                            uint32_t h, const int16_t filter_x[8], const int16_t filter_y[8], int32_t is_16bit,
                                            int32_t bit_depth, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Frame-level loop restoration: svt_av1_loop_restoration_filter_frame (restoration.c:1179-1248) = for every restoration
 * unit svt_av1_loop_restoration_filter_unit (:1067-1147) = for every 64-row processing stripe of the unit
 * {svt_aom_setup_processing_stripe_boundary (:288-384) -> stripe filter (Wiener :437-466, :1017-1038 or self-guided
 * :994-1015, :1040-1062) -> svt_aom_restore_processing_stripe_boundary (:386-435)}.
 *
 * The reference patches the three rows above / below a stripe INTO the picture, filters, and patches them back.  On the
 * device the same rows are selected while the stripe's tile is assembled in LDS (nothing is ever written into the source
 * plane), one workgroup per (64 >> ss_x)-wide processing unit of a stripe, all planes in one launch:
 *   rows above the first stripe / below the last stripe / left and right of the picture: edge replication (svt_extend_frame);
 *   other stripes, optimized_lr == 0: two saved DEBLOCKED rows from stripe_boundary_above / _below, used 0,0,1 / 0,1,1
 *                                     (svt_av1_loop_restoration_save_boundary_lines wrote them; row 2*stripe + k, element j is
 *                                     picture column j - SVT_HIP_LR_EXTRA_HORZ);
 *   optimized_lr == 1: the picture's own rows, the outermost of the three duplicated from its neighbour.
 * src and dst must be different planes; RESTORE_NONE units are copied. */
#define SVT_HIP_LR_EXTRA_HORZ 4 /* RESTORATION_EXTRA_HORZ (restoration.h) */
typedef struct SvtHipLrUnit {   /* RestorationUnitInfo (restoration.h:176-181) */
    uint8_t restoration_type;   /* 0 RESTORE_NONE, 1 RESTORE_WIENER, 2 RESTORE_SGRPROJ */
    uint8_t ep;                 /* sgrproj_info.ep */
    int16_t pad_;
    int32_t xqd[2];             /* sgrproj_info.xqd */
    int16_t hfilter[8], vfilter[8]; /* wiener_info (InterpKernel: 7 taps + 0, centre tap stored minus 128) */
} SvtHipLrUnit;
typedef struct SvtHipLrPlane {
    const void *src;            /* device: CDEF output, pointer to sample (0, 0) */
    void       *dst;            /* device: restored plane, sample (0, 0) */
    uint32_t    src_stride, dst_stride; /* samples */
    uint32_t    width, height;  /* plane size (cropped) */
    uint8_t     ss_x, ss_y, is_16bit, bit_depth;
    uint32_t    unit_size;      /* rsi->restoration_unit_size of this plane */
    uint32_t    horz_units, vert_units; /* rsi->horz_units_per_tile, vert_units_per_tile */
    const SvtHipLrUnit *units;  /* device [vert_units][horz_units] */
    const void *boundary_above, *boundary_below; /* device: rsb->stripe_boundary_above / _below (NULL when optimized_lr) */
    uint32_t    boundary_stride; /* samples */
    uint32_t    optimized_lr;
} SvtHipLrPlane;
SVT_HIP_API int32_t svt_hip_restoration_filter_frame(const SvtHipLrPlane *planes, uint32_t n_planes, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The Wiener decision of one plane between svt_hip_wiener_stats (which leaves M and H in device memory) and
 * svt_hip_restoration_filter_frame (which takes the units from device memory), for pictures whose loop restoration is
 * Wiener only (presets M4-M8).  Reference, all in restoration_pick.c:
 *   per unit    search_wiener_seg (:1296-1378): wiener_decompose_sep_sym (:906-936, int64, truncating division),
 *               finalize_sym_filter (:977-1006), compute_score (:937-975; a score above 0 rejects the filter),
 *               finer_tile_search_wiener_seg (:1042-1147); a trial is try_restoration_unit_seg (:129-165) with
 *               use_boundaries_in_rest_search == 0: the separable filter over the unit from the picture's own samples,
 *               edge-replicated outside the cropped plane (svt_extend_frame), then the SSE against the source
 *   per plane   search_wiener_finish (:1380-1431) over the units in raster order (`ref` starts at set_default_wiener and
 *               follows the last unit that chose Wiener), search_rest_type_finish (:1456-1465), rest_finish_search
 *               (:1555-1625) for RESTORE_NONE against RESTORE_WIENER: Wiener wins only with a strictly smaller cost
 * Not covered: several tiles.  With the self-guided filter enabled (RESTORE_SGRPROJ, search_switchable: presets M3 and slower)
 * svt_hip_rest_pick_plane below takes this call's unit records and decides the plane.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SvtHipWienerPickParams { /* read on the host */
    int32_t  wiener_win;                /* 7 or 5 */
    int32_t  is_16bit, bit_depth;       /* as svt_hip_wiener_stats: 8 / 10 / 12, above 8 only with 16-bit samples */
    uint32_t plane_width, plane_height; /* cropped size of the plane: samples outside it replicate its edge */
    int32_t  use_refinement, max_one_refinement_step; /* WnFilterCtrls */
    int32_t  rdmult;                    /* x->rdmult */
    int32_t  wiener_restore_cost[2];    /* x->wiener_restore_cost */
} SvtHipWienerPickParams;

#define SVT_HIP_WIENER_PICK_UNIT_BYTES 64
typedef struct SvtHipWienerPickUnit { /* one per restoration unit, device memory */
    int64_t sse[2];                   /* [RESTORE_NONE], [RESTORE_WIENER]; the latter INT64_MAX where the score rejects */
    int16_t hfilter[8], vfilter[8];   /* after the finer search; zero where rejected */
    int64_t bits;                     /* what the unit adds to the rate of frame type WIENER before the decision: bits_wiener
                                       * = cost[1] + (count_wiener_bits << 9) against `ref`; cost[0] where rejected */
    int32_t best_rtype;               /* best_rtype[RESTORE_WIENER - 1]: 1 where cost_wiener < cost_none, else 0 */
    int32_t trials;                   /* try_restoration_unit_seg calls of the finer search; 0 where rejected */
} SvtHipWienerPickUnit;

typedef struct SvtHipWienerPickResult { /* ONE record in device memory */
    int32_t frame_restoration_type;     /* 0 RESTORE_NONE, 1 RESTORE_WIENER */
    int32_t n_wiener;                   /* units with best_rtype 1 */
    int64_t sse[2], bits[2];            /* rsc->sse / rsc->bits after search_rest_type_finish of each type */
    double  cost[2];                    /* RDCOST_DBL(rdmult, bits >> 4, sse) of each type */
} SvtHipWienerPickResult;

/* Bytes of d_workspace for n_units restoration units: layout arithmetic, no device; 0 for an empty plane. */
SVT_HIP_API uint64_t svt_hip_wiener_pick_workspace_bytes(uint32_t n_units);
/* prm and units are read on the host; everything else is device memory:
 *   units          the array svt_hip_wiener_stats took, in raster order of the plane's restoration units, limits as
 *                  svt_aom_foreach_rest_unit_in_frame gives them; dgd / src of every unit point at sample (0, 0) of the
 *                  plane, and every limit lies inside plane_width x plane_height
 *   d_M, d_H       as svt_hip_wiener_stats wrote them for wiener_win; not modified
 *   d_prev_units   NULL, or SvtHipLrUnit [n_units] of the previous frame (use_prev_frame_coeffs): a unit whose record is
 *                  RESTORE_WIENER takes those taps and skips the solver and the score (NULL on key / intra-only frames)
 *                  A record whose coded taps lie outside their ranges (no decision leaves one; the number of launches is derived
 *                  from the ranges) is not taken: that unit is solved like one without a record
 *   d_unit_records SvtHipWienerPickUnit [n_units]
 *   d_lr_units     SvtHipLrUnit [n_units] for svt_hip_restoration_filter_frame: RESTORE_WIENER with the taps where the
 *                  unit chose Wiener and the plane's type is Wiener, RESTORE_NONE otherwise
 * The call enqueues its launches on `stream` and returns SVT_HIP_OK or an SVT_HIP_ERR_* code; it neither synchronises nor reads
 * anything back.  Refused with SVT_HIP_ERR_BAD_PARAMETER and a message, before anything is enqueued:
 *   - a NULL prm, units, d_M, d_H, d_unit_records, d_result, d_lr_units or d_workspace (d_prev_units may be NULL);
 *   - n_units == 0 or n_units > 65535 (the units are one dimension of the launch grid);
 *   - a window other than 5 or 7; a bit depth other than 8 / 10 / 12, or above 8 with 8-bit samples;
 *   - an empty plane, or one wider or taller than 65536 samples;
 *   - a unit without dgd or src, with empty or negative limits, or reaching outside plane_width x plane_height;
 *   - a unit wider or taller than 4096 samples (the limit of svt_hip_wiener_stats);
 *   - workspace_bytes below svt_hip_wiener_pick_workspace_bytes(n_units); d_workspace, d_unit_records or d_result not 8-byte aligned. */
SVT_HIP_API int svt_hip_wiener_pick_plane(const SvtHipWienerPickParams *prm, const SvtHipWienerUnit *units, uint32_t n_units,
                                          const int64_t *d_M, const int64_t *d_H, const SvtHipLrUnit *d_prev_units,
                                          SvtHipWienerPickUnit *d_unit_records, SvtHipWienerPickResult *d_result,
                                          SvtHipLrUnit *d_lr_units, void *d_workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The restoration decision of one plane with the self-guided filter enabled (presets M3 and slower), between
 * svt_hip_wiener_stats / svt_hip_wiener_pick_plane and svt_hip_restoration_filter_frame.  Reference, all in restoration_pick.c:
 *   per unit    search_norestore_seg (:1432), search_sgrproj_seg (:1220-1264) = search_selfguided_restoration (:550-652: apply_sgr
 *               in processing units from the unit's top-left, svt_get_proj_subspace, encode_xq :508, finer_search_pixel_proj_error
 *               :320-411; the first strictly smallest error in candidate order wins) and try_restoration_unit_seg (:129-165) with
 *               use_boundaries_in_rest_search == 0: svt_apply_selfguided_restoration in the tiling of
 *               svt_av1_loop_restoration_filter_unit (stripes of 64 >> ss_y rows offset by 8 >> ss_y, tiles of 64 >> ss_x columns)
 *               from the picture's own samples, then the SSE against the source
 *   per plane   search_wiener_finish (:1380), search_sgrproj_finish (:1267), search_switchable (:1148), each over the units in
 *               raster order with its own `ref` (set_default_wiener / set_default_sgrproj, then the last unit of that pass that
 *               chose the type); rest_finish_search (:1555-1625) with num_rtypes = n_units > 1 ? 4 : 3; copy_unit_info (:1202)
 * With d_wiener_records == NULL the Wiener filter counts as disabled (force_restore_type_d == RESTORE_SGRPROJ): NONE and SGRPROJ
 * alone are costed.  With records, a unit's best_rtype[RESTORE_WIENER - 1] is the record's, and search_switchable counts the Wiener
 * taps with prm->wiener_win (the reference: 7 for luma, 5 for chroma, whatever window was searched).
 * Not covered: several tiles, use_boundaries_in_rest_search != 0, the ref-based ep range (sg_filter_ctrls.step_range < 16, which
 * the caller can resolve into the four sg_* fields).
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SvtHipRestPickParams {   /* read on the host; 76 bytes */
    int32_t  is_16bit, bit_depth;       /* 8 / 10 / 12, above 8 only with 16-bit samples */
    uint32_t plane_width, plane_height; /* cropped; samples outside replicate the edge (svt_extend_frame) */
    int32_t  ss_x, ss_y;                /* processing unit = 64 >> ss; stripe offset = 8 >> ss_y */
    int32_t  wiener_win;                /* 7 / 5: read only when Wiener records are given */
    int32_t  sg_start_ep, sg_end_ep, sg_ep_inc, sg_refine; /* the loop of search_selfguided_restoration :589, already resolved */
    int32_t  rdmult;                    /* x->rdmult */
    int32_t  wiener_restore_cost[2], sgrproj_restore_cost[2], switchable_restore_cost[3];
} SvtHipRestPickParams;

#define SVT_HIP_REST_PICK_UNIT_BYTES 64
typedef struct SvtHipRestPickUnit { /* one per restoration unit, device memory; offsets in bytes */
    int64_t sse[3];                 /*  0: [RESTORE_NONE], [RESTORE_WIENER] (the record's sse[1]; INT64_MAX without records),
                                     *     [RESTORE_SGRPROJ] (the trial with the winner) */
    int64_t search_err;             /* 24: the winning projection error of the search */
    int32_t ep, xqd[2];             /* 32, 36: rusi->sgrproj */
    int32_t best_rtype[3];          /* 44: best_rtype[RESTORE_WIENER - 1], [RESTORE_SGRPROJ - 1], [RESTORE_SWITCHABLE - 1]; 0 for a
                                     *     pass that did not run */
    int32_t trials;                 /* 56: get_pixel_proj_error calls of the winning ep */
    int32_t pad_;                   /* 60: zero */
} SvtHipRestPickUnit;

#define SVT_HIP_REST_PICK_RESULT_BYTES 184
typedef struct SvtHipRestPickResult { /* ONE record in device memory; offsets in bytes */
    int32_t frame_restoration_type;   /*   0: 0 RESTORE_NONE, 1 RESTORE_WIENER, 2 RESTORE_SGRPROJ, 3 RESTORE_SWITCHABLE */
    int32_t tested;                   /*   4: bit r set = rest_finish_search costed type r */
    int64_t sse[4], bits[4];          /*   8, 40: rsc->sse / rsc->bits after search_rest_type_finish of each tested type, else 0 */
    double  cost[4];                  /*  72: RDCOST_DBL(rdmult, bits >> 4, sse) of each tested type, else 0 */
    int32_t n_units_of_type[3];       /* 104: units of d_lr_units that are NONE / WIENER / SGRPROJ */
    int32_t pad_;                     /* 116: zero */
    int32_t sg_frame_ep_cnt[16];      /* 120: how many units' search chose each ep (:1256; rest_process.c:634 derives the next
                                       *      frame's sg_frame_ep from it) */
} SvtHipRestPickResult;

/* Bytes of d_workspace: layout arithmetic, no device; 0 for no units, an empty plane or n_ep < 1.  n_ep = the candidates of the
 * loop, (sg_end_ep - sg_start_ep + sg_ep_inc - 1) / sg_ep_inc.  The workspace holds, each rounded up to 256 bytes: 64 bytes per
 * (unit, candidate) (the five sums of svt_get_proj_subspace, then the candidate's error, xqd and trials), 16 bytes per unit (the
 * two SSE sums), and the filtered planes as int32 [n_ep][2][plane_width * plane_height] (flt0, flt1 of every candidate; a unit's
 * samples lie packed, pitch = its width, at the sum of the sizes of the units before it). */
SVT_HIP_API uint64_t svt_hip_rest_pick_workspace_bytes(uint32_t n_units, uint32_t plane_width, uint32_t plane_height, int32_t n_ep);
/* prm and units are read on the host; everything else is device memory:
 *   units            the array the Wiener calls take: raster order, limits as svt_aom_foreach_rest_unit_in_frame gives them, dgd / src
 *                    at sample (0, 0) of the plane; at most 384 x 384 samples each, and together no more than the plane holds
 *   d_wiener_records NULL (Wiener not searched on this plane), or what svt_hip_wiener_pick_plane wrote earlier on the same stream;
 *                    only sse[1], the taps and best_rtype are read
 *   d_lr_units       per unit the type copy_unit_info assigns under the plane's type, the taps where it is WIENER, ep / xqd where it
 *                    is SGRPROJ, every other field zero; a NONE plane gets all-NONE units
 * The call enqueues a fixed number of launches (and one memset) on `stream` and returns that number of launches (>= 1); it neither
 * synchronises nor reads anything back.  It returns an SVT_HIP_ERR_* code, sign-extended (negative), when it refuses or fails.
 * Refused with SVT_HIP_ERR_BAD_PARAMETER and a message, before anything is enqueued:
 *   - a NULL prm, units, d_unit_records, d_result, d_lr_units or d_workspace; any of the last four not 8-byte aligned;
 *   - n_units == 0 or n_units > 65535; a bit depth other than 8 / 10 / 12, or above 8 with 8-bit samples;
 *   - an empty plane, or one wider or taller than 65536 samples; ss_x / ss_y outside {0, 1};
 *   - sg_start_ep < 0, sg_end_ep > 16, sg_start_ep >= sg_end_ep or sg_ep_inc < 1; wiener_win not 5 or 7 while records are given;
 *   - a unit without dgd or src, with empty or negative limits, reaching outside the plane, or over 384 samples in either dimension;
 *   - units that together hold more samples than the plane; workspace_bytes below svt_hip_rest_pick_workspace_bytes(). */
SVT_HIP_API int64_t svt_hip_rest_pick_plane(const SvtHipRestPickParams *prm, const SvtHipWienerUnit *units, uint32_t n_units,
                                            const SvtHipWienerPickUnit *d_wiener_records, SvtHipRestPickUnit *d_unit_records,
                                            SvtHipRestPickResult *d_result, SvtHipLrUnit *d_lr_units, void *d_workspace,
                                            uint64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_LF_H */
