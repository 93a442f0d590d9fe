/*
 * svt_hip_inter.h — C-ABI for inter prediction: interpolation (the single-reference and the
 * compound ("jnt") families), the masked-compound and OBMC blends, the compound mask search, warped prediction (local warp
 * and global motion), the global-motion corner detection / matching and error / refinement, the full-pel and the sub-pel motion
 * search of mode decision and OBMC's weighted target and motion refinement.
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   Source/Lib/Codec/common_dsp_rtcd.h:185-221   svt_av1_convolve_{2d_sr,x_sr,y_sr,2d_copy_sr},
 *                                                svt_av1_jnt_convolve_{2d,x,y,2d_copy} and the highbd sets
 *   Source/Lib/Codec/inter_prediction.c:311-668, 670-1035   their C implementations
 *   callers: svt_aom_inter_predictor / highbd_inter_predictor via svt_aom_convolve[subpel_x != 0][subpel_y != 0][is_compound]
 *            (inter_prediction.c:1036-1062)
 *   Source/Lib/Codec/blend_a64_mask.c:34-367, inter_prediction.c:2374-2404   svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c,
 *                                                svt_aom_(highbd_)blend_a64_mask_c, the vmask / hmask blends of OBMC
 *   Source/Lib/C_DEFAULT/inter_prediction_c.c:15-40   svt_av1_build_compound_diffwtd_mask_d16_c
 *   Source/Lib/Codec/enc_inter_prediction.c:386-449, 501-547, 4676-4719   pick_interinter_wedge / pick_interinter_seg
 *                                                (use_rate == 0) and the residuals of svt_aom_calc_pred_masked_compound
 *   Source/Lib/Codec/warped_motion.c:570-680, 718-820   svt_av1_warp_affine_c, svt_aom_dec_svt_av1_highbd_warp_affine_c (the
 *                                                arithmetic of svt_av1_highbd_warp_affine_c on plain uint16 samples)
 *   Source/Lib/Codec/warped_motion.c:357-363, 1045-1068   is_affine_shear_allowed, svt_get_shear_params
 *   Source/Lib/Codec/enc_warped_motion.c:22-98   svt_av1_warp_error
 *   Source/Lib/Codec/corner_detect.c:19-30, third_party/fastfeat/{fast.c, fast_9.c, nonmax.c}   svt_av1_fast_corner_detect
 *   Source/Lib/Codec/corner_match.c:87-218       svt_av1_determine_correspondence with improve_correspondence
 *   Source/Lib/Codec/global_motion.c:86-251      add_param_offset, force_wmtype, svt_av1_refine_integerized_param
 *   Source/Lib/Codec/mcomp.c:609-775             svt_av1_find_best_sub_pixel_tree(_pruned) as md_subpel_search calls them
 *   Source/Lib/Codec/product_coding_loop.c:1781-2046, 2075-2498, 3087-3108, 3263   md_full_pel_search under md_sq_motion_search,
 *                                                md_nsq_motion_search and pme_search, and the MVP scoring
 *   Source/Lib/Codec/enc_inter_prediction.c:1592-1649, 1767-1827   calc_target_weighted_pred and its two visitors
 *   Source/Lib/Codec/mode_decision.c:2425-2533, av1me.c:709-1132   single_motion_search (OBMC_CAUSAL): svt_av1_obmc_full_pixel_search,
 *                                                svt_av1_find_best_obmc_sub_pixel_tree_up, svt_aom_obmc_sad* / svt_aom_obmc_variance*
 * The warp entry points are Tier B only: the RTCD pointers svt_av1_warp_affine / svt_av1_highbd_warp_affine have no leaf.
 * Prediction from a reference of another size (has_scale: svt_av1_convolve_2d_scale) is svt_hip_convolve_scale_batch of
 * svt_hip_scale.h, whose compound intermediates are the ones of this header; the entry points here take references of the
 * picture's size.  RANSAC over the correspondences of global motion and svt_find_projection stay on the host.  The rate model of the mask search (model_rd_with_curvfit) stays on the host.  An OBMC candidate needs no host
 * arithmetic: its neighbour predictions are SvtHipConvolveDesc descriptors, then svt_hip_obmc_target_batch,
 * svt_hip_obmc_search_batch, the prediction at the vector found and the SVT_HIP_BLEND_VMASK / _HMASK blends; which neighbours
 * overlap, and svt_aom_choose_best_av1_mv_pred behind the search, stay the caller's control logic.
 * Inter-intra prediction is in svt_hip_intra.h: the smooth form is an epilogue of svt_hip_intra_predict_batch, the wedge form is
 * that prediction followed by a SVT_HIP_BLEND_MASK descriptor here.
 */
#ifndef SVT_HIP_INTER_H
#define SVT_HIP_INTER_H

#include "svt_hip_lf.h" /* SvtHipConvolveParams */
#include "svt_hip_me.h" /* SvtHipMv */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SvtHipInterpFilterParams { /* InterpFilterParams, definitions.h:750-755 */
    const int16_t *filter_ptr;           /* [subpel_shifts][taps] */
    uint16_t       taps, subpel_shifts;
    int32_t        interp_filter;
} SvtHipInterpFilterParams;

/* Tier A: RTCD signatures, host pointers (the highbd functions take real uint16 pointers, as in the reference).
 * w, h: 1 .. 128, any value (not only the block sizes); filter_params->taps: an even number <= 8, the table [16][taps].  Anything
 * else is refused before a kernel runs ("unsupported block"), which takes the Tier A failure path of svt_hip.h: the hot path
 * is disabled and the host's own function completes the call. */
#define SVT_HIP_DECL_CONV(mode)                                                                                                  \
    SVT_HIP_API void svt_av1_convolve_##mode##_hip(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride,      \
                                                   int32_t w, int32_t h, SvtHipInterpFilterParams *filter_params_x,              \
                                                   SvtHipInterpFilterParams *filter_params_y, const int32_t subpel_x_q4,         \
                                                   const int32_t subpel_y_q4, SvtHipConvolveParams *conv_params);               \
    SVT_HIP_API void svt_av1_highbd_convolve_##mode##_hip(const uint16_t *src, int32_t src_stride, uint16_t *dst,               \
                                                          int32_t dst_stride, int32_t w, int32_t h,                             \
                                                          const SvtHipInterpFilterParams *filter_params_x,                      \
                                                          const SvtHipInterpFilterParams *filter_params_y,                      \
                                                          const int32_t subpel_x_q4, const int32_t subpel_y_q4,                 \
                                                          SvtHipConvolveParams *conv_params, int32_t bd);
SVT_HIP_DECL_CONV(2d_sr)
SVT_HIP_DECL_CONV(x_sr)
SVT_HIP_DECL_CONV(y_sr)
SVT_HIP_DECL_CONV(2d_copy_sr)
#undef SVT_HIP_DECL_CONV
/* compound: conv_params->dst / dst_stride is the ConvBufType (uint16) buffer; do_average == 0 stores the offset
 * intermediate there, do_average == 1 reads it, averages (use_jnt_comp_avg: fwd_offset / bck_offset weights) and writes
 * pixels to dst */
#define SVT_HIP_DECL_JNT(mode)                                                                                                   \
    SVT_HIP_API void svt_av1_jnt_convolve_##mode##_hip(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride,  \
                                                       int32_t w, int32_t h, SvtHipInterpFilterParams *filter_params_x,          \
                                                       SvtHipInterpFilterParams *filter_params_y, const int32_t subpel_x_q4,     \
                                                       const int32_t subpel_y_q4, SvtHipConvolveParams *conv_params);           \
    SVT_HIP_API void svt_av1_highbd_jnt_convolve_##mode##_hip(const uint16_t *src, int32_t src_stride, uint16_t *dst,           \
                                                              int32_t dst_stride, int32_t w, int32_t h,                         \
                                                              const SvtHipInterpFilterParams *filter_params_x,                  \
                                                              const SvtHipInterpFilterParams *filter_params_y,                  \
                                                              const int32_t subpel_x_q4, const int32_t subpel_y_q4,             \
                                                              SvtHipConvolveParams *conv_params, int32_t bd);
SVT_HIP_DECL_JNT(2d)
SVT_HIP_DECL_JNT(x)
SVT_HIP_DECL_JNT(y)
SVT_HIP_DECL_JNT(2d_copy)
#undef SVT_HIP_DECL_JNT

/* Tier B: one descriptor per predicted block, all pointers device memory.  taps_x / taps_y == 0 selects what the
 * reference dispatches to when that direction has no sub-pel offset (x_sr, y_sr, 2d_copy_sr).
 * Descriptors are NOT validated (they live in device memory): the launch covers the first 2 x 2 tiles of 64 x 64 of every
 * block, so of a block wider or taller than 128 only that part is written; taps above 8 or odd are undefined.  Exactly the
 * w x h rectangle of dst (compound 0, 2, 3) or of cbuf (compound 1) is written and nothing else; compound 1 never touches dst,
 * compound 2 / 3 only read cbuf. */
typedef struct SvtHipConvolveDesc {
    const void *src;        /* sample the block's (0,0) maps to in the reference plane; taps/2-1 samples are read to the
                             * left / above and taps/2 to the right / below, none in a direction with taps == 0; the
                             * result depends on no other sample */
    void       *dst;
    uint32_t    src_stride, dst_stride; /* in samples */
    uint16_t    w, h;                   /* 1 .. 128, any value (the reference's callers use 2 .. 128); a descriptor with w == 0 or
                                         * h == 0 is skipped, its pointers may be null */
    int16_t     filter_x[8], filter_y[8]; /* the kernels of this block's sub-pel phases (av1_get_interp_filter_subpel_kernel):
                                           * the first taps_x / taps_y entries, the rest is ignored */
    uint8_t     taps_x, taps_y;         /* 0, or an even number <= 8 */
    uint8_t     round_0, round_1;       /* ConvolveParams of get_conv_params (convolve.h:40-68) */
    uint8_t     bit_depth, is_16bit;
    uint8_t     compound;               /* 0 single reference; 1 first prediction of a compound: the offset intermediate goes to
                                         * cbuf; 2 second prediction, plain average with cbuf -> dst; 3 second prediction,
                                         * distance-weighted average (use_jnt_comp_avg) */
    uint8_t     fwd_offset, bck_offset; /* compound 3: weights of cbuf and of this prediction (sum 16, DIST_PRECISION_BITS 4) */
    uint8_t     pad_[3];
    uint16_t   *cbuf;                   /* ConvBufType [h][cbuf_stride] (compound != 0); a compound 2 / 3 descriptor must be
                                         * launched AFTER the call that ran the compound 1 descriptor filling its cbuf */
    uint32_t    cbuf_stride, pad2_;
} SvtHipConvolveDesc;
SVT_HIP_API int32_t svt_hip_convolve_batch(const SvtHipConvolveDesc *d_desc, uint32_t n, void *stream);
/* the same entry point under its first name */
SVT_HIP_API int32_t svt_hip_convolve_sr_batch(const SvtHipConvolveDesc *d_desc, uint32_t n, void *stream);

/* ---- Masked-compound and OBMC blends (Tier B) -------------------------------------------------------------------------
 * One descriptor = one block of one plane, all pointers device memory.
 *
 * Masks are CALLER DATA, like the interpolation kernels of SvtHipConvolveDesc: the wedge tables
 * (svt_aom_get_contiguous_soft_mask), the OBMC ramps (svt_av1_get_obmc_mask) and the inter-intra smooth masks are the
 * encoder's own arrays; the caller uploads them once.  The library generates none of them.
 *
 * Ordering: a descriptor that reads a mask (or a ConvBufType block) which another descriptor writes must be launched in a
 * LATER call on the same stream.  The chroma planes of a difference-weighted compound read the mask that the luma
 * descriptor (SVT_HIP_BLEND_D16_DIFFWTD) builds: luma in one call, chroma in the next.
 *
 * Descriptors live in device memory, so the host cannot validate them.  The kernel SKIPS a descriptor with w == 0 or
 * h == 0, and one whose kind, subw / subh, mask_type, sizes, rounds, bit depth or NULL pointers are out of range (see the
 * fields); a skipped descriptor leaves dst (and mask) untouched. */
#define SVT_HIP_BLEND_D16 0         /* svt_aom_{lowbd,highbd}_blend_a64_d16_mask_c as svt_aom_build_masked_compound_no_round calls them */
#define SVT_HIP_BLEND_D16_DIFFWTD 1 /* svt_av1_build_compound_diffwtd_mask_d16_c, then the d16 blend with that mask (plane 0) */
#define SVT_HIP_BLEND_MASK 2        /* svt_aom_blend_a64_mask_c / svt_aom_highbd_blend_a64_mask_c */
#define SVT_HIP_BLEND_VMASK 3       /* svt_aom_blend_a64_vmask_c / svt_aom_highbd_blend_a64_vmask_16bit_c: mask[h], one weight per row */
#define SVT_HIP_BLEND_HMASK 4       /* svt_aom_blend_a64_hmask_c / svt_aom_highbd_blend_a64_hmask_16bit_c: mask[w], one weight per column */
#define SVT_HIP_BLEND_KINDS 5

typedef struct SvtHipBlendDesc {
    const void *src0, *src1; /* D16 kinds: ConvBufType (uint16) blocks as compound-1 descriptors of svt_hip_convolve_batch leave
                              * them; the other kinds: pixels (uint8, or uint16 with is_16bit).  mask weighs src0, 64 - mask src1 */
    void       *dst;         /* pixels (uint8, or uint16 with is_16bit).  VMASK / HMASK / MASK: may be src0 or src1 (with that
                              * source's stride): OBMC blends in place */
    uint8_t    *mask;        /* D16, MASK: [.][mask_stride], read; sub-sampled planes read the luma-sized mask (subw / subh).
                              * D16_DIFFWTD: WRITTEN as [h][w] (stride w, the reference's layout; mask_stride is not used) and
                              * used for the blend in the same pass.  VMASK: h entries.  HMASK: w entries */
    uint32_t    src0_stride, src1_stride, dst_stride, mask_stride; /* in samples */
    uint16_t    w, h;        /* 1 .. 128 (D16 kinds: 4 .. 128); w == 0 or h == 0: skipped */
    uint8_t     kind;        /* SVT_HIP_BLEND_* */
    uint8_t     subw, subh;  /* D16, MASK: 0 / 1; (1,1): rounded mean of 2 x 2 mask samples, (1,0) / (0,1): AOM_BLEND_AVG of two.
                              * 0 for the other kinds */
    uint8_t     mask_type;   /* D16_DIFFWTD: 0 DIFFWTD_38, 1 DIFFWTD_38_INV; 0 for the other kinds */
    uint8_t     round_0, round_1; /* D16 kinds: ConvolveParams of the compound prediction, round_0 + round_1 <= 14 */
    uint8_t     bit_depth;   /* 8, 10 or 12; 8 unless is_16bit */
    uint8_t     is_16bit;    /* 0 / 1: sample type of dst (and of src0 / src1 for the pixel kinds) */
    uint32_t    pad_;
} SvtHipBlendDesc;
/* SVT_HIP_ERR_BAD_PARAMETER when d_desc == NULL or n == 0, SVT_HIP_ERR_NO_DEVICE before svt_hip_init(); nothing is launched
 * in either case.  Asynchronous on `stream` (NULL: the calling thread's stream). */
SVT_HIP_API int32_t svt_hip_blend_batch(const SvtHipBlendDesc *d_desc, uint32_t n, void *stream);

/* ---- Compound mask search (Tier B) ------------------------------------------------------------------------------------
 * One descriptor = one luma block of one compound candidate: what svt_aom_calc_pred_masked_compound computes behind the two
 * predictions, then pick_interinter_wedge and pick_interinter_seg with use_rate == 0 (rd = sse, strict <, first minimum). */
#define SVT_HIP_WEDGE_TYPES 16
#define SVT_HIP_MASK_SEARCH_OK 0
#define SVT_HIP_MASK_SEARCH_BAD_WEDGE_SIZE 1 /* wedge_masks != NULL for a size without wedges */
#define SVT_HIP_MASK_SEARCH_BAD_DESC 2       /* NULL block pointer, size, bit depth or sample type out of range */

typedef struct SvtHipMaskSearchDesc {
    const void    *src, *pred0, *pred1; /* pixels: uint8, or uint16 with is_16bit */
    const uint8_t *wedge_masks;         /* [2 * SVT_HIP_WEDGE_TYPES][h * w]: mask (2 * index + sign) of this block size, i.e. the
                                         * reference's svt_aom_get_contiguous_soft_mask(index, sign, bsize) in its own order
                                         * (one contiguous range of wedge_mask_buf per size); NULL: no wedge search.  Sizes with
                                         * wedges: 8x8 8x16 16x8 16x16 16x32 32x16 32x32 8x32 32x8 */
    uint32_t       src_stride, pred0_stride, pred1_stride; /* in samples */
    uint16_t       w, h;                /* 8, 16, 32, 64 or 128 each */
    uint8_t        bit_depth;           /* 8, 10 or 12; 8 unless is_16bit.  Selects the difference-weighted mask's scale */
    uint8_t        is_16bit;
    uint8_t        pad_[6];
} SvtHipMaskSearchDesc;

typedef struct SvtHipMaskSearchResult {
    uint64_t wedge_sse[SVT_HIP_WEDGE_TYPES];  /* svt_av1_wedge_sse_from_residuals under wedge_sign[i]; 0 without wedges */
    uint64_t diffwtd_sse[2];                  /* ... under DIFFWTD_38 and DIFFWTD_38_INV */
    uint32_t pred0_to_pred1_dist;             /* SAD(pred0, pred1) */
    uint8_t  wedge_sign[SVT_HIP_WEDGE_TYPES]; /* svt_av1_wedge_sign_from_residuals */
    int8_t   best_wedge_index;                /* -1 without wedges */
    int8_t   best_wedge_sign;
    uint8_t  best_diffwtd_type;
    uint8_t  status;                          /* SVT_HIP_MASK_SEARCH_*; non-zero: every other field is 0 */
} SvtHipMaskSearchResult;
/* d_result[i] belongs to d_desc[i].  Errors as svt_hip_blend_batch (d_result == NULL is a bad parameter too). */
SVT_HIP_API int32_t svt_hip_compound_mask_search_batch(const SvtHipMaskSearchDesc *d_desc, SvtHipMaskSearchResult *d_result,
                                                       uint32_t n, void *stream);

/* ---- Warped prediction (Tier B) ---------------------------------------------------------------------------------------
 * One descriptor = one block of one plane, all pointers device memory: svt_av1_warp_affine_c, and for uint16 samples
 * svt_aom_dec_svt_av1_highbd_warp_affine_c.  compound / fwd_offset / bck_offset / cbuf / cbuf_stride mean exactly what they
 * mean in SvtHipConvolveDesc, so a warped and an interpolated prediction can be averaged with each other in either order, and
 * SVT_HIP_BLEND_D16* descriptors can read a cbuf that a warp left.
 *
 * The filter table (svt_aom_warped_filter) is CALLER DATA like the wedge masks: one device pointer per call, [193][8] int16,
 * SVT_HIP_WARP_FILTER_BYTES bytes are read from it.  The library holds no copy.
 *
 * The kernel SKIPS a descriptor (dst and cbuf keep every byte) with p_width == 0 or p_height == 0, a NULL ref, dst (unless compound == 1,
 * which writes cbuf only) or cbuf (compound != 0), a field out of the range given below, or a shear that is_affine_shear_allowed refuses:
 * 4 |alpha| + 7 |beta| >= 65536 or 4 |gamma| + 4 |delta| >= 65536.  That last check is what keeps the filter index inside
 * the table. */
#define SVT_HIP_WARP_FILTER_ROWS 193
#define SVT_HIP_WARP_FILTER_BYTES (SVT_HIP_WARP_FILTER_ROWS * 8 * 2)

typedef struct SvtHipWarpDesc {
    const void *ref;        /* sample (0, 0) of the reference PLANE; reads are clamped to [0, width) x [0, height) as the
                             * reference clamps them: nothing outside the plane is read */
    void       *dst;        /* the predicted block (uint8, or uint16 with is_16bit) */
    uint16_t   *cbuf;       /* ConvBufType [p_height][cbuf_stride] (compound != 0) */
    uint32_t    ref_stride, dst_stride, cbuf_stride; /* in samples */
    uint32_t    width, height;                       /* of the reference plane, 1 .. 65536 */
    int32_t     p_col, p_row;                        /* position of the block in the plane, 0 .. 65535 */
    uint16_t    p_width, p_height;                   /* 4 .. 128 (4: the chroma of an 8 x 8, cropped in the vertical filter) */
    int32_t     mat[6];                              /* wmmat[0 .. 5]; ROTZOOM: the caller has set mat[5] = mat[2], mat[4] = -mat[3] */
    int16_t     alpha, beta, gamma, delta;           /* EbWarpedMotionParams (svt_hip_warp_shear_params) */
    uint8_t     subsampling_x, subsampling_y;        /* 0 / 1 */
    uint8_t     round_0, round_1;                    /* ConvolveParams of get_conv_params: round_0 1 .. 7; compound: round_0 + round_1 <= 14 */
    uint8_t     bit_depth, is_16bit;                 /* 8, 10 or 12 (8 unless is_16bit); 0 / 1 */
    uint8_t     compound;                            /* 0 .. 3, as SvtHipConvolveDesc.compound */
    uint8_t     fwd_offset, bck_offset;              /* compound 3 */
    uint8_t     pad_[7];
} SvtHipWarpDesc;
/* d_filter: the filter table on the device.  Errors as svt_hip_blend_batch (d_filter == NULL is a bad parameter too).
 * Asynchronous on `stream`. */
SVT_HIP_API int32_t svt_hip_warp_batch(const SvtHipWarpDesc *d_desc, uint32_t n, const int16_t *d_filter, void *stream);

/* svt_get_shear_params: alpha, beta, gamma, delta of mat into out[0 .. 3]; returns 1, or 0 for an invalid model (mat[2] <= 0 or
 * a shear that is not allowed; out then holds whatever the reference would have left in the model).  Host only, no device. */
SVT_HIP_API int32_t svt_hip_warp_shear_params(const int32_t mat[6], int16_t out[4]);

/* ---- Global-motion error of a whole picture (Tier B) ------------------------------------------------------------------
 * svt_av1_warp_error for 8-bit luma over the whole current picture, N candidate models per call: 32 x 32 error blocks in
 * raster order (the last column / row narrower), with chess_refn every other block (the start alternates per block row) and
 * the final sum doubled, and the early exit: as soon as the running, un-doubled sum exceeds the candidate's best_error, that
 * partial sum is the result.  Every visited block's SAD goes to the workspace; a raster-order prefix pass per candidate then
 * returns the first prefix > best_error, else the total.  ConvolveParams are those of get_conv_params(0, 0, 0, 8). */
#define SVT_HIP_WARP_ERROR_BLOCK 32
#define SVT_HIP_WARP_ERROR_OK 0
#define SVT_HIP_WARP_ERROR_BAD_SHEAR 1 /* is_affine_shear_allowed refuses alpha .. delta: error 0, blocks_summed 0 */

typedef struct SvtHipWarpErrorJob {  /* host memory; the pointers in it are device memory */
    const uint8_t *ref, *cur;        /* reference and current luma planes, sample (0, 0) */
    const int16_t *filter;           /* svt_aom_warped_filter, SVT_HIP_WARP_FILTER_BYTES */
    void          *workspace;        /* svt_hip_warp_error_workspace_bytes(cur_width, cur_height, n) */
    uint64_t       workspace_bytes;
    uint32_t       ref_stride, ref_width, ref_height;
    uint32_t       cur_stride, cur_width, cur_height;
    uint8_t        chess_refn;       /* 0 / 1 */
    uint8_t        pad_[7];
} SvtHipWarpErrorJob;

typedef struct SvtHipWarpCandidate {
    int32_t mat[6];                  /* as SvtHipWarpDesc.mat */
    int16_t alpha, beta, gamma, delta;
    int64_t best_error;              /* early-exit threshold */
} SvtHipWarpCandidate;

typedef struct SvtHipWarpErrorResult {
    int64_t  error;
    uint32_t blocks_summed;          /* 32 x 32 blocks that entered `error` */
    uint8_t  status;                 /* SVT_HIP_WARP_ERROR_* */
    uint8_t  pad_[3];
} SvtHipWarpErrorResult;
/* Layout only, needs no device: n * blocks * 4 bytes of block SADs, rounded up, plus one result slot that svt_hip_gm_refine uses.
 * 0 when width, height or n is 0. */
SVT_HIP_API uint64_t svt_hip_warp_error_workspace_bytes(uint32_t width, uint32_t height, uint32_t n);
/* d_result[i] belongs to d_cand[i].  SVT_HIP_ERR_BAD_PARAMETER for a NULL pointer, n == 0 or n > 65535, an empty picture, a stride smaller
 * than its width or a workspace that is too small.  Asynchronous on `stream`; calls on one stream may share a workspace. */
SVT_HIP_API int32_t svt_hip_warp_error_batch(const SvtHipWarpErrorJob *job, const SvtHipWarpCandidate *d_cand,
                                             SvtHipWarpErrorResult *d_result, uint32_t n, void *stream);

/* svt_av1_refine_integerized_param on device-resident pictures: the hill climb over wmmat[0 .. n_params) with step 16 halved
 * n_refinements times, every svt_av1_warp_error replaced by a one-candidate svt_hip_warp_error_batch and an 8-byte read-back,
 * in the reference's order with its running best_error as the threshold.  A model that fails svt_hip_warp_shear_params
 * evaluates to error 1, as in the reference.  wmtype in / out: TransformationType 0 IDENTITY, 1 TRANSLATION, 2 ROTZOOM,
 * 3 AFFINE.  job->workspace serves one candidate.  Synchronous. */
SVT_HIP_API int32_t svt_hip_gm_refine(const SvtHipWarpErrorJob *job, int32_t wmmat[8], int32_t *wmtype, int32_t n_refinements,
                                      int64_t best_frame_error, int64_t *error, void *stream);

/* ---- Global-motion front end: FAST-9 corners and correspondences (Tier B) ------------------------------------------------
 * svt_av1_fast_corner_detect and svt_av1_determine_correspondence (with improve_correspondence) on device-resident 8-bit luma
 * planes, bit-exact.  A picture's corners are detected once and serve whether the picture is the frame or a reference of a match;
 * one match call takes one frame against several references.  What follows on the host is RANSAC over the at most 64 KB of a
 * SvtHipGmMatches record, then svt_hip_gm_refine.
 * The two status exports return SVT_HIP_GM_STATUS(status) as uint16_t: 0, or the low 16 bits of the SvtHipStatus. */
#define SVT_HIP_GM_MAX_CORNERS 4096 /* MAX_CORNERS */
#define SVT_HIP_GM_MAX_PLANES 8     /* planes per detect call, jobs per match call */
#define SVT_HIP_GM_MAX_MATCH_SZ 13  /* the reference's match_sz_sq is a uint8_t and sumsq2 * match_sz_sq overflows int from 15 on */
#define SVT_HIP_GM_STATUS(s) ((uint16_t)((s) & 0xffff))

typedef struct SvtHipGmPlane { /* host memory */
    const uint8_t *luma;       /* device memory, sample (0, 0) */
    uint32_t       width, height, stride;
    uint32_t       pad_;
} SvtHipGmPlane;

typedef struct SvtHipGmCorners { /* device memory, one per plane */
    uint32_t count;              /* min(found, SVT_HIP_GM_MAX_CORNERS): what svt_av1_fast_corner_detect returns */
    uint32_t found;              /* corners that survive the suppression, before the cap */
    int32_t  xy[2 * SVT_HIP_GM_MAX_CORNERS]; /* x, y in raster order; entries from 2 * count on are not written */
} SvtHipGmCorners;

typedef struct SvtHipGmMatchJob { /* host memory */
    SvtHipGmPlane          frm, ref; /* equal width and height, the strides may differ */
    const SvtHipGmCorners *frm_corners, *ref_corners; /* device memory, 8-byte aligned; ref_corners in raster order (see the call) */
    uint8_t                frm_quarters, ref_quarters; /* 1 .. 4: the job uses the first count * quarters / 4 corners (gm_ctrls.corners) */
    uint8_t                match_sz;                   /* odd, 3 .. SVT_HIP_GM_MAX_MATCH_SZ */
    uint8_t                pad_[5];
} SvtHipGmMatchJob;

typedef struct SvtHipGmMatches { /* device memory, one per job */
    uint32_t count, pad_;        /* what svt_av1_determine_correspondence returns */
    int32_t  pts[4 * SVT_HIP_GM_MAX_CORNERS]; /* x, y, rx, ry: the reference's Correspondence records in its order; the entries
                                               * from 4 * count up to 4 * (frame corners used) are 0, the rest is not written */
} SvtHipGmMatches;

/* Layout only, needs no device: n_planes * (the byte score map, the survivor bit map and the row counts of one width x height plane,
 * each rounded up to 256); 0 for an empty plane.  A call over planes of different sizes needs the sum over its planes of the value
 * for (width, height, 1); the value for the largest width and height and the number of planes is enough. */
SVT_HIP_API uint64_t svt_hip_gm_corners_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_planes);
/* d_out[i] belongs to planes[i].  FAST-9 at barrier 18 on every pixel with 3 <= x < width - 3 and 3 <= y < height - 3, the score of
 * fast9_score, the suppression of nonmax.c (a corner goes when one of its eight neighbours is a corner with a score >= its own), the
 * survivors in raster order.  The order comes from per-row counts, never from atomics: two calls give identical records.
 * SVT_HIP_ERR_BAD_PARAMETER for a NULL pointer, n > SVT_HIP_GM_MAX_PLANES, an empty plane, a stride smaller than the width, a
 * workspace that is too small, and two refusals of this library's own: a plane of more than 16384 samples a side (the reference's
 * squared distances leave int beyond), and records or a workspace that are not 8-byte aligned.
 * n == 0 is SVT_HIP_OK and launches nothing.  Asynchronous on `stream`, no host step. */
SVT_HIP_API uint16_t svt_hip_gm_detect_corners(const SvtHipGmPlane *planes, uint32_t n, SvtHipGmCorners *d_out, void *workspace,
                                               uint64_t workspace_bytes, void *stream);
/* d_out[i] belongs to jobs[i]; jobs may share corner records, and the call may follow the detect call that writes them on the same
 * stream with nothing in between.  Per frame corner whose match_sz window lies inside the picture: the reference corner with the
 * largest svt_av1_compute_cross_correlation_c among those whose window lies inside and whose squared distance is at most
 * (max(width, height) >> 4) squared, the first one on ties; kept when that exceeds template_norm * 0.75 * 0.75; then both passes of
 * improve_correspondence.
 * PRECONDITION, NOT CHECKED: the corners of a reference record are in raster order (y ascending, x ascending within a row), as
 * svt_hip_gm_detect_corners writes them: the candidates of a frame corner are found by a binary search on y.  A caller that fills a
 * record itself must keep that order; any other order gives wrong correspondences and no error.  The frame record may be in any order.
 * SVT_HIP_ERR_BAD_PARAMETER for a NULL pointer, n > SVT_HIP_GM_MAX_PLANES, an empty plane, a stride smaller than the width, unequal
 * frame and reference sizes, quarters outside 1 .. 4, a match_sz that is even, below 3 or above SVT_HIP_GM_MAX_MATCH_SZ, and two
 * refusals of this library's own: a plane of more than 16384 samples a side, and corner or match records that are not 8-byte aligned.
 * n == 0 is SVT_HIP_OK and launches nothing.  Asynchronous on `stream`, no host step. */
SVT_HIP_API uint16_t svt_hip_gm_match_corners(const SvtHipGmMatchJob *jobs, uint32_t n, SvtHipGmMatches *d_out, void *stream);

/* ---- Sub-pel motion search of mode decision (Tier B) ---------------------------------------------------------------------
 * One descriptor = one luma block of one (list, reference): md_subpel_search (product_coding_loop.c:2502-2614) behind its
 * set-up, i.e. svt_av1_find_best_sub_pixel_tree or svt_av1_find_best_sub_pixel_tree_pruned (mcomp.c:609-775) with everything
 * they call: svt_upsampled_setup_center_error, the exits, svt_first_level_check / svt_second_level_check_v2 over
 * svt_aom_upsampled_pred_c (variance.c:204-254) + vf, two_level_checks_fast over the bilinear svf (variance.c:28-68, 308-318),
 * svt_mv_err_cost_ with all six MV_COST_TYPEs, and the reference's integer types (unsigned cost * weight wraps mod 2^32).
 * 8-bit only, as the reference (hbd_md = 0 there).  Not covered: the compound / masked / OBMC variants the reference leaves
 * commented out, scaled references (the reference searches with is_scaled = 0 on a reference svt_hip_resize_planes of svt_hip_scale.h
 * brought to the picture's size; only the final prediction is scaled, svt_hip_convolve_scale_batch), and the encoder hook.
 *
 * What is read: of src the w x h block; of ref the (w + 8) x (h + 8) window that starts 4 samples above and 4 to the left of the
 * sample start_mv points at, whatever the filter and the controls (with two iterations per step a candidate lies up to 14/8 pel
 * from start_mv, and the filter tables reach 2 samples before and 3 after): the caller's picture border must cover it. */
#define SVT_HIP_SUBPEL_TREE 0        /* SUBPEL_SEARCH_METHODS, definitions.h:743-748 */
#define SVT_HIP_SUBPEL_TREE_PRUNED 1
#define SVT_HIP_SUBPEL_USE_2_TAPS 1  /* SUBPEL_SEARCH_TYPE, definitions.h:736-741 */
#define SVT_HIP_SUBPEL_USE_4_TAPS 2
#define SVT_HIP_SUBPEL_USE_8_TAPS 3
/* SvtHipSubpelResult.exit: where the function returned */
#define SVT_HIP_SUBPEL_EXIT_NONE 0      /* bad descriptor */
#define SVT_HIP_SUBPEL_EXIT_EARLY 1     /* the early_exit flag */
#define SVT_HIP_SUBPEL_EXIT_VARIANCE 2  /* variance of the full-pel prediction below pred_variance_th */
#define SVT_HIP_SUBPEL_EXIT_ABS_TH 3    /* centre error below th_normalizer */
#define SVT_HIP_SUBPEL_EXIT_NO_ROUND 4  /* round == 0 */
#define SVT_HIP_SUBPEL_EXIT_ROUND_DEV 5 /* _pruned: deviation >= round_dev_th after a round */
#define SVT_HIP_SUBPEL_EXIT_END 6       /* every round ran */
/* SvtHipSubpelResult.status */
#define SVT_HIP_SUBPEL_OK 0
#define SVT_HIP_SUBPEL_BAD_SIZE 1     /* w x h is none of the 22 block sizes */
#define SVT_HIP_SUBPEL_BAD_POINTER 2  /* src or ref NULL */
#define SVT_HIP_SUBPEL_BAD_START_MV 3 /* start_mv not full-pel, or not inside MV_LOW .. MV_UPP */
#define SVT_HIP_SUBPEL_BAD_METHOD 4
#define SVT_HIP_SUBPEL_BAD_FILTER 5   /* subpel_search_type (checked under both methods) */
#define SVT_HIP_SUBPEL_BAD_COST 6     /* mv_cost_type out of range, or MV_COST_ENTROPY without the job's tables */

typedef struct SvtHipSubpelJob { /* host memory; the pointers in it are device memory.  What a picture's blocks share */
    int32_t        mvjcost[4];
    const int32_t *mvcost[2];    /* centres of the row / column tables, index MV_LOW .. MV_UPP (-(1 << 14) .. 1 << 14), as
                                  * SvtHipMvCostParam.mvcost; NULL: no descriptor uses MV_COST_ENTROPY */
} SvtHipSubpelJob;

typedef struct SvtHipSubpelDesc {
    const uint8_t *src, *ref;    /* the block's co-located first sample in the source and in the reference picture
                                  * (ms_buffers->src->buf / ref->buf); no alignment is required */
    uint32_t src_stride, ref_stride;
    uint16_t w, h;               /* one of the 22 sizes of init_fn_ptr (av1me.c:31-170) */
    SvtHipMv start_mv;           /* full-pel, in 1/8 units */
    SvtHipMv ref_mv;             /* the vector the cost is taken against */
    SvtHipMv best_mvp;           /* mvp_array[list][ref][best_fp_mvp_idx] (mvp_th rule) */
    int32_t  col_min, col_max, row_min, row_max; /* SubpelMvLimits (svt_hip_subpel_mv_limits) */
    int32_t  iters_per_step;
    int32_t  pred_variance_th, round_dev_th;
    int32_t  error_per_bit, early_exit_th;
    int32_t  hp_mv_th;
    uint32_t best_mvp_dist;      /* best_fp_mvp_dist[list][ref] */
    uint8_t  method;             /* SVT_HIP_SUBPEL_TREE / _PRUNED */
    uint8_t  subpel_search_type; /* SVT_HIP_SUBPEL_USE_*; _PRUNED always filters bilinearly */
    uint8_t  forced_stop;        /* SUBPEL_FORCE_STOP: 0 EIGHTH_PEL .. 3 FULL_PEL */
    uint8_t  allow_hp, bias_fp;
    uint8_t  skip_diag_refinement; /* 0 .. 4 */
    uint8_t  abs_th_mult, qp;
    uint8_t  mv_cost_type;       /* MV_COST_TYPE, see SvtHipMvCostParam */
    uint8_t  early_exit;         /* the flag of product_coding_loop.c:2595-2597 */
    uint8_t  mvp_th;             /* _TREE with SPEL_ME in PD_PASS_1: md_subpel_me_ctrls.mvp_th; 0: the rule is off */
    uint8_t  pad_;
} SvtHipSubpelDesc;

typedef struct SvtHipSubpelResult {
    SvtHipMv best_mv;
    int32_t  besterr;     /* the function's return value */
    int32_t  distortion;
    uint32_t sse;         /* *sse1; 0 when no candidate won (the centre does not write it) */
    uint32_t fullpel_err; /* the centre's error, what the reference stores in ctx->fp_me_dist */
    uint8_t  exit;        /* SVT_HIP_SUBPEL_EXIT_* */
    uint8_t  status;      /* SVT_HIP_SUBPEL_*; non-zero: every other field is 0 */
    uint8_t  pad_[2];
} SvtHipSubpelResult;
/* d_result[i] belongs to d_desc[i].  SVT_HIP_ERR_BAD_PARAMETER for a NULL job, d_desc or d_result; n == 0 is SVT_HIP_OK and launches
 * nothing.  Asynchronous on `stream`. */
SVT_HIP_API int32_t svt_hip_subpel_search_batch(const SvtHipSubpelJob *job, const SvtHipSubpelDesc *d_desc, SvtHipSubpelResult *d_result,
                                                uint32_t n, void *stream);
/* product_coding_loop.c:2527-2537: the MvLimits of a block at (mi_row, mi_col) of mi_width x mi_height mode-info units in a picture
 * of mi_rows x mi_cols, then svt_av1_set_mv_search_range and svt_av1_set_subpel_mv_search_range around ref_mv.
 * limits: col_min, col_max, row_min, row_max.  Host only, no device.  SVT_HIP_ERR_BAD_PARAMETER for a NULL pointer. */
SVT_HIP_API int32_t svt_hip_subpel_mv_limits(int32_t mi_row, int32_t mi_col, int32_t mi_width, int32_t mi_height, int32_t mi_rows,
                                             int32_t mi_cols, const SvtHipMv *ref_mv, int32_t limits[4]);

/* ---- Full-pel motion search of mode decision (Tier B) ----------------------------------------------------------------------
 * One descriptor = one luma block of one (list, reference): md_full_pel_search (product_coding_loop.c:1918-2046) with
 * md_full_pel_search_large_lbd / svt_pme_sad_loop_kernel_c behind it, chained the way its callers chain it:
 *   SVT_HIP_FPEL_MVP  the scoring of :3087-3108: vf (variance) at each of up to 4 vectors, no clip, no vector cost, strict < from
 *                     (uint32_t)~0 in index order -> best_fp_mvp_idx / best_fp_mvp_dist;
 *   SVT_HIP_FPEL_SQ   md_sq_motion_search (:2314-2498): the probe at the ME vector, the gate, sparse levels 0 -> 1 -> 2;
 *   SVT_HIP_FPEL_NSQ  md_nsq_motion_search (:2141-2241) from the MVC list on: the rounded MVCs into one search centre, then
 *                     steps 4, 2, 1, taken only if strictly below the centre's cost;
 *   SVT_HIP_FPEL_PME  the one md_full_pel_search call of pme_search (:3263): step 1 around the best MVP.
 * Restated with the reference's types: uint32_t cost + int vector cost wraps, vectors and their differences are int16_t, mv >> 3 is
 * arithmetic on vectors that need not be full-pel, a clip may leave start > end (nothing is visited, the outputs keep their incoming
 * values), the generic scan is column-major and the psad scan (dist_type SAD, enable_psad, end_x - start_x >= 7 after the clip)
 * row-major over eight columns out of every 7 + step with its width raised to a multiple of 8.  The first position in scan order wins a tie.
 * 8-bit only, as every caller (hbd_md = EB_8_BIT_MD).  Not covered: scaled references (as for the sub-pel search: the caller searches
 * the reference that svt_hip_resize_planes brought to the picture's size), the derivation of the MVCs and MVPs,
 * svt_aom_choose_best_av1_mv_pred, the early / post checks of pme_search and its q_weight modulation of the window, the encoder hook.
 *
 * What is read: of src the w x h block.  Of ref, per stage, the blocks at the visited positions and nothing outside the rectangle
 * they span: from (mv >> 3) + start (after the clip of :1933-1947) to the last visited column / row, plus w x h.  On the psad path
 * the last column is start_x + W - 1 with W = end_x - start_x raised to a multiple of 8: up to 6 columns beyond the clipped end_x.  In
 * MVP mode the blocks at mv[i] >> 3.  The caller's picture border must cover that.  Positions of a level-1 window that the level-0
 * skip removes lie inside that rectangle and may be staged though they are not scored. */
#define SVT_HIP_FPEL_MVP 0
#define SVT_HIP_FPEL_SQ 1
#define SVT_HIP_FPEL_NSQ 2
#define SVT_HIP_FPEL_PME 3
#define SVT_HIP_FPEL_SAD 0 /* DistortionType (definitions.h) */
#define SVT_HIP_FPEL_VAR 1
#define SVT_HIP_FPEL_SSD 2
#define SVT_HIP_FPEL_MAX_MV 6      /* MAX_MD_NSQ_SARCH_MVC_CNT; MVP mode takes up to SVT_HIP_FPEL_MAX_MVP */
#define SVT_HIP_FPEL_MAX_MVP 4     /* MAX_MVP_CANIDATES */
#define SVT_HIP_FPEL_TILE 32       /* search positions per axis of one LDS tile of the reference window */
#define SVT_HIP_FPEL_MAX_EXTENT 4095 /* largest end - start of a window, per axis, before the clip */
/* SvtHipFpelResult.status */
#define SVT_HIP_FPEL_OK 0
#define SVT_HIP_FPEL_BAD_SIZE 1    /* w x h is none of the 22 block sizes */
#define SVT_HIP_FPEL_BAD_POINTER 2 /* src or ref NULL */
#define SVT_HIP_FPEL_BAD_MODE 3
#define SVT_HIP_FPEL_BAD_DIST 4    /* dist_type above SVT_HIP_FPEL_SSD */
#define SVT_HIP_FPEL_BAD_COST 5    /* mv_cost_type out of range, or MV_COST_ENTROPY without the job's tables (not in MVP mode) */
#define SVT_HIP_FPEL_BAD_COUNT 6   /* n_mv 0 or above the mode's maximum */
#define SVT_HIP_FPEL_BAD_STEP 7    /* an enabled level with step 0: the reference's loop would not end */
#define SVT_HIP_FPEL_BAD_WINDOW 8  /* an enabled level with end - start above SVT_HIP_FPEL_MAX_EXTENT on an axis */
/* the return value of svt_hip_fpel_search_batch: a SvtHipStatus in 16 bits */
#define SVT_HIP_FPEL_STATUS(s) ((int16_t)((s) == 0 ? 0 : (0x8000 | ((s) & 0x7fff))))

typedef struct SvtHipFpelLevel {  /* one md_full_pel_search call: the window before the clip, in full-pel offsets from the centre */
    int16_t start_x, end_x, start_y, end_y;
    uint8_t enabled;              /* SQ only; elsewhere ignored */
    uint8_t step;                 /* SQ: sprs_levN_step; elsewhere ignored (NSQ 4, 2, 1; PME 1) */
    uint8_t pad_[2];
} SvtHipFpelLevel;

typedef struct SvtHipFpelDesc {
    const uint8_t *src, *ref;     /* the block's co-located first sample in the source and in the reference picture; any alignment */
    uint32_t src_stride, ref_stride;
    uint16_t w, h;                /* one of the 22 sizes of init_fn_ptr (av1me.c:31-170) */
    uint16_t blk_org_x, blk_org_y; /* ctx->blk_org_x / _y */
    uint16_t ref_org_x, ref_org_y, ref_max_width, ref_max_height; /* ref_pic->org_x, org_y, max_width, max_height: the clip */
    SvtHipMv ref_mv;              /* ctx->ref_mv, the vector the cost is taken against */
    int32_t  error_per_bit;       /* AOMMAX(rdmult >> RD_EPB_SHIFT, 1), rdmult as md_full_pel_search picks it for dist_type */
    uint32_t gate_th;             /* SQ: md_sq_me_ctrls.pame_distortion_th * bwidth * bheight */
    SvtHipMv mv[SVT_HIP_FPEL_MAX_MV]; /* MVP: mvp_array[0 .. n_mv); SQ: mv[0] = the ME vector; NSQ: the MVCs as :2079-2140 built them,
                                   * not yet rounded; PME: mv[0] = the best MVP */
    SvtHipFpelLevel level[3];     /* SQ: sparse levels 0 .. 2 (svt_hip_fpel_sq_windows); PME: level[0] = the window */
    uint8_t  mode;                /* SVT_HIP_FPEL_MVP .. _PME */
    uint8_t  dist_type;           /* SVT_HIP_FPEL_SAD .. _SSD; MVP mode always takes the variance */
    uint8_t  enable_psad;         /* the mode's controls' enable_psad */
    uint8_t  mv_cost_type;        /* MV_COST_TYPE, see SvtHipMvCostParam */
    uint8_t  n_mv;                /* MVP: 1 .. 4; NSQ: 1 .. 6; SQ, PME: ignored */
    uint8_t  gate_enabled;        /* SQ: blk_geom->sq_size <= 64 */
    uint8_t  search_area_multiplier; /* SQ: what check_temporal_mv_size / check_spatial_mv_size give; used only if the gate opens */
    uint8_t  nsq_search_width, nsq_search_height; /* NSQ: md_nsq_me_ctrls.full_pel_search_width / _height */
    uint8_t  pad_[7];
} SvtHipFpelDesc;

typedef struct SvtHipFpelResult {
    SvtHipMv best_mv;   /* MVP: mv[mvp_idx]; SQ, NSQ: *me_mv_x / _y as the function leaves them; PME: best_search_mv */
    uint32_t best_cost; /* MVP: best_fp_mvp_dist; SQ, NSQ: best_search_cost ((uint32_t)~0 if no search ran); PME: pme_mv_cost */
    uint32_t aux_cost;  /* SQ: pa_me_cost; NSQ: search_center_cost; otherwise 0 */
    uint8_t  expanded;  /* SQ: the gate opened with a non-zero multiplier and the sparse levels ran */
    uint8_t  mvp_idx;   /* MVP: best_fp_mvp_idx */
    uint8_t  status;    /* SVT_HIP_FPEL_*; non-zero: every other field is 0 */
    uint8_t  pad_;
} SvtHipFpelResult;
/* d_result[i] belongs to d_desc[i]; job: mvjcost and the two centred mvcost tables, read by descriptors with MV_COST_ENTROPY.  The stages
 * of a descriptor run back to back in one workgroup; the descriptors run in parallel.  Returns SVT_HIP_FPEL_STATUS(status):
 * SVT_HIP_ERR_BAD_PARAMETER for a NULL job, d_desc or d_result; n == 0 is 0 and launches nothing.  Asynchronous on `stream`.
 * best_mv / best_cost / mvp_idx feed SvtHipSubpelDesc.start_mv / best_mvp / best_mvp_dist. */
SVT_HIP_API int16_t svt_hip_fpel_search_batch(const SvtHipSubpelJob *job, const SvtHipFpelDesc *d_desc, SvtHipFpelResult *d_result,
                                              uint32_t n, void *stream);

typedef struct SvtHipFpelSqCtrls {  /* the fields of MdSqMotionSearchCtrls the windows are derived from; [2]: only enabled, step, w, h */
    uint16_t w[3], h[3], max_w[3], max_h[3]; /* sprs_levN_w, _h, max_sprs_levN_w, _h */
    int16_t  multiplier[3];                  /* sprs_levN_multiplier */
    uint8_t  enabled[3], step[3];
} SvtHipFpelSqCtrls;
/* product_coding_loop.c:2379-2393, 2423-2446, 2480-2487: the three windows of md_sq_motion_search before the clip, from the controls,
 * search_area_multiplier and dist = svt_aom_get_scaled_picture_distance(|picture_number - ref poc|): the uint16_t products, the / 100,
 * the rounding to multiples of the step and the % 4 == 0 -> -+ 2 widening of level 1.  A level with step 0 gets the window
 * (0, 0, 0, 0) and keeps its enabled flag and its step (enabled, the descriptor is SVT_HIP_FPEL_BAD_STEP).  Host only, no device; with a
 * NULL pointer nothing is written. */
SVT_HIP_API void svt_hip_fpel_sq_windows(const SvtHipFpelSqCtrls *ctrls, uint8_t search_area_multiplier, uint16_t dist, SvtHipFpelLevel level[3]);

/* ---- OBMC motion refinement (Tier B) ------------------------------------------------------------------------------------------
 * What svt_aom_precompute_obmc_data and svt_aom_obmc_motion_refinement compute between the neighbour predictions
 * (SvtHipConvolveDesc) and the final blends (SVT_HIP_BLEND_VMASK / _HMASK): the weighted target, then single_motion_search
 * (mode_decision.c:2425-2533) for OBMC_CAUSAL.  8-bit only, as the reference (calc_target_weighted_pred sets is16bit = 0,
 * single_motion_search "supports 8bit path only").  Not covered: the bilinear osvf path (use_accurate_subpel_search == 0, which the
 * encoder never takes), scaled references (neighbour predictions from one go through svt_hip_convolve_scale_batch of svt_hip_scale.h;
 * the search itself is not scaled), svt_aom_choose_best_av1_mv_pred and the validity check behind the search, and an
 * encoder hook.  wsrc and mask are int32_t arrays and must be 4-byte aligned; every other pointer may have any alignment. */
#define SVT_HIP_OBMC_MAX_NEIGHBOURS 4 /* max_neighbor_obmc[] never exceeds it */
/* status of both entry points */
#define SVT_HIP_OBMC_OK 0
#define SVT_HIP_OBMC_BAD_SIZE 1     /* w x h is none of the 22 block sizes */
#define SVT_HIP_OBMC_BAD_POINTER 2  /* a NULL pointer that would be read or written, or wsrc / mask not 4-byte aligned */
#define SVT_HIP_OBMC_BAD_SEGMENT 3  /* target: more than 4 neighbours on a side, an empty one, one that runs past the block, or two that
                                     * are not in ascending order without overlap */
#define SVT_HIP_OBMC_BAD_RANGE 4    /* search: fpel_search_range above 16 */
#define SVT_HIP_OBMC_BAD_START_MV 5 /* search: start_mv not inside MV_LOW .. MV_UPP */
#define SVT_HIP_OBMC_BAD_LIMITS 6   /* search: a minimum above its maximum, or full-pel limits outside -2048 .. 2048 */
#define SVT_HIP_OBMC_BAD_FILTER 7   /* search: subpel_search_type */
#define SVT_HIP_OBMC_BAD_COST 8     /* search: approx_inter_rate == 0 without the job's tables */

typedef struct SvtHipObmcNeighbour { /* one call of the visitor of foreach_overlappable_nb_above / _left (enc_inter_prediction.c:684-752) */
    uint8_t rel_mi;                  /* rel_mi_col / rel_mi_row: where the neighbour starts along the block's edge, in units of 4 samples */
    uint8_t mi_len;                  /* nb_mi_width / nb_mi_height: AOMMIN(xd->n4_w, mi_step), in the same units */
} SvtHipObmcNeighbour;

/* calc_target_weighted_pred (enc_inter_prediction.c:1767-1827) with svt_av1_calc_target_weighted_pred_above_c / _left_c: wsrc = 0,
 * mask = 64; the above neighbours write (64 - m) * above and m over min(h, 64) / 2 rows; both times 64; the left neighbours blend
 * min(w, 64) / 2 columns; wsrc = src * 4096 - wsrc.  The ramps m are svt_av1_get_obmc_mask(overlap), held by the kernel.
 * WHICH neighbours overlap is the caller's: the walk over the mode info, the pairs of 4-wide blocks, nb_max and the clip at
 * mi_cols / mi_rows give the (rel_mi, mi_len) lists.
 * What is read: of src the w x h block; of above the rows 0 .. min(h, 64) / 2 and of left the columns 0 .. min(w, 64) / 2 of the
 * listed neighbours' samples, both laid out block-sized from the block's (0, 0) as svt_aom_precompute_obmc_data lays them out.
 * What is written: wsrc[h][w] and mask[h][w] (stride w) and the status.  A descriptor with a non-zero status leaves wsrc and mask
 * zero (untouched where the size or the two pointers themselves are what is wrong). */
typedef struct SvtHipObmcTargetDesc {
    const uint8_t      *src, *above, *left; /* above / left may be NULL when that side is unavailable or lists no neighbour */
    int32_t            *wsrc, *mask;
    uint32_t            src_stride, above_stride, left_stride;
    uint16_t            w, h;               /* one of the 22 sizes of init_fn_ptr (av1me.c:31-170) */
    uint8_t             up_available, left_available;
    uint8_t             n_above, n_left;    /* 0 .. SVT_HIP_OBMC_MAX_NEIGHBOURS; ignored on a side that is not available */
    SvtHipObmcNeighbour above_nb[SVT_HIP_OBMC_MAX_NEIGHBOURS], left_nb[SVT_HIP_OBMC_MAX_NEIGHBOURS];
    uint32_t            pad_;
} SvtHipObmcTargetDesc;
/* d_status[i] (SVT_HIP_OBMC_*) belongs to d_desc[i].  SVT_HIP_ERR_BAD_PARAMETER for a NULL d_desc or d_status; n == 0 is SVT_HIP_OK and
 * launches nothing.  Asynchronous on `stream`. */
SVT_HIP_API int32_t svt_hip_obmc_target_batch(const SvtHipObmcTargetDesc *d_desc, uint32_t *d_status, uint32_t n, void *stream);

/* single_motion_search for one block of one reference.
 * Full-pel stage (do_full_refine): svt_av1_obmc_full_pixel_search (av1me.c:721-776): start_mv >> 3 clamped into fp_limits, then
 * obmc_refining_search_sad over 4 or 8 neighbours for up to fpel_search_range rounds, error svt_aom_obmc_sad*, vector cost
 * mvsad_err_cost in both forms.  Without it the vector is start_mv >> 3.
 * Sub-pel stage (do_frac_refine): svt_av1_find_best_obmc_sub_pixel_tree_up (av1me.c:963-1132) on the accurate path
 * (svt_aom_upsampled_pred_c + svt_aom_obmc_variance*), limits from raw_limits as set_subpel_mv_search_range (av1me.c:778-790) derives
 * them, vector cost svt_aom_mv_err_cost / svt_aom_mv_err_cost_light.  Without it the vector is the full-pel one << 3.
 * rate_mv: svt_av1_mv_bit_cost(.., MV_COST_WEIGHT) or svt_av1_mv_bit_cost_light, as mode_decision.c:2529-2532.
 *
 * What is read: wsrc[h][w] and mask[h][w]; of ref, with R = fpel_search_range (0 without do_full_refine), the
 * (w + 2 R + 8) x (h + 2 R + 8) window that starts R + 4 samples above and R + 4 to the left of the sample the clamped start points at
 * (the full-pel stage moves at most R samples from there; the tree adds what the sub-pel section above states): the caller's
 * picture border must cover it. */
typedef struct SvtHipObmcSearchDesc {
    const int32_t *wsrc, *mask;  /* as svt_hip_obmc_target_batch leaves them */
    const uint8_t *ref;          /* the block's co-located first sample in the reference picture; no alignment is required */
    uint32_t ref_stride;
    uint16_t w, h;               /* one of the 22 sizes */
    SvtHipMv start_mv;           /* cand->mv, 1/8 units */
    SvtHipMv ref_mv;             /* cand->pred_mv */
    int32_t  raw_limits[4];      /* col_min, col_max, row_min, row_max in full-pel: x->mv_limits of mode_decision.c:2459-2462 */
    int32_t  fp_limits[4];       /* the same after svt_av1_set_mv_search_range (svt_hip_obmc_mv_limits gives both) */
    int32_t  sad_per_bit;        /* x->sadperbit16 */
    int32_t  error_per_bit;      /* x->errorperbit */
    int32_t  iters_per_step;     /* the encoder passes 2 */
    uint8_t  do_full_refine, do_frac_refine; /* the switch over refine_level at mode_decision.c:2430-2443 */
    uint8_t  fpel_search_range;  /* obmc_ctrls.fpel_search_range: 0 .. 16 */
    uint8_t  fpel_search_diag;   /* obmc_ctrls.fpel_search_diag: 0: 4 neighbours, otherwise 8 */
    uint8_t  approx_inter_rate;  /* ctx->approx_inter_rate: the light vector costs */
    uint8_t  allow_hp;
    uint8_t  subpel_search_type; /* SVT_HIP_SUBPEL_USE_2_TAPS .. _8_TAPS; the encoder passes 8 taps */
    uint8_t  forced_stop;        /* 0 .. 3; the encoder passes 0 */
    uint32_t pad_;
} SvtHipObmcSearchDesc;

typedef struct SvtHipObmcSearchResult {
    SvtHipMv best_mv;        /* x->best_mv, 1/8 units */
    SvtHipMv fullpel_mv;     /* the vector after the full-pel stage, in full-pel units */
    int32_t  besterr;        /* what the tree returns; 0 without do_frac_refine */
    int32_t  distortion;     /* dis; 0 without do_frac_refine */
    uint32_t sse;            /* sse1; 0 without do_frac_refine */
    int32_t  rate_mv;
    uint8_t  fullpel_rounds; /* rounds of the full-pel stage that moved the vector */
    uint8_t  status;         /* SVT_HIP_OBMC_*; non-zero: every other field is 0 */
    uint8_t  pad_[2];
} SvtHipObmcSearchResult;
/* d_result[i] belongs to d_desc[i]; job: mvjcost and the two centred mvcost tables (x->nmv_vec_cost, x->mv_cost_stack), read unless
 * approx_inter_rate.  SVT_HIP_ERR_BAD_PARAMETER for a NULL job, d_desc or d_result; n == 0 is SVT_HIP_OK and launches nothing.
 * Asynchronous on `stream`. */
SVT_HIP_API int32_t svt_hip_obmc_search_batch(const SvtHipSubpelJob *job, const SvtHipObmcSearchDesc *d_desc, SvtHipObmcSearchResult *d_result,
                                              uint32_t n, void *stream);
/* mode_decision.c:2459-2462: the full-pel MvLimits of a block at (mi_row, mi_col) of mi_width x mi_height mode-info units in a picture of
 * mi_rows x mi_cols into raw_limits, and the same after svt_av1_set_mv_search_range around ref_mv into fp_limits (col_min, col_max,
 * row_min, row_max each).  Host only, no device.  SVT_HIP_ERR_BAD_PARAMETER for a NULL pointer. */
SVT_HIP_API int32_t svt_hip_obmc_mv_limits(int32_t mi_row, int32_t mi_col, int32_t mi_width, int32_t mi_height, int32_t mi_rows,
                                           int32_t mi_cols, const SvtHipMv *ref_mv, int32_t raw_limits[4], int32_t fp_limits[4]);

/* ---- Interpolation filter search of mode decision (Tier B) ---------------------------------------------------------------
 * interpolation_filter_search (enc_inter_prediction.c:2413-2543) for a batch of luma blocks, bit-exact: for every pair of
 * filter_sets (:2402-2412, [0] the vertical and [1] the horizontal filter; only the three equal pairs without dual filter) the
 * switchable rate (svt_av1_get_switchable_rate :2157), the luma prediction of svt_aom_inter_prediction on its un-scaled path
 * (av1_get_convolve_filter_params: the 4-tap banks for a side <= 4, sharp mapping to 4-tap regular there; get_conv_params_no_round; the sr
 * family for one reference, the jnt family twice for a compound), the SSE of model_rd_for_sb (:2277) for plane 0, model_rd_from_sse (:2255)
 * with the Laplacian tables of model_rd_norm (:2178), RDCOST and the smooth bias (:2520-2525); strict <, the first minimum wins.
 * One descriptor is one luma block of one candidate; a call takes the candidates of a picture or of any part of it.
 * NOT covered, the caller's: masked (wedge / difference-weighted) compounds, OBMC and inter-intra candidates (the reference folds them
 * into the searched prediction at 8 bit); the packed 8 + 2 bit reference form; scaled references and intra block copy;
 * av1_is_interp_needed (:2388), the vector clamp of compute_subpel_params (:3166-3177) and the derivation of the two contexts;
 * chroma (the reference searches luma only); the encoder-side hook. */
#define SVT_HIP_IFS_COMBOS 9           /* DUAL_FILTER_SET_SIZE */
#define SVT_HIP_IFS_FILTER_BANKS 5     /* EIGHTTAP_REGULAR, EIGHTTAP_SMOOTH, MULTITAP_SHARP, then the two banks of av1_interp_4tap */
#define SVT_HIP_IFS_CONTEXTS 16        /* SWITCHABLE_FILTER_CONTEXTS */
/* SvtHipIfsResult.status */
#define SVT_HIP_IFS_OK 0
#define SVT_HIP_IFS_BAD_SIZE 1     /* w x h is none of the 22 block sizes */
#define SVT_HIP_IFS_BAD_POINTER 2  /* src or ref0 NULL, or ref1 NULL with compound != 0 */
#define SVT_HIP_IFS_BAD_PHASE 3    /* a phase above 15 */
#define SVT_HIP_IFS_BAD_CTX 4      /* a context >= SVT_HIP_IFS_CONTEXTS */
#define SVT_HIP_IFS_BAD_COMPOUND 5 /* compound 1 or above 3 */
#define SVT_HIP_IFS_BAD_WEIGHT 6   /* compound 3 with fwd_offset + bck_offset != 16 */
/* the SvtHipStatus of the call as the size_t that svt_hip_ifs_search_batch returns: its 32 bits, zero-extended */
#define SVT_HIP_IFS_STATUS(s) ((size_t)(uint32_t)(s))

typedef struct SvtHipIfsJob { /* host memory; the pointers in it are device memory.  What a picture's blocks share */
    const int32_t *d_switchable_rate; /* [SVT_HIP_IFS_CONTEXTS][3]: md_rate_est_ctx->switchable_interp_fac_bitss */
    const int16_t *d_filters;         /* [SVT_HIP_IFS_FILTER_BANKS][16][8], caller data: the library generates no filter */
    uint32_t       full_lambda;       /* already divided as :2429-2430 (>> 2 * (bit_depth - 8) at 10 bit) */
    int16_t        quantizer;         /* y_dequant_qtx[base_q_idx][1] of the search's bit depth */
    uint8_t        bit_depth;         /* 8: uint8 samples; 10: plain uint16 samples */
    uint8_t        enable_dual_filter;
    uint8_t        subsampled_distortion, skip_sse_rd_model; /* InterpolationSearchCtrls */
    uint16_t       smooth_bias_pct;   /* 0: none, else ifs_smooth_bias[picture_qp] (:2522-2525) */
    uint8_t        pad_[4];
} SvtHipIfsJob;

typedef struct SvtHipIfsDesc {
    const void *src;         /* the block's first sample in the source picture */
    const void *ref0, *ref1; /* the reference sample that the block's (0,0) maps to after the whole-sample part of the clamped vector:
                              * the contract of SvtHipConvolveDesc.src with 8 taps, so 3 samples are read to the left / above and 4 to
                              * the right / below in a direction whose phase is not 0, none otherwise.  ref1 is read only when compound */
    void       *dst;         /* NULL, or where the w x h prediction of the winning pair goes: byte for byte what svt_hip_convolve_batch
                              * writes for the same inputs; nothing but that rectangle is written */
    uint32_t    src_stride, ref0_stride, ref1_stride, dst_stride; /* in samples */
    uint16_t    w, h;        /* one of the 22 block sizes, 4 x 4 .. 128 x 128 */
    uint8_t     subpel_x0, subpel_y0, subpel_x1, subpel_y1; /* q4 phases 0 .. 15 of ref0 and ref1 */
    uint8_t     compound;    /* 0 single reference, 2 plain average, 3 distance-weighted average (SvtHipConvolveDesc.compound) */
    uint8_t     fwd_offset, bck_offset; /* compound 3: weights of ref0's and ref1's prediction, sum 16 */
    uint8_t     ctx[2];      /* svt_aom_get_pred_context_switchable_interp for dir 0 and dir 1 */
    uint8_t     pad_[3];
} SvtHipIfsDesc;

typedef struct SvtHipIfsResult {
    uint64_t rd;              /* the winner's cost */
    uint64_t sse;             /* the winner's sse as the distortion function returned it (before the bit-depth rounding) */
    uint32_t interp_filters;  /* av1_make_interp_filters(y, x): y | x << 16 */
    int32_t  switchable_rate;
    uint8_t  best;            /* index of the winner in filter_sets */
    uint8_t  status;          /* SVT_HIP_IFS_*; non-zero: every other field is 0 */
    uint8_t  pad_[6];
} SvtHipIfsResult;

typedef struct SvtHipIfsTrace { /* every pair's figures; a pair that was not tested (dual filter off) is all ones */
    uint64_t sse[SVT_HIP_IFS_COMBOS], rd[SVT_HIP_IFS_COMBOS];
} SvtHipIfsTrace;
/* d_result[i] (and d_trace[i] unless d_trace is NULL) belongs to d_desc[i]; a bad descriptor gets its status and zeroes in d_result,
 * zeroes in d_trace, and touches nothing else.  SVT_HIP_IFS_STATUS(SVT_HIP_ERR_BAD_PARAMETER), before any device is looked for, for a NULL job,
 * d_desc or d_result, a NULL table in the job and a bit depth other than 8 / 10; n == 0 is SVT_HIP_OK and launches nothing.
 * Asynchronous on `stream`. */
SVT_HIP_API size_t svt_hip_ifs_search_batch(const SvtHipIfsJob *job, const SvtHipIfsDesc *d_desc, SvtHipIfsResult *d_result,
                                            SvtHipIfsTrace *d_trace, uint32_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_INTER_H */
