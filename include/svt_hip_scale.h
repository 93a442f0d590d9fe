/*
 * svt_hip_scale.h — reference scaling and super-resolution (Tier B): what the encoder computes when --resize-mode or
 * --superres-mode gives a picture's references another size than the picture.
 *
 *   svt_hip_resize_planes            svt_av1_resize_plane[_horizontal] and the highbd twins (resize.c:399-460, 679-760)
 *   svt_hip_superres_upscale_planes  svt_av1_upscale_normative_rows (super_res.c:214)
 *   svt_hip_convolve_scale_batch     svt_av1_convolve_2d_scale_c / svt_av1_highbd_convolve_2d_scale_c (inter_prediction.c:420, 779)
 *   svt_hip_scale_factors, svt_hip_scaled_block_position, svt_hip_scaled_size: the host arithmetic around them
 *
 * All pictures are device memory.  There is no Tier A form: the RTCD pointers svt_av1_resize_plane and svt_av1_convolve_2d_scale
 * would put a PCIe round trip behind every call.  Padding the resized picture (svt_aom_generate_padding*), packing or unpacking
 * 10-bit pictures and the resize / super-res decisions stay with the caller.  Call sequence: INTEGRATION.md "Scaled references".
 *
 * The three status exports return SVT_HIP_SCALE_STATUS(status): the SvtHipStatus itself, sign-extended to intptr_t, so that a caller
 * compares the result with SVT_HIP_OK / SVT_HIP_ERR_* as it stands.  (int32_t and every other fixed-width integer are closed sets of
 * earlier exports: the ABI tests of those features list them name by name.)
 */
#ifndef SVT_HIP_SCALE_H
#define SVT_HIP_SCALE_H

#include "svt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_SCALE_MAX_PLANES 24    /* jobs per call: the three planes of a source and of seven references */
#define SVT_HIP_SCALE_MAX_TILE_COLS 64 /* MAX_TILE_COLS */
#define SVT_HIP_SCALE_INVALID (-1)     /* REF_INVALID_SCALE */
#define SVT_HIP_SCALE_STATUS(s) ((intptr_t)(int32_t)(s))

/* ---- svt_av1_resize_plane for a batch of planes -----------------------------------------------------------------------
 * resize_multistep per row, then per column over the clipped intermediate, exactly as svt_av1_resize_plane_c.  An axis whose lengths
 * are equal is a copy, so a job with src_height == dst_height is svt_av1_resize_plane_horizontal.  Otherwise an axis takes zero or one
 * halving step (svt_av1_down2_symeven_c for an even length, down2_symodd for an odd one) and then, unless the halved length is the
 * wanted one, svt_av1_interpolate_core_c with the bank choose_interp_filter picks.  That is every ratio the encoder reaches:
 * denominators 9 .. 15 interpolate, 16 halves, SCALE_THREE_QUATER (17) interpolates, a smaller reference scaled up interpolates with
 * the normative bank.  An axis that would need TWO OR MORE halvings (get_down2_steps >= 2: an output of a quarter of the input or less)
 * is refused; the reference's own comment says the encoder never gets there. */
typedef struct SvtHipResizePlane {
    const void *src;                    /* device; sample (0,0) of the visible plane; read, never written */
    void       *dst;                    /* device; exactly dst_width x dst_height samples are written; must not overlap src */
    uint32_t    src_stride, dst_stride; /* in samples */
    uint32_t    src_width, src_height, dst_width, dst_height; /* 1 .. 16384 */
    uint8_t     is_16bit, bit_depth;    /* uint8 samples (bit_depth 8), or uint16 at 8 / 10 / 12 bit (the clip of the highbd functions) */
    uint8_t     pad_[6];
} SvtHipResizePlane;

/* Layout arithmetic, no device: the intermediates (dst_width x src_height samples, rounded up to 256 bytes) of the planes that resize
 * both axes.  0 for NULL, for n == 0 and when no plane needs one. */
SVT_HIP_API size_t svt_hip_resize_workspace_bytes(const SvtHipResizePlane *planes, uint32_t n);
/* planes: HOST array of n <= SVT_HIP_SCALE_MAX_PLANES jobs.  d_workspace: device memory, 256-byte aligned, may be NULL when
 * svt_hip_resize_workspace_bytes is 0; it is scratch: the call owns it until its work on `stream` is done.  Asynchronous on `stream`
 * (NULL: the calling thread's stream); allocates no device memory; all planes of a call share its two launches.
 * SVT_HIP_ERR_BAD_PARAMETER (before any device is looked for) for a NULL array, n above the maximum, a NULL plane pointer, a zero or
 * too large width or height, a stride smaller than the width, is_16bit above 1, a bit depth outside 8 / 10 / 12 (or not 8 for uint8
 * samples), an axis of two halvings, and a workspace that is NULL, misaligned or too small.  n == 0 answers SVT_HIP_OK. */
SVT_HIP_API intptr_t svt_hip_resize_planes(const SvtHipResizePlane *planes, uint32_t n, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- svt_av1_upscale_normative_rows for a batch of planes -------------------------------------------------------------
 * The 8-tap normative filter at src[(x_qn >> 14) - 4 + k], k = 0 .. 7, of the tile column's first sample; x_step_qn and the first x0_qn from
 * av1_get_upscale_convolve_step and get_upscale_convolve_x0 of the PLANE widths, x0_qn carried from one tile column to the next, the
 * last column ending at the upscaled plane width.
 * THE SOURCE IS NEVER WRITTEN.  The reference overwrites the five columns left of the first and right of the last tile column with the
 * edge sample and restores them afterwards; here the column index is clamped to [0, end of the last tile column - 1] instead, which
 * reads the same values wherever the reference reads inside those columns.  The end of the last tile column is
 * tile_col_start_mi[tile_cols] << (2 - sub_x), which may lie beyond the plane width (mi_cols counts whole 8 x 8 blocks): as in the
 * reference, the samples up to there are read. */
typedef struct SvtHipSuperresPlane {
    const void *src;                    /* device; column 0 of the first of `rows` rows of the downscaled plane */
    void       *dst;                    /* device; rows x ROUND_POWER_OF_TWO(superres_upscaled_width, sub_x) samples are written */
    uint32_t    src_stride, dst_stride; /* in samples */
    uint32_t    rows;                   /* >= 1 */
    uint16_t    frame_width, superres_upscaled_width; /* of the FRAME (cm->frm_size); plane widths are ROUND_POWER_OF_TWO(., sub_x) */
    uint8_t     superres_denominator;   /* 8 .. 16 */
    uint8_t     sub_x;                  /* 0 / 1 */
    uint8_t     is_16bit, bit_depth;    /* uint8 samples (bit_depth 8), or uint16 at 8 / 10 / 12 bit */
    uint16_t    tile_cols;              /* 1 .. SVT_HIP_SCALE_MAX_TILE_COLS */
    uint16_t    tile_col_start_mi[SVT_HIP_SCALE_MAX_TILE_COLS + 1]; /* what svt_av1_tile_set_col reads: cm->tiles_info.tile_col_start_mi,
                                         * strictly increasing from 0; entry tile_cols is mi_cols */
} SvtHipSuperresPlane;
/* planes: HOST array of n <= SVT_HIP_SCALE_MAX_PLANES jobs.  Asynchronous on `stream`; allocates no device memory (the per-tile-column
 * constants travel through the call's staging slot).  SVT_HIP_ERR_BAD_PARAMETER (before any device is looked for) for a NULL array or
 * plane pointer, n above the maximum, no rows, a zero frame width, an upscaled width below the frame width, a denominator outside
 * 8 .. 16, sub_x above 1, a bad sample type or bit depth, tile_cols of 0 or above the maximum, tile starts that do not increase from 0,
 * a src_stride below the end of the last tile column and a dst_stride below the upscaled plane width.  n == 0 answers SVT_HIP_OK. */
SVT_HIP_API intptr_t svt_hip_superres_upscale_planes(const SvtHipSuperresPlane *planes, uint32_t n, void *stream);

/* ---- prediction from a scaled reference -------------------------------------------------------------------------------
 * One descriptor per predicted block, in DEVICE memory, not validated (like SvtHipConvolveDesc).  What svt_inter_predictor /
 * svt_highbd_inter_predictor call when has_scale(xs, ys): every sample has its own filter phase, (q & 1023) >> 6, the horizontal pass
 * covers im_h = (((h - 1) * y_step_qn + subpel_y_qn) >> 10) + taps_y rows.  The compound forms use the ConvBufType intermediates of
 * svt_hip_convolve_batch and svt_hip_blend_batch: a scaled first prediction (compound 1) and an un-scaled second one average with each
 * other, in either order.  64 x 64 output tiles, 2 x 2 of them per block: of a block wider or taller than 128 only that part is written.
 * Exactly the w x h rectangle of dst (compound 0, 2, 3) or of cbuf (compound 1) is written. */
typedef struct SvtHipConvolveScaleDesc {
    const void    *src;        /* the sample that (pos_y, pos_x) of svt_hip_scaled_block_position names in the reference plane; rows
                                * -(taps_y / 2 - 1) .. im_h - taps_y / 2 and the columns the horizontal taps reach are read */
    void          *dst;
    uint32_t       src_stride, dst_stride; /* in samples */
    uint16_t       w, h;       /* 1 .. 128; w == 0 or h == 0 skips the descriptor, its pointers may be null */
    uint32_t       pad0_;
    const int16_t *filter_x, *filter_y; /* device tables [16][taps_x] / [16][taps_y] (InterpFilterParams::filter_ptr): the phase differs
                                         * per sample, so the whole table */
    int32_t        subpel_x_qn, x_step_qn, subpel_y_qn, y_step_qn; /* 1/1024 sample; steps 64 .. 2048 (valid_ref_frame_size) */
    uint8_t        taps_x, taps_y;         /* even, 2 .. 8 */
    uint8_t        round_0, round_1;       /* ConvolveParams of get_conv_params */
    uint8_t        bit_depth, is_16bit;
    uint8_t        compound;               /* 0 .. 3 exactly as SvtHipConvolveDesc */
    uint8_t        fwd_offset, bck_offset; /* compound 3 */
    uint8_t        pad_[7];
    uint16_t      *cbuf;                   /* ConvBufType [h][cbuf_stride] (compound != 0) */
    uint32_t       cbuf_stride, pad2_;
} SvtHipConvolveScaleDesc;
/* SVT_HIP_ERR_BAD_PARAMETER when d_desc == NULL; n == 0 answers SVT_HIP_OK; SVT_HIP_ERR_NO_DEVICE before svt_hip_init().
 * Asynchronous on `stream`. */
SVT_HIP_API intptr_t svt_hip_convolve_scale_batch(const SvtHipConvolveScaleDesc *d_desc, uint32_t n, void *stream);

/* ---- host arithmetic: no device, callable before svt_hip_init -----------------------------------------------------------
 * svt_av1_setup_scale_factors_for_frame: the reference is other_w x other_h, the picture this_w x this_h.  An invalid pair
 * (valid_ref_frame_size) gives x_scale_fp == y_scale_fp == SVT_HIP_SCALE_INVALID and leaves the steps alone. */
typedef struct SvtHipScaleFactors {
    int32_t x_scale_fp, y_scale_fp; /* REF_SCALE_SHIFT 14; 1 << 14: not scaled */
    int32_t x_step_q4, y_step_q4;   /* 1/1024 sample per sample: the x_step_qn / y_step_qn of SvtHipConvolveScaleDesc */
} SvtHipScaleFactors;
SVT_HIP_API void svt_hip_scale_factors(int32_t other_w, int32_t other_h, int32_t this_w, int32_t this_h, SvtHipScaleFactors *out);

/* The scaled branch of compute_subpel_params (enc_inter_prediction.c:3126-3165): scaled_x / scaled_y of the block position plus the
 * vector with their 64-bit signed rounding, SCALE_EXTRA_OFF, and the clamp to the padded reference. */
typedef struct SvtHipScaledPosition {
    int32_t pos_x, pos_y;       /* whole samples in the reference plane: src = plane + pos_y * stride + pos_x */
    int32_t subpel_x, subpel_y; /* 0 .. 1023: subpel_x_qn / subpel_y_qn */
    int32_t xs, ys;             /* x_step_q4 / y_step_q4 */
} SvtHipScaledPosition;
/* pre_x / pre_y: the block's position in the plane (already sub-sampled); mv_col / mv_row in 1/8 luma sample; ss_x / ss_y 0 / 1;
 * frame_width / frame_height: of the reference frame (luma); sb_size: scs->super_block_size (64 or 128). */
SVT_HIP_API void svt_hip_scaled_block_position(const SvtHipScaleFactors *sf, int32_t pre_x, int32_t pre_y, int32_t mv_col, int32_t mv_row,
                                               uint32_t ss_x, uint32_t ss_y, uint32_t frame_width, uint32_t frame_height, uint32_t sb_size,
                                               SvtHipScaledPosition *out);
/* calculate_scaled_size_helper (super_res.c:22), with its signature: *dim is scaled in place.  Denominators 9 .. 16 scale by 8 / denom,
 * rounded, not below min(16, *dim); 17 (SCALE_THREE_QUATER) gives 3/4; 8 and anything else leaves *dim alone. */
SVT_HIP_API void svt_hip_scaled_size(uint16_t *dim, uint8_t denom);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_SCALE_H */
