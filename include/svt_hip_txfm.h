/*
 * svt_hip_txfm.h — C-ABI for forward / inverse 2-D transforms and quantisation (SURVEY.md §8 rows a6–a8).
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   Source/Lib/Codec/aom_dsp_rtcd.h:85-205     svt_av1_fwd_txfm2d_{WxH}[_N2|_N4]           (57 pointers)
 *   Source/Lib/Codec/aom_dsp_rtcd.h:214-237    svt_handle_transform{16x64,32x64,64x16,64x32,64x64}[_N2_N4]
 *   Source/Lib/Codec/aom_dsp_rtcd.h:244-260    svt_aom_quantize_b, svt_aom_highbd_quantize_b, svt_av1_quantize_b_qm,
 *                                              svt_av1_highbd_quantize_b_qm, svt_av1_quantize_fp[_32x32|_64x64|_qm],
 *                                              svt_av1_highbd_quantize_fp[_qm]
 *   Source/Lib/Codec/common_dsp_rtcd.c:482-500 svt_av1_inv_txfm2d_add_{WxH}                 (19 pointers)
 *   Source/Lib/Codec/full_loop.c:1462-1686     svt_aom_quantize_inv_quantize (the per-TB driver: Tier B batch)
 *   Source/Lib/Codec/transforms.c:3100-3154    svt_aom_estimate_transform     (the per-TB driver: Tier B batch)
 *
 * TxType is the reference's enum (definitions.h:981-998, 0 = DCT_DCT ... 15 = H_FLIPADST); TranLow is int32_t;
 * QmVal is uint8_t.
 */
#ifndef SVT_HIP_TXFM_H
#define SVT_HIP_TXFM_H

#include "svt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Tier A — ABI-identical per-call entry points (host pointers).
 * ------------------------------------------------------------------------------------------- */
#define SVT_HIP_FWD_DECL(W, H)                                                                                     \
    SVT_HIP_API void svt_av1_fwd_txfm2d_##W##x##H##_hip(int16_t *input, int32_t *output, uint32_t input_stride,    \
                                                        int32_t transform_type, uint8_t bit_depth);               \
    SVT_HIP_API void svt_av1_fwd_txfm2d_##W##x##H##_N2_hip(int16_t *input, int32_t *output, uint32_t input_stride, \
                                                           int32_t transform_type, uint8_t bit_depth);            \
    SVT_HIP_API void svt_av1_fwd_txfm2d_##W##x##H##_N4_hip(int16_t *input, int32_t *output, uint32_t input_stride, \
                                                           int32_t transform_type, uint8_t bit_depth);
SVT_HIP_FWD_DECL(4, 4) SVT_HIP_FWD_DECL(8, 8) SVT_HIP_FWD_DECL(16, 16) SVT_HIP_FWD_DECL(32, 32) SVT_HIP_FWD_DECL(64, 64)
SVT_HIP_FWD_DECL(4, 8) SVT_HIP_FWD_DECL(8, 4) SVT_HIP_FWD_DECL(8, 16) SVT_HIP_FWD_DECL(16, 8) SVT_HIP_FWD_DECL(16, 32)
SVT_HIP_FWD_DECL(32, 16) SVT_HIP_FWD_DECL(32, 64) SVT_HIP_FWD_DECL(64, 32) SVT_HIP_FWD_DECL(4, 16) SVT_HIP_FWD_DECL(16, 4)
SVT_HIP_FWD_DECL(8, 32) SVT_HIP_FWD_DECL(32, 8) SVT_HIP_FWD_DECL(16, 64) SVT_HIP_FWD_DECL(64, 16)

/* svt_handle_transformWxH / _N2_N4: energy of the discarded 64-point area + repack to 32-wide */
SVT_HIP_API uint64_t svt_handle_transform16x64_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform32x64_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform64x16_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform64x32_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform64x64_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform16x64_N2_N4_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform32x64_N2_N4_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform64x16_N2_N4_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform64x32_N2_N4_hip(int32_t *output);
SVT_HIP_API uint64_t svt_handle_transform64x64_N2_N4_hip(int32_t *output);

/* inverse + add; the three signature flavours of common_dsp_rtcd.h (square / 4xN / the rest) */
#define SVT_HIP_INV_DECL_SQ(W, H)                                                                                    \
    SVT_HIP_API void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *input, uint16_t *output_r, int32_t stride_r, \
                                                            uint16_t *output_w, int32_t stride_w, int32_t tx_type,  \
                                                            int32_t bd);
#define SVT_HIP_INV_DECL_TS(W, H)                                                                                    \
    SVT_HIP_API void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *input, uint16_t *output_r, int32_t stride_r, \
                                                            uint16_t *output_w, int32_t stride_w, int32_t tx_type,  \
                                                            int32_t tx_size, int32_t bd);
#define SVT_HIP_INV_DECL_EOB(W, H)                                                                                   \
    SVT_HIP_API void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *input, uint16_t *output_r, int32_t stride_r, \
                                                            uint16_t *output_w, int32_t stride_w, int32_t tx_type,  \
                                                            int32_t tx_size, int32_t eob, int32_t bd);
SVT_HIP_INV_DECL_SQ(4, 4) SVT_HIP_INV_DECL_SQ(8, 8) SVT_HIP_INV_DECL_SQ(16, 16) SVT_HIP_INV_DECL_SQ(32, 32)
SVT_HIP_INV_DECL_SQ(64, 64) SVT_HIP_INV_DECL_TS(4, 8) SVT_HIP_INV_DECL_TS(8, 4) SVT_HIP_INV_DECL_TS(4, 16)
SVT_HIP_INV_DECL_TS(16, 4) SVT_HIP_INV_DECL_EOB(8, 16) SVT_HIP_INV_DECL_EOB(16, 8) SVT_HIP_INV_DECL_EOB(16, 32)
SVT_HIP_INV_DECL_EOB(32, 16) SVT_HIP_INV_DECL_EOB(32, 64) SVT_HIP_INV_DECL_EOB(64, 32) SVT_HIP_INV_DECL_EOB(8, 32)
SVT_HIP_INV_DECL_EOB(32, 8) SVT_HIP_INV_DECL_EOB(16, 64) SVT_HIP_INV_DECL_EOB(64, 16)

/* quantizers */
#define SVT_HIP_QARGS                                                                                           \
    const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr,            \
        const int16_t *quant_ptr, const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,   \
        const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan
SVT_HIP_API void svt_aom_quantize_b_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int32_t log_scale);
SVT_HIP_API void svt_av1_quantize_b_qm_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int32_t log_scale);
SVT_HIP_API void svt_aom_highbd_quantize_b_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int32_t log_scale);
SVT_HIP_API void svt_av1_highbd_quantize_b_qm_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int32_t log_scale);
SVT_HIP_API void svt_av1_quantize_fp_hip(SVT_HIP_QARGS);
SVT_HIP_API void svt_av1_quantize_fp_32x32_hip(SVT_HIP_QARGS);
SVT_HIP_API void svt_av1_quantize_fp_64x64_hip(SVT_HIP_QARGS);
SVT_HIP_API void svt_av1_quantize_fp_qm_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int16_t log_scale);
SVT_HIP_API void svt_av1_highbd_quantize_fp_hip(SVT_HIP_QARGS, int16_t log_scale);
SVT_HIP_API void svt_av1_highbd_quantize_fp_qm_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int16_t log_scale);

/* Residual producer and transform-domain cost of the TPL dispenser / mode decision: svt_aom_subtract_block,
 * svt_aom_highbd_subtract_block (common_dsp_rtcd.h:234-237; src8 / pred8 of the highbd form are uint16 planes) and
 * svt_aom_satd (aom_dsp_rtcd.h:206-207). */
/* Mirror of TxfmParam (definitions.h:1051-1063): TxType, TxSize and TxSetType are one-byte (packed) enums there. */
typedef struct SvtHipTxfmParam {
    uint8_t tx_type;
    uint8_t tx_size;
    int32_t lossless;
    int32_t bd;
    int32_t is_hbd;
    uint8_t tx_set_type;
    int32_t eob;
} SvtHipTxfmParam;
/* svt_av1_inv_txfm_add (common_dsp_rtcd.h:150; inv_transforms.c:3177-3193): 8-bit prediction + inverse transform ->
 * 8-bit reconstruction, size and type taken from txfm_param.  bd must be 8 and lossless 0 (all the reference passes). */
SVT_HIP_API void svt_av1_inv_txfm_add_hip(const int32_t *dqcoeff, uint8_t *dst_r, int32_t stride_r, uint8_t *dst_w,
                                          int32_t stride_w, const SvtHipTxfmParam *txfm_param);
/* svt_residual_kernel8bit / 16bit (common_dsp_rtcd.h:163,174), svt_spatial_full_distortion_kernel (:171),
 * svt_full_distortion_kernel16_bits (:173: byte pointers that hold 16-bit samples; offsets and strides in samples) */
SVT_HIP_API void svt_residual_kernel8bit_hip(uint8_t *input, uint32_t input_stride, uint8_t *pred, uint32_t pred_stride,
                                             int16_t *residual, uint32_t residual_stride, uint32_t area_width,
                                             uint32_t area_height);
SVT_HIP_API void svt_residual_kernel16bit_hip(uint16_t *input, uint32_t input_stride, uint16_t *pred, uint32_t pred_stride,
                                              int16_t *residual, uint32_t residual_stride, uint32_t area_width,
                                              uint32_t area_height);
SVT_HIP_API uint64_t svt_spatial_full_distortion_kernel_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride,
                                                            uint8_t *recon, int32_t recon_offset, uint32_t recon_stride,
                                                            uint32_t area_width, uint32_t area_height);
SVT_HIP_API uint64_t svt_full_distortion_kernel16_bits_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride,
                                                           uint8_t *pred, int32_t pred_offset, uint32_t pred_stride,
                                                           uint32_t area_width, uint32_t area_height);
/* Tier B form of the two distortion leaves: the sum of squared differences of two DEVICE planes (strides in samples) into *d_out (device,
 * zeroed by the call).  Caller: picture_sse_calculations (deblocking_filter.c:716-834) after every trial of the deblocking level search
 * (try_filter_frame :842-882) — the filtered trial picture then never leaves the device, 8 bytes come back. */
SVT_HIP_API int32_t svt_hip_plane_sse(const void *d_a, uint32_t a_stride, const void *d_b, uint32_t b_stride, uint32_t width, uint32_t height, int32_t is_16bit,
                                      uint64_t *d_out, void *stream);
SVT_HIP_API void svt_aom_subtract_block_hip(int rows, int cols, int16_t *diff_ptr, ptrdiff_t diff_stride, const uint8_t *src_ptr,
                                            ptrdiff_t src_stride, const uint8_t *pred_ptr, ptrdiff_t pred_stride);
SVT_HIP_API void svt_aom_highbd_subtract_block_hip(int rows, int cols, int16_t *diff_ptr, ptrdiff_t diff_stride,
                                                   const uint8_t *src_ptr, ptrdiff_t src_stride, const uint8_t *pred_ptr,
                                                   ptrdiff_t pred_stride, int bd);
SVT_HIP_API int svt_aom_satd_hip(const int32_t *coeff, int length);
/* Transform-domain distortion of the full loop: svt_full_distortion_kernel32_bits and its cbf-zero form
 * (common_dsp_rtcd.h:166-167, pic_operators.c:150-221); distortion_result = {residual, prediction}. */
SVT_HIP_API void svt_full_distortion_kernel32_bits_hip(int32_t *coeff, uint32_t coeff_stride, int32_t *recon_coeff,
                                                       uint32_t recon_coeff_stride, uint64_t distortion_result[2],
                                                       uint32_t area_width, uint32_t area_height);
SVT_HIP_API void svt_full_distortion_kernel_cbf_zero32_bits_hip(int32_t *coeff, uint32_t coeff_stride, uint64_t distortion_result[2],
                                                                uint32_t area_width, uint32_t area_height);

/* ---------------------------------------------------------------------------------------------
 * Tier B — batched, fused transform block processing on device-resident data:
 *   residual --fwd txfm--> coeff --[64-pt: energy + repack]--> quantize --> qcoeff/dqcoeff/eob
 *            --[optional]--> inverse txfm + prediction --> reconstruction
 * One call = n blocks of ONE size (w x h); type / shape / quantizer parameters vary per block.
 * All offsets are BYTE offsets into one device arena `d_base`; SVT_HIP_NO_OFFSET disables an output.
 * ------------------------------------------------------------------------------------------- */
#define SVT_HIP_NO_OFFSET (~(uint64_t)0)

enum { /* SvtHipTxfmDesc::quant_mode */
    SVT_HIP_QUANT_NONE = 0,
    SVT_HIP_QUANT_B,        /* svt_aom_quantize_b          (full_loop.c:25-75)   */
    SVT_HIP_QUANT_B_HBD,    /* svt_aom_highbd_quantize_b   (full_loop.c:145-194) */
    SVT_HIP_QUANT_FP,       /* svt_av1_quantize_fp*        (full_loop.c:278-338) */
    SVT_HIP_QUANT_FP_HBD    /* svt_av1_highbd_quantize_fp* (full_loop.c:383-449) */
};
enum { /* SvtHipTxfmDesc::flags */
    SVT_HIP_TX_FWD     = 1, /* run the forward transform from `residual_off` */
    SVT_HIP_TX_INV     = 2, /* run the inverse transform + add (needs dqcoeff: computed here or read from dqcoeff_off) */
    SVT_HIP_TX_PIXEL16 = 4, /* pred / recon are uint16 planes (else uint8, bit_depth must be 8) */
    SVT_HIP_TX_FULLCOEFF = 8, /* coeff_off receives the complete [h][w] array even for 64-point sizes (no repack) */
    /* The residual is formed on the fly, svt_aom_subtract_block / svt_aom_highbd_subtract_block semantics
     * (inter_prediction.c:35-60): residual_off / residual_stride address the SOURCE pixels, pred_off / pred_stride the
     * prediction (uint8, or uint16 with SVT_HIP_TX_PIXEL16); strides in pixels. */
    SVT_HIP_TX_SRC_PRED = 16,
    /* result.satd = svt_aom_satd (common_dsp_rtcd.c:71-78) over the retained coefficients of the forward transform.
     * FWD | SRC_PRED | SATD with DCT_DCT is the TPL dispenser's block cost (src_ops_process.c:734-748, 861-873): pass the
     * sub-sampled transform size as w x h and the strides pre-shifted by subsample_tx exactly as the reference does, and
     * shift the result left by subsample_tx.  (For sizes with a 64-point side the retained 32x32 block is summed once;
     * the reference's length = 64*64 walk also re-reads the stale rows 16..31 of the un-repacked array.) */
    SVT_HIP_TX_SATD = 32
};

typedef struct SvtHipTxfmDesc {
    uint64_t residual_off;            /* int16 [h][residual_stride] */
    uint64_t coeff_off;               /* int32 out: [h][w], or [min(h,32)][min(w,32)] repacked for 64-point sizes */
    uint64_t qcoeff_off, dqcoeff_off; /* int32 [n], n = min(w,32)*min(h,32) */
    uint64_t pred_off, recon_off;     /* pixel planes (SVT_HIP_TX_INV) */
    uint64_t iscan_off;               /* int16 iscan[n] (position of raster index in scan order) */
    uint64_t qm_off, iqm_off;         /* uint8 [n] quantisation matrices or SVT_HIP_NO_OFFSET */
    uint32_t residual_stride;         /* in int16 units */
    uint32_t pred_stride, recon_stride; /* in pixels */
    int16_t  zbin[2], round[2], quant[2], quant_shift[2], dequant[2]; /* [0] DC, [1] AC */
    uint8_t  tx_type, shape /* 0 full, 1 N2, 2 N4 */, bit_depth, quant_mode, log_scale, flags;
    uint8_t  dist_w, dist_h; /* svt_hip_txfm_distortion_batch: cropped_tx_width / cropped_tx_height of the caller
                              * (0 = min(w,32) / min(h,32)) */
} SvtHipTxfmDesc;

typedef struct SvtHipTxfmResult {
    uint64_t three_quad_energy; /* svt_handle_transformWxH return value (0 for sizes without a 64-point side) */
    uint16_t eob;
    uint16_t pad_;
    uint32_t satd; /* SVT_HIP_TX_SATD, else 0 */
} SvtHipTxfmResult;

SVT_HIP_API int32_t svt_hip_txfm_quant_batch(uint8_t *d_base, const SvtHipTxfmDesc *d_desc, SvtHipTxfmResult *d_result,
                                             uint32_t n_blocks, uint32_t w, uint32_t h, void *stream);
/* Test aid.  svt_hip_txfm_quant_batch runs a kernel that holds the common class of blocks only (8/10-bit, forward + inverse,
 * quantize_b without matrices, amplitudes within the 24-bit arithmetic) and hands the blocks of every wave that meets anything
 * else to the general kernel, launched behind it.  *out = how many blocks the calling thread's last svt_hip_txfm_quant_batch
 * handed over (0 when that call used the general kernel alone, or when the thread's scratch has been taken for something else
 * since); waits for the stream that call ran on, which must still exist. */
SVT_HIP_API int32_t svt_hip_debug_txfm_fallback_blocks(uint32_t *out);

/* Transform-domain distortion of the same blocks, what svt_aom_full_loop_core reads right after the quantiser
 * (svt_aom_picture_full_distortion32_bits_single, pic_operators.c:150-234): d_distortion[i] = {DIST_CALC_RESIDUAL =
 * sum (coeff - dqcoeff)^2, DIST_CALC_PREDICTION = sum coeff^2} over the dist_w x dist_h top-left area of the retained
 * coefficient block of descriptor i ({0, 0} when it has no coeff_off / dqcoeff_off).  Run it after
 * svt_hip_txfm_quant_batch on the same stream with the same descriptors (that call writes the coefficient arrays). */
SVT_HIP_API int32_t svt_hip_txfm_distortion_batch(const uint8_t *d_base, const SvtHipTxfmDesc *d_desc, uint64_t (*d_distortion)[2],
                                                  uint32_t n_blocks, uint32_t w, uint32_t h, void *stream);

/* Stand-alone batched quantiser over device coefficient arrays (same descriptor; coeff_off is the INPUT). */
SVT_HIP_API int32_t svt_hip_quantize_batch(uint8_t *d_base, const SvtHipTxfmDesc *d_desc, SvtHipTxfmResult *d_result,
                                           uint32_t n_blocks, uint32_t n_coeffs, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tier B — coefficient rate of transform blocks: svt_av1_cost_coeffs_txb (rd_cost.c:434-559) as mode decision reaches it
 * through svt_aom_txb_estimate_coeff_bits (rd_cost.c:1405-1450) with allow_update_cdf = 0, and the cost tx_type_search forms
 * from it (product_coding_loop.c:4737-4786).  Run after svt_hip_txfm_quant_batch and svt_hip_txfm_distortion_batch on the
 * same stream, it completes cost = RDCOST(lambda, bits, dist) of every candidate on the device.  No Tier A leaf: one PCIe
 * round trip per transform block would cost more than the table look-ups it replaces.
 * ------------------------------------------------------------------------------------------- */
/* LvMapCoeffCost (md_rate_estimation.h:41-49), field for field: txb_skip_cost, base_eob_cost, base_cost, eob_extra_cost,
 * dc_sign_cost, lps_cost.  eob_extra holds the first 9 rows of eob_extra_cost (the reference declares EOB_COEF_CONTEXTS = 22
 * rows, get_eob_cost reaches rows eob_pt - 3 = 0 .. 8); every other array has the reference's dimensions. */
typedef struct SvtHipCoeffCost {
    int32_t txb_skip[13][2];
    int32_t base_eob[4][3];
    int32_t base[42][8];
    int32_t eob_extra[9][2];
    int32_t dc_sign[3][2];
    int32_t lps[21][26];
} SvtHipCoeffCost;

/* One set of rate tables (one picture, or one CDF state); the caller copies four fields of MdRateEstimationContext
 * (md_rate_estimation.h:127-133), each array with the reference's own dimensions:
 *   coeff[txs_ctx][plane]             = coeff_fac_bits[txs_ctx][plane], array by array
 *   eob[size][plane][ctx][pt]         = eob_frac_bits[size][plane].eob_cost[ctx][pt]
 *   intra_tx_type[set][sq][dir][type] = intra_tx_type_fac_bits
 *   inter_tx_type[set][sq][type]      = inter_tx_type_fac_bits */
typedef struct SvtHipRateTables {
    SvtHipCoeffCost coeff[5][2];
    int32_t         eob[7][2][2][11];
    int32_t         intra_tx_type[3][4][13][17];
    int32_t         inter_tx_type[4][4][17];
} SvtHipRateTables;

enum { /* SvtHipTxbCostDesc::est_mode: which of the three rates of product_coding_loop.c:4757-4782 a block gets */
    SVT_HIP_TXB_COST_EXACT = 0,    /* coeff_rate_est_lvl 1: always svt_av1_cost_coeffs_txb */
    SVT_HIP_TXB_COST_SHORT_SMALL,  /* coeff_rate_est_lvl >= 2: bits = 6000 + 1000 * eob when eob < (w * h) >> 6, else exact */
    SVT_HIP_TXB_COST_SHORT_ALL     /* coeff_rate_est_lvl 0: the same, and bits = 3000 + 100 * eob for every other eob */
};
enum { /* SvtHipTxbCostDesc::flags */
    SVT_HIP_TXB_COST_NO_SHIFT = 1  /* bits of a non-zero eob are not shifted by subres_step (c_start still depends on it): what
                                    * svt_aom_txb_estimate_coeff_bits does for the two chroma blocks (rd_cost.c:1455-1500) */
};

typedef struct SvtHipTxbCostDesc {
    uint64_t qcoeff_off;           /* int32 qcoeff[n], n = min(w,32) * min(h,32): the quantiser's output in the arena */
    uint64_t iscan_off;            /* int16 iscan[n], the table the quantiser descriptor carries; iscan[0] is 0 in every AV1 scan */
    uint32_t table;                /* index into d_tables (clamped to n_tables - 1) */
    uint32_t lambda;               /* full_lambda of the block; enters rd_cost only */
    uint16_t eob;                  /* ignored when d_txfm_result is given */
    uint8_t  tx_type;              /* TxType, 0 .. 15 */
    uint8_t  plane_type;           /* 0 luma (pays the transform-type rate), 1 chroma */
    uint8_t  txb_skip_ctx;         /* 0 .. 12 */
    uint8_t  dc_sign_ctx;          /* 0 .. 2 */
    uint8_t  pred_mode;            /* PredictionMode of the candidate: 0 .. 12 intra, 13 .. 24 inter (is_inter_mode) */
    uint8_t  filter_intra_mode;    /* 0 .. 4, or 5 (FILTER_INTRA_MODES) for none */
    uint8_t  reduced_tx_set;       /* frm_hdr->reduced_tx_set */
    uint8_t  fast_coeff_est_level; /* ctx->mds_fast_coeff_est_level */
    uint8_t  subres_step;          /* ctx->mds_subres_step */
    uint8_t  est_mode;             /* SVT_HIP_TXB_COST_EXACT ... */
    uint8_t  flags;
    uint8_t  pad_[3];
} SvtHipTxbCostDesc;

typedef struct SvtHipTxbCost {
    uint64_t bits;
    uint64_t rd_cost;
} SvtHipTxbCost;

/* d_out[i] for n_blocks transform blocks of ONE size w x h (any of the 19 transform sizes).
 *   eob == 0:  bits = txb_skip[txb_skip_ctx][1], not shifted (av1_cost_skip_txb, rd_cost.c:1447).
 *   eob  > 0:  bits = svt_av1_cost_coeffs_txb(...) << subres_step (rd_cost.c:1433-1445): txb_skip[ctx][0] + the transform-type rate (luma only)
 *              + the eob cost + the coefficient loop, the latter over scan positions eob-1, 0 and c_start .. 1 with
 *              c_start = MIN(eob - 2, eob / MAX(1, fast_coeff_est_level - subres_step)) (rd_cost.c:408).
 *   est_mode 1, 2 replace either by the closed forms above (which are not shifted).
 * The levels that the contexts are formed from (svt_av1_txb_init_levels, get_nz_mag, get_br_ctx) come from the WHOLE
 * retained array min(w,32) x min(h,32), also from positions at or beyond eob in scan order, because that is what the
 * reference reads.  An eob above min(w,32) * min(h,32) is clamped to it; field values beyond the ranges given with the
 * descriptor are clamped into the tables, so that nothing is read out of bounds.  A zero coefficient at scan position
 * eob - 1 (the reference asserts against it and reads one entry before the row) costs base_eob[ctx][0].
 *   d_txfm_result (or NULL): eob = d_txfm_result[i].eob as svt_hip_txfm_quant_batch left it, three_quad_energy likewise.
 *   d_distortion (or NULL, then rd_cost = 0): d_distortion[i][0] is DIST_CALC_RESIDUAL of svt_hip_txfm_distortion_batch,
 *       dist    = RIGHT_SIGNED_SHIFT(d_distortion[i][0] + three_quad_energy, (MAX_TX_SCALE - tx_scale(w, h)) * 2) << subres_step
 *       rd_cost = RDCOST(lambda, bits, dist)                                                        (rd_cost.h:37)
 * Returns SVT_HIP_ERR_BAD_PARAMETER, before any device is touched, for a w x h that is no transform size, for n_tables == 0
 * and for a NULL d_desc, d_tables or d_out with n_blocks > 0; n_blocks == 0 succeeds. */
SVT_HIP_API int32_t svt_hip_txb_cost_batch(const uint8_t *d_base, const SvtHipTxbCostDesc *d_desc, const SvtHipRateTables *d_tables,
                                           uint32_t n_tables, const SvtHipTxfmResult *d_txfm_result, const uint64_t (*d_distortion)[2],
                                           SvtHipTxbCost *d_out, uint32_t n_blocks, uint32_t w, uint32_t h, void *stream);
/* The same with the placement of the two SvtHipCoeffCost tables of the launch chosen by the caller (a measuring aid):
 * 0 read through the cache, 1 staged into LDS once per workgroup.  svt_hip_txb_cost_batch uses the faster one. */
SVT_HIP_API int32_t svt_hip_txb_cost_batch_placed(const uint8_t *d_base, const SvtHipTxbCostDesc *d_desc, const SvtHipRateTables *d_tables,
                                                  uint32_t n_tables, const SvtHipTxfmResult *d_txfm_result,
                                                  const uint64_t (*d_distortion)[2], SvtHipTxbCost *d_out, uint32_t n_blocks, uint32_t w,
                                                  uint32_t h, uint32_t tables_in_lds, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tier B — the RDOQ stage of the quantiser: svt_aom_quantize_inv_quantize (full_loop.c:1562-1685) from the point after its first
 * quantiser, that is the SATD gate, the eob_th / eob_fast_th decisions, svt_fast_optimize_b, svt_av1_optimize_b (:1124-1331, the
 * trellis) and svt_av1_compute_cul_level_c, with allow_update_cdf = 0.  Run after svt_hip_txfm_quant_batch on the same stream with
 * the same d_txfm_desc: that call has written coeff, qcoeff, dqcoeff (quant_mode QUANT_FP[_HBD], or the B family where the encoder
 * has fp_q_y / fp_q_uv off), eob and, with SVT_HIP_TX_SATD, satd.  No Tier A leaf, for the reason the rate has none.
 *
 * The five launches of one transform-type search, all on one stream:
 *   svt_hip_txfm_quant_batch (FWD + QUANT_FP[_HBD] + SATD, result array A) -> svt_hip_rdoq_batch (A) ->
 *   svt_hip_txfm_quant_batch (quant_mode NONE, flags TX_INV: reads dqcoeff_off; result array B) ->
 *   svt_hip_txfm_distortion_batch -> svt_hip_txb_cost_batch (A).
 * The INV-only pass writes eob = 0 into the result array it is given, so it gets a second array B; A keeps the trellis's eob
 * for the rate.
 * svt_hip_txt_search_batch (the transform-type search, below) enqueues this chain and the decision behind it in one call.
 * ------------------------------------------------------------------------------------------- */
enum { /* SvtHipRdoqDesc::flags */
    SVT_HIP_RDOQ_PERFORM   = 1, /* the host-known part of perform_rdoq: (!mds_skip_rdoq || is_encode_pass) && rdoq_level, and for
                                 * mode decision !(dct_dct_only && tx_type != DCT_DCT) && !(skip_uv && chroma) */
    SVT_HIP_RDOQ_FAST_MODE = 2, /* fast_mode of svt_av1_optimize_b: the eob_fast_{y,uv}_{inter,intra} control of the block */
    SVT_HIP_RDOQ_SHARPNESS = 4  /* use_sharpness && delta_q_present && luma && sb qindex below the picture's: rweight 0, sharpness 1 */
};
enum { /* SvtHipRdoqResult::path: the low three bits say which way the block went, the others what happened on the way */
    SVT_HIP_RDOQ_PATH_NOT_FLAGGED = 0, /* no SVT_HIP_RDOQ_PERFORM: arrays and eob untouched */
    SVT_HIP_RDOQ_PATH_EOB_ZERO,        /* eob 0 on entry, or after svt_fast_optimize_b (then with SVT_HIP_RDOQ_PATH_FAST_TRIM) */
    SVT_HIP_RDOQ_PATH_REQUANT_SATD,    /* the SATD gate refused the trellis: quantised with the quantize_b family */
    SVT_HIP_RDOQ_PATH_REQUANT_EOB,     /* eob_perc >= eob_th: quantised with the quantize_b family */
    SVT_HIP_RDOQ_PATH_EARLY_EXIT,      /* the early exit of svt_av1_optimize_b */
    SVT_HIP_RDOQ_PATH_TRELLIS,         /* svt_av1_optimize_b ran */
    SVT_HIP_RDOQ_PATH_MASK      = 7,
    SVT_HIP_RDOQ_PATH_FAST_TRIM = 8,   /* update_coeff_eob_fast ran (eob_fast_th, fast_mode or both) */
    SVT_HIP_RDOQ_PATH_SKIP      = 16,  /* update_skip chose the all-zero block */
    SVT_HIP_RDOQ_PATH_BAD_EOB   = 32   /* qcoeff[scan[eob - 1]] was zero where the trellis would start: see below */
};

typedef struct SvtHipRdoqDesc {
    uint32_t table;                 /* index into d_tables (clamped to n_tables - 1) */
    uint32_t lambda;                /* the lambda svt_aom_quantize_inv_quantize is given */
    int16_t  zbin[2], round[2], quant[2], quant_shift[2]; /* [0] DC, [1] AC of the quantize_b family (zbin_qtx, round_qtx,
                                                           * quant_qtx, quant_shift_qtx), read only where a block is re-quantised */
    uint32_t early_exit_limit;      /* sq_size_idx * rdoq_ctrls.early_exit_th, sq_size_idx = 7 - log2(blk_geom->sq_size) */
    uint8_t  plane_type;            /* 0 luma, 1 chroma */
    uint8_t  txb_skip_ctx;          /* 0 .. 12 */
    uint8_t  dc_sign_ctx;           /* 0 .. 2 */
    uint8_t  is_inter;              /* pred_mode >= NEARESTMV */
    uint8_t  eob_th, eob_fast_th;   /* rdoq_ctrls, percent of w * h; 255 = never */
    uint8_t  satd_factor;           /* rdoq_ctrls.satd_factor; 255 = no SATD gate */
    uint8_t  dequant_shift;         /* hbd_md ? bit depth of the picture - 5 : 3 */
    uint8_t  flags;                 /* SVT_HIP_RDOQ_* */
    uint8_t  pic_bit_depth;         /* bit depth of the picture (enhanced_pic->bit_depth), which the SATD gate scales by whatever depth
                                     * the block is quantised at; 0 = the transform descriptor's bit_depth */
    uint8_t  pad_[2];
} SvtHipRdoqDesc;

typedef struct SvtHipRdoqResult {
    uint16_t eob;       /* the final eob, also written to d_txfm_result[i].eob */
    uint8_t  cul_level; /* svt_av1_compute_cul_level_c of the final arrays (a caller with update_skip_ctx_dc_sign_ctx off ignores it) */
    uint8_t  path;      /* SVT_HIP_RDOQ_PATH_* */
} SvtHipRdoqResult;

/* n_blocks transform blocks of ONE size w x h (any of the 19 transform sizes).  Of d_txfm_desc[i] the call reads coeff_off (input),
 * qcoeff_off / dqcoeff_off (updated in place), iscan_off, qm_off, iqm_off, dequant, tx_type, bit_depth, quant_mode and log_scale;
 * of d_txfm_result[i] eob (in and out) and satd (in; it is svt_aom_satd over the retained coefficients).  three_quad_energy and satd are never written.  Per block:
 *   not SVT_HIP_RDOQ_PERFORM:  nothing but cul_level.
 *   satd_factor != 255 and (satd >> ..) > satd_factor * (dequant[1] >> dequant_shift) * sqrt_tx_pixels_2d (full_loop.c:1574-1584),
 *   or eob * 100 / (w * h) >= eob_th (:1630-1658):  coeff is quantised again with svt_aom_quantize_b / svt_aom_highbd_quantize_b
 *       (qm / iqm included; the high-bit-depth form behind QUANT_FP_HBD) from this descriptor's zbin / round / quant / quant_shift;
 *       a block whose quant_mode is already of the B family is left as it is.
 *   eob * 100 / (w * h) >= eob_fast_th:  svt_fast_optimize_b.
 *   then svt_av1_optimize_b, all of it.
 * An eob above min(w,32) * min(h,32) is clamped to it; descriptor fields beyond their ranges are clamped into the tables.  The
 * reference asserts qcoeff[scan[eob - 1]] != 0 where the trellis starts and the project's quantisers guarantee it; a block that
 * breaks it keeps its arrays and eob, gets cul_level and path = PATH_TRELLIS | PATH_BAD_EOB, and nothing is read or written
 * out of bounds.  iscan must hold values below min(w,32) * min(h,32); larger ones are reduced modulo that count.
 * Returns SVT_HIP_ERR_BAD_PARAMETER, before any device is touched, for a w x h that is no transform size, for n_tables == 0 and for
 * a NULL d_base, d_txfm_desc, d_desc, d_tables, d_txfm_result or d_out with n_blocks > 0; n_blocks == 0 succeeds. */
SVT_HIP_API int32_t svt_hip_rdoq_batch(uint8_t *d_base, const SvtHipTxfmDesc *d_txfm_desc, const SvtHipRdoqDesc *d_desc,
                                       const SvtHipRateTables *d_tables, uint32_t n_tables, SvtHipTxfmResult *d_txfm_result /* eob in/out, satd in */,
                                       SvtHipRdoqResult *d_out, uint32_t n_blocks, uint32_t w, uint32_t h, void *stream);
/* The same with the work split chosen by the caller (a measuring aid): 0 a lane group per block, the block's walking lane goes on
 * through update_coeff_simple in scan order; 1 a lane group per block, its lanes take one anti-diagonal per round; 2 one lane per
 * block, which exists up to 128 retained coefficients (SVT_HIP_ERR_BAD_PARAMETER above, and for any other value).  All leave the same
 * arrays; svt_hip_rdoq_batch uses the fastest one of each size. */
SVT_HIP_API int32_t svt_hip_rdoq_batch_mapped(uint8_t *d_base, const SvtHipTxfmDesc *d_txfm_desc, const SvtHipRdoqDesc *d_desc,
                                              const SvtHipRateTables *d_tables, uint32_t n_tables, SvtHipTxfmResult *d_txfm_result,
                                              SvtHipRdoqResult *d_out, uint32_t n_blocks, uint32_t w, uint32_t h, uint32_t mapping, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tier B — the transform-type search of a transform block: tx_type_search (product_coding_loop.c:4458-4940), all of it on the
 * device.  The five launches above leave one set of records per CANDIDATE (one transform type of one transform block); the calls
 * below add the spatial distortion of :4697-4718, replay the loop's decision (:4581-4812) per block, gather the winner's arrays and
 * leave ONE record per transform block.  No Tier A leaf, for the reason the rate has none.
 *
 * Out of scope (the caller keeps such blocks on the host): mds_subres_step != 0 (the inverse then runs at another size than the
 * forward transform), tx_search_skip_flag, tune_ssim_level > 0 (the SSIM pass of :4815-4911), chroma, and the encoder-side hook.
 * ------------------------------------------------------------------------------------------- */
/* Where the source pixels of one candidate lie (svt_hip_txfm_spatial_distortion_batch) */
typedef struct SvtHipSpatialSrc {
    uint64_t src_off;        /* source pixels: uint8, or uint16 where the candidate's descriptor has SVT_HIP_TX_PIXEL16 */
    uint32_t src_stride;     /* in pixels */
    uint8_t  crop_w, crop_h; /* cropped_tx_width / cropped_tx_height, 1 .. w and 1 .. h; 0 or more than the side = the whole side */
    uint8_t  pad_[2];
} SvtHipSpatialSrc;

/* d_distortion[i] = {DIST_CALC_RESIDUAL = sum (src - recon)^2, DIST_CALC_PREDICTION = sum (src - pred)^2} << 4 over the top-left
 * crop_w x crop_h pixels of candidate i: svt_spatial_full_distortion_kernel, or svt_full_distortion_kernel16_bits with
 * SVT_HIP_TX_PIXEL16, as product_coding_loop.c:4697-4718 calls them.  pred_off / recon_off, their strides and the flag come from
 * d_desc[i]; run it behind the pass that wrote recon_off.  A candidate without pred_off or recon_off gets {0, 0}.  Any stride and
 * any offset that is a multiple of the pixel size will do.
 * Returns SVT_HIP_ERR_BAD_PARAMETER, before any device is touched, for a w x h that is no transform size and for a NULL pointer with
 * n_blocks > 0; n_blocks == 0 succeeds. */
SVT_HIP_API int32_t svt_hip_txfm_spatial_distortion_batch(const uint8_t *d_base, const SvtHipTxfmDesc *d_desc, const SvtHipSpatialSrc *d_src,
                                                          uint64_t (*d_distortion)[2], uint32_t n_blocks, uint32_t w, uint32_t h, void *stream);

#define SVT_HIP_TXT_MAX_CAND 16 /* TX_TYPES */
enum { /* SvtHipTxtDesc::flags */
    SVT_HIP_TXT_EARLY_EXIT  = 1, /* ssim_level <= SSIM_LVL_1 && !only_dct_dct: the coefficient-count / cost exit of :4798-4811 */
    SVT_HIP_TXT_SPATIAL_SSE = 2  /* mds_spatial_sse || (!is_inter && tx_depth): the distortion is the spatial one */
};
enum { /* flags of svt_hip_txt_search_batch */
    SVT_HIP_TXT_SEARCH_INVERSE = 1 /* some block has SVT_HIP_TXT_SPATIAL_SSE or a recon destination: run the inverse-only pass and the
                                    * spatial distortion.  The block descriptors live on the device, so the call cannot derive this: the
                                    * caller, who filled them, MUST set it whenever any block has SVT_HIP_TXT_SPATIAL_SSE.  Without it the
                                    * call has neither spatial sums nor reconstructions: every block is decided as if SVT_HIP_TXT_SPATIAL_SSE
                                    * were clear, on the transform-domain distortion, and dst_recon_off is skipped. */
};

/* What the host knows of one transform block before the loop.  Its candidates are the n_cand consecutive entries from first_cand of
 * the per-candidate arrays, in the reference's loop order: after tx_type_group[_sc], only_dct_dct and av1_ext_tx_used have been
 * applied.  A candidate's transform type is the tx_type of its SvtHipTxbCostDesc. */
typedef struct SvtHipTxtDesc {
    uint64_t src_off;             /* source pixels of the block (SVT_HIP_TXT_SPATIAL_SSE) */
    uint64_t dst_qcoeff_off, dst_dqcoeff_off; /* int32 [n] each: where the winner's arrays go; SVT_HIP_NO_OFFSET skips one */
    uint64_t dst_recon_off;       /* the winner's w x h reconstruction, pixel type of the winner's descriptor; SVT_HIP_NO_OFFSET skips it */
    uint32_t first_cand;
    uint32_t src_stride, dst_recon_stride; /* in pixels */
    uint32_t full_lambda;
    uint32_t early_exit_coeff_th, early_exit_dist_th; /* txt_ctrls */
    uint32_t tx_pixels;           /* blk_geom->tx_width[tx_depth] * blk_geom->tx_height[tx_depth] */
    uint16_t satd_early_exit_th;  /* already q-weighted as at :4533-4541; 0 = no SATD test */
    uint16_t txt_rate_cost_th;    /* txt_ctrls.txt_rate_cost_th; 0 = none */
    uint16_t group_start;         /* bit k: candidate k is the first of a transform-type group (best_tx_non_coeff = 64 * 64) */
    uint8_t  n_cand;              /* 1 .. SVT_HIP_TXT_MAX_CAND; more are clamped */
    uint8_t  flags;               /* SVT_HIP_TXT_* */
    uint8_t  crop_w, crop_h;      /* as SvtHipSpatialSrc */
    uint8_t  pad_[2];
} SvtHipTxtDesc;

typedef struct SvtHipTxtResult {
    uint64_t bits;          /* y_txb_coeff_bits_txt[best_tx_type] */
    uint64_t distortion[2]; /* txb_full_distortion_txt[DIST_SSD][best_tx_type][DIST_CALC_RESIDUAL, DIST_CALC_PREDICTION] */
    uint64_t cost;          /* best_cost_tx_search (~0 where no candidate reached the comparison) */
    uint16_t eob;
    uint16_t quant_mask;    /* bit k: the reference would have run the quantiser of candidate k (it passed the rate-cost and SATD tests) */
    uint16_t cost_mask;     /* bit k: candidate k reached the cost comparison */
    uint8_t  tx_type;       /* best_tx_type */
    uint8_t  cand;          /* the winner's index within the block, 0xFF if no candidate reached the comparison */
    uint8_t  cul_level;     /* the winner's SvtHipRdoqResult::cul_level (0 without RDOQ results) */
    uint8_t  pad_[7];
} SvtHipTxtResult;

/* The decision for n_blocks transform blocks of ONE size w x h over the records of n_cand candidates: d_txfm_result (array A of the
 * chain: eob, satd, three_quad_energy), d_rdoq_result (or NULL), d_distortion and d_cost (its bits).  Per block, candidates in order,
 * from best_cost = dct_cost = ~0, best_satd = INT_MAX, best_tx_type = DCT_DCT (tx_type, txt_rate = the transform-type rate
 * svt_hip_txb_cost_batch charges the candidate: av1_txt_rate_est, 0 where the set has one type):
 *     if the group starts here: best_non_coeff = 64 * 64
 *     if tx_type != DCT_DCT && txt_rate_cost_th && (uint64_t)RDCOST(lambda, txt_rate, 0) * 1000 > dct_cost * txt_rate_cost_th: continue
 *     if satd_early_exit_th: satd < best_satd ? best_satd = satd : if (satd - best_satd) * 100 > best_satd * satd_early_exit_th: continue
 *     (quant_mask)  if eob == 0 && tx_type != DCT_DCT: continue
 *     if (uint64_t)RDCOST(lambda, 0, dist[RESIDUAL]) > best_cost: continue
 *     (cost_mask)  cost = RDCOST(lambda, bits, dist[RESIDUAL]); if cost < best_cost: this is the best; DCT_DCT also sets dct_cost
 *     with SVT_HIP_TXT_EARLY_EXIT: if best_non_coeff < early_exit_coeff_th || best_cost < (early_exit_dist_th ?
 *                                     RDCOST(lambda, 1, tx_pixels * early_exit_dist_th) : 0): the search ends
 * in the reference's integer types (the uint64_t products wrap as in C, the SATD test is int).  Ties keep the earlier candidate.
 * dist is d_distortion[i] itself with SVT_HIP_TXT_SPATIAL_SSE, else RIGHT_SIGNED_SHIFT(d_distortion[i] + three_quad_energy,
 * (MAX_TX_SCALE - tx_scale) * 2) << min(subres_step, 2) for both entries, the residual figure svt_hip_txb_cost_batch forms.
 * Where no candidate reaches the comparison the record is the reference's zero-initialised locals with DCT_DCT, and nothing is copied.
 * Then the winner's qcoeff, dqcoeff (n = min(w,32) * min(h,32) int32 each) and w x h reconstruction (recon_off / recon_stride of its
 * SvtHipTxfmDesc) are copied to the block's destinations; nothing is copied where a destination is the winner's own array (the
 * reference's DCT_DCT case).  first_cand + n_cand beyond n_cand_total is cut at it; table and context fields are clamped as in
 * svt_hip_txb_cost_batch.  Arena offsets are the caller's, as everywhere in this header.
 * Returns SVT_HIP_ERR_BAD_PARAMETER, before any device is touched, for a w x h that is no transform size, for n_tables == 0 and for
 * a NULL pointer other than d_rdoq_result with n_blocks > 0; n_blocks == 0 succeeds. */
SVT_HIP_API int32_t svt_hip_txt_select_batch(uint8_t *d_base, const SvtHipTxtDesc *d_desc, const SvtHipTxfmDesc *d_txfm_desc,
                                             const SvtHipTxbCostDesc *d_cost_desc, const SvtHipRateTables *d_tables, uint32_t n_tables,
                                             const SvtHipTxfmResult *d_txfm_result, const SvtHipRdoqResult *d_rdoq_result,
                                             const uint64_t (*d_distortion)[2], const SvtHipTxbCost *d_cost, SvtHipTxtResult *d_out,
                                             uint32_t n_cand_total, uint32_t n_blocks, uint32_t w, uint32_t h, void *stream);
/* The same with the work split chosen by the caller (a measuring aid): 0 one lane per block replays the loop, then the wavefront copies
 * the winners of its 64 blocks one after the other; 1 the replay in one kernel and the copies in a second one, a wavefront per block.
 * Both leave the same bytes; svt_hip_txt_select_batch uses the faster one.  Any other value is SVT_HIP_ERR_BAD_PARAMETER. */
SVT_HIP_API int32_t svt_hip_txt_select_batch_mapped(uint8_t *d_base, const SvtHipTxtDesc *d_desc, const SvtHipTxfmDesc *d_txfm_desc,
                                                    const SvtHipTxbCostDesc *d_cost_desc, const SvtHipRateTables *d_tables, uint32_t n_tables,
                                                    const SvtHipTxfmResult *d_txfm_result, const SvtHipRdoqResult *d_rdoq_result,
                                                    const uint64_t (*d_distortion)[2], const SvtHipTxbCost *d_cost, SvtHipTxtResult *d_out,
                                                    uint32_t n_cand_total, uint32_t n_blocks, uint32_t w, uint32_t h, uint32_t mapping,
                                                    void *stream);

/* Bytes of scratch svt_hip_txt_search_batch needs for n_cand candidates of n_blocks blocks (host arithmetic only) */
SVT_HIP_API size_t svt_hip_txt_search_scratch_bytes(uint32_t n_cand, uint32_t n_blocks);

/* The whole search of n_blocks transform blocks of ONE size w x h with n_cand candidates in all, enqueued on one stream:
 *   1. svt_hip_txfm_quant_batch over d_txfm_desc (the caller sets FWD, a quantiser and SATD)
 *   2. svt_hip_rdoq_batch where d_rdoq_desc is given
 *   3. with SVT_HIP_TXT_SEARCH_INVERSE the inverse-only pass over the SAME descriptors: it reads dqcoeff_off and writes recon_off of
 *      every candidate that has dqcoeff_off, pred_off and recon_off, as quant_mode NONE / flags TX_INV would; its results go to an
 *      array of its own in the scratch
 *   4. svt_hip_txfm_distortion_batch, and with SVT_HIP_TXT_SEARCH_INVERSE (only then) the spatial distortion for the candidates of
 *      blocks with SVT_HIP_TXT_SPATIAL_SSE
 *   5. svt_hip_txb_cost_batch
 *   6. svt_hip_txt_select_batch into d_out[n_blocks]; without SVT_HIP_TXT_SEARCH_INVERSE it takes SVT_HIP_TXT_SPATIAL_SSE as clear and
 *      dst_recon_off as SVT_HIP_NO_OFFSET in every block
 * The per-candidate records live in d_scratch (caller-owned, svt_hip_txt_search_scratch_bytes; 16-byte aligned) and may be reused by
 * the next call on the same stream.  d_out is all a caller has to download.
 * Returns SVT_HIP_ERR_BAD_PARAMETER, before any device is touched, for a w x h that is no transform size, for n_tables == 0, for a
 * scratch smaller than svt_hip_txt_search_scratch_bytes(n_cand, n_blocks) and for a NULL pointer other than d_rdoq_desc with
 * n_blocks > 0; n_blocks == 0 succeeds. */
SVT_HIP_API int32_t svt_hip_txt_search_batch(uint8_t *d_base, const SvtHipTxfmDesc *d_txfm_desc, const SvtHipRdoqDesc *d_rdoq_desc,
                                             const SvtHipTxbCostDesc *d_cost_desc, const SvtHipRateTables *d_tables, uint32_t n_tables,
                                             const SvtHipTxtDesc *d_desc, void *d_scratch, size_t scratch_bytes, SvtHipTxtResult *d_out,
                                             uint32_t n_cand, uint32_t n_blocks, uint32_t w, uint32_t h, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_TXFM_H */
