/*
 * svt_hip_intra.h — C-ABI for intra prediction: (1) the open-loop intra search of TPL level 1 (presets M0 - M4), (2) the AV1 intra
 * predictor of any transform-block size as mode decision and EncDec call it, with the smooth inter-intra combination, and (3) CfL.
 *
 * (1) svt_hip_intra_search_frames: the source-based intra search of every 16x16 block of one or more pictures over the intra modes
 * DC_PRED .. intra_mode_end, with SAD or SATD cost.
 * Reference interface replaced (paths relative to the reference's Source/Lib):
 *   Codec/src_ops_process.c:519-760   the intra part of the source-based path of tpl_mc_flow_dispenser_sb_generic at
 *                                     dispenser_search_level 0 (16x16 blocks, TX_16X16) with in_loop_ois = 1, when the fast
 *                                     DC-only SAD path does not apply (use_sad_in_src_search == 0 or intra_mode_end > DC_PRED)
 * Per block at (x, y) of the 16x16 raster, searched when x + 8 <= width && y + 8 <= height (at least half inside):
 *   svt_aom_update_neighbor_samples_array_open_loop_mb(1, 1, ...) on the SOURCE picture; then for mode = DC_PRED .. intra_mode_end:
 *   directional modes other than V / H get a filtered copy of the edges (filter_intra_edge with max_input_luma_width / _height),
 *   svt_aom_intra_prediction_open_loop_mb (no angle deltas), cost = svt_nxm_sad_kernel_sub_sampled (the plain 16x16 SAD) or
 *   svt_aom_subtract_block -> svt_av1_wht_fwd_txfm (DCT_DCT 16x16, pf_shape) -> svt_aom_satd; the first strict minimum wins.
 * A searched block may reach 8 samples past the right / bottom edge of the picture: its cost then reads the source padding.
 * All pictures of one call are searched in one launch (one wavefront per block).
 * Not provided by the search: the rest of TPL level 1 (SATD in the inter source search, the quarter-pel tree without diagonal
 * refinement, the rate estimate), subsample_tx != 0, 10-bit input, other block sizes, angle deltas.
 *
 * (2) svt_hip_intra_predict_batch: one descriptor = one transform block of one plane, device-resident (Tier B).
 * Reference interface replaced:
 *   Codec/enc_intra_prediction.c:60-435   build_intra_predictors / build_intra_predictors_high, behind svt_av1_predict_intra_block
 *                                     and svt_av1_predict_intra_block_16bit: the need_* rules, the early-return fill, copy /
 *                                     replication / fall-backs of the edges, filter_intra_edge_corner[_high],
 *                                     svt_aom_intra_edge_filter_strength, svt_av1_filter_intra_edge[_high]_c,
 *                                     svt_aom_use_intra_edge_upsample, svt_av1_upsample_intra_edge[_high]_c, svt_aom_dr_predictor /
 *                                     svt_aom_highbd_dr_predictor (z1 / z2 / z3, both upsampling flags), the DC family, V, H, the
 *                                     SMOOTH modes, PAETH, svt_av1_filter_intra_predictor_c / svt_aom_highbd_filter_intra_predictor
 *   Codec/inter_prediction.c:2128-2214, 2341-2372   svt_aom_combine_interintra[_highbd] with use_wedge_interintra == 0 as an optional
 *                                     epilogue: the smooth mask and the unblended intra prediction never reach memory.  The
 *                                     wedge form needs no code of its own: predict into a buffer with this call, then blend it
 *                                     with the inter prediction by a SVT_HIP_BLEND_MASK descriptor (src0 = the intra prediction,
 *                                     mask = the wedge mask) of svt_hip_blend_batch in a later call on the same stream.
 * (3) svt_hip_cfl_predict_batch: one descriptor = one chroma block of one plane for one alpha (4:2:0).
 *   Codec/intra_prediction.c:420-465, C_DEFAULT/cfl_c.c   svt_cfl_luma_subsampling_420_{lbd,hbd}_c, svt_subtract_average_c,
 *                                     svt_cfl_predict_{lbd,hbd}_c as compute_cfl_ac_components (product_coding_loop.c:3615-3650)
 *                                     and the alpha search call them.
 * Neither is an RTCD leaf: a leaf would put a round trip over the bus behind every intra call of the encoder.
 * (4) - (6), further down: the luma palette (search with its rate terms, prediction) and the screen-content decision.
 * Not provided: intra block copy, chroma palettes, the 4:4:4 and 4:2:2 CfL sub-sampling, the derivation of the availability
 * counts (svt_aom_intra_has_top_right / _bottom_left, tile and frame edges: control logic of the caller), and the caller that keeps
 * mode decision's candidates on the device.
 */
#ifndef SVT_HIP_INTRA_H
#define SVT_HIP_INTRA_H

#include "svt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_HIP_INTRA_MODES 13 /* DC_PRED .. PAETH_PRED */

typedef struct SvtHipIntraCtrls { /* the fields of TplControls / SequenceControlSet the search reads */
    uint8_t  intra_mode_end; /* last mode searched: 0 DC_PRED .. 12 PAETH_PRED (PredictionMode order) */
    uint8_t  use_sad;        /* use_sad_in_src_search: 1 SAD, 0 SATD */
    uint8_t  pf_shape;       /* coefficient shape of the SATD transform: 0 DEFAULT_SHAPE, 1 N2_SHAPE, 2 N4_SHAPE */
    uint8_t  subsample_tx;   /* only 0 is accepted (the 16x16 blocks of dispenser_search_level 0) */
    uint16_t max_input_luma_width, max_input_luma_height; /* scs->max_input_luma_*: bound the edge filter (filter_intra_edge) */
} SvtHipIntraCtrls;

/* One picture.  Every pointer is device memory.  Outputs are [rows][cols] with cols = ceil(width / 16), rows = ceil(height / 16), in
 * raster order of the 16x16 cells; a cell whose block is not searched gets best_mode 0xFF, best_cost INT64_MAX and INT64_MAX in all
 * its mode_cost entries.  mode_cost entries of modes after intra_mode_end are INT64_MAX; pred entries of those modes and of cells
 * that are not searched are left as they are. */
typedef struct SvtHipIntraSearchJob {
    SvtHipPlane8     src;        /* source luma.  stride >= org_x + ceil16(width); rows down to org_y + ceil16(height) must exist */
    SvtHipIntraCtrls ctrls;
    uint8_t         *best_mode;  /* [rows][cols]: best PredictionMode */
    int64_t         *best_cost;  /* [rows][cols]: its SAD / SATD */
    int64_t         *mode_cost;  /* optional (NULL): [rows][cols][SVT_HIP_INTRA_MODES], the cost of every mode */
    uint8_t         *pred;       /* optional (NULL): [rows][cols][SVT_HIP_INTRA_MODES][16 * 16], every mode's prediction */
} SvtHipIntraSearchJob;

/* `jobs` is a HOST array of n (1 .. 65535) pictures.  Asynchronous on `stream`.  Every job is validated before anything is launched:
 * SVT_HIP_ERR_BAD_PARAMETER (with svt_hip_last_error set) for ctrls out of range, subsample_tx != 0, a NULL source or required
 * output, an empty picture or a stride that cannot hold org_x + ceil16(width). */
SVT_HIP_API int32_t svt_hip_intra_search_frames(const SvtHipIntraSearchJob *jobs, uint32_t n, void *stream);

/* ---- Intra prediction of one transform block (Tier B) ------------------------------------------------------------------
 * The arguments of build_intra_predictors[_high], flat.  Every pointer is device memory; samples are uint8, or uint16 with
 * is_16bit.  Descriptors live in device memory, so the host cannot validate them: the kernel SKIPS a descriptor (dst keeps every
 * byte) whose fields are out of the ranges given here, or whose uint16 pointers are odd.  Exactly the w x h rectangle of dst is
 * written.  No descriptor of a call may read (above, left, inter) what another descriptor of the same call writes; `inter` may be
 * `dst` itself (with its stride). */
#define SVT_HIP_FILTER_INTRA_NONE 5 /* FILTER_INTRA_MODES: no filter-intra */

typedef struct SvtHipIntraPredDesc {
    const void *above;       /* sample [0] of the row above the block; [-1] is the top-left sample, read only when n_top_px > 0 and
                              * n_left_px > 0.  n_top_px (+ n_topright_px for modes that look right) samples are read.  May be
                              * NULL when n_top_px == 0 */
    const void *left;        /* the sample left of row 0; row i is at left[i * left_stride].  n_left_px (+ n_bottomleft_px)
                              * samples are read.  May be NULL when n_left_px == 0 */
    void       *dst;         /* the predicted block */
    const void *inter;       /* NULL: plain intra prediction.  Otherwise the inter prediction of the block: dst gets
                              * AOM_BLEND_A64(smooth mask of ii_mode, intra, inter) */
    uint32_t    left_stride; /* in samples: 1 for a neighbour array, the plane's stride for a reconstructed picture */
    uint32_t    dst_stride, inter_stride; /* in samples */
    uint8_t     w, h;        /* tx_size_wide / tx_size_high: one of the 19 transform shapes, 4 .. 64 each, 1:1, 1:2, 1:4 */
    uint8_t     mode;        /* PredictionMode 0 DC_PRED .. 12 PAETH_PRED */
    int8_t      angle_delta; /* -3 .. 3 for V_PRED .. D67_PRED, 0 for the others */
    uint8_t     filter_intra_mode;   /* 0 .. 4, or SVT_HIP_FILTER_INTRA_NONE; a filter mode needs mode == DC_PRED, w <= 32, h <= 32 */
    uint8_t     disable_edge_filter; /* 0 / 1 */
    uint8_t     filt_type;   /* 0 / 1: get_filt_type, i.e. whether the above or the left block is smooth (the caller knows them) */
    uint8_t     ii_mode;     /* with inter: InterIntraMode 0 II_DC_PRED, 1 II_V_PRED, 2 II_H_PRED, 3 II_SMOOTH_PRED */
    uint8_t     n_top_px, n_topright_px;   /* n_top_px <= w; n_topright_px <= w, and n_top_px == w unless it is 0 */
    uint8_t     n_left_px, n_bottomleft_px; /* n_left_px <= h; n_bottomleft_px <= h, and n_left_px == h unless it is 0 */
    uint8_t     is_16bit;    /* 0 / 1 */
    uint8_t     bit_depth;   /* 8, 10 or 12; 8 unless is_16bit */
    uint8_t     pad_[6];
} SvtHipIntraPredDesc;
/* SVT_HIP_ERR_BAD_PARAMETER when d_desc == NULL or n == 0, SVT_HIP_ERR_NO_DEVICE before svt_hip_init(); nothing is launched in
 * either case.  Asynchronous on `stream` (NULL: the calling thread's stream); n is not limited by the grid (2^20 and more). */
SVT_HIP_API int32_t svt_hip_intra_predict_batch(const SvtHipIntraPredDesc *d_desc, uint32_t n, void *stream);
/* The same with the number of descriptors that share a workgroup chosen by the caller (1, 2 or 4 wavefronts, one descriptor each;
 * svt_hip_intra_predict_batch uses 4): a tuning aid, the results do not depend on it.  Any other value is a bad parameter. */
SVT_HIP_API int32_t svt_hip_intra_predict_batch_packed(const SvtHipIntraPredDesc *d_desc, uint32_t n, uint32_t waves_per_workgroup,
                                                       void *stream);

/* ---- CfL of one chroma block (Tier B, 4:2:0) -----------------------------------------------------------------------------
 * Luma sub-sampling, average removal and the prediction for one alpha.  A descriptor derives the AC block from luma itself, so an
 * alpha search is N descriptors over the same luma block and no descriptor reads what another writes.  Skipped (dst and ac_out
 * keep every byte): NULL luma / pred / dst, w or h not 4, 8, 16 or 32, |alpha_q3| > 16, bit depth fields out of range, odd
 * uint16 pointers. */
#define SVT_HIP_CFL_BUF_LINE 32

typedef struct SvtHipCflDesc {
    const void *luma;        /* the reconstructed luma block, 2 w x 2 h samples */
    const void *pred;        /* the chroma DC prediction, w x h samples; may be dst */
    void       *dst;         /* clip(pred + ROUND_POWER_OF_TWO_SIGNED(alpha_q3 * ac, 6)) */
    int16_t    *ac_out;      /* optional (NULL): the AC block in Q3, [h][SVT_HIP_CFL_BUF_LINE], w entries of a row written */
    uint32_t    luma_stride, pred_stride, dst_stride; /* in samples */
    int8_t      alpha_q3;    /* -16 .. 16 */
    uint8_t     w, h;        /* 4, 8, 16 or 32 each */
    uint8_t     is_16bit, bit_depth; /* as SvtHipIntraPredDesc */
    uint8_t     pad_[7];
} SvtHipCflDesc;
/* Errors as svt_hip_intra_predict_batch. */
SVT_HIP_API int32_t svt_hip_cfl_predict_batch(const SvtHipCflDesc *d_desc, uint32_t n, void *stream);

/* ---- Luma palette: search, rate and prediction (Tier B), and the screen-content decision ---------------------------------
 * (4) svt_hip_palette_search_batch: one descriptor = one luma block of 8x8 .. 64x64.
 * Reference interface replaced:
 *   Codec/palette.c:309-434           search_palette_luma with everything below it: svt_av1_count_colors[_highbd],
 *                                     svt_get_palette_cache_y (palette.c:159-201), the dominant colours, svt_av1_k_means_dim1_c
 *                                     (k_means_template.h), palette_rd_y with optimize_palette_colors, av1_remove_duplicates,
 *                                     svt_av1_calc_indices_dim1 and extend_palette_color_map, and the rule that a candidate keeps
 *                                     its slot only when more than 2 colours are left
 *   Codec/rd_cost.c:691-704           the palette terms of av1_intra_fast_cost for every kept candidate: palette_ysize_fac_bits +
 *                                     svt_aom_write_uniform_cost, svt_av1_palette_color_cost_y and svt_av1_cost_color_map
 * (5) svt_hip_palette_predict_batch: the palette branch of svt_av1_predict_intra_block[_16bit]
 *     (Codec/enc_intra_prediction.c:501-510, 647-656).
 * (6) svt_hip_sc_classify: svt_aom_is_screen_content (Codec/pic_analysis_process.c:1848-1917).
 * Not provided: chroma palettes (the reference never uses them), 12 bit, the palette_ymode_fac_bits term (its context comes from
 * the neighbours' modes), svt_av1_tokenize_color_map and the CDF update, intra block copy, and the caller inside the encoder. */
/* The three status exports of this part return SVT_HIP_PALETTE_STATUS(status) as uint64_t: 0, or the SvtHipStatus zero-extended
 * (SVT_HIP_ERR_BAD_PARAMETER arrives as 0x80001005). */
#define SVT_HIP_PALETTE_STATUS(s) ((uint64_t)(uint32_t)(s))
#define SVT_HIP_PALETTE_MAX_SIZE  8  /* PALETTE_MAX_SIZE */
#define SVT_HIP_PALETTE_MAX_CANDS 14 /* what search_palette_luma can keep for one block */
#define SVT_HIP_PALETTE_DOMINANT  0  /* SvtHipPaletteCand.origin */
#define SVT_HIP_PALETTE_KMEANS    1

typedef struct SvtHipPaletteRates { /* of MdRateEstimationContext */
    int32_t palette_ysize_fac_bits[7][7]; /* the 7 sizes of each row (the reference's rows have CDF_SIZE(7) = 8 entries) */
    int32_t palette_ycolor_fac_bitss[7][5][8];
} SvtHipPaletteRates;

typedef struct SvtHipPaletteCtrls {
    const SvtHipPaletteRates *d_rates; /* device memory, 4-byte aligned: the picture's table */
    uint8_t dominant_color_step;       /* palette_ctrls.dominant_color_step: 1 or 2 */
    uint8_t bit_depth;                 /* 8: uint8 samples; 10: 10-bit samples in uint16 */
    uint8_t max_itr;                   /* 1 .. 50; the reference uses 50 */
    uint8_t pad_[5];
} SvtHipPaletteCtrls;

typedef struct SvtHipPaletteCand {
    uint8_t  origin;           /* SVT_HIP_PALETTE_DOMINANT / _KMEANS */
    uint8_t  n;                /* the n of the loop the candidate came from */
    uint8_t  palette_size;     /* 3 .. 8: after the cache snap and the removal of duplicates */
    uint8_t  pad_;
    uint16_t palette_colors[SVT_HIP_PALETTE_MAX_SIZE]; /* ascending; entries from palette_size on are 0 */
    int32_t  size_bits;        /* palette_ysize_fac_bits[bsize_ctx][palette_size - 2] + svt_aom_write_uniform_cost(palette_size, map[0]) */
    int32_t  color_bits;       /* svt_av1_palette_color_cost_y */
    int32_t  map_bits;         /* svt_av1_cost_color_map */
} SvtHipPaletteCand;

typedef struct SvtHipPaletteRecord { /* every byte of it is written; pads and unused entries are 0 */
    uint16_t          colors;  /* svt_av1_count_colors over rows x cols; 0 when a 10-bit sample is out of range, as in the reference */
    uint8_t           n_cands; /* 0 unless 1 < colors <= 64 */
    uint8_t           n_cache; /* entries of cache: svt_get_palette_cache_y */
    uint16_t          cache[2 * SVT_HIP_PALETTE_MAX_SIZE];
    uint8_t           pad_[12];
    SvtHipPaletteCand cand[SVT_HIP_PALETTE_MAX_CANDS]; /* in the reference's order */
} SvtHipPaletteRecord;

typedef struct SvtHipPaletteDesc {
    const void          *src;    /* the source luma PLANE (device): sample (org_y + r, org_x + c) is src[(org_y + r) * stride + org_x + c] */
    SvtHipPaletteRecord *record; /* device, 8-byte aligned */
    uint8_t             *maps;   /* device, 4-byte aligned, SVT_HIP_PALETTE_MAX_CANDS * width * height bytes: the colour index map of
                                  * candidate i at i * width * height, width x height (extended); maps of slots from n_cands on are
                                  * left as they are */
    uint32_t stride;             /* in samples */
    uint32_t org_x, org_y;       /* the block's origin in the plane */
    uint8_t  width, height;      /* 8, 16, 32 or 64 each, at most 1:4: the 14 block sizes of 8x8 .. 64x64 (of the 16 that
                                  * svt_aom_allow_palette admits, 4x16 and 16x4 are left out) */
    uint8_t  rows, cols;         /* inside the picture (svt_aom_get_block_dimensions): 1 .. height, 1 .. width */
    uint8_t  above_n, left_n;    /* 0 .. 8: palette_size of the neighbours; above_n = 0 on a superblock-row boundary */
    uint8_t  pad_[6];
    uint16_t above[SVT_HIP_PALETTE_MAX_SIZE], left[SVT_HIP_PALETTE_MAX_SIZE]; /* their palette_colors: ascending, below 1 << bit_depth */
} SvtHipPaletteDesc;

/* `ctrls` and `desc` are HOST memory (desc an array of n >= 1); everything they point to is device memory.  Every descriptor is
 * validated before anything is launched: SVT_HIP_PALETTE_STATUS(SVT_HIP_ERR_BAD_PARAMETER), with svt_hip_last_error naming the function and the descriptor, for
 * NULL arguments, a size other than 8 .. 64, rows / cols of 0 or beyond the block, a bit depth other than 8 or 10, a step other than
 * 1 or 2, max_itr outside 1 .. 50, neighbour palettes longer than 8 or with a colour beyond the bit depth, a misaligned record, map
 * storage or table, or an odd uint16 plane.  Asynchronous on `stream`; one workgroup per descriptor.  The same inputs give the same bytes. */
SVT_HIP_API uint64_t svt_hip_palette_search_batch(const SvtHipPaletteCtrls *ctrls, const SvtHipPaletteDesc *desc, uint32_t n, void *stream);

/* dst[r][c] = palette[map[(r + y) * map_width + c + x]] for r < h, c < w.  Descriptors live in DEVICE memory, as those of
 * svt_hip_intra_predict_batch do: the kernel SKIPS a descriptor (dst keeps every byte) with a NULL pointer, w or h of 0, x + w > map_width,
 * a bit depth other than 8 or 10 (8 unless is_16bit), or an odd uint16 dst.  A map entry is taken modulo 8. */
typedef struct SvtHipPalettePredDesc {
    const uint8_t  *map;       /* the block's colour index map, where the search left it */
    const uint16_t *colors;    /* SvtHipPaletteCand.palette_colors of the chosen candidate */
    void           *dst;
    uint32_t        dst_stride; /* in samples */
    uint16_t        map_width;  /* the block's width */
    uint8_t         x, y, w, h; /* the transform block inside the map */
    uint8_t         is_16bit;   /* 0: uint8 samples; 1: uint16, clamped to (1 << bit_depth) - 1 */
    uint8_t         bit_depth;
    uint8_t         pad_[4];
} SvtHipPalettePredDesc;
/* Errors as svt_hip_intra_predict_batch. */
SVT_HIP_API uint64_t svt_hip_palette_predict_batch(const SvtHipPalettePredDesc *d_desc, uint32_t n, void *stream);

typedef struct SvtHipScClass {
    uint32_t counts_1;      /* whole 16x16 blocks with 2 .. 4 colours */
    uint32_t counts_2;      /* those of them whose rounded per-pixel variance against 128 is > 0 */
    uint32_t blocks;        /* whole 16x16 blocks of the plane */
    uint8_t  sc_class[4];   /* sc_class0 .. sc_class3 */
    uint32_t pad_[2];
} SvtHipScClass;
/* An 8-bit luma plane in device memory; d_out (device, 4-byte aligned) is written whole.  BAD_PARAMETER for NULL, an empty plane, a
 * side beyond 16384, more than 2^31 / 50 pixels (the reference's int products) or stride < width. */
SVT_HIP_API uint64_t svt_hip_sc_classify(const uint8_t *d_plane, uint32_t width, uint32_t height, uint32_t stride, SvtHipScClass *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_INTRA_H */
