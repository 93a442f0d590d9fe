/*
 * svt_hip_intra.h — C-ABI for the open-loop intra search of TPL level 1 (presets M0 - M4): the source-based intra search of every
 * 16x16 block of one or more pictures over the intra modes DC_PRED .. intra_mode_end, with SAD or SATD cost.
 *
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
 * Not provided: the rest of TPL level 1 (SATD in the inter source search, the quarter-pel tree without diagonal refinement, the rate
 * estimate), subsample_tx != 0, 10-bit input, 32x32 / 64x64 blocks, angle deltas, CfL, filter-intra.
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

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_INTRA_H */
