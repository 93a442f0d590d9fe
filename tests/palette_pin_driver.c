/* TEST INFRASTRUCTURE — pins the golden fixture and the Python restatement of tests/palette_cases.py against the reference's own
 * functions (oracle/_ref/libsvtref.so):
 *   search_palette_luma (palette.c:309-434) on zeroed, fabricated PictureControlSet / PictureParentControlSet / SequenceControlSet /
 *     ModeDecisionContext / BlkStruct / MacroBlockD objects that carry only what it reads; then, per candidate it kept,
 *     svt_av1_cost_color_map, svt_av1_palette_color_cost_y and the two size terms of rd_cost.c:691-693
 *   svt_get_palette_cache_y on the same MacroBlockD
 *   svt_av1_k_means_dim1_c directly: only this call takes a max_itr other than 50
 *   svt_aom_is_screen_content on a fabricated PictureParentControlSet
 *   the rate table svt_aom_estimate_syntax_rate builds from svt_aom_init_mode_probs
 * Built by tests/test_palette_abi.py (and by tests/golden/make_golden_palette.py) into a temporary directory with the include paths and
 * defines of oracle/Makefile and linked against oracle/_ref/libsvtref.so; nothing compiled is committed. */
#include <stdlib.h>
#include <string.h>

#include "definitions.h"
#include "md_process.h"
#include "md_rate_estimation.h"
#include "pcs.h"
#include "rd_cost.h"
#include "sequence_control_set.h"

void ref_init(void);
void init_fn_ptr(void);
void search_palette_luma(PictureControlSet *pcs, ModeDecisionContext *ctx, PaletteInfo *palette_cand, uint8_t *palette_size_array,
                         uint32_t *tot_palette_cands);
int  svt_av1_cost_color_map(ModeDecisionCandidate *cand, MdRateEstimationContext *rate_table, BlkStruct *blk_ptr, int plane, BlockSize bsize,
                            COLOR_MAP_TYPE type);
int  svt_av1_palette_color_cost_y(const PaletteModeInfo *const pmi, uint16_t *color_cache, const int palette_size, int n_cache, int bit_depth);
int  svt_get_palette_cache_y(const MacroBlockD *const xd, uint16_t *cache);
int  svt_aom_get_palette_bsize_ctx(BlockSize bsize);
int  svt_aom_write_uniform_cost(int n, int v);
void svt_av1_k_means_dim1_c(const int *data, int *centroids, uint8_t *indices, int n, int k, int max_itr);
void svt_aom_is_screen_content(PictureParentControlSet *pcs);

static void pin_init(void) {
    static int done;
    if (!done)
        ref_init(), init_fn_ptr(), done = 1;
}

typedef struct PinTables {
    MdRateEstimationContext rate;
    FRAME_CONTEXT           fc;
} PinTables;

static PinTables *tables(void) {
    static PinTables *t;
    if (!t) {
        pin_init();
        t = calloc(1, sizeof(*t));
        svt_aom_init_mode_probs(&t->fc);
        svt_aom_estimate_syntax_rate(&t->rate, 1, 1, 0, 1, 0, &t->fc);
    }
    return t;
}

/* ysize[7][7] and ycolor[7][5][8], as the device table holds them */
void pin_tables(int32_t *ysize, int32_t *ycolor) {
    const MdRateEstimationContext *r = &tables()->rate;
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) ysize[7 * i + j] = r->palette_ysize_fac_bits[i][j];
    memcpy(ycolor, r->palette_ycolor_fac_bitss, 7 * 5 * 8 * sizeof(int32_t));
}

typedef struct PinPalette {
    int32_t  width, height, rows, cols, bit_depth, step, stride, org_x, org_y, above_n, left_n;
    uint16_t above[8], left[8];
} PinPalette;

/* hdr: colors are not observable (a local): n_cands, n_cache.  Per kept candidate: sizes[i], colors[8 * i ..], maps[4096 * i ..] (width x
 * height), bits[3 * i ..] = size, colour and map bits.  Returns -1 when no BlockSize has this width and height. */
int32_t pin_palette_search(const PinPalette *a, void *plane, int32_t *hdr, uint16_t *cache, uint8_t *sizes, uint16_t *colors, uint8_t *maps, int32_t *bits) {
    pin_init();
    int bsize = -1;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == a->width && block_size_high[b] == a->height)
            bsize = b;
    if (bsize < 0)
        return -1;
    PictureControlSet       *pcs  = calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    SequenceControlSet      *scs  = calloc(1, sizeof(*scs));
    ModeDecisionContext     *ctx  = calloc(1, sizeof(*ctx));
    BlkStruct               *blk  = calloc(1, sizeof(*blk));
    MacroBlockD             *xd   = calloc(1, sizeof(*xd));
    MbModeInfo              *above = calloc(1, sizeof(*above)), *left = calloc(1, sizeof(*left));
    PALETTE_BUFFER          *pb   = calloc(1, sizeof(*pb));
    EbPictureBufferDesc      pic;
    BlockGeom                geom;
    memset(&pic, 0, sizeof(pic)), memset(&geom, 0, sizeof(geom));
    pic.buffer_y = plane, pic.stride_y = a->stride;
    geom.bsize   = (BlockSize)bsize;
    pcs->ppcs = ppcs, ppcs->scs = scs, scs->encoder_bit_depth = a->bit_depth, ppcs->palette_ctrls.dominant_color_step = a->step;
    if (a->bit_depth > 8)
        pcs->input_frame16bit = &pic, ctx->hbd_md = 1;
    else
        ppcs->enhanced_pic = &pic;
    ctx->blk_org_x = a->org_x, ctx->blk_org_y = a->org_y, ctx->blk_geom = &geom, ctx->blk_ptr = blk, ctx->palette_buffer = pb, blk->av1xd = xd;
    xd->mb_to_bottom_edge = (a->rows - a->height) * 8, xd->mb_to_right_edge = (a->cols - a->width) * 8;
    xd->mb_to_top_edge    = -8 * 8; /* row 8: not on a superblock-row boundary, the above palette counts */
    if (a->above_n) {
        above->palette_mode_info.palette_size = a->above_n, memcpy(above->palette_mode_info.palette_colors, a->above, sizeof(a->above));
        xd->above_mbmi = above;
    }
    if (a->left_n) {
        left->palette_mode_info.palette_size = a->left_n, memcpy(left->palette_mode_info.palette_colors, a->left, sizeof(a->left));
        xd->left_mbmi = left;
    }
    PaletteInfo cand[14];
    uint8_t     size_array[14] = {0};
    uint32_t    tot            = 0;
    memset(cand, 0, sizeof(cand));
    for (int i = 0; i < 14; i++) cand[i].color_idx_map = calloc(MAX_PALETTE_SQUARE, 1);
    search_palette_luma(pcs, ctx, cand, size_array, &tot);
    uint16_t  color_cache[16] = {0};
    const int n_cache         = svt_get_palette_cache_y(xd, color_cache);
    hdr[0] = (int32_t)tot, hdr[1] = n_cache;
    memcpy(cache, color_cache, sizeof(color_cache));
    const int bsize_ctx = svt_aom_get_palette_bsize_ctx((BlockSize)bsize);
    for (uint32_t i = 0; i < tot; i++) {
        ModeDecisionCandidate mdc;
        memset(&mdc, 0, sizeof(mdc));
        mdc.palette_info = &cand[i], mdc.palette_size[0] = size_array[i];
        sizes[i] = size_array[i];
        memcpy(colors + 8 * i, cand[i].pmi.palette_colors, 8 * sizeof(uint16_t));
        memcpy(maps + 4096 * i, cand[i].color_idx_map, (size_t)a->width * a->height);
        bits[3 * i] = tables()->rate.palette_ysize_fac_bits[bsize_ctx][size_array[i] - PALETTE_MIN_SIZE] + svt_aom_write_uniform_cost(size_array[i], cand[i].color_idx_map[0]);
        bits[3 * i + 1] = svt_av1_palette_color_cost_y(&cand[i].pmi, color_cache, size_array[i], n_cache, a->bit_depth);
        bits[3 * i + 2] = svt_av1_cost_color_map(&mdc, &tables()->rate, blk, 0, (BlockSize)bsize, PALETTE_MAP);
    }
    for (int i = 0; i < 14; i++) free(cand[i].color_idx_map);
    free(pcs), free(ppcs), free(scs), free(ctx), free(blk), free(xd), free(above), free(left), free(pb);
    return 0;
}

/* search_palette_luma over every width x height block of an 8-bit picture (tools/palette_time.py), the objects made once: per block
 * n_cands[i] and check[i] = sum over the kept candidates c and their colours j of (31 * c + j + 1) * colour + size.  Returns the seconds
 * spent inside search_palette_luma. */
#include <time.h>
double pin_palette_picture(uint8_t *plane, int32_t pic_w, int32_t pic_h, int32_t stride, int32_t width, int32_t height, int32_t step, int32_t *n_cands,
                           uint32_t *check) {
    pin_init();
    int bsize = -1;
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == width && block_size_high[b] == height)
            bsize = b;
    PictureControlSet       *pcs  = calloc(1, sizeof(*pcs));
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    SequenceControlSet      *scs  = calloc(1, sizeof(*scs));
    ModeDecisionContext     *ctx  = calloc(1, sizeof(*ctx));
    BlkStruct               *blk  = calloc(1, sizeof(*blk));
    MacroBlockD             *xd   = calloc(1, sizeof(*xd));
    PALETTE_BUFFER          *pb   = calloc(1, sizeof(*pb));
    EbPictureBufferDesc      pic;
    BlockGeom                geom;
    PaletteInfo              cand[14];
    memset(&pic, 0, sizeof(pic)), memset(&geom, 0, sizeof(geom)), memset(cand, 0, sizeof(cand));
    for (int i = 0; i < 14; i++) cand[i].color_idx_map = calloc(MAX_PALETTE_SQUARE, 1);
    pic.buffer_y = plane, pic.stride_y = stride, geom.bsize = (BlockSize)bsize;
    pcs->ppcs = ppcs, ppcs->scs = scs, scs->encoder_bit_depth = 8, ppcs->palette_ctrls.dominant_color_step = step, ppcs->enhanced_pic = &pic;
    ctx->blk_geom = &geom, ctx->blk_ptr = blk, ctx->palette_buffer = pb, blk->av1xd = xd;
    double spent = 0;
    int    at    = 0;
    for (int y = 0; y < pic_h; y += height)
        for (int x = 0; x < pic_w; x += width, at++) {
            uint8_t  size_array[14] = {0};
            uint32_t tot = 0, sum = 0;
            ctx->blk_org_x = x, ctx->blk_org_y = y;
            xd->mb_to_bottom_edge = (pic_h - y - height) * 8, xd->mb_to_right_edge = (pic_w - x - width) * 8;
            struct timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            search_palette_luma(pcs, ctx, cand, size_array, &tot);
            clock_gettime(CLOCK_MONOTONIC, &t1);
            spent += (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
            for (uint32_t c = 0; c < tot; c++) {
                sum += size_array[c];
                for (int j = 0; j < size_array[c]; j++) sum += (31 * c + j + 1) * cand[c].pmi.palette_colors[j];
            }
            n_cands[at] = (int32_t)tot, check[at] = sum;
        }
    for (int i = 0; i < 14; i++) free(cand[i].color_idx_map);
    free(pcs), free(ppcs), free(scs), free(ctx), free(blk), free(xd), free(pb);
    return spent;
}

int32_t pin_count_colors(const void *src, int32_t stride, int32_t rows, int32_t cols, int32_t bit_depth) {
    static int count_buf[1 << 12];
    int        svt_av1_count_colors(const uint8_t *src, int stride, int rows, int cols, int *val_count);
    int        svt_av1_count_colors_highbd(uint16_t * src, int stride, int rows, int cols, int bit_depth, int *val_count);
    return bit_depth > 8 ? svt_av1_count_colors_highbd((uint16_t *)src, stride, rows, cols, bit_depth, count_buf)
                         : svt_av1_count_colors(src, stride, rows, cols, count_buf);
}

void pin_k_means(const int32_t *data, int32_t *centroids, uint8_t *indices, int32_t n, int32_t k, int32_t max_itr) {
    pin_init();
    svt_av1_k_means_dim1_c(data, centroids, indices, n, k, max_itr);
}

/* out: sc_class0 .. sc_class3 (counts_1 and counts_2 are locals of the reference) */
void pin_sc_classify(uint8_t *plane, int32_t width, int32_t height, int32_t stride, int32_t *out) {
    pin_init();
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    EbPictureBufferDesc      pic;
    memset(&pic, 0, sizeof(pic));
    pic.buffer_y = plane, pic.stride_y = stride, pic.width = width, pic.height = height;
    ppcs->enhanced_pic = &pic;
    svt_aom_is_screen_content(ppcs);
    out[0] = ppcs->sc_class0, out[1] = ppcs->sc_class1, out[2] = ppcs->sc_class2, out[3] = ppcs->sc_class3;
    free(ppcs);
}
