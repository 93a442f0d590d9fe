// txb_geometry.hpp — what a transform size w x h means to the kernels instantiated per RETAINED shape min(w,32) x min(h,32)
// (txfm_rate.hip, txfm_rdoq.hip): the size rule, what the reference derives from the size, the work split, the capped grid and the
// one list of the 14 retained shapes.  Plain C++17 without a HIP header: tests/test_rdoq_abi.py compiles it with a host compiler alone.
#pragma once
#include <stdint.h>
#include <type_traits>

namespace svthip {

// TX_4X4 .. TX_64X64 of one side, -1 for a length that is no side of a transform
constexpr int tx_side_index(uint32_t v) { return v == 4 ? 0 : v == 8 ? 1 : v == 16 ? 2 : v == 32 ? 3 : v == 64 ? 4 : -1; }

// the lanes that share a block of `retained` coefficients: 16-, 32- and 64-coefficient blocks sit 4, 2 and 1 to a wavefront
constexpr uint32_t group_lanes(uint32_t retained) { return retained < 64 ? retained : 64; }

// min(ceil(n_blocks / per_wg), cap): a workgroup walks the batch in steps of per_wg blocks, so the grid never exceeds the batch
constexpr uint32_t grid_blocks(uint32_t n_blocks, uint32_t per_wg, uint32_t cap) {
    const uint32_t wanted = n_blocks / per_wg + (n_blocks % per_wg != 0);
    return wanted < cap ? wanted : cap;
}

struct TxbGeometry {
    int      sw, sh;             // tx_side_index of w and h
    bool     valid;              // one of the 19 transform sizes: ratios 1:1, 1:2 and 1:4
    int      orient;             // sign of w - h: which family of eb_av1_nz_map_ctx_offset the size uses
    int      sqr, sqr_up;        // txsize_sqr_map, txsize_sqr_up_map: TX_4X4 .. TX_64X64 of min(w, h) and max(w, h)
    int      txs_ctx;            // (txsize_sqr_map + txsize_sqr_up_map + 1) >> 1
    uint32_t pixels;             // w * h
    int      tx_scale;           // av1_get_tx_scale_tab (full_loop.h:52)
    uint32_t iw, ih, retained;   // a 64-point side keeps its 32 low frequencies; iw * ih
    uint32_t sqrt_retained = 1;  // sqrt_tx_pixels_2d (full_loop.c:1112): the root of the retained coefficient count, rounded up

    constexpr TxbGeometry(uint32_t w, uint32_t h)
        : sw(tx_side_index(w)), sh(tx_side_index(h)), valid(sw >= 0 && sh >= 0 && (sw > sh ? sw - sh : sh - sw) <= 2),
          orient((sw > sh) - (sw < sh)), sqr(sw < sh ? sw : sh), sqr_up(sw > sh ? sw : sh), txs_ctx((sqr + sqr_up + 1) >> 1),
          pixels(w * h), tx_scale(pixels > 1024 ? 2 : pixels > 256 ? 1 : 0), iw(w < 32 ? w : 32), ih(h < 32 ? h : 32), retained(iw * ih) {
        while (sqrt_retained * sqrt_retained < retained) sqrt_retained++;
    }
};

// The 14 retained shapes of the 19 transform sizes, the only place they are listed: calls f(W, H) with iw and ih as
// std::integral_constant and returns true, or returns false when iw x ih is none of them.
template <class F>
constexpr bool for_retained_shape(uint32_t iw, uint32_t ih, F &&f) {
    const auto at = [&](auto W, auto H) { return iw == (uint32_t)W && ih == (uint32_t)H ? (f(W, H), true) : false; };
    constexpr std::integral_constant<int, 4> _4{};
    constexpr std::integral_constant<int, 8> _8{};
    constexpr std::integral_constant<int, 16> _16{};
    constexpr std::integral_constant<int, 32> _32{};
    return at(_4, _4) || at(_8, _8) || at(_16, _16) || at(_32, _32) || at(_4, _8) || at(_8, _4) || at(_8, _16) || at(_16, _8) ||
           at(_16, _32) || at(_32, _16) || at(_4, _16) || at(_16, _4) || at(_8, _32) || at(_32, _8);
}

}  // namespace svthip
