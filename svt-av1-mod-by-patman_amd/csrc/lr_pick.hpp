// lr_pick.hpp — what the two plane picks (loopfilter_wiener_pick.hip, loopfilter_rest_pick.hip) decide with, once: the restoration
// types, the default references and bit counts of the signalled parameters (restoration_pick.c), and the checks of the arguments the
// two entry points share.  The filters, the searches and the reductions are in lr_device.hpp.
#pragma once

#include "../../include/svt_hip_lf.h"
#include "common.hpp"
#include "lr_device.hpp"

namespace svthip {
namespace lr {

constexpr int       RESTORE_NONE = 0, RESTORE_WIENER = 1, RESTORE_SGRPROJ = 2, RESTORE_SWITCHABLE = 3;
constexpr long long SSE_REJECTED = 0x7fffffffffffffffLL;  // INT64_MAX

__device__ __forceinline__ void lds_add(long long *p, long long v) { atomicAdd((unsigned long long *)p, (unsigned long long)v); }

__device__ __forceinline__ int tap_min(int p) { return p == 0 ? -5 : (p == 1 ? -23 : -17); }  // WIENER_FILT_TAPn_MINV
__device__ __forceinline__ int tap_max(int p) { return p == 0 ? 10 : (p == 1 ? 8 : 46); }     // WIENER_FILT_TAPn_MAXV
// set_default_wiener, set_default_sgrproj: ref = vfilter[0..2], hfilter[0..2] / xqd
__device__ __forceinline__ void set_default_wiener(int ref[6]) {
    for (int t = 0; t < 6; t++) ref[t] = t % 3 == 0 ? 3 : (t % 3 == 1 ? -7 : 15);  // WIENER_FILT_TAPn_MIDV
}
__device__ __forceinline__ void set_default_sgrproj(int ref[2]) { ref[0] = (PRJ_MIN0 + PRJ_MAX0) / 2, ref[1] = (PRJ_MIN1 + PRJ_MAX1) / 2; }

// the bits of tap p of a Wiener filter against its reference
__device__ inline int wiener_tap_bits(int p, int ref, int v) { return count_refsubexpfin(16 << p, p + 1, ref - tap_min(p), v - tap_min(p)); }
// count_wiener_bits (:1008-1037): taps = vfilter[0..2], hfilter[0..2]; count(p, ref, v) = wiener_tap_bits or a table of it
template <class Count> __device__ __forceinline__ int count_wiener_bits(int win, const int16_t *taps, const int *ref, Count count) {
    int c = 0;
    for (int t = 0; t < 6; t++)
        if (win == 7 || t % 3 != 0)
            c += count(t % 3, ref[t], taps[t]);
    return c;
}
// count_sgrproj_bits (:655-669)
__device__ inline int count_sgrproj_bits(int ep, const int *xqd, const int *ref) {
    int bits = 4;  // SGRPROJ_PARAMS_BITS
    if (SGR_PRM[ep][0] > 0)
        bits += count_refsubexpfin(PRJ_MAX0 - PRJ_MIN0 + 1, 4, ref[0] - PRJ_MIN0, xqd[0] - PRJ_MIN0);
    if (SGR_PRM[ep][1] > 0)
        bits += count_refsubexpfin(PRJ_MAX1 - PRJ_MIN1 + 1, 4, ref[1] - PRJ_MIN1, xqd[1] - PRJ_MIN1);
    return bits;
}

}  // namespace lr

// ---- the argument checks of svt_hip_wiener_pick_plane and svt_hip_rest_pick_plane; fn is the entry point's name, the result SVT_HIP_OK or refuse()'s
inline int32_t pick_plane_ok(const char *fn, int bit_depth, int is_16bit, uint32_t plane_w, uint32_t plane_h) {
    if ((bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || (bit_depth > 8 && !is_16bit))
        return refuse("%s: bit depth %d with %s samples", fn, bit_depth, is_16bit ? "16-bit" : "8-bit");
    if (plane_w == 0 || plane_h == 0 || plane_w > 65536 || plane_h > 65536)
        return refuse("%s: plane of %u x %u", fn, plane_w, plane_h);
    return SVT_HIP_OK;
}
// Every unit in order: pointers, limits inside the plane, at most max_side samples a side; an accepted unit goes to each(i, unit, w, h)
template <class Each>
int32_t pick_units_ok(const char *fn, const SvtHipWienerUnit *units, uint32_t n_units, uint32_t plane_w, uint32_t plane_h, int max_side, Each each) {
    for (uint32_t i = 0; i < n_units; i++) {
        const SvtHipWienerUnit &u = units[i];
        if (!u.dgd || !u.src || u.h_start < 0 || u.v_start < 0 || u.h_end <= u.h_start || u.v_end <= u.v_start || (uint32_t)u.h_end > plane_w ||
            (uint32_t)u.v_end > plane_h)
            return refuse("%s: unit %u: limits [%d, %d) x [%d, %d) outside the plane of %u x %u", fn, i, u.h_start, u.h_end, u.v_start, u.v_end, plane_w, plane_h);
        const int uw = u.h_end - u.h_start, uh = u.v_end - u.v_start;
        if (uw > max_side || uh > max_side)
            return refuse("%s: unit %u: %d x %d samples, %d at the most", fn, i, uw, uh, max_side);
        each(i, u, uw, uh);
    }
    return SVT_HIP_OK;
}

}  // namespace svthip
