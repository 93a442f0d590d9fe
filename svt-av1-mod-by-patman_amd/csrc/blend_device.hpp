// blend_device.hpp — device helpers shared by the blend and the mask-search kernels of inter_blend.hip: loads and stores of
// four adjacent samples (one 4- / 8-byte access where the address allows it, single samples otherwise) and wave sums.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace svthip {
namespace blend {

// n (1 .. 4) adjacent uint8 / uint16 samples at p into v[0 .. n); v[n ..) = 0
template <bool IS16> __device__ inline void load4(const void *p, int n, int v[4]) {
    if (IS16) {
        const uint16_t *s = (const uint16_t *)p;
        if (n == 4 && ((uintptr_t)s & 7) == 0) {
            const uint2 q = *(const uint2 *)s;
            v[0] = q.x & 0xFFFF, v[1] = q.x >> 16, v[2] = q.y & 0xFFFF, v[3] = q.y >> 16;
            return;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = k < n ? s[k] : 0;
    } else {
        const uint8_t *s = (const uint8_t *)p;
        if (n == 4 && ((uintptr_t)s & 3) == 0) {
            const uint32_t q = *(const uint32_t *)s;
            v[0] = q & 0xFF, v[1] = (q >> 8) & 0xFF, v[2] = (q >> 16) & 0xFF, v[3] = q >> 24;
            return;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = k < n ? s[k] : 0;
    }
}

// 2 * n (n = 1 .. 4) adjacent bytes at p into v[0 .. 2 n); the rest 0
__device__ inline void load8_u8(const uint8_t *p, int n, int v[8]) {
    if (n == 4 && ((uintptr_t)p & 7) == 0) {
        const uint2 q = *(const uint2 *)p;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (q.x >> (8 * k)) & 0xFF, v[4 + k] = (q.y >> (8 * k)) & 0xFF;
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = k < 2 * n ? p[k] : 0;
}

template <bool IS16> __device__ inline void store4(void *p, int n, const int v[4]) {
    if (IS16) {
        uint16_t *d = (uint16_t *)p;
        if (n == 4 && ((uintptr_t)d & 7) == 0) {
            *(uint2 *)d = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
            return;
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n)
                d[k] = (uint16_t)v[k];
    } else {
        uint8_t *d = (uint8_t *)p;
        if (n == 4 && ((uintptr_t)d & 3) == 0) {
            *(uint32_t *)d = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
            return;
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n)
                d[k] = (uint8_t)v[k];
    }
}

// sum over the 64 lanes of a wave, in every lane
__device__ inline uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// Exact sum of values < 2^31 over up to 2^15 samples in two 32-bit words: low 16 bits and the rest apart, so that lanes and
// waves can add the words independently (a 64-bit sum would need carries across a shuffle).
struct SplitSum {
    uint32_t lo, hi;
    __device__ void add(uint32_t v) { lo += v & 0xFFFF, hi += v >> 16; }
    __device__ static uint64_t total(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 16) + lo; }
};

__device__ inline int clamp_i16(int v) { return min(max(v, -32768), 32767); }

}  // namespace blend
}  // namespace svthip
