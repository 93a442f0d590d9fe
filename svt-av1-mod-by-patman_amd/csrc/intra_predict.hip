// intra_predict.hip — intra prediction of any transform block on gfx950: svt_hip_intra_predict_batch (build_intra_predictors[_high]
// with the smooth inter-intra combination as an epilogue) and svt_hip_cfl_predict_batch (include/svt_hip_intra.h).  The device
// functions are in intra_pred_device.hpp.
//
// One wave per descriptor: the descriptor is wave-uniform (scalar loads), the edges are built once in the wave's own LDS slice, a
// lane produces four adjacent samples of a row.  Nothing is shared between descriptors and no wave waits for another, so small
// blocks are packed by putting WAVES descriptors into one workgroup: a 4 x 4 block still leaves lanes idle, but its wave shares
// the workgroup's launch and its LDS allocation with three others.  svt_hip_intra_predict_batch uses WAVES = 4;
// svt_hip_intra_predict_batch_packed lets tools/intra_pred_time.py measure 1, 2 and 4 side by side.
#include "../../include/svt_hip_intra.h"
#include "common.hpp"
#include "intra_pred_device.hpp"

using namespace svthip;
using namespace svthip::intrapred;

namespace {

constexpr int PACKED_WAVES = 4;

// The descriptor index is folded into grid.x alone (up to 2^31 - 1 workgroups): n is not limited by a 65 535 dimension.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void intra_predict_kernel(const SvtHipIntraPredDesc *__restrict__ descs, uint32_t n) {
    __shared__ WaveLds lds[WAVES];
    const int          wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const uint32_t     i    = blockIdx.x * WAVES + (uint32_t)wave;
    if (i >= n)
        return;
    const SvtHipIntraPredDesc d = descs[i];  // uniform: scalar loads
    if (!pred_desc_ok(d))
        return;
    predict_block(d, lds[wave], lane);
}

template <int WAVES> __global__ __launch_bounds__(64 * WAVES) void cfl_predict_kernel(const SvtHipCflDesc *__restrict__ descs, uint32_t n) {
    const int      wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const uint32_t i    = blockIdx.x * WAVES + (uint32_t)wave;
    if (i >= n)
        return;
    const SvtHipCflDesc d = descs[i];  // uniform: scalar loads
    if (!cfl_desc_ok(d))
        return;
    d.is_16bit ? cfl_block<true>(d, lane) : cfl_block<false>(d, lane);
}

template <int WAVES> void launch_predict(const SvtHipIntraPredDesc *d_desc, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(intra_predict_kernel<WAVES>, dim3((n + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, d_desc, n);
}

int32_t predict_batch(const char *fn, const SvtHipIntraPredDesc *d_desc, uint32_t n, uint32_t waves, void *stream) {
    if (!d_desc || n == 0 || (waves != 1 && waves != 2 && waves != 4))
        return refuse("%s: bad argument", fn);
    TierBCall c(fn, stream);
    if (!c.ok())
        return c.status();
    hipStream_t st = c.stream();
    if (waves == 4)
        launch_predict<4>(d_desc, n, st);
    else if (waves == 2)
        launch_predict<2>(d_desc, n, st);
    else
        launch_predict<1>(d_desc, n, st);
    return c.finish();
}

}  // namespace

extern "C" int32_t svt_hip_intra_predict_batch(const SvtHipIntraPredDesc *d_desc, uint32_t n, void *stream) {
    return predict_batch("svt_hip_intra_predict_batch", d_desc, n, PACKED_WAVES, stream);
}

extern "C" int32_t svt_hip_intra_predict_batch_packed(const SvtHipIntraPredDesc *d_desc, uint32_t n, uint32_t waves_per_workgroup,
                                                      void *stream) {
    return predict_batch("svt_hip_intra_predict_batch_packed", d_desc, n, waves_per_workgroup, stream);
}

extern "C" int32_t svt_hip_cfl_predict_batch(const SvtHipCflDesc *d_desc, uint32_t n, void *stream) {
    if (!d_desc || n == 0)
        return refuse("svt_hip_cfl_predict_batch: bad argument");
    TierBCall c("svt_hip_cfl_predict_batch", stream);
    if (!c.ok())
        return c.status();
    hipLaunchKernelGGL(cfl_predict_kernel<PACKED_WAVES>, dim3((n + PACKED_WAVES - 1) / PACKED_WAVES), dim3(64 * PACKED_WAVES), 0,
                       c.stream(), d_desc, n);
    return c.finish();
}

SVT_HIP_MODULE_WARMUP(intra_predict)
