// The second launch of the deterministic loss sums (pair_score.hip, group_score.hip): ONE workgroup adds the fp64 partials the first
// launch wrote, one per workgroup, in a fixed order.  Internal linkage: each translation unit that includes this carries its own copy
// of the same code, so the order of the additions -- and with it every bit of the result -- is the same whoever launches it.
#pragma once
#include "npi_common.h"

namespace npi {

constexpr int PS_SUM_THREADS = 256;            // the workgroup that adds the partials

// loss[0] = sum of partials[0 .. n) in a fixed order: thread t adds t, t + 256, ... in fp64, then a fixed tree over the workgroup
static __global__ void __launch_bounds__(PS_SUM_THREADS)
pair_loss_sum_kernel(const double* __restrict__ partials, int n, float* __restrict__ loss) {
    __shared__ double acc[PS_SUM_THREADS];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += PS_SUM_THREADS) v += partials[i];
    acc[threadIdx.x] = v;
    __syncthreads();
    for (int s = PS_SUM_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) acc[threadIdx.x] += acc[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)acc[0];
}

}  // namespace npi
