// Butterfly reductions of a double over the 64 lanes of a wave (__shfl_xor on doubles): every lane gets the result. The sum adds in
// the butterfly's fixed order, which the host twins of the kernels emulate (ringiou.hip, crownzonal.hip; also regionrelate.hip).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double wave_sum(double v) {
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}
