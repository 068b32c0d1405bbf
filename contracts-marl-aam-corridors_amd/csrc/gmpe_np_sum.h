// gmpe_np_sum.h — NumPy's pairwise_sum leaf, shared by the kernels that must equal float64 NumPy bit for bit (gmpe_eval.hip: sums over agents;
// gmpe_infos.hip: the leaves of the chunked pairwise sums over envs). Internal: not installed. Include it under `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>

// NumPy's pairwise_sum (numpy/_core/src/umath/loops_utils.h.src) for n <= 128, on values produced by f(i)
template <typename F>
__device__ __forceinline__ double np_sum(int n, F f) {
    if (n < 8) {
        double r = -0.0;
        for (int i = 0; i < n; ++i) r += f(i);
        return r;
    }
    double r0 = f(0), r1 = f(1), r2 = f(2), r3 = f(3), r4 = f(4), r5 = f(5), r6 = f(6), r7 = f(7);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += f(i); r1 += f(i + 1); r2 += f(i + 2); r3 += f(i + 3);
        r4 += f(i + 4); r5 += f(i + 5); r6 += f(i + 6); r7 += f(i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += f(i);
    return res;
}
