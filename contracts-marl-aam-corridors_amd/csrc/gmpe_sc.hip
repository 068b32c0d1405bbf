// gmpe_sc.hip — one scenario variant of the fused kernel per translation unit (compiled with -DGMPE_SC=<variant>, in
// parallel): tile shapes BLOCK in {64,128,256} x exact-size instantiations AP in {0,3,10}, plus the steady-state instantiation
// <256, 10, SC, FL = 1> (run-time flags folded) that the C2/C3-shaped workloads run, plus the rollout instantiations
// <64, 0, SC, 2>, <256, {0, 10}, SC, 2> (FL = 2: K steps inside one launch, gmpe_rollout_steps), and the compile-time-G variants of the 4096 x 10 tile shapes:
// <256, 10, SC, 2, GC = 4 | 6> and <256, 10, SC, 1, GC = 4>.
// env_kernel<SC> is the one place that says which of them runs: gmpe_step.hip launches what it returns (launch_env), asks the runtime
// for the residency of what it returns (tile-shape search) and opts every instantiation it can return in to > 64 KiB of LDS.
#include "gmpe_kernel.h"

#ifndef GMPE_SC
#error "compile with -DGMPE_SC=<scenario variant>"
#endif

#ifndef GMPE_PART
#define GMPE_PART 0
#endif

namespace gmpe {

// The two steady-state step kernels (FL = 1: one launch per step, the closed-loop shape) live in a translation unit of their own (-DGMPE_PART=1) that is compiled with the max-ILP
// machine scheduler (-mllvm -amdgpu-sched-strategy=max-ilp): a step launch is one dependent chain per tile, and scheduling for ILP instead of occupancy shortens it (c2 closed loop
// 24.1 -> 23.6 us per step, c3 24.5 -> 24.2) while the rollout kernels, which interleave chains of several tiles, are 0.5 % faster with the default strategy (profiles/r04_notes.md).
#if GMPE_PART == 1
template __global__ void k_env<256, 10, GMPE_SC, 1>(const KParams);
template __global__ void k_env<256, 10, GMPE_SC, 1, 4>(const KParams);
#else
extern template __global__ void k_env<256, 10, GMPE_SC, 1>(const KParams);
extern template __global__ void k_env<256, 10, GMPE_SC, 1, 4>(const KParams);

template <int BLOCK, int AP, int SC, int FL, int GC = 0>
static EnvKernel kernel_of() {
    // the separate pair-force buffer exists only where the fused distance + next-step-force pass can run (FUSE_OK in gmpe_kernel.h)
    return {reinterpret_cast<const void*>(&k_env<BLOCK, AP, SC, FL, GC>), BLOCK, FL == 2 && AP == 10};
}

template <int SC>
EnvKernel env_kernel(int block, int ap, int fl, int G) {
    if (fl == 2) {
        // persistent rollout kernel: BLOCK 64 (run-time sizes) or 256 (run-time sizes, or exact-size for A = L = 10). Register budgets
        // (__launch_bounds__ in gmpe_kernel.h), measured per scenario on one box (profiles/README.md): navigation_graph exact-size at four
        // tiles per CU (G = 4; spills 5 dwords, 17.0 us per step vs 18.3 at three tiles / G = 6 without a spill, 19.9 run-time sizes); the
        // kinematic scenarios exact-size at three tiles per CU (G = 6, no spill: July 15.8 us vs 18.0 at four tiles with a 14-dword spill).
        if (block == 64) return kernel_of<64, 0, SC, 2>();
        if (ap == 10 && G == 4) return kernel_of<256, 10, SC, 2, 4>();      // envs per tile folded too (the 4096 x 10 shapes)
        if (ap == 10 && G == 6) return kernel_of<256, 10, SC, 2, 6>();
        if (ap == 10) return kernel_of<256, 10, SC, 2>();
        return kernel_of<256, 0, SC, 2>();
    }
    if (fl == 1 && block == 256 && ap == 10) return G == 4 ? kernel_of<256, 10, SC, 1, 4>() : kernel_of<256, 10, SC, 1>();
    if (block == 64) return ap == 10 ? kernel_of<64, 10, SC, 0>() : (ap == 3 ? kernel_of<64, 3, SC, 0>() : kernel_of<64, 0, SC, 0>());
    if (block == 128) return ap == 10 ? kernel_of<128, 10, SC, 0>() : (ap == 3 ? kernel_of<128, 3, SC, 0>() : kernel_of<128, 0, SC, 0>());
    return ap == 10 ? kernel_of<256, 10, SC, 0>() : (ap == 3 ? kernel_of<256, 3, SC, 0>() : kernel_of<256, 0, SC, 0>());
}

template EnvKernel env_kernel<GMPE_SC>(int, int, int, int);
#endif  // GMPE_PART

}  // namespace gmpe
