// gmpe_expand.h — the per-row arithmetic of the learner-side expansions from entity tables (gmpe_outputs.entity_table), shared by every kernel that rebuilds
// node_obs rows or adjacency entries from a table: k_node_expand / k_adj_from_table (gmpe_step.hip: gmpe_expand_node_obs, gmpe_expand_adj) and the minibatch
// gather (gmpe_minibatch.hip). Every translation unit that includes it is compiled with the same -ffp-contract=off flags, so all of them produce the same bits
// as the engine (tests/test_gpu_gather.py, tests/test_gpu_minibatch.py).
#pragma once
#include "gmpe_device.h"

namespace gmpe {

// Node row of entity k seen by ego ei, from the table T of one env-step (W doubles). The operations repeat stream_graph_fn's three row variants operation for
// operation. KIND 0: relative, F = 8 (…_july.py:1694-1771), d 16-byte aligned; 1: rot_inv family, F = 7 (rot_inv.py:1690-1766; two: goal = corridor exit,
// two_phase_graph.py:1405); 2: graph_feat_type 'global', F = 7 (…_july.py:1672-1691).
template <int KIND>
__device__ __forceinline__ void node_row_from_table(const double* __restrict__ T, float* __restrict__ d, int A, int L, int E, int W, int two, int ei, int k) {
    const double* ex = T; const double* ey = T + E;
    const double* vox = T + 2 * E; const double* voy = vox + A; const double* vnx = voy + A; const double* vny = vnx + A;
    const bool kag = k < A;
    const int kk = kag ? k : 0;
    const bool post = k <= ei;                                           // agent k's re-drawn velocity is visible to ego ei iff k <= ei (ordered-visibility rule)
    const float typ = kag ? 0.0f : (k < A + L ? 1.0f : 2.0f);
    if (KIND == 0) {
        const double kx = ex[k], ky = ey[k];
        const double kvox = kag ? vox[kk] : 0.0, kvoy = kag ? voy[kk] : 0.0, kvnx = kag ? vnx[kk] : 0.0, kvny = kag ? vny[kk] : 0.0;
        const double gx = kag ? ex[A + kk] : kx, gy = kag ? ey[A + kk] : ky;
        const double px = ex[ei], py = ey[ei], evx = vnx[ei], evy = vny[ei];
        float4* d4 = reinterpret_cast<float4*>(d);
        d4[0] = make_float4((float)((post ? kvnx : kvox) - evx), (float)((post ? kvny : kvoy) - evy), (float)(kx - px), (float)(ky - py));
        d4[1] = make_float4((float)(gx - px), (float)(gy - py), kag ? 0.0f : 1.0f, typ);
    } else if (KIND == 1) {
        const double* cn = vny + A; const double* sn = cn + A;
        const float kx = (float)ex[k], ky = (float)ey[k];
        const float kvox = kag ? (float)vox[kk] : 0.0f, kvoy = kag ? (float)voy[kk] : 0.0f, kvnx = kag ? (float)vnx[kk] : 0.0f, kvny = kag ? (float)vny[kk] : 0.0f;
        const int wx = W - (E + 31) / 32 - 2;                              // two_phase_graph: exit x, y sit right before the mask words
        const float gxk = two ? (float)T[wx] : (kag ? (float)ex[A + kk] : 0.0f), gyk = two ? (float)T[wx + 1] : (kag ? (float)ey[A + kk] : 0.0f);
        const float apx = (float)ex[ei], apy = (float)ey[ei], avx = (float)vnx[ei], avy = (float)vny[ei];
        const double cs = cn[ei], s_ = sn[ei];
        const float rvx = (post ? kvnx : kvox) - avx, rvy = (post ? kvny : kvoy) - avy;
        const float rpx = kx - apx, rpy = ky - apy;
        double o0, o1, o2, o3, o4, o5;
        rot2(cs, s_, (double)rvx, (double)rvy, o0, o1);
        rot2(cs, s_, (double)rpx, (double)rpy, o2, o3);
        if (kag) rot2(cs, s_, (double)(gxk - apx), (double)(gyk - apy), o4, o5); else { o4 = o2; o5 = o3; }
        d[0] = (float)o0; d[1] = (float)o1; d[2] = (float)o2; d[3] = (float)o3; d[4] = (float)o4; d[5] = (float)o5; d[6] = typ;
    } else {
        const float kx = (float)ex[k], ky = (float)ey[k];
        const float kvox = kag ? (float)vox[kk] : 0.0f, kvoy = kag ? (float)voy[kk] : 0.0f, kvnx = kag ? (float)vnx[kk] : 0.0f, kvny = kag ? (float)vny[kk] : 0.0f;
        const float gx = kag ? (float)ex[A + kk] : kx, gy = kag ? (float)ey[A + kk] : ky;
        d[0] = post ? kvnx : kvox; d[1] = post ? kvny : kvoy; d[2] = kx; d[3] = ky; d[4] = gx; d[5] = gy; d[6] = typ;
    }
}

// Entry (r, c) of the E x E adjacency of one env-step from its table: f32(sqrt(dx^2 + dy^2)) with delta = pos[min(r,c)] - pos[max(r,c)]
// (World.calculate_distances, core.py:600-624 — distance_trip's expression, so the bits are the engine's), zero diagonal, rows / columns of masked nodes zeroed
// (…_july.py:1627-1648).
__device__ __forceinline__ float adj_entry_from_table(const double* __restrict__ T, int E, int W, int r, int c) {
    const double* ex = T; const double* ey = T + E;
    const double* mw = T + (W - (E + 31) / 32);
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    const unsigned wr = (unsigned)mw[r >> 5], wc = (unsigned)mw[c >> 5];
    const bool masked = ((wr >> (r & 31)) | (wc >> (c & 31))) & 1u;
    const double dx = ex[lo] - ex[hi], dy = ey[lo] - ey[hi];
    return (r == c || masked) ? 0.0f : (float)sqrt(dx * dx + dy * dy);
}

}  // namespace gmpe
