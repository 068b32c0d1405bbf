// gmpe_mb_map.h — the row map of a PPO minibatch (include/gmpe.h, GMPE_MB_FEED_FORWARD / GMPE_MB_RECURRENT): output row r -> sample (t, n, a) of the rollout,
// shared by every kernel that draws a minibatch through a permutation: the gather (gmpe_minibatch.hip) and the edge lists (gmpe_mb_edges.hip). One definition, so
// graph r of gmpe_minibatch_edges is row r of gmpe_minibatch_gather by construction (tests/test_gpu_minibatch_edges.py compares them).
#pragma once
#include <stdint.h>

#include "../../include/gmpe.h"

namespace gmpe {

// Sample (t, n, a) of output row r (chunk r for a chunk head); ok = false for a permutation entry out of range.
struct Sample { uint32_t t, n, a; bool ok; };

// P carries: perm, offset (int64), T, N, A, L, chunks, n_valid (uint32), mode. IDENT: the identity permutation (perm is not read), entry k = offset + k.
template <bool IDENT = false, class P>
__device__ __forceinline__ Sample sample_of(const P& p, uint32_t r, bool head) {
    Sample s{0u, 0u, 0u, false};
    if (p.mode == GMPE_MB_FEED_FORWARD) {
        const int64_t j = IDENT ? p.offset + r : p.perm[p.offset + r];
        if (j < 0 || j >= (int64_t)p.n_valid) return s;
        const uint32_t u = (uint32_t)j, na = p.N * p.A;
        s.t = u / na;
        const uint32_t rem = u - s.t * na;
        s.n = rem / p.A;
        s.a = rem - s.n * p.A;
    } else {
        const uint32_t k = head ? r : r % p.chunks, l = head ? 0u : r / p.chunks;
        const int64_t c = IDENT ? p.offset + k : p.perm[p.offset + k];
        if (c < 0 || c >= (int64_t)p.n_valid) return s;
        const uint32_t f = (uint32_t)c * p.L + l, at = p.A * p.T;
        s.n = f / at;
        const uint32_t rem = f - s.n * at;
        s.a = rem / p.T;
        s.t = rem - s.a * p.T;
    }
    s.ok = true;
    return s;
}

}  // namespace gmpe
