// gmpe_head.hip — the policy's action head on the device (include/gmpe.h gmpe_head_forward / gmpe_head_backward / gmpe_act_head): the Linear of the
// reference's Categorical (onpolicy/algorithms/utils/distributions.py:72-91, `self.linear`) under a single Discrete ACTLayer (act.py:27-29), weight [K, 64],
// bias [K], K <= 64 — the one layer between the RNN's features and the masked categorical of gmpe_ppo_rows.h. Forward is ONE launch, backward THREE,
// the rollout form (Linear + mask + sample + log-prob) ONE, plus the one-thread counter launch with draw_dev.
//
// Mapping. The row kernels are gmpe_ppo_rows.h's: one lane per row, TILE = 256 rows per workgroup, the logits tile in LDS at the odd stride S = K | 1.
// In front of it (gmpe_head_rows.h): the tile's features, 64 KiB contiguous in memory, come in as coalesced 16-byte loads into LDS at row stride 68 dwords,
// where a lane then reads its own row as sixteen conflict-free 16-byte reads into 64 registers; the weights and the bias (K * 65 floats, <= 16.25 KiB) stand
// behind the rows region and are read at wave-uniform addresses, every read a broadcast. Behind a barrier the logits tile takes the features tile's place, so
// a workgroup holds 256 * 68 * 4 = 68 KiB + the parameters: 74.3 KiB at the shipped K = 25 — two workgroups per CU of 160 KiB up to K = 47, one above.
// k_head_bwd_rows is the mirror image: the grad_logits tile at stride S, 64 accumulators per lane, the gradient tile out through the same 68-dword rows.
//
// The arithmetic, a function of the row and the parameters alone (not of rows, of the row's place in the call, of the width of the loads):
//   logits[r, k]        = fmaf chain from bias[k] over h = 0 .. 63 ascending of features[r, h] * weight[k, h]           (gmpe_head_rows.h head_dot)
//   grad_features[r, h] = fmaf chain from 0.0f over k = 0 .. K-1 ascending of grad_logits[r, k] * weight[k, h]
// and the parameter gradients in an order that is a function of rows alone (gmpe_wgrad.h, shared with the other layer files):
//   grad_weight[k, h]   = sum over r of grad_logits[r, k] * features[r, h]: partition(rows) parts, a part's exact double products added in ascending row
//                         order (k_head_wgrad: part_products, the columns k >= K of its 64-wide block are zeros), the parts added in ascending order, rounded
//                         to float32 once (k_head_finish: sum_parts);
//   grad_bias[k]        = sum over r of grad_logits[r, k] in double: within a tile of 256 rows the four runs of 64 rows each ascending, the four runs in order
//                         (k_head_bwd_rows), then the tiles as 16 interleaved slices and the slices in slice order, rounded once (k_head_finish: sum_slices).
// No atomics, no allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "gmpe_act_rows.h"      // gmpe_host.h, gmpe_ppo_rows.h; the rollout row's routine and the act plan's checks, shared with gmpe_act.hip
#include "gmpe_head_rows.h"     // the dot product and the features tile
#include "gmpe_wgrad.h"         // the weight-gradient parts and the ordered finish sums, shared with gmpe_gru.hip and gmpe_mlp.hip

#pragma clang fp contract(off)

namespace {

using namespace gmpe_ppo;         // TILE, Geom, Tile, tile_copy
using gmpe_head::H;
using gmpe_head::FS;
using gmpe_head::ROWS_LDS;
using gmpe_wgrad::FIN_COLS;
using gmpe_wgrad::FIN_SLICES;
static_assert(H == gmpe_wgrad::H && TILE == gmpe_wgrad::BLOCK, "gmpe_wgrad.h's workgroup");
static_assert(TILE * (GMPE_PPO_MAX_ACTIONS | 1) <= ROWS_LDS, "the logits tile fits the rows region");
constexpr int NRUN = TILE / 64;                         // runs of 64 rows in a tile's bias sums

struct HeadArgs {
    Geom g;
    const float *feat, *w, *b, *gl;
    float *logits, *gf, *gw, *gb;
    double *partW, *partC;                              // workspace: [nparts][64][64], [ntiles][64]
    int64_t part_rows, ntiles;
    int nparts;
    int vec_feat, vec_w, vec_k, vec_gf;                 // 16-byte units for: features, weight, the [rows, K] arrays, grad_features
};

// a [rows, K] tile between LDS (stride S) and memory
template <bool IN>
__device__ __forceinline__ void tileK(const HeadArgs& p, const Tile& t, float* g, float* sh) {
    if (p.vec_k) tile_copy<true, IN>(g + t.g0, sh, t.n, p.g.K, p.g.S, p.g.magic);
    else tile_copy<false, IN>(g + t.g0, sh, t.n, p.g.K, p.g.S, p.g.magic);
}

__global__ __launch_bounds__(TILE) void k_head_fwd(HeadArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const Tile t = tile_of(p.g, sh);
    gmpe_head::logits_rows(p.feat + t.row0 * H, t.rows, t.live, p.vec_feat, p.w, p.b, p.vec_w, p.g.K, sh, t.row);
    __syncthreads();
    tileK<false>(p, t, p.logits, sh);
}

// gmpe_act_sample's launch with the logits formed here: the features tile, the Linear, then the availability and the row routine of gmpe_act_rows.h
__global__ __launch_bounds__(TILE) void k_head_act(ActArgs p, HeadArgs h) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int K = p.g.K;
    const Tile t = tile_of(p.g, sh);
    uint64_t avail = act_avail0(p, t);
    float* w = sh + ROWS_LDS;
    gmpe_head::params_in(h.w, h.b, K, h.vec_w, w);
    gmpe_head::tile64_copy<true>(const_cast<float*>(h.feat) + t.row0 * H, sh, t.rows, h.vec_feat);
    __syncthreads();
    float x[H];
    gmpe_head::row_in(sh, t.live, x);
    __syncthreads();
    if (p.avail) {                                      // the tile of available_actions passes through the rows the logits then take
        tileK<true>(h, t, const_cast<float*>(p.avail), sh);
        __syncthreads();
        if (t.live) avail = avail_bits(t.row, K);
        __syncthreads();
    }
#pragma unroll 1
    for (int k = 0; k < K; ++k) t.row[k] = gmpe_head::head_dot(x, w + k * H, w[K * H + k]);
    if (h.logits) {
        __syncthreads();
        tileK<false>(h, t, h.logits, sh);
        __syncthreads();                                // the row routine overwrites the row other lanes have just read
    }
    if (!t.live) return;
    act_row(p, t.r, t.row, avail);
}

// backward 1: grad_features of the tile's rows, and the tile's double sums of grad_logits' columns -> partC[tile]
__global__ __launch_bounds__(TILE) void k_head_bwd_rows(HeadArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    __shared__ double bs[NRUN][H];
    const int K = p.g.K, S = p.g.S, tid = threadIdx.x;
    const Tile t = tile_of(p.g, sh);
    float* w = sh + ROWS_LDS;
    gmpe_head::params_in(p.w, nullptr, K, p.vec_w, w);
    tileK<true>(p, t, const_cast<float*>(p.gl), sh);
    __syncthreads();
    {
        const int k = tid & 63, q = tid >> 6, r1 = (q + 1) * 64 < t.rows ? (q + 1) * 64 : t.rows;
        double s = 0.0;
        if (k < K)
            for (int r = q * 64; r < r1; ++r) s += (double)sh[r * S + k];
        bs[q][k] = s;
    }
    float acc[H];
#pragma unroll
    for (int h = 0; h < H; ++h) acc[h] = 0.0f;
    if (p.gf && t.live) {
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const float g = t.row[k];
            const float* wk = w + k * H;
#pragma unroll
            for (int h = 0; h < H; h += 4) {
                const float4 q = *reinterpret_cast<const float4*>(wk + h);
                acc[h] = fmaf(g, q.x, acc[h]); acc[h + 1] = fmaf(g, q.y, acc[h + 1]);
                acc[h + 2] = fmaf(g, q.z, acc[h + 2]); acc[h + 3] = fmaf(g, q.w, acc[h + 3]);
            }
        }
    }
    __syncthreads();                                    // every lane has read its grad_logits row and the runs' sums are written
    if (tid < H) {
        double s = bs[0][tid];
        for (int q = 1; q < NRUN; ++q) s += bs[q][tid];
        p.partC[(int64_t)blockIdx.x * H + tid] = s;     // columns k >= K: zeros
    }
    if (!p.gf) return;
    float* my = sh + tid * FS;
#pragma unroll
    for (int h = 0; h < H; h += 4) *reinterpret_cast<float4*>(my + h) = make_float4(acc[h], acc[h + 1], acc[h + 2], acc[h + 3]);
    __syncthreads();
    gmpe_head::tile64_copy<false>(p.gf + t.row0 * H, sh, t.rows, p.vec_gf);
}

// backward 2: part blockIdx.x of the rows: the [64][64] block of exact double products grad_logits^T features
__global__ __launch_bounds__(TILE) void k_head_wgrad(HeadArgs p) {
    const int K = p.g.K;
    const int64_t m0 = (int64_t)blockIdx.x * p.part_rows, m1 = m0 + p.part_rows < p.g.B ? m0 + p.part_rows : p.g.B;
    gmpe_wgrad::part_products(
        m0, m1, [&](int64_t m, int k) { return k < K ? p.gl[m * K + k] : 0.0f; }, [&](int64_t m, int k) { return p.feat[m * H + k]; },
        p.partW + (int64_t)blockIdx.x * H * H);
}

// backward 3: the partial sums in their fixed order, rounded once. Workgroups 0 .. wblocks-1: one weight element per thread; then 16 bias columns each.
__global__ __launch_bounds__(TILE) void k_head_finish(HeadArgs p, int wblocks) {
    __shared__ double cs[FIN_SLICES][FIN_COLS];
    const int tid = threadIdx.x, K = p.g.K;
    if ((int)blockIdx.x < wblocks) {
        const int e = blockIdx.x * TILE + tid;
        if (p.gw && e < K * H) p.gw[e] = (float)gmpe_wgrad::sum_parts(p.partW, p.nparts, (int64_t)H * H, e);
        return;
    }
    const int col0 = ((int)blockIdx.x - wblocks) * FIN_COLS;
    const double tot = gmpe_wgrad::sum_slices(p.partC, p.ntiles, H, col0, cs);
    if (tid < FIN_COLS && col0 + tid < K && p.gb) p.gb[col0 + tid] = (float)tot;
}

using gmpe::fail;

struct Layout {
    size_t partW, partC, total;
    int64_t ntiles, part_rows;
    int nparts;
};

bool layout(int64_t rows, Layout& y) {
    if (rows < 1 || rows > (int64_t)1 << 40) return false;
    y.ntiles = num_tiles(rows);
    const gmpe_wgrad::Parts parts = gmpe_wgrad::partition(rows);
    y.nparts = parts.nparts; y.part_rows = parts.part_rows;
    gmpe::Carver c;
    y.partW = c.take((size_t)y.nparts * H * H * sizeof(double));
    y.partC = c.take((size_t)y.ntiles * H * sizeof(double));
    y.total = c.total();
    return true;
}

enum Use { FORWARD, BACKWARD, ACT };

// the checks the three entry points make alike, before any device call
int check_plan(const char* fn, const gmpe_head_plan* pl, Use use, Layout& y) {
    if (!pl) return fail(fn, use == ACT ? "null head_plan" : "null plan");
    if (pl->rows < 1) return fail(fn, "rows must be >= 1");
    if (pl->n_actions < 1 || pl->n_actions > GMPE_PPO_MAX_ACTIONS) return fail(fn, "n_actions must be in 1 .. " + std::to_string(GMPE_PPO_MAX_ACTIONS));
    if (pl->hidden != H) return fail(fn, "unsupported hidden = " + std::to_string(pl->hidden) + ": only 64 is built");
    if (!layout(pl->rows, y)) return fail(fn, "rows is too large");
    if (y.ntiles > 0x7fffffffLL) return fail(fn, "rows: too many for one launch");
    const bool bwd = use == BACKWARD;
    const gmpe::PtrField ps[] = {
        {pl->features, "features", true}, {pl->weight, "weight", true}, {pl->bias, "bias", !bwd}, {pl->logits_out, "logits_out", use == FORWARD},
        {pl->grad_logits, "grad_logits", bwd}, {pl->grad_features, "grad_features", false}, {pl->grad_weight, "grad_weight", false},
        {pl->grad_bias, "grad_bias", false}};
    if (int rc = gmpe::check_ptrs(fn, ps)) return rc;
    return gmpe::check_workspace(fn, pl->workspace, pl->workspace_bytes, bwd ? y.total : 0, bwd, "workspace is required",
                                 "gmpe_head_workspace_bytes(rows, n_actions, 1)");
}

HeadArgs bind(const gmpe_head_plan* pl, const Layout& y) {
    HeadArgs a = {};
    a.g = geometry(pl->rows, pl->n_actions);
    a.feat = pl->features; a.w = pl->weight; a.b = pl->bias; a.gl = pl->grad_logits;
    a.logits = pl->logits_out; a.gf = pl->grad_features; a.gw = pl->grad_weight; a.gb = pl->grad_bias;
    a.partW = gmpe::at<double>(pl->workspace, y.partW); a.partC = gmpe::at<double>(pl->workspace, y.partC);
    a.part_rows = y.part_rows; a.ntiles = y.ntiles; a.nparts = y.nparts;
    a.vec_feat = !((uintptr_t)pl->features & 15); a.vec_w = !((uintptr_t)pl->weight & 15); a.vec_gf = !((uintptr_t)pl->grad_features & 15);
    return a;
}

}  // namespace

extern "C" {

int gmpe_head_workspace_bytes(int64_t rows, int32_t n_actions, int32_t want_backward, size_t* bytes_out) {
    const char* fn = "gmpe_head_workspace_bytes";
    Layout y;
    const std::string dims = n_actions < 1 || n_actions > GMPE_PPO_MAX_ACTIONS ? "n_actions must be in 1 .. " + std::to_string(GMPE_PPO_MAX_ACTIONS) : std::string();
    if (int rc = gmpe::check_workspace_query(fn, bytes_out, dims, want_backward)) return rc;
    if (!layout(rows, y)) return fail(fn, "rows must be >= 1 (and not absurd)");
    *bytes_out = want_backward ? y.total : 0;
    return GMPE_OK;
}

int gmpe_head_forward(int device, const gmpe_head_plan* pl, void* stream) {
    Layout y;
    if (int rc = check_plan("gmpe_head_forward", pl, FORWARD, y)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_head_fwd), device, 0, gmpe_head::LDS_MAX)) return rc;
    HeadArgs a = bind(pl, y);
    a.vec_k = !((uintptr_t)pl->logits_out & 15);        // tiles start at multiples of 1 KiB
    GMPE_LAUNCH(k_head_fwd, dim3((unsigned)y.ntiles), dim3(TILE), gmpe_head::lds_bytes(pl->n_actions), static_cast<hipStream_t>(stream), a);
    return GMPE_OK;
}

int gmpe_head_backward(int device, const gmpe_head_plan* pl, void* stream) {
    Layout y;
    if (int rc = check_plan("gmpe_head_backward", pl, BACKWARD, y)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_head_bwd_rows), device, 1, gmpe_head::LDS_MAX)) return rc;
    HeadArgs a = bind(pl, y);
    a.vec_k = !((uintptr_t)pl->grad_logits & 15);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = pl->n_actions, wblocks = (K * H + TILE - 1) / TILE;
    GMPE_LAUNCH(k_head_bwd_rows, dim3((unsigned)y.ntiles), dim3(TILE), gmpe_head::lds_bytes(K), st, a);
    if (pl->grad_weight) GMPE_LAUNCH(k_head_wgrad, dim3((unsigned)y.nparts), dim3(TILE), 0, st, a);
    GMPE_LAUNCH(k_head_finish, dim3((unsigned)(wblocks + H / FIN_COLS)), dim3(TILE), 0, st, a, wblocks);
    return GMPE_OK;
}

int gmpe_act_head(int device, const gmpe_act_plan* ap, const gmpe_head_plan* hp, void* stream) {
    const char* fn = "gmpe_act_head";
    Layout y;
    if (int rc = gmpe::check_act_plan(fn, ap, false)) return rc;
    if (int rc = check_plan(fn, hp, ACT, y)) return rc;
    if (hp->rows != ap->rows) return fail(fn, "head_plan->rows differs from act_plan->rows");
    if (hp->n_actions != ap->n_actions) return fail(fn, "head_plan->n_actions differs from act_plan->n_actions");
    GMPE_HIP_CHECK(hipSetDevice(device));
    if (int rc = gmpe::raise_dynamic_lds_once(reinterpret_cast<const void*>(k_head_act), device, 2, gmpe_head::LDS_MAX)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ActArgs a = act_args(ap);
    HeadArgs h = bind(hp, y);
    h.vec_k = !(((uintptr_t)hp->logits_out | (uintptr_t)ap->available_actions) & 15);
    GMPE_LAUNCH(k_head_act, dim3((unsigned)y.ntiles), dim3(TILE), gmpe_head::lds_bytes(ap->n_actions), st, a, h);
    if (ap->draw_dev && ap->draw_inc) return gmpe::act_advance(ap->draw_dev, ap->draw_inc, st);   // adding zero changes nothing: no launch
    return GMPE_OK;
}

}  // extern "C"
