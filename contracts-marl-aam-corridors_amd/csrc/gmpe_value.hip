// gmpe_value.hip — the critic's value head on the device (include/gmpe.h gmpe_value_forward / gmpe_value_backward): v_out of the reference's GR_Critic
// (onpolicy/algorithms/graph_actor_critic.py:395), an nn.Linear(64, 1) or a PopArt(64, 1) read as one: weight [1, 64], bias [1]. Forward is ONE launch,
// backward TWO. It is a bandwidth-bound row pass: 256 B read per row, 4 B written (forward); 4 B + 256 B read, 256 B written (backward).
//
// Mapping (the feature mapping of gmpe_ppo_popart.hip at H = 64). A workgroup of 256 lanes owns a tile of TILE = 256 rows; wave w owns rows 64w .. 64w+63 of
// the tile and works on four of them at once: lane = sub * 16 + c holds columns 4c .. 4c+3 of row 4 * pass + sub, pass = 0 .. 15, so a wave instruction moves
// four whole rows, 1 KiB contiguous, 16 bytes per lane (4-byte units where the array is not 16-byte aligned: the same registers, the same arithmetic).
// Nothing goes through LDS on the way in. The 64 values of a wave go out as one contiguous 256-byte store: lane l takes the value of row l from the lane
// group that formed it (one cross-lane read per pass).
//
// The arithmetic, a function of the row and the parameters alone (not of rows, of the row's place in the call, of the width of the loads):
//   values[r]           = the dot product gmpe_ppo_loss_popart evaluates at H = 64, bit for bit: acc = 0.0f; acc = acc + f[i] * w[i] for the lane's four
//                         columns ascending, multiply and add each rounded on its own; the 16 lanes of the row by an xor tree over offsets 1, 2, 4, 8 with
//                         the lower lane as the left operand; then + bias.
//   grad_features[r, j] = grad_values[r] * weight[j], one float32 product.
// and the parameter gradients in an order that is a function of rows alone:
//   grad_weight[j]      = sum over r of grad_values[r] * features[r, j], grad_bias = sum over r of grad_values[r], of exact double products: a lane over
//                         its 16 passes ascending, the wave's four row groups by an xor tree (offsets 16, 32, the lower lane the left operand), the four
//                         waves in wave order: one row of COLS doubles per tile (k_value_bwd_rows); then the tiles as 16 interleaved slices and the slices
//                         in slice order, rounded to float32 once (k_value_finish: gmpe_wgrad.h sum_slices).
// No atomics, no allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "gmpe_host.h"          // include/gmpe.h, the error text, GMPE_HIP_CHECK, the plan and workspace checks of the layer files
#include "gmpe_wgrad.h"         // the ordered slice sums, shared with the other layer files

#pragma clang fp contract(off)

namespace {

constexpr int H = 64, TILE = 256, NW = TILE / 64;
constexpr int LANES = H / 4;                            // lanes per row
constexpr int RP = 64 / LANES, PASSES = 64 / RP;        // rows per pass of a wave, passes per wave
constexpr int COLS = 80;                                // a tile's row of partial sums: 64 weight columns, the bias column, zeros up to 5 * FIN_COLS
using gmpe_wgrad::FIN_COLS;
using gmpe_wgrad::FIN_SLICES;
static_assert(H == gmpe_wgrad::H && TILE == gmpe_wgrad::BLOCK && COLS % FIN_COLS == 0 && COLS > H, "gmpe_wgrad.h's workgroup");

struct ValueArgs {
    int64_t rows, ntiles;
    const float *feat, *w, *b, *gv;
    float *values, *gf, *gw, *gb;
    double* part;                                       // workspace: [ntiles][COLS]
};

// columns 4c .. 4c+3 of a features row
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* __restrict__ p, float (&f)[4]) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = p[i];
    }
}

// forward: the values of tile blockIdx.x
template <bool VEC>
__global__ __launch_bounds__(TILE) void k_value_fwd(ValueArgs p) {
    const int lane = threadIdx.x & 63, wv0 = (int)(threadIdx.x >> 6) * 64;
    const int c = lane & (LANES - 1), sub = lane / LANES;
    const int64_t row0 = (int64_t)blockIdx.x * TILE + wv0;                  // the wave's first row
    float wq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wq[i] = p.w[4 * c + i];
    const float bias = *p.b;
    float mine = 0.0f;
#pragma unroll 4
    for (int ps = 0; ps < PASSES; ++ps) {
        const int64_t r = row0 + ps * RP + sub;
        float acc = 0.0f;
        if (r < p.rows) {
            float f[4];
            load_quad<VEC>(p.feat + r * H + 4 * c, f);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __fadd_rn(acc, __fmul_rn(f[i], wq[i]));
        }
#pragma unroll
        for (int off = 1; off < LANES; off <<= 1) {                         // every lane of the wave takes part; lanes of other rows are never mixed in
            const float o = __shfl_xor(acc, off);
            acc = (lane & off) ? __fadd_rn(o, acc) : __fadd_rn(acc, o);
        }
        const float v = __shfl(__fadd_rn(acc, bias), (lane & (RP - 1)) * LANES);    // row 4 * ps + (lane % 4), from the group that holds it
        if ((lane >> 2) == ps) mine = v;
    }
    if (row0 + lane < p.rows) p.values[row0 + lane] = mine;
}

// backward 1: grad_features of tile blockIdx.x, and the tile's double sums of g * F over its rows and of g -> part[tile]
template <bool VEC>
__global__ __launch_bounds__(TILE) void k_value_bwd_rows(ValueArgs p) {
    __shared__ double colsum[COLS];
    const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6), wv0 = wave * 64;
    const int c = lane & (LANES - 1), sub = lane / LANES;
    const int64_t row0 = (int64_t)blockIdx.x * TILE + wv0;
    const bool sums = p.gw || p.gb;
    float wq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wq[i] = p.w[4 * c + i];
    double da[4] = {0.0, 0.0, 0.0, 0.0}, dg = 0.0;
#pragma unroll 4
    for (int ps = 0; ps < PASSES; ++ps) {
        const int64_t r = row0 + ps * RP + sub;
        if (r < p.rows) {
            const float g = p.gv[r];
            const double gd = (double)g;
            if (sums) {
                float f[4];
                load_quad<VEC>(p.feat + r * H + 4 * c, f);
#pragma unroll
                for (int i = 0; i < 4; ++i) da[i] += gd * (double)f[i];     // the product is exact in double
                dg += gd;
            }
            if (p.gf) {
                float* gr = p.gf + r * H + 4 * c;
                if (VEC) {
                    *reinterpret_cast<float4*>(gr) = make_float4(__fmul_rn(g, wq[0]), __fmul_rn(g, wq[1]), __fmul_rn(g, wq[2]), __fmul_rn(g, wq[3]));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) gr[i] = __fmul_rn(g, wq[i]);
                }
            }
        }
    }
    if (!sums) return;                                                      // uniform over the launch
#pragma unroll
    for (int off = LANES; off < 64; off <<= 1) {                            // the wave's four row groups, the lower lane the left operand
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double o = __shfl_xor(da[i], off);
            da[i] = (lane & off) ? o + da[i] : da[i] + o;
        }
        const double o = __shfl_xor(dg, off);
        dg = (lane & off) ? o + dg : dg + o;
    }
    for (int w = 0; w < NW; ++w) {                                          // the four waves in wave order
        if (wave == w && sub == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) colsum[4 * c + i] = w == 0 ? da[i] : colsum[4 * c + i] + da[i];
            if (c == 0) colsum[H] = w == 0 ? dg : colsum[H] + dg;
        }
        __syncthreads();
    }
    if (threadIdx.x < COLS) p.part[(int64_t)blockIdx.x * COLS + threadIdx.x] = threadIdx.x <= H ? colsum[threadIdx.x] : 0.0;
}

// backward 2: the tiles' rows in their fixed order, rounded once; workgroup b owns columns 16b .. 16b+15 of COLS
__global__ __launch_bounds__(TILE) void k_value_finish(ValueArgs p) {
    __shared__ double cs[FIN_SLICES][FIN_COLS];
    const int col0 = (int)blockIdx.x * FIN_COLS, col = col0 + (int)threadIdx.x;
    const double tot = gmpe_wgrad::sum_slices(p.part, p.ntiles, COLS, col0, cs);
    if ((int)threadIdx.x >= FIN_COLS) return;
    if (col < H) {
        if (p.gw) p.gw[col] = (float)tot;
    } else if (col == H && p.gb) {
        *p.gb = (float)tot;
    }
}

using gmpe::fail;

bool layout(int64_t rows, int64_t& ntiles, size_t& total) {
    if (rows < 1 || rows > (int64_t)1 << 40) return false;
    ntiles = (rows + TILE - 1) / TILE;
    gmpe::Carver c;
    c.take((size_t)ntiles * COLS * sizeof(double));
    total = c.total();
    return true;
}

// the checks the two entry points make alike, before any device call
int check_plan(const char* fn, const gmpe_value_plan* pl, bool bwd, int64_t& ntiles) {
    if (!pl) return fail(fn, "null plan");
    if (pl->rows < 1) return fail(fn, "rows must be >= 1");
    if (pl->hidden != H) return fail(fn, "unsupported hidden = " + std::to_string(pl->hidden) + ": only 64 is built");
    size_t total;
    if (!layout(pl->rows, ntiles, total)) return fail(fn, "rows is too large");
    if (ntiles > 0x7fffffffLL) return fail(fn, "rows: too many for one launch");
    const gmpe::PtrField ps[] = {
        {pl->features, "features", true}, {pl->weight, "weight", true}, {pl->bias, "bias", !bwd}, {pl->values_out, "values_out", !bwd},
        {pl->grad_values, "grad_values", bwd}, {pl->grad_features, "grad_features", false}, {pl->grad_weight, "grad_weight", false},
        {pl->grad_bias, "grad_bias", false}};
    if (int rc = gmpe::check_ptrs(fn, ps)) return rc;
    return gmpe::check_workspace(fn, pl->workspace, pl->workspace_bytes, bwd ? total : 0, bwd, "workspace is required",
                                 "gmpe_value_workspace_bytes(rows, 1)");
}

ValueArgs bind(const gmpe_value_plan* pl, int64_t ntiles) {
    ValueArgs a = {};
    a.rows = pl->rows; a.ntiles = ntiles;
    a.feat = pl->features; a.w = pl->weight; a.b = pl->bias; a.gv = pl->grad_values;
    a.values = pl->values_out; a.gf = pl->grad_features; a.gw = pl->grad_weight; a.gb = pl->grad_bias;
    a.part = gmpe::at<double>(pl->workspace, 0);
    return a;
}

}  // namespace

extern "C" {

int gmpe_value_workspace_bytes(int64_t rows, int32_t want_backward, size_t* bytes_out) {
    const char* fn = "gmpe_value_workspace_bytes";
    if (int rc = gmpe::check_workspace_query(fn, bytes_out, std::string(), want_backward)) return rc;
    int64_t ntiles;
    size_t total;
    if (!layout(rows, ntiles, total)) return fail(fn, "rows must be >= 1 (and not absurd)");
    *bytes_out = want_backward ? total : 0;
    return GMPE_OK;
}

int gmpe_value_forward(int device, const gmpe_value_plan* pl, void* stream) {
    int64_t ntiles;
    if (int rc = check_plan("gmpe_value_forward", pl, false, ntiles)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    const ValueArgs a = bind(pl, ntiles);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((uintptr_t)pl->features & 15) GMPE_LAUNCH(k_value_fwd<false>, dim3((unsigned)ntiles), dim3(TILE), 0, st, a);
    else GMPE_LAUNCH(k_value_fwd<true>, dim3((unsigned)ntiles), dim3(TILE), 0, st, a);
    return GMPE_OK;
}

int gmpe_value_backward(int device, const gmpe_value_plan* pl, void* stream) {
    int64_t ntiles;
    if (int rc = check_plan("gmpe_value_backward", pl, true, ntiles)) return rc;
    GMPE_HIP_CHECK(hipSetDevice(device));
    const ValueArgs a = bind(pl, ntiles);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (((uintptr_t)pl->features | (uintptr_t)pl->grad_features) & 15) GMPE_LAUNCH(k_value_bwd_rows<false>, dim3((unsigned)ntiles), dim3(TILE), 0, st, a);
    else GMPE_LAUNCH(k_value_bwd_rows<true>, dim3((unsigned)ntiles), dim3(TILE), 0, st, a);
    if (pl->grad_weight || pl->grad_bias) GMPE_LAUNCH(k_value_finish, dim3(COLS / FIN_COLS), dim3(TILE), 0, st, a);
    return GMPE_OK;
}

}  // extern "C"
