// The row grid: a grid of ROWS (loop perturbations, disturbances) over the plants of a handle in ONE launch and a finishing launch --
// the driver of pime_margin_sweep (margin_sweep.hip) and pime_disturb_sweep (disturb_sweep.hip), which supply a descriptor (below).
//
// Tiling.  A wave carries one TILE of pairs of ONE row, so whatever the row decodes to is wave-uniform (scalar loads of the row,
// uniform branches and switches on its fields).  With a policy a tile is 16 plants -- policy_forward16 (rollout_policy.hpp) on the
// packed image in LDS, the four lane groups holding bit-equal copies, lane group 0 storing; under the prior alone a tile is 64
// distinct plants and there is no LDS.  Tiles are numbered row-major (p * tiles_per_row + tile of the row); a 256-thread workgroup
// takes a QUAD of four consecutive tiles, one per wave (one wave per SIMD), and workgroups are PERSISTENT: the image is staged once
// per workgroup, then the workgroup walks quads blockIdx.x, blockIdx.x + gridDim.x, ...  There is no barrier after the staging one
// (policy_forward16 has none), so the four waves run their tiles independently and a wave past the last tile simply skips.  Every
// pair writes its rows into `pairs` (or the workspace copy when `pairs` is NULL); row_grid_finish_kernel (row_grid.hip), one wave
// per (row, segment, metric row), folds the plants of a row in the order pime_prior_sweep documents: blocks of 64 plants, the xor
// butterfly inside a block (the balanced pairwise tree over the index bits), the blocks in ascending sequence.  No atomics: two calls
// give the same bits; every workspace word read was written by the call.
//
// A descriptor `Sweep` is a plain struct of what differs between the sweeps, all of it resolved at compile time:
//   Args<S>            the kernel's argument block (env, n, P, n_seg, env_offset, the plant blocks, img, K, s and the sweep's own)
//   Row, row(r)        a decoded row of the grid and its decoder; kCols doubles per row
//   kRows              the metric rows a pair stores per segment
//   Sink               RowGridSink with the operator() the sweep's pair function calls per finished segment
//   ph(...), wt(...)   load lane i and run the sweep's pair function on it
//   kNoun              the sweep's name in "no ... sweep instantiation"
// Device only.
#pragma once
#include "prior_sweep.hpp"
#include "rollout_policy.hpp"

namespace pime {

constexpr int kRowGridThreads = 256;   // four waves: a quad of tiles

int mlp_check(int kind, int D, int Di, int md);

// summary[P][cells][PIME_SWEEP_STATS] from rows[cells][P][N] (row_grid.hip)
int launch_row_grid_finish(int P, int N, int cells, const double* rows, double* summary, hipStream_t stream);

// the policy of a device pair: the forward of the rollout kernels on the image in LDS
template <int T, int KIND>
struct RowGridPolicy {
    static constexpr bool kPolicy = true;
    const float* __restrict__ lds;
    MlpLayout L;
    int lane;
    template <int D>
    __device__ __forceinline__ float operator()(const float (&om)[D]) const {
        PIME_NO_HOIST();
        return policy_forward16<T, KIND, D, 1>(lds, L, om, lane);
    }
};

struct RowGridSink {
    double* __restrict__ rows;       // [n_seg][ROWS][P * N]: `pairs`, or the workspace copy
    double* __restrict__ actions;    // [n_steps][P * N] or nullptr
    double* __restrict__ outputs;    // [n_steps][P * N] or nullptr
    size_t PN, col;                  // P * N, p * N + i
    bool writer;                     // the one copy of a valid pair that stores

    __device__ __forceinline__ void step(int t, double u, double y) const {
        if (writer) {
            if (actions != nullptr) actions[(size_t)t * PN + col] = u;
            if (outputs != nullptr) outputs[(size_t)t * PN + col] = y;
        }
    }
    // the rows of a finished segment (the writer's: the caller has asked)
    template <int ROWS>
    __device__ __forceinline__ void store(int seg, const double (&v)[ROWS]) const {
#pragma unroll
        for (int row = 0; row < ROWS; ++row) rows[((size_t)seg * ROWS + row) * PN + col] = v[row];
    }
};

template <typename Sweep, int T, int KIND, int ENV, typename S>
__global__ __launch_bounds__(kRowGridThreads) void row_grid_kernel(const typename Sweep::template Args<S> a,
                                                                   const double* __restrict__ grid_rows, double* __restrict__ rows,
                                                                   double* __restrict__ actions, double* __restrict__ outputs,
                                                                   int tiles_per_row, long long n_tiles, long long n_quads) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int D = ENV == 0 ? 3 : 4;
    constexpr bool POLICY = KIND >= 0;
    constexpr int TILE = POLICY ? 16 : 64;
    MlpLayout L{};
    if constexpr (POLICY) {
        L = mlp_layout(KIND, D, 1, T * 32);
        stage_image(lds, a.img, L.total / 4);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int N = a.n;
    double K[D];
#pragma unroll
    for (int j = 0; j < D; ++j) K[j] = a.K.k[j];
    for (long long q = blockIdx.x; q < n_quads; q += gridDim.x) {
        PIME_NO_HOIST();
        const long long tile = q * (kRowGridThreads / 64) + wave;   // wave-uniform
        if (tile >= n_tiles) continue;
        const int p = (int)(tile / tiles_per_row), tr = (int)(tile - (long long)p * tiles_per_row);
        const int m = tr * TILE + (POLICY ? (lane & 15) : lane);
        const bool valid = m < N;
        const int i = valid ? m : N - 1;   // idle lanes shadow the last plant (compute, never store)
        const typename Sweep::Row row = Sweep::row(grid_rows + (size_t)p * Sweep::kCols);
        typename Sweep::Sink sink{{rows, actions, outputs, (size_t)a.P * N, (size_t)p * N + i, valid && (!POLICY || (lane >> 4) == 0)}};
        if constexpr (POLICY) {
            const RowGridPolicy<T, KIND> pol{lds, L, lane};
            if constexpr (ENV == 0) Sweep::template ph<S>(a, i, K, row, pol, sink);
            else Sweep::template wt<S>(a, i, K, row, pol, sink);
        } else {
            if constexpr (ENV == 0) Sweep::template ph<S>(a, i, K, row, PriorOnlyPolicy{}, sink);
            else Sweep::template wt<S>(a, i, K, row, PriorOnlyPolicy{}, sink);
        }
    }
}

template <typename Sweep, int T, int KIND, int ENV, typename S>
static int launch_row_grid_k(const typename Sweep::template Args<S>& a, const double* grid_rows, double* rows, double* actions,
                             double* outputs, hipStream_t s) {
    constexpr bool POLICY = KIND >= 0;
    constexpr int TILE = POLICY ? 16 : 64;
    size_t lds_bytes = 0;
    if constexpr (POLICY) {
        lds_bytes = (size_t)mlp_layout(KIND, ENV == 0 ? 3 : 4, 1, T * 32).total * sizeof(float);
        static LdsLimit lds_limit;  // per instantiation
        PIME_RAISE_LDS(lds_limit, (row_grid_kernel<Sweep, T, KIND, ENV, S>), 160 * 1024);
    }
    int dev = 0, cus = 0;
    PIME_HIP_TRY(hipGetDevice(&dev));
    PIME_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int tiles_per_row = (a.n + TILE - 1) / TILE;
    const long long n_tiles = (long long)a.P * tiles_per_row;
    const long long n_quads = (n_tiles + kRowGridThreads / 64 - 1) / (kRowGridThreads / 64);
    // resident workgroups per compute unit: what the image leaves of the 160 KB of LDS (one at width 128), eight without an image
    const int per_cu = POLICY ? (int)((160 * 1024) / lds_bytes > 4 ? 4 : (160 * 1024) / lds_bytes) : 8;
    const long long cap = (long long)(cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1);
    const unsigned grid = (unsigned)(n_quads < cap ? n_quads : cap);
    hipLaunchKernelGGL((row_grid_kernel<Sweep, T, KIND, ENV, S>), dim3(grid), dim3(kRowGridThreads), lds_bytes, s, a, grid_rows, rows,
                       actions, outputs, tiles_per_row, n_tiles, n_quads);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

// the grid launch of the served class (width, kind, env), then the finishing launch
template <typename Sweep, typename S>
int launch_row_grid(int kind, int md, const typename Sweep::template Args<S>& a, const double* grid_rows, double* pairs, double* summary,
                    double* actions, double* outputs, double* workspace, hipStream_t stream) {
    if (kind >= 0) {
        if (int rc = mlp_check(kind, a.env == 0 ? 3 : 4, kind == MLP_MODULAR_ACTOR ? 1 : 0, md)) return rc;
    }
    double* rows = pairs != nullptr ? pairs : workspace;
    const int T = kind < 0 ? 0 : md / 32;
    int rc = -1;
#define PIME_RG(TT, KK, EE)                       \
    if (T == TT && kind == KK && a.env == EE)     \
        rc = launch_row_grid_k<Sweep, (TT == 0 ? 2 : TT), KK, EE, S>(a, grid_rows, rows, actions, outputs, stream);
    PIME_RG(0, -1, 0) PIME_RG(0, -1, 1)
    PIME_RG(4, MLP_MODULAR_ACTOR, 0) PIME_RG(2, MLP_MODULAR_ACTOR, 0) PIME_RG(4, MLP_PLAIN_ACTOR, 0) PIME_RG(2, MLP_PLAIN_ACTOR, 0)
    PIME_RG(4, MLP_MODULAR_ACTOR, 1) PIME_RG(2, MLP_MODULAR_ACTOR, 1) PIME_RG(4, MLP_PLAIN_ACTOR, 1) PIME_RG(2, MLP_PLAIN_ACTOR, 1)
    PIME_RG(4, MLP_SAC_ACTOR, 0) PIME_RG(2, MLP_SAC_ACTOR, 0) PIME_RG(4, MLP_SAC_ACTOR, 1) PIME_RG(2, MLP_SAC_ACTOR, 1)
    PIME_RG(4, MLP_CRITIC, 0) PIME_RG(2, MLP_CRITIC, 0) PIME_RG(4, MLP_CRITIC, 1) PIME_RG(2, MLP_CRITIC, 1)
#undef PIME_RG
    if (rc == -1) {
        set_error("no %s sweep instantiation for env %d kind %d width %d", Sweep::kNoun, a.env, kind, md);
        return PIME_ERR_ARG;
    }
    if (rc != PIME_OK) return rc;
    return launch_row_grid_finish(a.P, a.n, a.n_seg * Sweep::kRows, rows, summary, stream);
}

}  // namespace pime
