// pime_policy_sweep: a grid of P POLICIES (packed image p, prior gain K[p]) over the plants of a handle in one launch and the
// finishing launch of the row grid (row_grid.hpp: RowGridPolicy, RowGridSink, policy_forward16, launch_row_grid_finish, all as they
// are; policy_sweep.hpp has the pair function).  What the row grid's driver cannot do is change the image: row_grid_kernel stages
// one image per workgroup, once.  Here the image depends on the row, so this file has a driver of its own.
//
// Tiling.  A tile is 16 plants of one row, the four lane groups of a wave holding bit-equal copies, lane group 0 storing.  A
// 256-thread workgroup takes a QUAD of four tiles of the SAME row, one per wave: quads_per_row = ceil(tiles_per_row / 4), quad q is
// row p = q / quads_per_row, tiles 4 * (q % quads_per_row) .. + 3 of that row, so a quad never straddles rows.  Workgroups are
// persistent and each walks a CONTIGUOUS range of quads [q0, q1), q0 = floor(b * n_quads / grid): consecutive quads share a row, and
// the image in LDS (ONE buffer: at width 128 it is 131 KB of the 160 KB) is re-staged only when p changes -- barrier, stage_image
// of image p, barrier.  K[p] is read from the device table with the row, wave-uniform (scalar loads).
//
// Why the barriers cannot hang.  __syncthreads sits inside the persistent loop, so every wave of a workgroup must reach every one of
// them the same number of times:
//   (1) the loop bounds q0 and q1 are functions of blockIdx.x, gridDim.x and the kernel argument n_quads alone -- the same value in
//       every thread of the workgroup; the loop has no `continue`, `break` or `return`, and nothing a lane or a wave computes feeds
//       its condition;
//   (2) the row p is a function of q and the kernel argument quads_per_row; `staged` starts at -1 and is assigned p under the test
//       p != staged only: both are workgroup-uniform, so either all 256 threads take the re-staging branch with its two barriers or
//       none does;
//   (3) a wave whose tile lies past the row's last tile (tr >= tiles_per_row: the idle waves of a row's last quad) skips the PAIR
//       WORK inside `if (tr < tiles_per_row)`, which holds no barrier (policy_forward16 has none, the pair functions have none, the
//       sink only stores), and then meets the next iteration's test like every other wave.  row_grid_kernel lets such a wave
//       `continue` because it has no barrier after the staging one; that form is not copied here;
//   (4) inside a tile the lanes past the last plant shadow plant N - 1 (compute, never store): no lane leaves the wave early.
// The first barrier of a re-staging keeps a fast wave from overwriting the image a slow wave of the previous quad still reads; the
// second publishes the new image.  stage_image reads L.total / 4 float4s from img + p * stride: the entry point has checked
// stride >= L.total, stride % 4 == 0 and the 16-byte alignment of the base, so every read lies inside image p's slot.
// No atomics: two calls give the same bits; every workspace word the finishing launch reads was written by this call's pairs.
#include "policy_sweep.hpp"
#include "row_grid.hpp"

namespace pime {

struct PolicySink : RowGridSink {
    __device__ __forceinline__ void operator()(int seg, const SegMetrics& M) const {
        if (writer) {
            double v[PIME_METRIC_ROWS];
            sweep_rows(M, v);
            store(seg, v);
        }
    }
};

template <int T, int KIND, int ENV, typename S>
__global__ __launch_bounds__(kRowGridThreads) void policy_sweep_kernel(const PolicyArgs<S> a, double* __restrict__ rows,
                                                                       double* __restrict__ actions, double* __restrict__ outputs,
                                                                       int tiles_per_row, int quads_per_row, long long n_quads) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int D = ENV == 0 ? 3 : 4;
    constexpr int TILE = 16, WAVES = kRowGridThreads / 64;
    const MlpLayout L = mlp_layout(KIND, D, 1, T * 32);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int N = a.n;
    // the workgroup's contiguous range of quads: workgroup-uniform (header, (1))
    const long long q0 = (long long)blockIdx.x * n_quads / gridDim.x, q1 = ((long long)blockIdx.x + 1) * n_quads / gridDim.x;
    int staged = -1;
    for (long long q = q0; q < q1; ++q) {
        PIME_NO_HOIST();
        const int p = (int)(q / quads_per_row), qr = (int)(q - (long long)p * quads_per_row);
        if (p != staged) {   // workgroup-uniform (header, (2)): every wave is done with the old image, then the new one is published
            __syncthreads();
            stage_image(lds, a.img + (size_t)p * (size_t)a.stride, L.total / 4);
            __syncthreads();
            staged = p;
        }
        const int tr = qr * WAVES + wave;   // wave-uniform
        if (tr < tiles_per_row) {           // an idle wave skips the pair work, never a barrier (header, (3))
            const int m = tr * TILE + (lane & 15);
            const bool valid = m < N;
            const int i = valid ? m : N - 1;   // idle lanes shadow the last plant (compute, never store)
            double K[D];
#pragma unroll
            for (int j = 0; j < D; ++j) K[j] = a.K[(size_t)p * D + j];
            PolicySink sink{{rows, actions, outputs, (size_t)a.P * N, (size_t)p * N + i, valid && (lane >> 4) == 0}};
            const RowGridPolicy<T, KIND> pol{lds, L, lane};
            if constexpr (ENV == 0) {
                PhLane<S> E{};
                ph_lane_load<S>(a.p, a.st, i, E);
                policy_ph_pair<S>(a.p, a.st.table, E, K, a.s, pol, sink);
            } else {
                const uint32_t gid = a.env_offset + (uint32_t)i;
                WtLane<S> W{};
                wt_lane_load<S>(a.wp, a.wst, i, W);
                policy_wt_pair<S>(a.wp, gid, W, K, a.s, pol, sink);
            }
        }
    }
}

template <int T, int KIND, int ENV, typename S>
static int launch_policy_sweep_k(const PolicyArgs<S>& a, double* rows, double* actions, double* outputs, hipStream_t s) {
    constexpr int TILE = 16, WAVES = kRowGridThreads / 64;
    const size_t lds_bytes = (size_t)mlp_layout(KIND, ENV == 0 ? 3 : 4, 1, T * 32).total * sizeof(float);
    static LdsLimit lds_limit;  // per instantiation
    PIME_RAISE_LDS(lds_limit, (policy_sweep_kernel<T, KIND, ENV, S>), 160 * 1024);
    int dev = 0, cus = 0;
    PIME_HIP_TRY(hipGetDevice(&dev));
    PIME_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int tiles_per_row = (a.n + TILE - 1) / TILE;
    const int quads_per_row = (tiles_per_row + WAVES - 1) / WAVES;
    const long long n_quads = (long long)a.P * quads_per_row;
    // resident workgroups per compute unit: the rule of launch_row_grid_k (what the image leaves of the 160 KB of LDS, at most four)
    const int per_cu = (int)((160 * 1024) / lds_bytes > 4 ? 4 : (160 * 1024) / lds_bytes);
    const long long cap = (long long)(cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1);
    const unsigned grid = (unsigned)(n_quads < cap ? n_quads : cap);
    hipLaunchKernelGGL((policy_sweep_kernel<T, KIND, ENV, S>), dim3(grid), dim3(kRowGridThreads), lds_bytes, s, a, rows, actions, outputs,
                       tiles_per_row, quads_per_row, n_quads);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

// the grid launch of the served class (width, kind, env), then the finishing launch of the row grid
template <typename S>
int launch_policy_sweep(int kind, int md, const PolicyArgs<S>& a, double* pairs, double* summary, double* actions, double* outputs,
                        double* workspace, hipStream_t stream) {
    if (int rc = mlp_check(kind, a.env == 0 ? 3 : 4, kind == MLP_MODULAR_ACTOR ? 1 : 0, md)) return rc;
    double* rows = pairs != nullptr ? pairs : workspace;
    const int T = md / 32;
    int rc = -1;
#define PIME_PS(TT, KK, EE) \
    if (T == TT && kind == KK && a.env == EE) rc = launch_policy_sweep_k<TT, KK, EE, S>(a, rows, actions, outputs, stream);
    PIME_PS(4, MLP_MODULAR_ACTOR, 0) PIME_PS(2, MLP_MODULAR_ACTOR, 0) PIME_PS(4, MLP_PLAIN_ACTOR, 0) PIME_PS(2, MLP_PLAIN_ACTOR, 0)
    PIME_PS(4, MLP_MODULAR_ACTOR, 1) PIME_PS(2, MLP_MODULAR_ACTOR, 1) PIME_PS(4, MLP_PLAIN_ACTOR, 1) PIME_PS(2, MLP_PLAIN_ACTOR, 1)
    PIME_PS(4, MLP_SAC_ACTOR, 0) PIME_PS(2, MLP_SAC_ACTOR, 0) PIME_PS(4, MLP_SAC_ACTOR, 1) PIME_PS(2, MLP_SAC_ACTOR, 1)
    PIME_PS(4, MLP_CRITIC, 0) PIME_PS(2, MLP_CRITIC, 0) PIME_PS(4, MLP_CRITIC, 1) PIME_PS(2, MLP_CRITIC, 1)
#undef PIME_PS
    if (rc == -1) {
        set_error("no policy sweep instantiation for env %d kind %d width %d", a.env, kind, md);
        return PIME_ERR_ARG;
    }
    if (rc != PIME_OK) return rc;
    return launch_row_grid_finish(a.P, a.n, a.n_seg * PIME_METRIC_ROWS, rows, summary, stream);
}

template int launch_policy_sweep<double>(int, int, const PolicyArgs<double>&, double*, double*, double*, double*, double*, hipStream_t);
template int launch_policy_sweep<float>(int, int, const PolicyArgs<float>&, double*, double*, double*, double*, double*, hipStream_t);

}  // namespace pime
