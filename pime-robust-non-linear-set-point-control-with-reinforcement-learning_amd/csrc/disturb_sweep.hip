// pime_disturb_sweep: a grid of disturbances (a load step at the plant input, a step of the plant parameters; a pulse of either)
// over the plants of a handle in ONE launch (disturb_sweep.hpp has the pair function) and a finishing launch.
//
// Tiling: that of margin_sweep.hip.  A wave carries one TILE of pairs of ONE disturbance row, so the onset, the length, the load and
// the multipliers are wave-uniform (scalar loads of `disturb`; "is the row active at step k" is a uniform branch, and so is the
// choice between the two plant sets a pair holds in registers).  With a policy a tile is 16 plants -- policy_forward16
// (rollout_policy.hpp) on the packed image in LDS, the four lane groups holding bit-equal copies, lane group 0 storing; under the
// prior alone a tile is 64 distinct plants and there is no LDS.  Tiles are numbered row-major (p * tiles_per_row + tile of the row);
// a 256-thread workgroup takes a QUAD of four consecutive tiles, one per wave, and workgroups are PERSISTENT: the image is staged
// once per workgroup, then the workgroup walks quads blockIdx.x, blockIdx.x + gridDim.x, ...  There is no barrier after the staging
// one, so a wave past the last tile simply skips.  Every pair writes its fifteen rows into `pairs` (or the workspace copy when
// `pairs` is NULL); disturb_sweep_finish_kernel, one wave per (row, segment, metric row), folds the plants of a disturbance row in the
// order pime_prior_sweep documents: blocks of 64 plants, the xor butterfly inside a block, the blocks in ascending sequence.  No
// atomics: two calls give the same bits; every workspace word read was written by the call.
#include "disturb_sweep.hpp"
#include "rollout_policy.hpp"

namespace pime {

constexpr int kDisturbThreads = 256;   // four waves: a quad of tiles

int mlp_check(int kind, int D, int Di, int md);

// the policy of a device pair: the forward of the rollout kernels on the image in LDS
template <int T, int KIND>
struct DisturbDevicePolicy {
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

struct DisturbDeviceSink {
    double* __restrict__ rows;       // [n_seg][kDisturbAllRows][P * N]: `pairs`, or the workspace copy
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
    __device__ __forceinline__ void operator()(int seg, const SegMetrics& M, const DistMetrics& Q) const {
        if (writer) {
            double v[kDisturbAllRows];
            disturb_rows(M, Q, v);
#pragma unroll
            for (int row = 0; row < kDisturbAllRows; ++row) rows[((size_t)seg * kDisturbAllRows + row) * PN + col] = v[row];
        }
    }
};

template <int T, int KIND, int ENV, typename S>
__global__ __launch_bounds__(kDisturbThreads) void disturb_sweep_kernel(const DisturbArgs<S> a, const double* __restrict__ disturb,
                                                                        double* __restrict__ rows, double* __restrict__ actions,
                                                                        double* __restrict__ outputs, int tiles_per_row, long long n_tiles,
                                                                        long long n_quads) {
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
        const long long tile = q * (kDisturbThreads / 64) + wave;   // wave-uniform
        if (tile >= n_tiles) continue;
        const int p = (int)(tile / tiles_per_row), tr = (int)(tile - (long long)p * tiles_per_row);
        const int m = tr * TILE + (POLICY ? (lane & 15) : lane);
        const bool valid = m < N;
        const int i = valid ? m : N - 1;   // idle lanes shadow the last plant (compute, never store)
        const DisturbRow row = disturb_row(disturb + (size_t)p * PIME_DISTURB_COLS);
        DisturbDeviceSink sink{rows, actions, outputs, (size_t)a.P * N, (size_t)p * N + i, valid && (!POLICY || (lane >> 4) == 0)};
        if constexpr (ENV == 0) {
            PhLane<S> E{};
            ph_lane_load<S>(a.p, a.st, i, E);
            E.qww = a.st.qww[i]; E.qc = a.st.qc[i];   // (ph_lane_load zeroes them; the disturbed plant is rebuilt from the stored pair)
            if constexpr (POLICY) {
                const DisturbDevicePolicy<T, KIND> pol{lds, L, lane};
                disturb_ph_pair<S>(a.p, a.st.table, E, K, row, a.s, pol, sink);
            } else {
                disturb_ph_pair<S>(a.p, a.st.table, E, K, row, a.s, DisturbNoPolicy{}, sink);
            }
        } else {
            const uint32_t gid = a.env_offset + (uint32_t)i;
            WtLane<S> W{};
            wt_lane_load<S>(a.wp, a.wst, i, W);
            if constexpr (POLICY) {
                const DisturbDevicePolicy<T, KIND> pol{lds, L, lane};
                disturb_wt_pair<S>(a.wp, gid, W, K, row, a.s, pol, sink);
            } else {
                disturb_wt_pair<S>(a.wp, gid, W, K, row, a.s, DisturbNoPolicy{}, sink);
            }
        }
    }
}

// summary[p][cell][:] from rows[cell][p][0 .. N): one wave per (p, cell), cell = seg * kDisturbAllRows + row.  Lane l of block b
// holds plant 64 b + l (coalesced); the butterfly is SweepDeviceSink's (prior_sweep.hip), the blocks follow in ascending order.
__global__ __launch_bounds__(kDisturbThreads) void disturb_sweep_finish_kernel(int P, int N, int cells, const double* __restrict__ rows,
                                                                               double* __restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * (kDisturbThreads / 64) + (threadIdx.x >> 6);
    if (wv >= (long long)P * cells) return;   // wave-uniform
    const int p = (int)(wv / cells), cell = (int)(wv - (long long)p * cells);
    const double* x = rows + ((size_t)cell * P + p) * N;
    double total = 0.0, mn_all = __builtin_huge_val(), mx_all = -__builtin_huge_val();
    int arg_all = -1, cnt_all = 0;
    for (int b = 0; b * kSweepBlockPlants < N; ++b) {
        const int i = b * kSweepBlockPlants + lane;
        const double v = i < N ? x[i] : 0.0;
        const bool c = i < N && sweep_counts(v);   // absent plants and uncounted values (the NaN rows among them): +0.0, +-inf, no index
        double s = c ? v : 0.0, mn = c ? v : __builtin_huge_val(), mx = c ? v : -__builtin_huge_val();
        int arg = c ? i : -1, cnt = c ? 1 : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            s += __shfl_xor(s, off, 64);
            const double mo = __shfl_xor(mn, off, 64), xo = __shfl_xor(mx, off, 64);
            const int ao = __shfl_xor(arg, off, 64);
            cnt += __shfl_xor(cnt, off, 64);
            mn = mo < mn ? mo : mn;
            if (xo > mx || (xo == mx && ao < arg)) { mx = xo; arg = ao; }   // a tie: the smaller plant index
        }
        total = b == 0 ? s : total + s;
        mn_all = mn < mn_all ? mn : mn_all;
        if (b == 0 || mx > mx_all) { mx_all = mx; arg_all = arg; }   // strictly: a tie keeps the earlier block
        cnt_all += cnt;
    }
    if (lane == 0) {
        double* q = summary + ((size_t)p * cells + cell) * PIME_SWEEP_STATS;
        q[PIME_SWEEP_SUM] = total; q[PIME_SWEEP_MIN] = mn_all; q[PIME_SWEEP_MAX] = mx_all; q[PIME_SWEEP_ARGMAX] = (double)arg_all;
        q[PIME_SWEEP_FINITE] = (double)cnt_all;
    }
}

template <int T, int KIND, int ENV, typename S>
static int launch_disturb_k(const DisturbArgs<S>& a, const double* disturb, double* rows, double* actions, double* outputs, hipStream_t s) {
    constexpr bool POLICY = KIND >= 0;
    constexpr int TILE = POLICY ? 16 : 64;
    size_t lds_bytes = 0;
    if constexpr (POLICY) {
        lds_bytes = (size_t)mlp_layout(KIND, ENV == 0 ? 3 : 4, 1, T * 32).total * sizeof(float);
        static LdsLimit lds_limit;  // per instantiation
        PIME_RAISE_LDS(lds_limit, (disturb_sweep_kernel<T, KIND, ENV, S>), 160 * 1024);
    }
    int dev = 0, cus = 0;
    PIME_HIP_TRY(hipGetDevice(&dev));
    PIME_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int tiles_per_row = (a.n + TILE - 1) / TILE;
    const long long n_tiles = (long long)a.P * tiles_per_row;
    const long long n_quads = (n_tiles + kDisturbThreads / 64 - 1) / (kDisturbThreads / 64);
    // resident workgroups per compute unit: what the image leaves of the 160 KB of LDS (one at width 128), eight without an image
    const int per_cu = POLICY ? (int)((160 * 1024) / lds_bytes > 4 ? 4 : (160 * 1024) / lds_bytes) : 8;
    const long long cap = (long long)(cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1);
    const unsigned grid = (unsigned)(n_quads < cap ? n_quads : cap);
    hipLaunchKernelGGL((disturb_sweep_kernel<T, KIND, ENV, S>), dim3(grid), dim3(kDisturbThreads), lds_bytes, s, a, disturb, rows, actions,
                       outputs, tiles_per_row, n_tiles, n_quads);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

template <typename S>
int launch_disturb_sweep(int kind, int md, const DisturbArgs<S>& a, const double* disturb, double* pairs, double* summary, double* actions,
                         double* outputs, double* workspace, hipStream_t stream) {
    if (kind >= 0) {
        if (int rc = mlp_check(kind, a.env == 0 ? 3 : 4, kind == MLP_MODULAR_ACTOR ? 1 : 0, md)) return rc;
    }
    double* rows = pairs != nullptr ? pairs : workspace;
    const int T = kind < 0 ? 0 : md / 32;
    int rc = -1;
#define PIME_DS(TT, KK, EE) \
    if (T == TT && kind == KK && a.env == EE) rc = launch_disturb_k<(TT == 0 ? 2 : TT), KK, EE, S>(a, disturb, rows, actions, outputs, stream);
    PIME_DS(0, -1, 0) PIME_DS(0, -1, 1)
    PIME_DS(4, MLP_MODULAR_ACTOR, 0) PIME_DS(2, MLP_MODULAR_ACTOR, 0) PIME_DS(4, MLP_PLAIN_ACTOR, 0) PIME_DS(2, MLP_PLAIN_ACTOR, 0)
    PIME_DS(4, MLP_MODULAR_ACTOR, 1) PIME_DS(2, MLP_MODULAR_ACTOR, 1) PIME_DS(4, MLP_PLAIN_ACTOR, 1) PIME_DS(2, MLP_PLAIN_ACTOR, 1)
    PIME_DS(4, MLP_SAC_ACTOR, 0) PIME_DS(2, MLP_SAC_ACTOR, 0) PIME_DS(4, MLP_SAC_ACTOR, 1) PIME_DS(2, MLP_SAC_ACTOR, 1)
    PIME_DS(4, MLP_CRITIC, 0) PIME_DS(2, MLP_CRITIC, 0) PIME_DS(4, MLP_CRITIC, 1) PIME_DS(2, MLP_CRITIC, 1)
#undef PIME_DS
    if (rc == -1) {
        set_error("no disturbance-rejection sweep instantiation for env %d kind %d width %d", a.env, kind, md);
        return PIME_ERR_ARG;
    }
    if (rc != PIME_OK) return rc;
    const int cells = a.n_seg * kDisturbAllRows;
    const long long waves = (long long)a.P * cells;
    hipLaunchKernelGGL(disturb_sweep_finish_kernel, dim3((unsigned)((waves + kDisturbThreads / 64 - 1) / (kDisturbThreads / 64))),
                       dim3(kDisturbThreads), 0, stream, a.P, a.n, cells, rows, summary);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

template int launch_disturb_sweep<double>(int, int, const DisturbArgs<double>&, const double*, double*, double*, double*, double*, double*,
                                          hipStream_t);
template int launch_disturb_sweep<float>(int, int, const DisturbArgs<float>&, const double*, double*, double*, double*, double*, double*,
                                         hipStream_t);

}  // namespace pime
