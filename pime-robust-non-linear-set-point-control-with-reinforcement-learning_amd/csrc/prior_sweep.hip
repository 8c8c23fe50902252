// pime_prior_sweep: a grid of prior gains over the plants of a handle in ONE launch (prior_sweep.hpp has the pair function) and a
// finishing launch.  One thread per (gain row, plant) pair, so a wave carries 64 DISTINCT pairs (the tile kernels of
// rollout_eval.hip carry 16 under the prior controller alone).  A wave is (gain row g, block b of 64 consecutive plants): lanes run
// along the plants, so the lane-state loads and the `pairs` stores coalesce; the gain row, the set-points and every loop bound are
// wave-uniform (kernel arguments and a readfirstlane'd wave index: scalar loads), the step loop has no divergence, no LDS and no
// barrier.  At the end of a segment -- once per segment and row, never per step -- the wave folds each row over its 64 plants with an
// xor butterfly (__shfl_xor 1, 2, .., 32: the balanced pairwise tree over the index bits, a + b == b + a bit for bit, so every lane
// holds the same result and the order is fixed) and lane 0 stores the block's partial.  prior_sweep_finish_kernel then walks the
// blocks of a gain in ascending order.  No atomics: two calls give the same bits; every workspace word read was written by the call.
#include "prior_sweep.hpp"

namespace pime {

constexpr int kSweepBlock = 256;   // four waves: four (gain, plant block) pairs of consecutive wave index

template <typename T>
__device__ __forceinline__ T sweep_xor(T v, int off) { return __shfl_xor(v, off, 64); }

// the sink of a device pair: `pairs` (if asked) and the block partial of each row
struct SweepDeviceSink {
    double* __restrict__ pairs;      // [n_seg][ROWS][G * N] or nullptr
    double* __restrict__ partial;    // this wave's [n_seg][ROWS][STATS]
    int GN, col;                     // G * N, g * N + i
    int plant;                       // i
    bool valid, first;               // a plant of the handle; lane 0 of the wave

    __device__ __forceinline__ void operator()(int seg, const SegMetrics& M) const {
        double v[PIME_METRIC_ROWS];
        sweep_rows(M, v);
#pragma unroll
        for (int row = 0; row < PIME_METRIC_ROWS; ++row) {
            if (pairs != nullptr && valid) pairs[((size_t)seg * PIME_METRIC_ROWS + row) * GN + col] = v[row];
            const bool c = valid && sweep_counts(v[row]);   // absent plants and uncounted values: +0.0, +-inf, no index
            double s = c ? v[row] : 0.0, mn = c ? v[row] : __builtin_huge_val(), mx = c ? v[row] : -__builtin_huge_val();
            int arg = c ? plant : -1, cnt = c ? 1 : 0;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                s += sweep_xor(s, off);
                const double mo = sweep_xor(mn, off), xo = sweep_xor(mx, off);
                const int ao = sweep_xor(arg, off);
                cnt += sweep_xor(cnt, off);
                mn = mo < mn ? mo : mn;
                if (xo > mx || (xo == mx && ao < arg)) { mx = xo; arg = ao; }   // a tie: the smaller plant index
            }
            if (first) {
                double* q = partial + ((size_t)seg * PIME_METRIC_ROWS + row) * PIME_SWEEP_STATS;
                q[PIME_SWEEP_SUM] = s; q[PIME_SWEEP_MIN] = mn; q[PIME_SWEEP_MAX] = mx; q[PIME_SWEEP_ARGMAX] = (double)arg;
                q[PIME_SWEEP_FINITE] = (double)cnt;
            }
        }
    }
};

template <int ENV, typename S>
__global__ __launch_bounds__(kSweepBlock) void prior_sweep_kernel(const SweepArgs<S> a, const double* __restrict__ gains,
                                                                  double* __restrict__ pairs, double* __restrict__ partial) {
    constexpr int D = ENV == 0 ? 3 : 4;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kSweepBlock / 64) + (threadIdx.x >> 6)));
    if (wv >= a.G * a.n_blocks) return;                    // wave-uniform (G * n_blocks <= G * N <= 2^31 - 1)
    const int g = wv / a.n_blocks, b = wv - g * a.n_blocks;
    const int N = a.n;
    const int m = b * kSweepBlockPlants + lane;
    const bool valid = m < N;
    const int i = valid ? m : N - 1;                       // idle lanes shadow the last plant (compute, never store)
    double K[D];
#pragma unroll
    for (int j = 0; j < D; ++j) K[j] = gains[(size_t)g * D + j];
    SweepDeviceSink sink{pairs, partial + (size_t)wv * a.n_seg * PIME_METRIC_ROWS * PIME_SWEEP_STATS, a.G * N, g * N + i, i, valid,
                         lane == 0};
    if constexpr (ENV == 0) {
        PhLane<S> E{};
        ph_lane_load<S>(a.p, a.st, i, E);
        sweep_ph_pair<S>(a.p, a.st.table, E, K, a.s, sink);
    } else {
        WtLane<S> W{};
        wt_lane_load<S>(a.wp, a.wst, i, W);
        sweep_wt_pair<S>(a.wp, a.env_offset + (uint32_t)i, W, K, a.s, sink);
    }
}

// summary[g][seg][row][:] from the block partials of gain g: block 0's, then the others in ascending order.  One thread per
// (g, seg, row); consecutive threads read consecutive 40-byte partials.
__global__ __launch_bounds__(kSweepBlock) void prior_sweep_finish_kernel(int G, int n_blocks, int per_gain /* n_seg * ROWS */,
                                                                         const double* __restrict__ partial,
                                                                         double* __restrict__ summary) {
    const long long idx = (long long)blockIdx.x * kSweepBlock + threadIdx.x;
    if (idx >= (long long)G * per_gain) return;
    const long long g = idx / per_gain;
    const int cell = (int)(idx - g * per_gain);
    const double* p = partial + ((size_t)g * n_blocks * per_gain + cell) * PIME_SWEEP_STATS;
    double s = p[PIME_SWEEP_SUM], mn = p[PIME_SWEEP_MIN], mx = p[PIME_SWEEP_MAX], arg = p[PIME_SWEEP_ARGMAX], cnt = p[PIME_SWEEP_FINITE];
    for (int b = 1; b < n_blocks; ++b) {
        p += (size_t)per_gain * PIME_SWEEP_STATS;
        s += p[PIME_SWEEP_SUM];
        mn = p[PIME_SWEEP_MIN] < mn ? p[PIME_SWEEP_MIN] : mn;
        if (p[PIME_SWEEP_MAX] > mx) { mx = p[PIME_SWEEP_MAX]; arg = p[PIME_SWEEP_ARGMAX]; }   // strictly: a tie keeps the earlier block
        cnt += p[PIME_SWEEP_FINITE];
    }
    double* q = summary + (size_t)idx * PIME_SWEEP_STATS;
    q[PIME_SWEEP_SUM] = s; q[PIME_SWEEP_MIN] = mn; q[PIME_SWEEP_MAX] = mx; q[PIME_SWEEP_ARGMAX] = arg; q[PIME_SWEEP_FINITE] = cnt;
}

template <typename S>
int launch_prior_sweep(const SweepArgs<S>& a, const double* gains, double* pairs, double* summary, double* workspace, hipStream_t stream) {
    const long long waves = (long long)a.G * a.n_blocks;
    const dim3 grid((unsigned)((waves + kSweepBlock / 64 - 1) / (kSweepBlock / 64))), block(kSweepBlock);
    if (a.env == 0) hipLaunchKernelGGL((prior_sweep_kernel<0, S>), grid, block, 0, stream, a, gains, pairs, workspace);
    else hipLaunchKernelGGL((prior_sweep_kernel<1, S>), grid, block, 0, stream, a, gains, pairs, workspace);
    PIME_HIP_TRY(hipGetLastError());
    const int per_gain = a.n_seg * PIME_METRIC_ROWS;
    const long long cells = (long long)a.G * per_gain;
    hipLaunchKernelGGL(prior_sweep_finish_kernel, dim3((unsigned)((cells + kSweepBlock - 1) / kSweepBlock)), block, 0, stream, a.G,
                       a.n_blocks, per_gain, workspace, summary);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

template int launch_prior_sweep<double>(const SweepArgs<double>&, const double*, double*, double*, double*, hipStream_t);
template int launch_prior_sweep<float>(const SweepArgs<float>&, const double*, double*, double*, double*, hipStream_t);

}  // namespace pime
