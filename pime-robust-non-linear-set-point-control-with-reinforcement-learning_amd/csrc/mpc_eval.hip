// pime_mpc_eval: the receding-horizon benchmark controller over every plant of a handle in ONE launch (mpc_eval.hpp has the closed
// loop).  One wave is one plant and the lane index is the candidate index: each lane rolls ITS constant action `horizon` lane steps
// forward in registers, a six-level xor butterfly over (J, c) with the choice rule of mpc_prefer leaves the same winner in every lane
// (a strict total order: the result does not depend on the pairing), and every lane then steps its own redundant copy of the true
// plant with the winner -- the copies stay bit-equal, so nothing is broadcast and the plant state, the set-points, the horizon, the
// passes and every loop bound are the same in all 64 lanes (kernel arguments and a readfirstlane'd wave index: scalar loads).  The
// step loop has no divergent branch, no LDS, no barrier and no atomics; inside the horizon loop the only memory traffic is the pH
// table gather (the tank has none).  Lane 0 stores the step's action / output and the segment's rows.  Four waves per workgroup;
// waves past the last plant exit wave-uniformly.  The handle is read through ph_lane_load / wt_lane_load and never written.
#include "mpc_eval.hpp"

namespace pime {

constexpr int kMpcBlock = 256;   // four waves: four plants of consecutive index

// candidate index = lane: f runs once, the butterfly finds the winner
struct MpcWaveSearch {
    int lane;
    template <typename F>
    __device__ __forceinline__ MpcBest argmin(const F& f) const {
        double J = f(lane);
        int c = lane;
#pragma unroll
        for (int off = 1; off < kMpcCandidates; off <<= 1) {
            const double Jo = __shfl_xor(J, off, 64);
            const int co = __shfl_xor(c, off, 64);
            const bool take = mpc_prefer(Jo, co, J, c);
            J = take ? Jo : J;
            c = take ? co : c;
        }
        return MpcBest{J, c};
    }
    __device__ __forceinline__ void chosen(int, double) const {}
};

struct MpcDeviceSink {
    double* __restrict__ metrics;    // [n_seg][ROWS][N]
    double* __restrict__ actions;    // [n_steps][N] or nullptr
    double* __restrict__ outputs;    // [n_steps][N] or nullptr
    int N, i;
    bool first;                      // lane 0 of the wave

    __device__ __forceinline__ void step(int t, double u, double y) const {
        if (first) {
            if (actions != nullptr) actions[(size_t)t * N + i] = u;
            if (outputs != nullptr) outputs[(size_t)t * N + i] = y;
        }
    }
    __device__ __forceinline__ void operator()(int seg, const SegMetrics& M) const {
        if (first) M.store(metrics, seg, N, i);
    }
};

template <int ENV, typename S>
__global__ __launch_bounds__(kMpcBlock) void mpc_eval_kernel(const MpcArgs<S> a, const double* __restrict__ model_plants,
                                                             double* __restrict__ metrics, double* __restrict__ actions,
                                                             double* __restrict__ outputs) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kMpcBlock / 64) + (threadIdx.x >> 6)));
    if (i >= a.n) return;                                  // wave-uniform
    MpcWaveSearch search{lane};
    MpcDeviceSink sink{metrics, actions, outputs, a.n, i, lane == 0};
    if constexpr (ENV == 0) {
        PhLane<S> E{};
        ph_lane_load<S>(a.p, a.st, i, E);
        mpc_ph_plant<S>(a.p, a.st.table, E, a.s, a.m, search, sink);
    } else {
        WtLane<S> W{};
        wt_lane_load<S>(a.wp, a.wst, i, W);
        const bool has_model = model_plants != nullptr;
        S m1 = S(0), m2 = S(0), mk = S(0);
        if (has_model) {
            m1 = (S)model_plants[(size_t)i * 3]; m2 = (S)model_plants[(size_t)i * 3 + 1]; mk = (S)model_plants[(size_t)i * 3 + 2];
        }
        mpc_wt_plant<S>(a.wp, a.env_offset + (uint32_t)i, W, has_model, m1, m2, mk, a.s, a.m, search, sink);
    }
}

template <typename S>
int launch_mpc_eval(const MpcArgs<S>& a, const double* model_plants, double* metrics, double* actions, double* outputs,
                    hipStream_t stream) {
    const dim3 grid((unsigned)((a.n + kMpcBlock / 64 - 1) / (kMpcBlock / 64))), block(kMpcBlock);
    if (a.env == 0) hipLaunchKernelGGL((mpc_eval_kernel<0, S>), grid, block, 0, stream, a, model_plants, metrics, actions, outputs);
    else hipLaunchKernelGGL((mpc_eval_kernel<1, S>), grid, block, 0, stream, a, model_plants, metrics, actions, outputs);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

template int launch_mpc_eval<double>(const MpcArgs<double>&, const double*, double*, double*, double*, hipStream_t);
template int launch_mpc_eval<float>(const MpcArgs<float>&, const double*, double*, double*, double*, hipStream_t);

}  // namespace pime
