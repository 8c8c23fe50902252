// pime_env_replay_error: recorded runs replayed over a grid of candidate plants in ONE launch (replay_error.hpp has the lane
// function).  One thread per (lane, record) pair: lanes along x in workgroups of 256, records along the grid's second dimension
// (grid-stride beyond 65 535 records), so an 81-plant grid with many records still fills the device.  A record's action and
// measurement rows are the same for every lane: their addresses are wave-uniform (kernel arguments and blockIdx only) and the
// buffers are read-only for the launch (__restrict__ kernel arguments), so they go through the scalar data cache -- 16 to 40 bytes
// per WAVE and step -- and no LDS staging, no barrier, sits between two steps of a lane.  Every store is a per-lane vector
// store into a lane-minor row (err, sim): coalesced.  No atomics; a pair's result does not depend on the grid.
#include "replay_error.hpp"

namespace pime {

constexpr int kReplayBlock = 256;
constexpr int kReplayMaxGridY = 65535;

template <int ENV, typename S, int MODE>
__global__ __launch_bounds__(kReplayBlock) void replay_error_kernel(const ReplayArgs<S> a, const double* __restrict__ action,
                                                                    const double* __restrict__ output,
                                                                    const double* __restrict__ state0, double* __restrict__ err,
                                                                    double* __restrict__ sim) {
    const int i = blockIdx.x * kReplayBlock + threadIdx.x;
    if (i >= a.n) return;
    ReplayRecords rec;
    rec.action = action; rec.output = output; rec.state0 = state0; rec.E = a.E; rec.T = a.T;
    if constexpr (ENV == 0) {
        const double A = a.A[i], B = a.B[i], C = a.C[i];
        for (int e = blockIdx.y; e < a.E; e += gridDim.y) {
            ReplayErr acc;
            replay_ph_lane<S>(a.p, a.table, A, B, C, rec, e, a.skip, acc, sim ? sim + i : nullptr, a.n);
            acc.store(err, e, a.n, i);
        }
    } else {
        const S a1 = a.a1[i], a2 = a.a2[i], kp = a.kp[i];
        for (int e = blockIdx.y; e < a.E; e += gridDim.y) {
            ReplayErr acc;
            replay_wt_lane<S, MODE>(a.wp, a1, a2, kp, rec, e, a.skip, acc, sim ? sim + i : nullptr, a.n);
            acc.store(err, e, a.n, i);
        }
    }
}

template <typename S>
int launch_replay_error(const ReplayArgs<S>& a, const double* action, const double* output, const double* state0, double* err,
                        double* sim, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n + kReplayBlock - 1) / kReplayBlock), (unsigned)(a.E < kReplayMaxGridY ? a.E : kReplayMaxGridY));
    const dim3 block(kReplayBlock);
    if (a.env == 0)
        hipLaunchKernelGGL((replay_error_kernel<0, S, PIME_REPLAY_SIMULATE>), grid, block, 0, stream, a, action, output, state0, err, sim);
    else if (a.mode == PIME_REPLAY_PREDICT)
        hipLaunchKernelGGL((replay_error_kernel<1, S, PIME_REPLAY_PREDICT>), grid, block, 0, stream, a, action, output, state0, err, sim);
    else
        hipLaunchKernelGGL((replay_error_kernel<1, S, PIME_REPLAY_SIMULATE>), grid, block, 0, stream, a, action, output, state0, err, sim);
    PIME_HIP_TRY(hipGetLastError());
    return PIME_OK;
}

template int launch_replay_error<double>(const ReplayArgs<double>&, const double*, const double*, const double*, double*, double*, hipStream_t);
template int launch_replay_error<float>(const ReplayArgs<float>&, const double*, const double*, const double*, double*, double*, hipStream_t);

}  // namespace pime
