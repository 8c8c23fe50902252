// Policy sweep (pime_policy_sweep): ONE (policy row, plant lane) pair, the lane in registers, its step response reduced to the rows of
// eval_metrics.hpp while it runs.  The loop is the nominal loop of sweep_ph_pair / sweep_wt_pair (prior_sweep.hpp) -- the same
// boundaries, the same lane step, the same SegMetrics calls -- with the policy argument and the action sum of margin_ph_pair /
// margin_wt_pair (margin_sweep.hpp) for the row (1, 0, 0): a_env = tanh(mean(obs)) + obs @ K, the prior term in double, ascending j
// from 0.0, the policy term added on the left; no measurement noise, no delay line, no gain.  So a pair of row p is bit for bit a
// lane of pime_rollout_eval_metrics(kind, md, image p, K[p]) from the same lane state; the tank's process noise is keyed on the
// PLANT's global lane, never on the pair: every policy meets the same disturbance, as every gain of pime_prior_sweep does.
// Device only: under the prior alone this call would be pime_prior_sweep, so there is no host build.
#pragma once
#include "env_device.hpp"
#include "prior_sweep.hpp"

namespace pime {

// the action of a step from the env's observation: the controller of margin_action without the measurement and the actuator
template <int D, typename Pol>
__device__ __forceinline__ double policy_action(const float (&obs)[D], const double (&K)[D], const Pol& pol) {
    double a_c = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) a_c += (double)obs[j] * K[j];
    return residual_tanh(pol(obs)) + a_c;
}

// One pH pair: lane E (a copy), the row's gain K and policy pol.  sink.step(t, a_env, y) once per step, sink(seg, M) once per
// finished segment, both at wave-uniform points.
template <typename S, typename Pol, typename Sink>
__device__ __forceinline__ void policy_ph_pair(const PhParams& p, const S* __restrict__ table, PhLane<S> E, const double (&K)[3],
                                               const SweepSchedule& s, const Pol& pol, Sink& sink) {
    float obs[3];
    obs[0] = (float)ph_lookup<S>(p, table, E.C, E.x); obs[1] = (float)E.r; obs[2] = (float)E.I;
    SegMetrics M{};
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {   // segment boundary: set r, zero I and t, a new episode beyond the first one
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            E.r = (S)sp; E.I = S(0); E.t = 0; E.episode += bump; obs[1] = (float)E.r; obs[2] = 0.f;
        }
        if (k == 0) M.begin((double)ph_lookup<S>(p, table, E.C, E.x), (double)E.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
        const double a_env = policy_action<3>(obs, K, pol);
        float rew;
        (void)ph_lane_step<S>(p, table, a_env, E, obs, rew);
        double y;   // y after the step in the state's precision (float state: the observation is that value)
        if constexpr (sizeof(S) == sizeof(float)) y = (double)obs[0];
        else y = (double)ph_lookup<S>(p, table, E.C, E.x);
        sink.step(t, a_env, y);
        M.step(k, y, a_env, rew, s.band);
        if (++k == M.len) {
            sink(seg, M);
            ++seg; k = 0;
        }
    }
}

// One tank pair (Integrator observation).  gid: the PLANT's global lane, the key of its process noise -- the same for every policy.
template <typename S, typename Pol, typename Sink>
__device__ __forceinline__ void policy_wt_pair(const WtParams& p, uint32_t gid, WtLane<S> W, const double (&K)[4], const SweepSchedule& s,
                                               const Pol& pol, Sink& sink) {
    float obs[4];
    obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
    SegMetrics M{};
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            W.r = (S)sp; W.I = S(0); W.t = 0; W.episode += bump; obs[2] = (float)W.r; obs[3] = 0.f;
        }
        if (k == 0) M.begin((double)W.h2, (double)W.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
        const double a_env = policy_action<4>(obs, K, pol);
        float rew;
        double z1n, z2n;
        wt_lane_noise<S>(p, gid, W, nullptr, z1n, z2n);
        (void)wt_lane_step<S>(p, a_env, z1n, z2n, W, rew);
        obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
        sink.step(t, a_env, (double)W.h2);
        M.step(k, (double)W.h2, a_env, rew, s.band);
        if (++k == M.len) {
            sink(seg, M);
            ++seg; k = 0;
        }
    }
}

// the argument errors of pime_policy_sweep, checked before anything runs (the style of check_row_grid_args)
inline int check_policy_sweep_args(const char* fn, int N, const float* packed_actors, long long image_stride, long long packed_floats,
                                   const double* priorK, int P, int n_steps, int seg_len, const double* setpoints, int n_setpoints,
                                   double band, int tail, const double* summary) {
    PIME_REQUIRE(P >= 1, "%s: P = %d (>= 1)", fn, P);
    PIME_REQUIRE((long long)P * N <= 2147483647LL, "%s: P x N = %d x %d pairs exceed 2^31 - 1", fn, P, N);
    PIME_REQUIRE(packed_actors != nullptr, "%s: packed_actors is NULL", fn);
    PIME_REQUIRE(summary != nullptr, "%s: summary is NULL", fn);
    PIME_REQUIRE(priorK != nullptr, "%s: priorK is NULL", fn);
    PIME_REQUIRE(image_stride >= packed_floats, "%s: image_stride %lld is smaller than a packed image (%lld floats)", fn, image_stride,
                 packed_floats);
    PIME_REQUIRE(image_stride % 4 == 0, "%s: image_stride %lld is not a multiple of 4 floats", fn, image_stride);
    PIME_REQUIRE(reinterpret_cast<uintptr_t>(packed_actors) % 16 == 0, "%s: packed_actors is not 16-byte aligned", fn);
    return check_schedule_args(fn, n_steps, seg_len, setpoints, n_setpoints, band, tail);
}

// (policy_sweep.hip)
template <typename S>
struct PolicyArgs {
    int env;                 // 0 pH, 1 water tank (Integrator observation)
    int n, P;                // plants (the handle's lanes), policy rows
    int n_seg;
    uint32_t env_offset;
    PhParams p;
    PhPtrs<S> st;
    WtParams wp;
    WtPtrs<S> wst;
    const float* img;        // P packed actor forward images (pime_mlp_pack), image p at img + p * stride
    long long stride;        // floats between two images: >= the packed size, a multiple of 4
    const double* K;         // [P][D] on the device: row p's prior gain
    SweepSchedule s;
};
// workspace: float64[n_seg][PIME_METRIC_ROWS][P][N], the copy of `pairs` the finishing launch reads when `pairs` is NULL
template <typename S>
int launch_policy_sweep(int kind, int md, const PolicyArgs<S>& a, double* pairs, double* summary, double* actions, double* outputs,
                        double* workspace, hipStream_t stream);

}  // namespace pime
