// Prior-gain sweep (pime_prior_sweep): ONE (gain row, plant lane) pair under the prior controller alone, the lane in registers, its
// step response reduced to the rows of eval_metrics.hpp while it runs.  The loop is the loop body of rollout_eval_kernel with
// KIND = -1 (rollout_eval.hip) on a register copy of the lane -- the same boundaries, the same a_env sum, the same lane step, the
// same SegMetrics calls -- so a pair's rows are bit for bit the metrics pime_rollout_eval_metrics(kind = -1, priorK = the gain row)
// writes from the same lane state.  __host__ __device__: prior_sweep.hip runs it one thread per pair, prior_sweep_host.hip compiles
// the SAME source into libpime_sweep_host.so (float64 state; test infrastructure like the CPU twins).
#pragma once
#include "env_device.hpp"
#include "rollout_eval.hpp"

namespace pime {

// the set-point schedule and the metric arguments of a sweep, the same for every pair (kernel argument: wave-uniform)
struct SweepSchedule {
    int n_steps, seg_len, tail;
    double band;
    double setpoint[kMaxSetpoints];
};

__host__ __device__ __forceinline__ int sweep_segments(int n_steps, int seg_len) {
    return seg_len > 0 ? (n_steps + seg_len - 1) / seg_len : 1;
}

// the rows of a finished segment in registers: what SegMetrics::store writes, as one lane of one segment
__host__ __device__ __forceinline__ void sweep_rows(const SegMetrics& M, double (&v)[PIME_METRIC_ROWS]) { M.store(v, 0, 1, 0); }

// a value counts in the summary if it is finite (NaN fails the comparison)
__host__ __device__ __forceinline__ bool sweep_counts(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// One pH pair: lane E (a copy), gain row K.  sink(seg, M) is called once per finished segment, at a wave-uniform point.
template <typename S, typename Sink>
__host__ __device__ __forceinline__ void sweep_ph_pair(const PhParams& p, const S* __restrict__ table, PhLane<S> E, const double (&K)[3],
                                                       const SweepSchedule& s, Sink& sink) {
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
        double a_env = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) a_env += (double)obs[j] * K[j];
        float rew;
        (void)ph_lane_step<S>(p, table, a_env, E, obs, rew);
        double y;   // y after the step in the state's precision (float state: the observation is that value)
        if constexpr (sizeof(S) == sizeof(float)) y = (double)obs[0];
        else y = (double)ph_lookup<S>(p, table, E.C, E.x);
        M.step(k, y, a_env, rew, s.band);
        if (++k == M.len) {
            sink(seg, M);
            ++seg; k = 0;
        }
    }
}

// One tank pair (Integrator observation).  gid: the PLANT's global lane, the key of its process noise -- the same for every gain.
template <typename S, typename Sink>
__host__ __device__ __forceinline__ void sweep_wt_pair(const WtParams& p, uint32_t gid, WtLane<S> W, const double (&K)[4],
                                                       const SweepSchedule& s, Sink& sink) {
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
        double a_env = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) a_env += (double)obs[j] * K[j];
        float rew;
        double z1n, z2n;
        wt_lane_noise<S>(p, gid, W, nullptr, z1n, z2n);
        (void)wt_lane_step<S>(p, a_env, z1n, z2n, W, rew);
        obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
        M.step(k, (double)W.h2, a_env, rew, s.band);
        if (++k == M.len) {
            sink(seg, M);
            ++seg; k = 0;
        }
    }
}

// the schedule, band and tail errors every plant-grid call and its host build share, after the call's own checks; `fn` names the
// entry point.  The schedule's checks and messages are pime_rollout_eval_metrics' (abi.hip: rollout_eval_common).
inline int check_schedule_args(const char* fn, int n_steps, int seg_len, const double* setpoints, int n_setpoints, double band,
                               int tail) {
    PIME_REQUIRE(band >= 0.0 && band <= 1.79769313486231570815e308, "%s: band %g (finite, >= 0)", fn, band);   // (NaN fails both)
    PIME_REQUIRE(tail >= 1, "%s: tail %d (>= 1)", fn, tail);
    PIME_REQUIRE(n_steps >= 1, "%s: bad arguments (n_steps %d, >= 1)", fn, n_steps);
    PIME_REQUIRE(n_setpoints >= 0 && n_setpoints <= kMaxSetpoints, "%s: n_setpoints %d (0 .. %d)", fn, n_setpoints, kMaxSetpoints);
    PIME_REQUIRE(seg_len >= 0 && (seg_len == 0 || (setpoints && n_setpoints >= 1 && n_setpoints <= kMaxSetpoints &&
                                                   (n_steps + seg_len - 1) / seg_len <= n_setpoints)),
                 "%s: the set-point schedule does not cover n_steps (at most %d segments)", fn, kMaxSetpoints);
    return PIME_OK;
}

inline void fill_sweep_schedule(SweepSchedule& s, int n_steps, int seg_len, const double* setpoints, int n_setpoints, double band,
                                int tail) {
    s.n_steps = n_steps; s.seg_len = seg_len; s.tail = tail; s.band = band;
    for (int j = 0; j < kMaxSetpoints; ++j) s.setpoint[j] = seg_len > 0 && j < n_setpoints ? setpoints[j] : 0.0;
}

// the argument errors of pime_prior_sweep and of its host build, checked before anything runs
inline int check_sweep_args(const char* fn, int N, const double* gains, int G, int n_steps, int seg_len, const double* setpoints,
                            int n_setpoints, double band, int tail, const double* summary) {
    PIME_REQUIRE(G >= 1, "%s: G = %d (>= 1)", fn, G);
    PIME_REQUIRE((long long)G * N <= 2147483647LL, "%s: G x N = %d x %d pairs exceed 2^31 - 1", fn, G, N);
    PIME_REQUIRE(gains != nullptr, "%s: gains is NULL", fn);
    PIME_REQUIRE(summary != nullptr, "%s: summary is NULL", fn);
    return check_schedule_args(fn, n_steps, seg_len, setpoints, n_setpoints, band, tail);
}

// the prior controller alone: the policy argument of the pair functions that take one (margin_sweep.hpp, disturb_sweep.hpp) and
// the only policy of their host builds
struct PriorOnlyPolicy {
    static constexpr bool kPolicy = false;
};

// the argument errors of a row-grid call (pime_margin_sweep, pime_disturb_sweep) and of its host build, checked before anything
// runs; `fn` names the entry point, `rows_name` its grid argument
inline int check_row_grid_args(const char* fn, int N, const double* priorK, const double* rows, const char* rows_name, int P,
                               int n_steps, int seg_len, const double* setpoints, int n_setpoints, double band, int tail,
                               const double* summary) {
    PIME_REQUIRE(P >= 1, "%s: P = %d (>= 1)", fn, P);
    PIME_REQUIRE((long long)P * N <= 2147483647LL, "%s: P x N = %d x %d pairs exceed 2^31 - 1", fn, P, N);
    PIME_REQUIRE(rows != nullptr, "%s: %s is NULL", fn, rows_name);
    PIME_REQUIRE(summary != nullptr, "%s: summary is NULL", fn);
    PIME_REQUIRE(priorK != nullptr, "%s: priorK is NULL", fn);
    return check_schedule_args(fn, n_steps, seg_len, setpoints, n_setpoints, band, tail);
}

constexpr int kSweepBlockPlants = 64;   // the plants of one block of the summary's sum: one wave

// (prior_sweep.hip)
template <typename S>
struct SweepArgs {
    int env;                 // 0 pH, 1 water tank (Integrator observation)
    int n, G;                // plants (the handle's lanes), gain rows
    int n_blocks;            // ceil(n / 64)
    int n_seg;
    uint32_t env_offset;
    PhParams p;
    PhPtrs<S> st;
    WtParams wp;
    WtPtrs<S> wst;
    SweepSchedule s;
};
// workspace: float64[G][n_blocks][n_seg][PIME_METRIC_ROWS][PIME_SWEEP_STATS], every word written by the first launch
inline long long sweep_workspace_doubles(int G, int N, int n_seg) {
    return (long long)G * ((N + kSweepBlockPlants - 1) / kSweepBlockPlants) * n_seg * PIME_METRIC_ROWS * PIME_SWEEP_STATS;
}
template <typename S>
int launch_prior_sweep(const SweepArgs<S>& a, const double* gains, double* pairs, double* summary, double* workspace, hipStream_t stream);

}  // namespace pime
