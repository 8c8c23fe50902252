// Receding-horizon benchmark controller (pime_mpc_eval): ONE plant in closed loop with a non-linear MPC on the plant's own model.
// At every control step 64 constant-action candidates per pass are rolled forward `horizon` steps through the product's lane step
// (env_device.hpp) on a register copy of the lane with the process noise at zero, the cheapest is applied to the TRUE plant, and the
// true plant's loop is the loop of sweep_ph_pair / sweep_wt_pair (prior_sweep.hpp) with a_env = u* in place of obs @ K: the same
// boundaries, the same noise key, the same lane step, the same SegMetrics calls -- a plant's rows are comparable with
// pime_rollout_eval_metrics and pime_prior_sweep on the same handle.  __host__ __device__: mpc_eval.hip runs it one wave per plant
// with the lane index as the candidate index (Search = a wave butterfly), mpc_eval_host.hip compiles the SAME source into
// libpime_mpc_host.so with the candidates in a plain loop (float64 and float32 state; test infrastructure).  The rules -- candidates,
// cost, choice -- are stated in include/pime_hip.h; the build has -ffp-contract=off, every product rounds before it is added.
#pragma once
#include "prior_sweep.hpp"

namespace pime {

constexpr int kMpcCandidates = 64;     // per pass: one wave
constexpr int kMpcMaxHorizon = 64;
constexpr int kMpcMaxPasses = 3;

struct MpcConfig {
    int horizon, passes;
    double rho;
};

struct MpcBest {
    double J;
    int c;
};

// THE choice rule, used by both builds: is candidate (Ja, ca) preferred to (Jb, cb)?  The smaller cost; on a tie the smaller index; a
// non-finite cost loses to any finite one; among non-finite costs the smaller index (so c = 0 if none is finite).  A strict total
// order on distinct indices: a butterfly and a sequential scan end on the same winner.
__host__ __device__ __forceinline__ bool mpc_prefer(double Ja, int ca, double Jb, int cb) {
    const bool fa = sweep_counts(Ja), fb = sweep_counts(Jb);
    if (fa != fb) return fa;
    if (!fa) return ca < cb;
    return Ja < Jb || (Ja == Jb && ca < cb);
}

// candidate c of a pass: pass 0 the grid -1 + c * (2/63); pass p >= 1 the grid of step `step` around the previous winner `ustar`
__host__ __device__ __forceinline__ double mpc_candidate(int pass, int c, double ustar, double step) {
    const double u = pass == 0 ? -1.0 + (double)c * step : ustar + (double)(c - kMpcCandidates / 2) * step;
    return clip(u, -1.0, 1.0);
}

// The passes of one control step.  cost(u) -> J of the constant action u; search.argmin(f) -> MpcBest over f(c), c = 0 .. 63, by
// mpc_prefer (device: c is the lane and f runs once; host: a loop); search.chosen(pass, J) records the winner's cost (host only).
template <typename Search, typename Cost>
__host__ __device__ __forceinline__ double mpc_choose(const MpcConfig& m, Search& search, const Cost& cost) {
    double ustar = 0.0, step = 2.0 / 63.0;
    for (int pass = 0; pass < m.passes; ++pass) {
        if (pass > 0) step = step / 32.0;
        const MpcBest b = search.argmin([&](int c) { return cost(mpc_candidate(pass, c, ustar, step)); });
        ustar = mpc_candidate(pass, b.c, ustar, step);
        search.chosen(pass, b.J);
    }
    return ustar;
}

// J = sum_{k = 1 .. H} (y_k - r)^2 (ascending k, from 0.0) + rho * (u - u_prev)^2 on a copy of the lane; TimeLimit ignored
template <typename S>
__host__ __device__ __forceinline__ double mpc_cost_ph(const PhParams& p, const S* __restrict__ table, PhLane<S> E, const MpcConfig& m,
                                                       double u, double u_prev) {
    const double r = (double)E.r;
    double J = 0.0;
    float obs[3], rew;
    for (int k = 0; k < m.horizon; ++k) {
        (void)ph_lane_step<S>(p, table, u, E, obs, rew);
        double y;
        if constexpr (sizeof(S) == sizeof(float)) y = (double)obs[0];
        else y = (double)ph_lookup<S>(p, table, E.C, E.x);
        const double e = y - r;
        J += e * e;
    }
    const double du = u - u_prev;
    return J + m.rho * (du * du);
}

template <typename S>
__host__ __device__ __forceinline__ double mpc_cost_wt(const WtParams& p, WtLane<S> W, const MpcConfig& m, double u, double u_prev) {
    const double r = (double)W.r;
    double J = 0.0;
    float rew;
    for (int k = 0; k < m.horizon; ++k) {
        (void)wt_lane_step<S>(p, u, 0.0, 0.0, W, rew);
        const double e = (double)W.h2 - r;
        J += e * e;
    }
    const double du = u - u_prev;
    return J + m.rho * (du * du);
}

// One pH plant in closed loop.  sink.step(t, u, y) once per step, sink(seg, M) once per finished segment (wave-uniform points).
template <typename S, typename Search, typename Sink>
__host__ __device__ __forceinline__ void mpc_ph_plant(const PhParams& p, const S* __restrict__ table, PhLane<S> E, const SweepSchedule& s,
                                                      const MpcConfig& m, Search& search, Sink& sink) {
    float obs[3];   // written by the lane step; the controller reads the lane, never the observation
    SegMetrics M{};
    int seg = 0, k = 0;
    double u_prev = 0.0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {   // segment boundary: set r, zero I and t, a new episode beyond the first one
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            E.r = (S)sp; E.I = S(0); E.t = 0; E.episode += bump;
        }
        if (k == 0) M.begin((double)ph_lookup<S>(p, table, E.C, E.x), (double)E.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
        const double a_env = mpc_choose(m, search, [&](double u) { return mpc_cost_ph<S>(p, table, E, m, u, u_prev); });
        float rew;
        (void)ph_lane_step<S>(p, table, a_env, E, obs, rew);
        double y;   // y after the step in the state's precision (float state: the observation is that value)
        if constexpr (sizeof(S) == sizeof(float)) y = (double)obs[0];
        else y = (double)ph_lookup<S>(p, table, E.C, E.x);
        M.step(k, y, a_env, rew, s.band);
        sink.step(t, a_env, y);
        u_prev = a_env;
        if (++k == M.len) {
            sink(seg, M);
            ++seg; k = 0;
        }
    }
}

// One tank plant (Integrator observation).  gid: the plant's global lane, the key of its process noise.  has_model: the candidates
// roll a copy whose (a1, a2, kp) are the model row, rounded to the state's precision as a lane holds them; the levels are measured.
template <typename S, typename Search, typename Sink>
__host__ __device__ __forceinline__ void mpc_wt_plant(const WtParams& p, uint32_t gid, WtLane<S> W, bool has_model, S m_a1, S m_a2, S m_kp,
                                                      const SweepSchedule& s, const MpcConfig& m, Search& search, Sink& sink) {
    SegMetrics M{};
    int seg = 0, k = 0;
    double u_prev = 0.0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            W.r = (S)sp; W.I = S(0); W.t = 0; W.episode += bump;
        }
        if (k == 0) M.begin((double)W.h2, (double)W.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
        WtLane<S> model = W;
        if (has_model) { model.a1 = m_a1; model.a2 = m_a2; model.kp = m_kp; }
        const double a_env = mpc_choose(m, search, [&](double u) { return mpc_cost_wt<S>(p, model, m, u, u_prev); });
        float rew;
        double z1n, z2n;
        wt_lane_noise<S>(p, gid, W, nullptr, z1n, z2n);
        (void)wt_lane_step<S>(p, a_env, z1n, z2n, W, rew);
        M.step(k, (double)W.h2, a_env, rew, s.band);
        sink.step(t, a_env, (double)W.h2);
        u_prev = a_env;
        if (++k == M.len) {
            sink(seg, M);
            ++seg; k = 0;
        }
    }
}

// the argument errors of pime_mpc_eval and of its host build, checked before anything runs (check_sweep_args' pattern: the
// schedule's checks and messages are pime_rollout_eval_metrics')
inline int check_mpc_args(const char* fn, bool is_ph, const double* model_plants, int horizon, int passes, double rho, int n_steps,
                          int seg_len, const double* setpoints, int n_setpoints, double band, int tail, const double* metrics) {
    PIME_REQUIRE(horizon >= 1 && horizon <= kMpcMaxHorizon, "%s: horizon %d (1 .. %d)", fn, horizon, kMpcMaxHorizon);
    PIME_REQUIRE(passes >= 1 && passes <= kMpcMaxPasses, "%s: passes %d (1 .. %d)", fn, passes, kMpcMaxPasses);
    PIME_REQUIRE(rho >= 0.0 && rho <= 1.79769313486231570815e308, "%s: rho %g (finite, >= 0)", fn, rho);   // (NaN fails both)
    PIME_REQUIRE(metrics != nullptr, "%s: metrics is NULL", fn);
    PIME_REQUIRE(!(is_ph && model_plants != nullptr), "%s: model_plants on a pH handle (its state x is not measured)", fn);
    return check_schedule_args(fn, n_steps, seg_len, setpoints, n_setpoints, band, tail);
}

// (mpc_eval.hip)
template <typename S>
struct MpcArgs {
    int env;                 // 0 pH, 1 water tank (Integrator observation)
    int n;                   // plants (the handle's lanes)
    uint32_t env_offset;
    PhParams p;
    PhPtrs<S> st;
    WtParams wp;
    WtPtrs<S> wst;
    SweepSchedule s;
    MpcConfig m;
};
template <typename S>
int launch_mpc_eval(const MpcArgs<S>& a, const double* model_plants, double* metrics, double* actions, double* outputs,
                    hipStream_t stream);

}  // namespace pime
