// Loop-perturbation sweep (pime_margin_sweep): ONE (perturbation row, plant lane) pair, the lane in registers.  The loop is the loop
// of rollout_eval_kernel with metrics (rollout_eval.hip) on a register copy of the lane -- the same boundaries, the same lane step,
// the same SegMetrics calls -- with three things inserted per launch step t between the observation and the plant:
//   MEASUREMENT  obs_m = obs, and for the measured plant outputs (pH: column 0, y; tank: columns 0 and 1, h1 and h2)
//                obs_m[j] = obs[j] + (float)sigma * n_j in float32; (n_0, n_1) the Box-Muller pair (cosine, sine) of
//                philox_pair(noise_seed, env_offset + i, noise_epoch, t, STREAM_MEASURE), computed in double and rounded to float32.
//                The key is the PLANT, never the pair: every row meets the same noise sequence, scaled (common random numbers).
//                sigma == 0: nothing is drawn.  The set-point column and the integrator column are the env's own: the env integrates
//                the TRUE error, the controller reads that integral unperturbed.
//   CONTROLLER   a_c = tanh(mean(obs_m)) + obs_m @ priorK, formed as rollout_eval_kernel forms it (the prior term in double, ascending
//                j from 0.0; the policy term added on the left); Pol::kPolicy false: the prior controller alone.
//   ACTUATOR     a_env(t) = g * a_c(t - d), a_c(s) = 0.0 for s < 0: a delay line of eight doubles that a segment boundary does NOT
//                clear (the actuator knows nothing of set-points).  The metrics and the recorded action are the APPLIED a_env.
// With (g, d, sigma) = (1, 0, 0) a pair is bit for bit a lane of pime_rollout_eval_metrics (1.0 * a_c == a_c).
// __host__ __device__: margin_sweep.hip runs it on 16-lane tiles (64-lane tiles under the prior alone), margin_sweep_host.hip
// compiles the SAME source into libpime_margin_host.so (prior controller only; test infrastructure like the CPU twins).
#pragma once
#include "env_device.hpp"
#include "prior_sweep.hpp"

namespace pime {

enum : uint32_t { STREAM_MEASURE = 3 };   // Philox stream of the measurement noise (0 reset, 1 process noise)

// a decoded row of `perturb` (wave-uniform on the device)
struct MarginRow {
    double g;      // loop gain
    int d;         // dead time in sample periods, 0 .. PIME_MARGIN_MAX_DELAY
    float sigma;   // measurement-noise scale
    bool noisy;    // sigma != 0: draw
};
__host__ __device__ __forceinline__ MarginRow margin_row(const double* __restrict__ r) {
    MarginRow m;
    m.g = r[PIME_PERTURB_GAIN];
    const double dd = rint(r[PIME_PERTURB_DELAY]);   // (NaN fails both comparisons: 0)
    m.d = dd >= (double)PIME_MARGIN_MAX_DELAY ? PIME_MARGIN_MAX_DELAY : (dd >= 0.0 ? (int)dd : 0);
    m.sigma = (float)r[PIME_PERTURB_SIGMA];
    m.noisy = !(r[PIME_PERTURB_SIGMA] == 0.0);
    return m;
}

// the key of the measurement noise, the same for every pair of a call
struct MarginNoise {
    uint64_t seed;
    uint32_t epoch;
};

// the actuator's delay line: q[k] = a_c(t - 1 - k).  Shifted by unrolled moves and read through a switch on the (wave-uniform)
// delay: every index is a compile-time constant, so the line lives in registers.
struct MarginDelay {
    double q[PIME_MARGIN_MAX_DELAY];
    __host__ __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < PIME_MARGIN_MAX_DELAY; ++k) q[k] = 0.0;
    }
    // a_c(t - d), and a_c(t) enters the line
    __host__ __device__ __forceinline__ double push(int d, double a_c) {
        double out;
        switch (d) {
            case 0: out = a_c; break;
            case 1: out = q[0]; break;
            case 2: out = q[1]; break;
            case 3: out = q[2]; break;
            case 4: out = q[3]; break;
            case 5: out = q[4]; break;
            case 6: out = q[5]; break;
            case 7: out = q[6]; break;
            default: out = q[7]; break;
        }
#pragma unroll
        for (int k = PIME_MARGIN_MAX_DELAY - 1; k > 0; --k) q[k] = q[k - 1];
        q[0] = a_c;
        return out;
    }
};

// the measured columns of step t: NM = 1 (pH: y) or 2 (tank: h1, h2)
template <int NM, int D>
__host__ __device__ __forceinline__ void margin_measure(const MarginNoise& nz, uint32_t gid, int t, float sigma, float (&om)[D]) {
    double ua, ub;
    philox_pair(nz.seed, gid, nz.epoch, (uint32_t)t, STREAM_MEASURE, ua, ub);
    const double rad = sqrt(-2.0 * log(1.0 - ua)), ang = 6.283185307179586476925286766559 * ub;
    double sn, cs;
    sincos(ang, &sn, &cs);
    const float n0 = (float)(rad * cs), n1 = (float)(rad * sn);
    om[0] = om[0] + sigma * n0;
    if constexpr (NM > 1) om[1] = om[1] + sigma * n1;
}

// measurement, controller, actuator: the applied action of step t from the env's observation
template <int NM, int D, typename Pol>
__host__ __device__ __forceinline__ double margin_action(const float (&obs)[D], const double (&K)[D], const MarginRow& row,
                                                         const MarginNoise& nz, uint32_t gid, int t, const Pol& pol, MarginDelay& line) {
    float om[D];
#pragma unroll
    for (int j = 0; j < D; ++j) om[j] = obs[j];
    if (row.noisy) margin_measure<NM, D>(nz, gid, t, row.sigma, om);   // (wave-uniform)
    double a_c = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) a_c += (double)om[j] * K[j];
    if constexpr (Pol::kPolicy) a_c = residual_tanh(pol(om)) + a_c;
    return row.g * line.push(row.d, a_c);
}

// One pH pair: lane E (a copy).  gid: the PLANT's global lane.  sink.step(t, a_env, y) once per step, sink(seg, M) once per
// finished segment, both at wave-uniform points.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void margin_ph_pair(const PhParams& p, const S* __restrict__ table, uint32_t gid, PhLane<S> E,
                                                        const double (&K)[3], const MarginRow& row, const MarginNoise& nz,
                                                        const SweepSchedule& s, const Pol& pol, Sink& sink) {
    float obs[3];
    obs[0] = (float)ph_lookup<S>(p, table, E.C, E.x); obs[1] = (float)E.r; obs[2] = (float)E.I;
    SegMetrics M{};
    MarginDelay line;
    line.clear();
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {   // segment boundary: set r, zero I and t, a new episode beyond the first one
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            E.r = (S)sp; E.I = S(0); E.t = 0; E.episode += bump; obs[1] = (float)E.r; obs[2] = 0.f;
        }
        if (k == 0) M.begin((double)ph_lookup<S>(p, table, E.C, E.x), (double)E.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
        const double a_env = margin_action<1, 3>(obs, K, row, nz, gid, t, pol, line);
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

// One tank pair (Integrator observation).  gid keys the process noise AND the measurement noise: the same for every row.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void margin_wt_pair(const WtParams& p, uint32_t gid, WtLane<S> W, const double (&K)[4],
                                                        const MarginRow& row, const MarginNoise& nz, const SweepSchedule& s,
                                                        const Pol& pol, Sink& sink) {
    float obs[4];
    obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
    SegMetrics M{};
    MarginDelay line;
    line.clear();
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            W.r = (S)sp; W.I = S(0); W.t = 0; W.episode += bump; obs[2] = (float)W.r; obs[3] = 0.f;
        }
        if (k == 0) M.begin((double)W.h2, (double)W.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
        const double a_env = margin_action<2, 4>(obs, K, row, nz, gid, t, pol, line);
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

// (margin_sweep.hip)
template <typename S>
struct MarginArgs {
    int env;                 // 0 pH, 1 water tank (Integrator observation)
    int n, P;                // plants (the handle's lanes), perturbation rows
    int n_seg;
    uint32_t env_offset;
    PhParams p;
    PhPtrs<S> st;
    WtParams wp;
    WtPtrs<S> wst;
    const float* img;        // packed actor forward image (pime_mlp_pack), unused for the prior controller alone
    PriorK K;
    MarginNoise nz;
    SweepSchedule s;
};
// workspace: float64[n_seg][PIME_METRIC_ROWS][P][N], the copy of `pairs` the finishing launch reads when `pairs` is NULL
template <typename S>
int launch_margin_sweep(int kind, int md, const MarginArgs<S>& a, const double* perturb, double* pairs, double* summary, double* actions,
                        double* outputs, double* workspace, hipStream_t stream);

}  // namespace pime
