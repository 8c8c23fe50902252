// Disturbance-rejection sweep (pime_disturb_sweep): ONE (disturbance row, plant lane) pair, the lane in registers.  The loop is the
// loop of rollout_eval_kernel with metrics (rollout_eval.hip) on a register copy of the lane -- the same boundaries, the same lane
// step, the same SegMetrics calls -- with a disturbance that is ACTIVE at segment step k iff k >= k0 && (L == 0 || k - k0 < L)
// (the row is wave-uniform and so is k: a uniform branch).  Every segment starts on the nominal plant again.  While active:
//   LOAD    a_env = a_c + d_u, one double addition IN FRONT of the actuator (pH's clip inside ph_lane_step sees the sum; the tank does
//           not clip).  While inactive a_env = a_c with no addition at all: a -0.0 stays -0.0, the nominal row keeps its bits.
//   PLANT   the lane steps on the disturbed parameter set.  Both sets are formed ONCE per pair before the step loop and one of them
//           is copied into the lane per step.  Tank: a1' = (S)((double)a1 * M0), a2' with M1, kp' with M2 (x * 1.0 == x: a unit
//           multiplier is the stored word).  pH: q = qww_V * M0, e = -q * sample_t, A' = exp(e), B' = -expm1(e) / q, C' = qc_V * M1 in
//           double, as the resample branch of ph_lane_reset; M0 == 1 keeps the STORED A and B, M1 == 1 the stored C, never recomputed
//           (exp would move the nominal row by an ulp).
// SegMetrics and the recorded action receive the CONTROLLER's output a_c (ACTION_VAR is controller effort); the applied action is
// a_c + d_u by the same single addition.  DistMetrics accumulates PIME_DISTURB_ROWS more rows per segment over the window k >= k0.
// With d_u = 0 and unit multipliers, for any ONSET and LENGTH, the eight SegMetrics rows are bit for bit a lane of
// pime_rollout_eval_metrics.
// __host__ __device__: disturb_sweep.hip runs it on 16-lane tiles (64-lane tiles under the prior alone), disturb_sweep_host.hip
// compiles the SAME source into libpime_disturb_host.so (prior controller only; test infrastructure like the CPU twins).
#pragma once
#include "env_device.hpp"
#include "prior_sweep.hpp"

namespace pime {

constexpr int kDisturbAllRows = PIME_METRIC_ROWS + PIME_DISTURB_ROWS;   // the rows of a pair per segment
constexpr int kDisturbMaxSteps = 1 << 30;                               // ONSET and LENGTH are clamped into 0 .. 2^30
constexpr int kDisturbNever = 2147483647;                               // ONSET NaN: no segment step reaches it

// a decoded row of `disturb` (wave-uniform on the device)
struct DisturbRow {
    int k0, len;         // onset within each segment; pulse length, 0: to the end of the segment
    double du;           // load, normalised action units
    double m0, m1, m2;   // multipliers of the plant parameters while active
    __host__ __device__ __forceinline__ bool active(int k) const { return k >= k0 && (len == 0 || k - k0 < len); }
};
// rint, clamped into 0 .. 2^30; NaN (fails every comparison): `nan_value`
__host__ __device__ __forceinline__ int disturb_steps(double v, int nan_value) {
    const double r = rint(v);
    return r >= (double)kDisturbMaxSteps ? kDisturbMaxSteps : (r >= 0.0 ? (int)r : (r < 0.0 ? 0 : nan_value));
}
__host__ __device__ __forceinline__ DisturbRow disturb_row(const double* __restrict__ r) {
    DisturbRow d;
    d.k0 = disturb_steps(r[PIME_DISTURB_ONSET], kDisturbNever);
    d.len = disturb_steps(r[PIME_DISTURB_LENGTH], 0);
    d.du = r[PIME_DISTURB_LOAD];
    d.m0 = r[PIME_DISTURB_M0]; d.m1 = r[PIME_DISTURB_M1]; d.m2 = r[PIME_DISTURB_M2];
    return d;
}

// The rejection rows of one segment over the window k >= k0.  All sums are sequential double additions in ascending step order and
// (double)(k - k0 + 1) * |e| rounds before it is added (-ffp-contract=off), so numpy reproduces them bit for bit from the traces.
struct DistMetrics {
    double e0, peak, iae, itae, apeak;
    double a_ref, a_last, y_last;
    int peak_step, recovery;
    bool seen;           // the window is not empty (wave-uniform)

    // y_start: the controlled output before the segment's first step
    __host__ __device__ __forceinline__ void begin(double y_start) {
        e0 = peak = iae = itae = apeak = a_ref = 0.0;
        a_last = 0.0;    // a_c(-1) := 0.0
        y_last = y_start;
        peak_step = recovery = 0;
        seen = false;
    }
    // step k of the segment: r the segment's set-point, y the controlled output after the step, a_c the controller's output
    __host__ __device__ __forceinline__ void step(int k, int k0, double r, double y, double a_c, double band) {
        if (k >= k0) {   // (wave-uniform)
            const double ae = fabs(r - y);
            const int w = k - k0 + 1;
            if (k == k0) {
                e0 = r - y_last;
                a_ref = a_last;
                peak = ae; peak_step = 1;
                apeak = fabs(a_c - a_ref);
                seen = true;
            } else {
                if (ae > peak) { peak = ae; peak_step = w; }   // strictly: the first step that attains it
                const double da = fabs(a_c - a_ref);
                apeak = da > apeak ? da : apeak;
            }
            iae += ae;
            itae += (double)w * ae;
            if (ae > band) recovery = w;
        }
        a_last = a_c; y_last = y;
    }
    // rows PIME_METRIC_ROWS .. of v; a segment the row never starts in: NaN
    __host__ __device__ __forceinline__ void rows(double* v) const {
        const double nan = __builtin_nan("");
        v[PIME_DISTURB_E0] = seen ? e0 : nan;
        v[PIME_DISTURB_PEAK] = seen ? peak : nan;
        v[PIME_DISTURB_PEAK_STEP] = seen ? (double)peak_step : nan;
        v[PIME_DISTURB_RECOVERY] = seen ? (double)recovery : nan;
        v[PIME_DISTURB_IAE] = seen ? iae : nan;
        v[PIME_DISTURB_ITAE] = seen ? itae : nan;
        v[PIME_DISTURB_ACTION_PEAK] = seen ? apeak : nan;
    }
};

// the fifteen rows of a finished segment in registers
__host__ __device__ __forceinline__ void disturb_rows(const SegMetrics& M, const DistMetrics& Q, double (&v)[kDisturbAllRows]) {
    M.store(v, 0, 1, 0);
    Q.rows(v + PIME_METRIC_ROWS);
}

// the controller's output from the env's observation, formed as rollout_eval_kernel forms it (the prior term in double, ascending j
// from 0.0; the policy term added on the left)
template <int D, typename Pol>
__host__ __device__ __forceinline__ double disturb_controller(const float (&obs)[D], const double (&K)[D], const Pol& pol) {
    double a_c = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) a_c += (double)obs[j] * K[j];
    if constexpr (Pol::kPolicy) a_c = residual_tanh(pol(obs)) + a_c;
    return a_c;
}

// One pH pair: lane E (a copy) with E.qww and E.qc the lane's STORED qww_V and qc_V (ph_lane_load zeroes them: the caller loads
// them).  sink.step(t, a_c, y) once per step, sink(seg, M, Q) once per finished segment, both at wave-uniform points.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void disturb_ph_pair(const PhParams& p, const S* __restrict__ table, PhLane<S> E, const double (&K)[3],
                                                         const DisturbRow& row, const SweepSchedule& s, const Pol& pol, Sink& sink) {
    const double An = E.A, Bn = E.B, Cn = E.C;   // the nominal set: the stored words
    double Ad = An, Bd = Bn, Cd = Cn;            // the disturbed set
    if (!(row.m0 == 1.0)) {                      // (wave-uniform) update_system (ph.py:114-121) on qww_V * M0
        const double q = E.qww * row.m0, e = -q * p.sample_t;
        Ad = exp(e);
        Bd = -expm1(e) / q;
    }
    if (!(row.m1 == 1.0)) Cd = E.qc * row.m1;
    float obs[3];
    obs[0] = (float)ph_lookup<S>(p, table, E.C, E.x); obs[1] = (float)E.r; obs[2] = (float)E.I;
    SegMetrics M{};
    DistMetrics Q{};
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {   // segment boundary: set r, zero I and t, a new episode beyond the first one
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            E.r = (S)sp; E.I = S(0); E.t = 0; E.episode += bump; obs[1] = (float)E.r; obs[2] = 0.f;
        }
        if (k == 0) {   // the segment starts on the nominal plant
            const double y_start = (double)ph_lookup<S>(p, table, Cn, E.x);
            M.begin(y_start, (double)E.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
            Q.begin(y_start);
        }
        const bool on = row.active(k);   // (wave-uniform)
        if (on) { E.A = Ad; E.B = Bd; E.C = Cd; }
        else { E.A = An; E.B = Bn; E.C = Cn; }
        const double a_c = disturb_controller<3>(obs, K, pol);
        double a_env = a_c;
        if (on) a_env = a_c + row.du;
        float rew;
        (void)ph_lane_step<S>(p, table, a_env, E, obs, rew);
        double y;   // y after the step in the state's precision (float state: the observation is that value)
        if constexpr (sizeof(S) == sizeof(float)) y = (double)obs[0];
        else y = (double)ph_lookup<S>(p, table, E.C, E.x);
        sink.step(t, a_c, y);
        M.step(k, y, a_c, rew, s.band);
        Q.step(k, row.k0, M.r, y, a_c, s.band);
        if (++k == M.len) {
            sink(seg, M, Q);
            ++seg; k = 0;
        }
    }
}

// One tank pair (Integrator observation).  gid: the PLANT's global lane, the key of its process noise -- the same for every row.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void disturb_wt_pair(const WtParams& p, uint32_t gid, WtLane<S> W, const double (&K)[4],
                                                         const DisturbRow& row, const SweepSchedule& s, const Pol& pol, Sink& sink) {
    const S a1n = W.a1, a2n = W.a2, kpn = W.kp;   // the nominal set: the stored words
    const S a1d = (S)((double)a1n * row.m0), a2d = (S)((double)a2n * row.m1), kpd = (S)((double)kpn * row.m2);
    float obs[4];
    obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
    SegMetrics M{};
    DistMetrics Q{};
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            W.r = (S)sp; W.I = S(0); W.t = 0; W.episode += bump; obs[2] = (float)W.r; obs[3] = 0.f;
        }
        if (k == 0) {
            M.begin((double)W.h2, (double)W.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
            Q.begin((double)W.h2);
        }
        const bool on = row.active(k);   // (wave-uniform)
        if (on) { W.a1 = a1d; W.a2 = a2d; W.kp = kpd; }
        else { W.a1 = a1n; W.a2 = a2n; W.kp = kpn; }
        const double a_c = disturb_controller<4>(obs, K, pol);
        double a_env = a_c;
        if (on) a_env = a_c + row.du;
        float rew;
        double z1n, z2n;
        wt_lane_noise<S>(p, gid, W, nullptr, z1n, z2n);
        (void)wt_lane_step<S>(p, a_env, z1n, z2n, W, rew);
        obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
        sink.step(t, a_c, (double)W.h2);
        M.step(k, (double)W.h2, a_c, rew, s.band);
        Q.step(k, row.k0, M.r, (double)W.h2, a_c, s.band);
        if (++k == M.len) {
            sink(seg, M, Q);
            ++seg; k = 0;
        }
    }
}

// (disturb_sweep.hip)
template <typename S>
struct DisturbArgs {
    int env;                 // 0 pH, 1 water tank (Integrator observation)
    int n, P;                // plants (the handle's lanes), disturbance rows
    int n_seg;
    uint32_t env_offset;
    PhParams p;
    PhPtrs<S> st;
    WtParams wp;
    WtPtrs<S> wst;
    const float* img;        // packed actor forward image (pime_mlp_pack), unused for the prior controller alone
    PriorK K;
    SweepSchedule s;
};
// workspace: float64[n_seg][kDisturbAllRows][P][N], the copy of `pairs` the finishing launch reads when `pairs` is NULL
template <typename S>
int launch_disturb_sweep(int kind, int md, const DisturbArgs<S>& a, const double* disturb, double* pairs, double* summary, double* actions,
                         double* outputs, double* workspace, hipStream_t stream);

}  // namespace pime
