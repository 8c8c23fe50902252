// Actuator-limits sweep (pime_actuator_sweep): ONE (actuator row, plant lane) pair, the lane in registers.  The loop is the loop of
// rollout_eval_kernel with metrics (rollout_eval.hip) on a register copy of the lane -- the same boundaries, the same lane step, the
// same SegMetrics calls -- with a real SENSOR in front of the controller and a real ACTUATOR behind it.  Per launch step t:
//   SENSOR      obs_m = obs, and with QY on, for the measured plant outputs (pH: column 0, y; tank: columns 0 and 1, h1 and h2)
//               obs_m[j] = (float)(QY * rint((double)obs[j] / QY)).  The set-point and integrator columns are the env's own.
//   CONTROLLER  a_c from obs_m as disturb_controller forms it.
//   ACTUATOR    in double on v = a_c and the previous APPLIED action u_prev (0.0 before the launch's first step, NOT cleared at a
//               segment boundary: the actuator knows nothing of set-points), each stage only if the row has it on, in this order:
//                 dead-band  if (fabs(v - u_prev) <= DEADBAND) v = u_prev;
//                 slew       v = u_prev + clip(v - u_prev, -RATE, RATE);
//                 quantise   v = QU * rint(v / QU);
//                 clamp      v = clip(v, LO, HI);            (last: a limit holds exactly)
//               clip(x, lo, hi): x < lo ? lo : x, then x > hi ? hi : x.  u = v, the lane steps on u (pH's own clip inside
//               ph_lane_step still sees it), u_prev = u.
// Every stage branch is on a field of the row and so wave-uniform; a stage that is off performs no arithmetic and rewrites no word: a
// row with all six columns off is bit for bit a lane of pime_rollout_eval_metrics (a -0.0 stays -0.0).  SegMetrics and `actions`
// receive the APPLIED u, `commands` the controller's a_c.  ActMetrics accumulates PIME_ACT_ROWS more rows per segment.
// __host__ __device__: actuator_sweep.hip runs it on 16-lane tiles (64-lane tiles under the prior alone), actuator_sweep_host.hip
// compiles the SAME source into libpime_actuator_host.so (prior controller only; test infrastructure like the CPU twins).
#pragma once
#include "disturb_sweep.hpp"

namespace pime {

constexpr int kActAllRows = PIME_METRIC_ROWS + PIME_ACT_ROWS;   // the rows of a pair per segment

// a decoded row of `actuator` (wave-uniform on the device): the six columns and which stages they switch on
struct ActRow {
    double lo, hi, rate, db, qu, qy;
    bool clamp, slew, hold, quant, sense;
};
__host__ __device__ __forceinline__ ActRow act_row(const double* __restrict__ r) {
    const double inf = __builtin_huge_val();
    ActRow a;
    a.lo = r[PIME_ACT_LO]; a.hi = r[PIME_ACT_HI]; a.rate = r[PIME_ACT_RATE];
    a.db = r[PIME_ACT_DEADBAND]; a.qu = r[PIME_ACT_QU]; a.qy = r[PIME_ACT_QY];
    a.clamp = a.lo > -inf || a.hi < inf;        // (NaN fails both: off; a NaN limit beside a real one never binds)
    a.slew = a.rate > 0.0 && a.rate < inf;
    a.hold = a.db > 0.0;
    a.quant = a.qu > 0.0;
    a.sense = a.qy > 0.0;
    return a;
}

// the sensor: the measured columns of the observation on the ADC's levels.  NM = 1 (pH: y) or 2 (tank: h1, h2)
template <int NM, int D>
__host__ __device__ __forceinline__ void act_measure(const ActRow& row, const float (&obs)[D], float (&om)[D]) {
#pragma unroll
    for (int j = 0; j < D; ++j) om[j] = obs[j];
    if (row.sense) {   // (wave-uniform)
#pragma unroll
        for (int j = 0; j < NM; ++j) om[j] = (float)(row.qy * rint((double)obs[j] / row.qy));
    }
}

// which stages changed the command of one step
struct ActFlags {
    bool held, slewed, clamped;
};

// the actuator: the applied action of a step from the controller's command and the previous applied action
__host__ __device__ __forceinline__ double act_apply(const ActRow& row, double a_c, double u_prev, ActFlags& f) {
    double v = a_c;
    f.held = f.slewed = f.clamped = false;
    if (row.hold) {
        if (fabs(v - u_prev) <= row.db) { v = u_prev; f.held = true; }
    }
    if (row.slew) {
        const double d = v - u_prev;
        double dc = d < -row.rate ? -row.rate : d;
        dc = dc > row.rate ? row.rate : dc;
        f.slewed = dc != d;
        v = u_prev + dc;
    }
    if (row.quant) v = row.qu * rint(v / row.qu);
    if (row.clamp) {
        if (v < row.lo) { v = row.lo; f.clamped = true; }
        if (v > row.hi) { v = row.hi; f.clamped = true; }
    }
    return v;
}

// The actuator rows of one segment over all its steps.  Counts are integers; GAP_IAE is a sequential double sum in ascending step
// order; the tail window is SegMetrics' (k >= tail_from), so numpy reproduces every row bit for bit from the three traces.
struct ActMetrics {
    double gap_peak, gap_iae, y_min, y_max, u_min, u_max;
    int sat, rate, hold, rev;
    int last;   // the sign of the last non-zero move of this segment, 0: none yet

    __host__ __device__ __forceinline__ void begin() {
        gap_peak = gap_iae = 0.0;
        y_min = y_max = u_min = u_max = 0.0;
        sat = rate = hold = rev = 0;
        last = 0;
    }
    // step k of the segment: the command, the applied action, the one before it, the controlled output after the step
    __host__ __device__ __forceinline__ void step(int k, int tail_from, double a_c, double u, double u_prev, double y, const ActFlags& f) {
        sat += f.clamped ? 1 : 0;
        rate += f.slewed ? 1 : 0;
        hold += f.held ? 1 : 0;
        const double g = fabs(a_c - u);
        gap_peak = g > gap_peak ? g : gap_peak;
        gap_iae += g;
        const double m = u - u_prev;
        const int s = m > 0.0 ? 1 : (m < 0.0 ? -1 : 0);
        if (s != 0) {
            if (last != 0 && s != last) ++rev;
            last = s;
        }
        if (k == tail_from) {   // (wave-uniform)
            y_min = y_max = y;
            u_min = u_max = u;
        } else if (k > tail_from) {
            y_min = y < y_min ? y : y_min; y_max = y > y_max ? y : y_max;
            u_min = u < u_min ? u : u_min; u_max = u > u_max ? u : u_max;
        }
    }
    __host__ __device__ __forceinline__ void rows(double* v) const {
        v[PIME_ACT_SAT_STEPS] = (double)sat;
        v[PIME_ACT_RATE_STEPS] = (double)rate;
        v[PIME_ACT_HOLD_STEPS] = (double)hold;
        v[PIME_ACT_GAP_PEAK] = gap_peak;
        v[PIME_ACT_GAP_IAE] = gap_iae;
        v[PIME_ACT_REVERSALS] = (double)rev;
        v[PIME_ACT_TAIL_Y_P2P] = y_max - y_min;
        v[PIME_ACT_TAIL_U_P2P] = u_max - u_min;
    }
};

// the sixteen rows of a finished segment in registers
__host__ __device__ __forceinline__ void act_rows(const SegMetrics& M, const ActMetrics& Q, double (&v)[kActAllRows]) {
    M.store(v, 0, 1, 0);
    Q.rows(v + PIME_METRIC_ROWS);
}

// One pH pair: lane E (a copy).  sink.step(t, u, y) and sink.command(t, a_c) once per step, sink(seg, M, Q) once per finished
// segment, all at wave-uniform points.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void act_ph_pair(const PhParams& p, const S* __restrict__ table, PhLane<S> E, const double (&K)[3],
                                                     const ActRow& row, const SweepSchedule& s, const Pol& pol, Sink& sink) {
    float obs[3];
    obs[0] = (float)ph_lookup<S>(p, table, E.C, E.x); obs[1] = (float)E.r; obs[2] = (float)E.I;
    SegMetrics M{};
    ActMetrics Q{};
    double u_prev = 0.0;
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {   // segment boundary: set r, zero I and t, a new episode beyond the first one
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            E.r = (S)sp; E.I = S(0); E.t = 0; E.episode += bump; obs[1] = (float)E.r; obs[2] = 0.f;
        }
        if (k == 0) {
            M.begin((double)ph_lookup<S>(p, table, E.C, E.x), (double)E.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
            Q.begin();
        }
        float om[3];
        act_measure<1, 3>(row, obs, om);
        const double a_c = disturb_controller<3>(om, K, pol);
        ActFlags f;
        const double u = act_apply(row, a_c, u_prev, f);
        float rew;
        (void)ph_lane_step<S>(p, table, u, E, obs, rew);
        double y;   // y after the step in the state's precision (float state: the observation is that value)
        if constexpr (sizeof(S) == sizeof(float)) y = (double)obs[0];
        else y = (double)ph_lookup<S>(p, table, E.C, E.x);
        sink.step(t, u, y);
        sink.command(t, a_c);
        M.step(k, y, u, rew, s.band);
        Q.step(k, M.tail_from, a_c, u, u_prev, y, f);
        u_prev = u;
        if (++k == M.len) {
            sink(seg, M, Q);
            ++seg; k = 0;
        }
    }
}

// One tank pair (Integrator observation).  gid: the PLANT's global lane, the key of its process noise -- the same for every row.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void act_wt_pair(const WtParams& p, uint32_t gid, WtLane<S> W, const double (&K)[4], const ActRow& row,
                                                     const SweepSchedule& s, const Pol& pol, Sink& sink) {
    float obs[4];
    obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
    SegMetrics M{};
    ActMetrics Q{};
    double u_prev = 0.0;
    int seg = 0, k = 0;
    for (int t = 0; t < s.n_steps; ++t) {
        if (s.seg_len > 0 && t % s.seg_len == 0) {
            const double sp = s.setpoint[t / s.seg_len];
            const int bump = t > 0 ? 1 : 0;
            W.r = (S)sp; W.I = S(0); W.t = 0; W.episode += bump; obs[2] = (float)W.r; obs[3] = 0.f;
        }
        if (k == 0) {
            M.begin((double)W.h2, (double)W.r, segment_steps(s.n_steps, s.seg_len, seg), s.tail);
            Q.begin();
        }
        float om[4];
        act_measure<2, 4>(row, obs, om);
        const double a_c = disturb_controller<4>(om, K, pol);
        ActFlags f;
        const double u = act_apply(row, a_c, u_prev, f);
        float rew;
        double z1n, z2n;
        wt_lane_noise<S>(p, gid, W, nullptr, z1n, z2n);
        (void)wt_lane_step<S>(p, u, z1n, z2n, W, rew);
        obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
        sink.step(t, u, (double)W.h2);
        sink.command(t, a_c);
        M.step(k, (double)W.h2, u, rew, s.band);
        Q.step(k, M.tail_from, a_c, u, u_prev, (double)W.h2, f);
        u_prev = u;
        if (++k == M.len) {
            sink(seg, M, Q);
            ++seg; k = 0;
        }
    }
}

// (actuator_sweep.hip)
template <typename S>
struct ActArgs {
    int env;                 // 0 pH, 1 water tank (Integrator observation)
    int n, P;                // plants (the handle's lanes), actuator rows
    int n_seg;
    uint32_t env_offset;
    PhParams p;
    PhPtrs<S> st;
    WtParams wp;
    WtPtrs<S> wst;
    const float* img;        // packed actor forward image (pime_mlp_pack), unused for the prior controller alone
    PriorK K;
    SweepSchedule s;
    double* commands;        // [n_steps][P * N] or nullptr: the third trace (the row grid carries two)
};
// workspace: float64[n_seg][kActAllRows][P][N], the copy of `pairs` the finishing launch reads when `pairs` is NULL
template <typename S>
int launch_actuator_sweep(int kind, int md, const ActArgs<S>& a, const double* actuator, double* pairs, double* summary, double* actions,
                          double* outputs, double* workspace, hipStream_t stream);

}  // namespace pime
