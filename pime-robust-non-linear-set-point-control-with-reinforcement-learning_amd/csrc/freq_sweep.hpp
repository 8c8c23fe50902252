// Frequency-response sweep (pime_freq_sweep): ONE (excitation row, plant lane) pair, the lane in registers.  The loop is the loop of
// rollout_eval_kernel with metrics (rollout_eval.hip) on a register copy of the lane -- the same boundaries, the same lane step, the
// same SegMetrics calls -- with an excitation e_k = A * s_k at EVERY segment step k, (c_k, s_k) = wave[k] the row's table (wave-uniform:
// one 16-byte uniform load per step, no transcendental in the loop), entering at the row's POINT:
//   SETPOINT     the lane's set-point word of step k is (S)(sp + e_k), sp the segment's set-point in double (the lane's stored word when
//                the schedule has no boundary), and the observation's set-point column follows it: the env integrates the error
//                against the modulated set-point.  SegMetrics keeps the segment's NOMINAL set-point.
//   LOAD         a_env = a_c + e_k, one double addition IN FRONT of the actuator (pH's clip inside ph_lane_step sees the sum).
//   MEASUREMENT  the controller reads obs[c] + (float)e_k in float32, c the controlled output's column (pH 0: y, tank 1: h2); the env
//                integrates the TRUE error (margin_sweep.hpp).
// A == 0.0 is a wave-uniform branch under which nothing is added and no word is rewritten: the eight SegMetrics rows are then bit for
// bit a lane of pime_rollout_eval_metrics, for any POINT, ONSET and table.
// SegMetrics and the recorded action receive the CONTROLLER's output a_c.  FreqMetrics accumulates PIME_FREQ_ROWS lock-in rows per
// segment over the window k >= k0.
// __host__ __device__: freq_sweep.hip runs it on 16-lane tiles (64-lane tiles under the prior alone), freq_sweep_host.hip compiles the
// SAME source into libpime_freq_host.so (prior controller only; test infrastructure like the CPU twins).
#pragma once
#include "disturb_sweep.hpp"

namespace pime {

constexpr int kFreqAllRows = PIME_METRIC_ROWS + PIME_FREQ_ROWS;   // the rows of a pair per segment

// a decoded row of `excite` (wave-uniform on the device)
struct FreqRow {
    int point;    // enum pime_freq_point
    int k0;       // the correlation window starts at segment step k0
    double A;     // amplitude
    bool on;      // A != 0: excite
};
__host__ __device__ __forceinline__ FreqRow freq_row(const double* __restrict__ r) {
    FreqRow f;
    const double pt = rint(r[PIME_FREQ_POINT]);   // (NaN fails both comparisons: 0)
    f.point = pt >= (double)PIME_FREQ_MEASUREMENT ? PIME_FREQ_MEASUREMENT : (pt >= 0.0 ? (int)pt : 0);
    f.A = r[PIME_FREQ_AMPLITUDE];
    f.k0 = disturb_steps(r[PIME_FREQ_ONSET], kDisturbNever);
    f.on = !(f.A == 0.0);
    return f;
}

// the table's refusals of an entry point `fn` (after check_row_grid_args: n_steps and seg_len are sound)
inline int check_freq_wave(const char* fn, const double* wave, int wave_len, int n_steps, int seg_len) {
    PIME_REQUIRE(wave != nullptr, "%s: wave is NULL", fn);
    const int L = seg_len > 0 ? seg_len : n_steps;
    PIME_REQUIRE(wave_len == L, "%s: wave_len %d is not %d (seg_len, or n_steps when seg_len is 0)", fn, wave_len, L);
    return PIME_OK;
}

// The lock-in rows of one segment over the window k >= k0.  All sums are sequential double additions in ascending step order from 0.0
// and every product rounds before it is added (-ffp-contract=off), so numpy reproduces them bit for bit from the traces and the table.
struct FreqMetrics {
    double yc, ys, uc, us, y0, u0, y2, u2;
    bool seen;           // the window is not empty (wave-uniform)

    __host__ __device__ __forceinline__ void begin() {
        yc = ys = uc = us = y0 = u0 = y2 = u2 = 0.0;
        seen = false;
    }
    // step k of the segment: y the controlled output after the step, a_c the controller's output, (c, s) the table's pair of step k
    __host__ __device__ __forceinline__ void step(int k, int k0, double y, double a_c, double c, double s) {
        if (k >= k0) {   // (wave-uniform)
            yc += y * c; ys += y * s;
            uc += a_c * c; us += a_c * s;
            y0 += y; u0 += a_c;
            y2 += y * y; u2 += a_c * a_c;
            seen = true;
        }
    }
    // rows PIME_METRIC_ROWS .. of v; a segment that never reaches k0: NaN
    __host__ __device__ __forceinline__ void rows(double* v) const {
        const double nan = __builtin_nan("");
        v[PIME_FREQ_YC] = seen ? yc : nan; v[PIME_FREQ_YS] = seen ? ys : nan;
        v[PIME_FREQ_UC] = seen ? uc : nan; v[PIME_FREQ_US] = seen ? us : nan;
        v[PIME_FREQ_Y0] = seen ? y0 : nan; v[PIME_FREQ_U0] = seen ? u0 : nan;
        v[PIME_FREQ_Y2] = seen ? y2 : nan; v[PIME_FREQ_U2] = seen ? u2 : nan;
    }
};

// the sixteen rows of a finished segment in registers
__host__ __device__ __forceinline__ void freq_rows(const SegMetrics& M, const FreqMetrics& Q, double (&v)[kFreqAllRows]) {
    M.store(v, 0, 1, 0);
    Q.rows(v + PIME_METRIC_ROWS);
}

// the controller's output from the env's observation with the measurement excitation on column C (disturb_controller's order)
template <int C, int D, typename Pol>
__host__ __device__ __forceinline__ double freq_controller(const float (&obs)[D], const double (&K)[D], bool measure, double e,
                                                           const Pol& pol) {
    if (!measure) return disturb_controller<D>(obs, K, pol);   // (wave-uniform)
    float om[D];
#pragma unroll
    for (int j = 0; j < D; ++j) om[j] = obs[j];
    om[C] = om[C] + (float)e;
    return disturb_controller<D>(om, K, pol);
}

// the segment's nominal set-point in double: the schedule's (a uniform load; kept live per lane it cost two registers and, in one
// class, a wave per SIMD), or the lane's stored word
template <typename S>
__host__ __device__ __forceinline__ double freq_setpoint(const SweepSchedule& s, int seg, S r0) {
    return s.seg_len > 0 ? s.setpoint[seg] : (double)r0;
}

// One pH pair: lane E (a copy); wave: the ROW's table, [L][2] doubles (c_k, s_k), L >= every segment's steps.  sink.step(t, a_c, y)
// once per step, sink(seg, M, Q) once per finished segment, both at wave-uniform points.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void freq_ph_pair(const PhParams& p, const S* __restrict__ table, PhLane<S> E, const double (&K)[3],
                                                      const FreqRow& row, const double* __restrict__ wave, const SweepSchedule& s,
                                                      const Pol& pol, Sink& sink) {
    const bool at_sp = row.on && row.point == PIME_FREQ_SETPOINT, at_load = row.on && row.point == PIME_FREQ_LOAD,
               at_meas = row.on && row.point == PIME_FREQ_MEASUREMENT;
    float obs[3];
    obs[0] = (float)ph_lookup<S>(p, table, E.C, E.x); obs[1] = (float)E.r; obs[2] = (float)E.I;
    SegMetrics M{};
    FreqMetrics Q{};
    const S r0 = E.r;   // without a schedule the segment's set-point is the lane's stored word
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
        const double c = wave[2 * k], sn = wave[2 * k + 1];   // (wave-uniform)
        const double e = row.A * sn;
        if (at_sp) { E.r = (S)(freq_setpoint(s, seg, r0) + e); obs[1] = (float)E.r; }
        const double a_c = freq_controller<0, 3>(obs, K, at_meas, e, pol);
        double a_env = a_c;
        if (at_load) a_env = a_c + e;
        float rew;
        (void)ph_lane_step<S>(p, table, a_env, E, obs, rew);
        double y;   // y after the step in the state's precision (float state: the observation is that value)
        if constexpr (sizeof(S) == sizeof(float)) y = (double)obs[0];
        else y = (double)ph_lookup<S>(p, table, E.C, E.x);
        sink.step(t, a_c, y);
        M.step(k, y, a_c, rew, s.band);
        Q.step(k, row.k0, y, a_c, c, sn);
        if (++k == M.len) {
            sink(seg, M, Q);
            ++seg; k = 0;
        }
    }
}

// One tank pair (Integrator observation).  gid: the PLANT's global lane, the key of its process noise -- the same for every row.
template <typename S, typename Pol, typename Sink>
__host__ __device__ __forceinline__ void freq_wt_pair(const WtParams& p, uint32_t gid, WtLane<S> W, const double (&K)[4],
                                                      const FreqRow& row, const double* __restrict__ wave, const SweepSchedule& s,
                                                      const Pol& pol, Sink& sink) {
    const bool at_sp = row.on && row.point == PIME_FREQ_SETPOINT, at_load = row.on && row.point == PIME_FREQ_LOAD,
               at_meas = row.on && row.point == PIME_FREQ_MEASUREMENT;
    float obs[4];
    obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
    SegMetrics M{};
    FreqMetrics Q{};
    const S r0 = W.r;
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
        const double c = wave[2 * k], sn = wave[2 * k + 1];   // (wave-uniform)
        const double e = row.A * sn;
        if (at_sp) { W.r = (S)(freq_setpoint(s, seg, r0) + e); obs[2] = (float)W.r; }
        const double a_c = freq_controller<1, 4>(obs, K, at_meas, e, pol);
        double a_env = a_c;
        if (at_load) a_env = a_c + e;
        float rew;
        double z1n, z2n;
        wt_lane_noise<S>(p, gid, W, nullptr, z1n, z2n);
        (void)wt_lane_step<S>(p, a_env, z1n, z2n, W, rew);
        obs[0] = (float)W.h1; obs[1] = (float)W.h2; obs[2] = (float)W.r; obs[3] = (float)W.I;
        sink.step(t, a_c, (double)W.h2);
        M.step(k, (double)W.h2, a_c, rew, s.band);
        Q.step(k, row.k0, (double)W.h2, a_c, c, sn);
        if (++k == M.len) {
            sink(seg, M, Q);
            ++seg; k = 0;
        }
    }
}

// (freq_sweep.hip) DisturbArgs plus the table
template <typename S>
struct FreqArgs : DisturbArgs<S> {
    const double* wave;      // [P][wave_len][2]: (c_k, s_k) of row p at segment step k
    int wave_len;            // seg_len, or n_steps without a schedule: no segment is longer
};
// workspace: float64[n_seg][kFreqAllRows][P][N], the copy of `pairs` the finishing launch reads when `pairs` is NULL
template <typename S>
int launch_freq_sweep(int kind, int md, const FreqArgs<S>& a, const double* excite, double* pairs, double* summary, double* actions,
                      double* outputs, double* workspace, hipStream_t stream);

}  // namespace pime
