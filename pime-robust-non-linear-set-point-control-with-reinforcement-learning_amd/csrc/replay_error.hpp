// Replay of recorded runs (pime_env_replay_error): ONE candidate plant over ONE record, the lane in registers, the output error
// reduced while the record runs -- no trace, no handle state.  The step is ph_lane_step / wt_lane_step of env_device.hpp on a register
// copy of the lane, so a replayed step is bit for bit the arithmetic of pime_env_step with zero process noise.  __host__ __device__:
// replay_error.hip runs it one thread per (lane, record) pair, replay_error_host.hip compiles the SAME source into
// libpime_replay_host.so (float64 state; test infrastructure like the CPU twins).
#pragma once
#include "env_device.hpp"

namespace pime {

// a record set as the kernels see it (include/pime_hip.h: pime_replay_records); all float64, shared by every lane
struct ReplayRecords {
    const double* action;   // [E][T]
    const double* output;   // [E][T + 1][C]
    const double* state0;   // [E] (pH) or nullptr
    int E, T;
};

// The error rows of one (record, lane) pair.  All sums are sequential double additions in ascending step order, channel 0 before
// channel 1 (the build has -ffp-contract=off: d * d rounds before it is added), so a numpy reduction of the launch's own `sim`
// reproduces them bit for bit.  A NaN measurement is a gap: no term, not counted.
struct ReplayErr {
    double sse[2], mx[2];
    int count;
    __host__ __device__ __forceinline__ void begin() { sse[0] = sse[1] = mx[0] = mx[1] = 0.0; count = 0; }
    __host__ __device__ __forceinline__ void term(int c, double sim, double meas) {
        if (meas != meas) return;
        const double d = sim - meas, ad = fabs(d);
        sse[c] += d * d;
        mx[c] = ad > mx[c] ? ad : mx[c];
        count += 1;
    }
    // one coalesced store per row: lane i of record e
    __host__ __device__ __forceinline__ void store(double* __restrict__ err, int e, int N, int i) const {
        double* q = err + (size_t)e * PIME_REPLAY_ROWS * N + i;
        q[(size_t)PIME_REPLAY_SSE0 * N] = sse[0];
        q[(size_t)PIME_REPLAY_MAX0 * N] = mx[0];
        q[(size_t)PIME_REPLAY_SSE1 * N] = sse[1];
        q[(size_t)PIME_REPLAY_MAX1 * N] = mx[1];
        q[(size_t)PIME_REPLAY_COUNT * N] = (double)count;
    }
};

// Hidden pH state at row 0: the smallest table index whose entry is <= y0 (the table is strictly decreasing, so the index is
// unique), clamped to the table; y0 is compared in the table's precision S.  The same for every lane of a record.
template <typename S>
__host__ __device__ __forceinline__ int replay_ph_k0(const S* __restrict__ table, int table_len, double y0) {
    const S y = (S)y0;
    int lo = 0, hi = table_len;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (table[mid] <= y) hi = mid;
        else lo = mid + 1;
    }
    return lo < table_len ? lo : table_len - 1;
}

// pH: plant (A, B, C) over record e.  sim: this lane's column of [E][T][1][N] or nullptr.
template <typename S>
__host__ __device__ __forceinline__ void replay_ph_lane(const PhParams& p, const S* __restrict__ table, double A, double B, double C,
                                                        const ReplayRecords& rec, int e, int skip, ReplayErr& acc,
                                                        double* __restrict__ sim, int N) {
    const int T = rec.T;
    const double* __restrict__ act = rec.action + (size_t)e * T;
    const double* __restrict__ out = rec.output + (size_t)e * (T + 1);
    PhLane<S> L;
    L.A = A; L.B = B; L.C = C; L.qww = L.qc = 0.0;
    L.I = L.r = L.last_a = S(0);
    L.t = L.episode = 0;
    L.plant_changed = false;
    if (rec.state0) L.x = rec.state0[e];
    else L.x = (double)replay_ph_k0<S>(table, p.table_len, out[0]) / (C * p.table_scale);
    acc.begin();
    double* __restrict__ q = sim ? sim + (size_t)e * T * N : nullptr;
    for (int t = 0; t < T; ++t) {
        float obs[3], rew;
        L.t = 0;                                       // no TimeLimit, no reset: T may exceed max_steps
        (void)ph_lane_step<S>(p, table, act[t], L, obs, rew);
        const double y = (double)ph_lookup<S>(p, table, L.C, L.x);   // the y of the step (obs[0] is its float32 rounding)
        if (q) q[(size_t)t * N] = y;
        if (t >= skip) acc.term(0, y, out[t + 1]);
    }
}

// water tank: plant (a1, a2, kp) over record e.  sim: this lane's column of [E][T][2][N] or nullptr.
template <typename S, int MODE>
__host__ __device__ __forceinline__ void replay_wt_lane(const WtParams& p, S a1, S a2, S kp, const ReplayRecords& rec, int e, int skip,
                                                        ReplayErr& acc, double* __restrict__ sim, int N) {
    const int T = rec.T;
    const double* __restrict__ act = rec.action + (size_t)e * T;
    const double* __restrict__ out = rec.output + (size_t)e * (T + 1) * 2;
    WtLane<S> L;
    L.a1 = a1; L.a2 = a2; L.kp = kp;
    L.r = L.I = S(0);
    L.t = L.episode = 0;
    L.plant_changed = false;
    L.h1 = (S)out[0]; L.h2 = (S)out[1];
    acc.begin();
    double* __restrict__ q = sim ? sim + (size_t)e * T * 2 * N : nullptr;
    for (int t = 0; t < T; ++t) {
        if (MODE == PIME_REPLAY_PREDICT) {             // one step ahead: from the measured state; a gap keeps the simulated one
            const double m1 = out[2 * t], m2 = out[2 * t + 1];
            if (m1 == m1) L.h1 = (S)m1;
            if (m2 == m2) L.h2 = (S)m2;
        }
        float rew;
        L.t = 0;
        (void)wt_lane_step<S>(p, act[t], 0.0, 0.0, L, rew);          // process noise is zero whatever wt_noise_scale says
        const double y1 = (double)L.h1, y2 = (double)L.h2;
        if (q) { q[(size_t)(2 * t) * N] = y1; q[(size_t)(2 * t + 1) * N] = y2; }
        if (t >= skip) {
            acc.term(0, y1, out[2 * (t + 1)]);
            acc.term(1, y2, out[2 * (t + 1) + 1]);
        }
    }
}

// the argument errors of pime_env_replay_error and of its host build, checked before anything runs; `fn` names the entry point
inline int check_replay_args(const char* fn, bool is_ph, const pime_replay_records* rec, int mode, int skip, const double* err) {
    PIME_REQUIRE(rec != nullptr, "%s: rec is NULL", fn);
    PIME_REQUIRE(rec->E >= 1, "%s: E = %d (>= 1)", fn, rec->E);
    PIME_REQUIRE(rec->T >= 1, "%s: T = %d (>= 1)", fn, rec->T);
    PIME_REQUIRE(skip >= 0 && skip < rec->T, "%s: skip = %d (0 .. T - 1 = %d)", fn, skip, rec->T - 1);
    PIME_REQUIRE(rec->action != nullptr, "%s: rec.action is NULL", fn);
    PIME_REQUIRE(rec->output != nullptr, "%s: rec.output is NULL", fn);
    PIME_REQUIRE(err != nullptr, "%s: err is NULL", fn);
    PIME_REQUIRE(mode == PIME_REPLAY_SIMULATE || mode == PIME_REPLAY_PREDICT, "%s: unknown mode %d", fn, mode);
    PIME_REQUIRE(is_ph || rec->state0 == nullptr, "%s: rec.state0 is a pH argument (the tank's state at row 0 is rec.output's)", fn);
    PIME_REQUIRE(!is_ph || mode == PIME_REPLAY_SIMULATE, "%s: PIME_REPLAY_PREDICT on a pH env (its state x is not measured)", fn);
    return PIME_OK;
}

// (replay_error.hip)
template <typename S>
struct ReplayArgs {
    int env;                 // 0 pH, 1 water tank
    int n;
    PhParams p;
    WtParams wp;
    const S* table;          // pH
    const double *A, *B, *C;
    const S *a1, *a2, *kp;   // water tank
    int E, T, mode, skip;
};
template <typename S>
int launch_replay_error(const ReplayArgs<S>& a, const double* action, const double* output, const double* state0, double* err,
                        double* sim, hipStream_t stream);

}  // namespace pime
