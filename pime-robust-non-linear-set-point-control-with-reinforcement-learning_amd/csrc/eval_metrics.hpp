// Step-response metrics of the fused evaluation kernels (pime_rollout_eval_metrics): per lane and set-point segment the control
// indices one reads off a step response, accumulated in registers while the response runs and written once per segment --
// metrics [n_segments][PIME_METRIC_ROWS][N] float64 -- instead of a float64 trace of every step reduced on the host.
// Shared by rollout_eval.hip's rollout_eval_kernel and the evaluation mode of mlp16.hip's rollout16_kernel, in both as a
// compile-time variant (MODE, kEvalNone / kEvalMetrics / kEvalBand): the launches without metrics, and the training rollouts that share rollout16_kernel, carry none
// of this (profiles/eval_metrics_kernel_resources.txt).
#pragma once
#include "pime_common.hpp"

namespace pime {

struct EvalMetricsArgs {
    double* out;     // [n_segments][PIME_METRIC_ROWS][N], NULL: no metrics
    double band;     // settling band on |e|
    int tail;        // steady-state window (steps)
};

// All sums are sequential double additions in ascending step order (the build has -ffp-contract=off: e * e and (k + 1) * |e| round
// before they are added), so a numpy reduction of the launch's own trace reproduces them bit for bit.
struct SegMetrics {
    double iae, ise, itae, peak, tail_sum, ret, av;
    double r, dir, a_prev;
    int settle;      // 1 + the last step outside the band
    int len;         // steps this segment has (wave-uniform)
    int tail_from;   // first step of the steady-state window (wave-uniform)

    // y_start: the controlled output before the segment's first step; r: the segment's set-point as the lane state holds it
    __host__ __device__ __forceinline__ void begin(double y_start, double r_, int len_, int tail) {
        iae = ise = itae = tail_sum = ret = av = 0.0;
        peak = 0.0;                                  // max(0, .): the running maximum starts at the clamp
        r = r_;
        dir = r_ >= y_start ? 1.0 : -1.0;
        a_prev = 0.0;
        settle = 0;
        len = len_;
        tail_from = len_ - (tail < len_ ? tail : len_);
    }
    // step k of the segment: y the controlled output after it, a_env the env action as the trace records it, rew its float32 reward
    __host__ __device__ __forceinline__ void step(int k, double y, double a_env, float rew, double band) {
        const double e = r - y, ae = fabs(e);
        iae += ae;
        ise += e * e;
        itae += (double)(k + 1) * ae;
        const double o = dir * (y - r);
        peak = o > peak ? o : peak;
        if (ae > band) settle = k + 1;
        if (k >= tail_from) tail_sum += e;
        ret += (double)rew;
        if (k > 0) av += fabs(a_env - a_prev);
        a_prev = a_env;
    }
    // one coalesced store per row: lane i of segment seg
    __host__ __device__ __forceinline__ void store(double* out, int seg, int N, int i) const {
        double* q = out + (size_t)seg * PIME_METRIC_ROWS * N + i;
        q[(size_t)PIME_METRIC_IAE * N] = iae;
        q[(size_t)PIME_METRIC_ISE * N] = ise;
        q[(size_t)PIME_METRIC_ITAE * N] = itae;
        q[(size_t)PIME_METRIC_OVERSHOOT * N] = peak;
        q[(size_t)PIME_METRIC_SETTLING * N] = (double)settle;
        q[(size_t)PIME_METRIC_SSE * N] = tail_sum / (double)(len - tail_from);
        q[(size_t)PIME_METRIC_RETURN * N] = ret;
        q[(size_t)PIME_METRIC_ACTION_VAR * N] = av;
    }
};

// ---- response band (pime_rollout_eval_band): every step reduced ACROSS lanes ------------------------------------------------
// The third value of the kernels' compile-time mode; the band variant also produces the metrics.
constexpr int kEvalNone = 0, kEvalMetrics = 1, kEvalBand = 2;

struct EvalBandArgs {
    double* partial;       // workspace [n_steps][n_tiles][PIME_BAND_ROWS]: one 128-byte partial per 16-lane tile and step
    unsigned* hist;        // [n_steps][groups][bins] counts of Y, or NULL
    int n_tiles;           // ceil(N / 16)
    int tiles_per_group;   // group_lanes / 16 (one group: n_tiles)
    int groups, bins;
    double lo, hi, scale;  // scale = bins / (hi - lo)
};

// v of the lane a row-DPP control names (0x140 row_mirror: 15 - i; 0x141 row_half_mirror: 7 - i within the half row; quad_perm
// 0x1B: 3 - i, 0xB1: i ^ 1 within the quad).  All 64 lanes are active where the band runs (the step loop is wave-uniform).
template <int CTRL>
__device__ __forceinline__ double band_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// One step of one 16-lane tile.  The four lane groups of a wave hold copies of the same 16 lanes (bit-equal: the policy head ends
// in a butterfly over the lane groups), so lane group q reduces signal q -- Y, E, A, R -- over its 16 lanes, the row of a DPP
// operation: four mirrored folds (16 -> 8 -> 4 -> 2 -> 1 distinct values; a + b == b + a bit for bit, so both partners of a fold
// hold the same value and the order is fixed), no LDS crossbar.  Lane 0 of the lane group stores SUM, SUMSQ, MIN, MAX: 32 bytes,
// 128 per tile.  Idle lanes (shadows of lane N - 1) add 0 and +-inf.  `store`: lane 0 of a lane group of the wave that owns the
// tile (QUAD: wave 0), the tile has a valid lane; `writer`: the one copy of a valid lane that counts in the histogram.
__device__ __forceinline__ void band_step(const EvalBandArgs& b, int t, int tile, int q, bool valid, bool store, bool writer, int grp,
                                          double y, double e, double a, double r) {
    const double x = q == 0 ? y : (q == 1 ? e : (q == 2 ? a : r));
    double s = valid ? x : 0.0, ss = valid ? x * x : 0.0;
    double mn = valid ? x : __builtin_huge_val(), mx = valid ? x : -__builtin_huge_val();
#define PIME_BAND_FOLD(CTRL)                                                      \
    {                                                                             \
        s += band_dpp<CTRL>(s);                                                   \
        ss += band_dpp<CTRL>(ss);                                                 \
        const double mo = band_dpp<CTRL>(mn), xo = band_dpp<CTRL>(mx);            \
        mn = mo < mn ? mo : mn;                                                   \
        mx = xo > mx ? xo : mx;                                                   \
    }
    PIME_BAND_FOLD(0x140) PIME_BAND_FOLD(0x141) PIME_BAND_FOLD(0x1B) PIME_BAND_FOLD(0xB1)
#undef PIME_BAND_FOLD
    if (store) {
        double* p = b.partial + ((size_t)t * b.n_tiles + tile) * PIME_BAND_ROWS + 4 * q;
        p[PIME_BAND_SUM] = s; p[PIME_BAND_SUMSQ] = ss; p[PIME_BAND_MIN] = mn; p[PIME_BAND_MAX] = mx;
    }
    if (b.hist != nullptr && writer) {
        int bin = 0;
        if (y >= b.hi) bin = b.bins - 1;
        else if (y >= b.lo) {
            bin = (int)floor((y - b.lo) * b.scale);
            bin = bin > b.bins - 1 ? b.bins - 1 : bin;
        }
        atomicAdd(b.hist + ((size_t)t * b.groups + grp) * b.bins + bin, 1u);   // integer counts: exact, order-free
    }
}

// the steps segment `seg` has in a launch of n_steps with a boundary every seg_len steps (seg_len 0: one segment)
__host__ __device__ __forceinline__ int segment_steps(int n_steps, int seg_len, int seg) {
    if (seg_len <= 0) return n_steps;
    const int left = n_steps - seg * seg_len;
    return left < seg_len ? left : seg_len;
}

}  // namespace pime
