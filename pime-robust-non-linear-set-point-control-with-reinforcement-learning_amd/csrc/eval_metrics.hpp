// Step-response metrics of the fused evaluation kernels (pime_rollout_eval_metrics): per lane and set-point segment the control
// indices one reads off a step response, accumulated in registers while the response runs and written once per segment --
// metrics [n_segments][PIME_METRIC_ROWS][N] float64 -- instead of a float64 trace of every step reduced on the host.
// Shared by rollout_eval.hip's rollout_eval_kernel and the evaluation mode of mlp16.hip's rollout16_kernel, in both as a
// compile-time variant (METRICS): the launches without metrics, and the training rollouts that share rollout16_kernel, carry none
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
    __device__ __forceinline__ void begin(double y_start, double r_, int len_, int tail) {
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
    __device__ __forceinline__ void step(int k, double y, double a_env, float rew, double band) {
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
    __device__ __forceinline__ void store(double* out, int seg, int N, int i) const {
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

// the steps segment `seg` has in a launch of n_steps with a boundary every seg_len steps (seg_len 0: one segment)
__device__ __forceinline__ int segment_steps(int n_steps, int seg_len, int seg) {
    if (seg_len <= 0) return n_steps;
    const int left = n_steps - seg * seg_len;
    return left < seg_len ? left : seg_len;
}

}  // namespace pime
