// What the host builds of the plant-grid calls share (prior_sweep_host.hip, mpc_eval_host.hip, margin_sweep_host.hip,
// disturb_sweep_host.hip, freq_sweep_host.hip; the error buffer also replay_error_host.hip): the last-error buffer, the opening checks of an entry point, a lane of pime_sweep_lanes as the
// register copy the pair / plant functions take, the metric-row and trace sinks and THE host statement of the summary's order of additions.
// Host only and test infrastructure like the libraries that include it; each of them is one translation unit, so set_error is
// defined here.
#pragma once
#include <vector>

#include "env_handle.hpp"
#include "pime_sweep_host.h"
#include "prior_sweep.hpp"

namespace pime {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// the parameter blocks of N lanes under cfg
struct HostGrid {
    bool is_ph;
    PhParams ph;
    WtParams wt;
};

// the opening of an entry point: cfg, lanes and N, the state mode (where the build serves float32 state too), Stacking, the lane
// arrays; then g.  The checks, their order and their texts are the device entry points'.
inline int host_grid_open(const char* fn, const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int N, bool check_state_mode,
                          HostGrid& g) {
    if (int rc = check_cfg(cfg)) return rc;
    PIME_REQUIRE(lanes != nullptr && N >= 1, "%s: NULL lanes or N = %d", fn, N);
    g.is_ph = cfg->kind == PIME_ENV_PH;
    if (check_state_mode)
        PIME_REQUIRE(cfg->state_mode == PIME_STATE_F64 || cfg->state_mode == PIME_STATE_MIXED, "%s: not served for state_mode %d", fn,
                     cfg->state_mode);
    PIME_REQUIRE(g.is_ph || cfg->num_stack == 0, "%s: not served for the Stacking observation", fn);
    PIME_REQUIRE(lanes->r && lanes->I && lanes->t && lanes->episode, "%s: a lane array (r, I, t, episode) is NULL", fn);
    if (g.is_ph) PIME_REQUIRE(lanes->ph_x && lanes->ph_A && lanes->ph_B && lanes->ph_C, "%s: a pH lane array is NULL", fn);
    else PIME_REQUIRE(lanes->wt_h1 && lanes->wt_h2 && lanes->wt_a1 && lanes->wt_a2 && lanes->wt_kp, "%s: a tank lane array is NULL", fn);
    pime_env_cfg c = *cfg;
    c.n_envs = N;
    fill_params(c, g.is_ph ? 3 : 4, g.ph, g.wt);
    return PIME_OK;
}

// lane i in state type S
template <typename S>
PhLane<S> host_ph_lane(const PhParams& ph, const pime_sweep_lanes* lanes, int i) {
    PhLane<S> E{};
    E.x = lanes->ph_x[i]; E.A = lanes->ph_A[i]; E.B = lanes->ph_B[i]; E.C = lanes->ph_C[i];
    E.I = (S)lanes->I[i]; E.r = (S)lanes->r[i]; E.t = lanes->t[i]; E.episode = lanes->episode[i];
    E.last_a = ph.has_punish && lanes->ph_last_a ? (S)lanes->ph_last_a[i] : S(0);
    return E;
}
template <typename S>
WtLane<S> host_wt_lane(const pime_sweep_lanes* lanes, int i) {
    WtLane<S> W{};
    W.h1 = (S)lanes->wt_h1[i]; W.h2 = (S)lanes->wt_h2[i]; W.r = (S)lanes->r[i]; W.I = (S)lanes->I[i];
    W.a1 = (S)lanes->wt_a1[i]; W.a2 = (S)lanes->wt_a2[i]; W.kp = (S)lanes->wt_kp[i];
    W.t = lanes->t[i]; W.episode = lanes->episode[i];
    return W;
}

// the titration table in S (empty for the tank)
template <typename S>
std::vector<S> host_table(const pime_env_cfg* cfg) {
    if (cfg->kind != PIME_ENV_PH) return {};
    return std::vector<S>(cfg->ph_table, cfg->ph_table + cfg->ph_table_len);
}

// a host pair keeps its rows: vals [n_seg][ROWS][N], column i
struct HostRowSink {
    double* vals;
    int N, i;
    void operator()(int seg, const SegMetrics& M) const { M.store(vals, seg, N, i); }
};

// one row over the N plants, into out[PIME_SWEEP_STATS], in the order pime_prior_sweep documents: blocks of 64 plants, the balanced
// pairwise tree inside a block, the blocks in ascending order
inline void host_reduce_row(const double* x, int N, double* out) {
    double total = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    int arg = -1, cnt = 0;
    for (int b = 0; b * kSweepBlockPlants < N; ++b) {
        double w[kSweepBlockPlants];
        for (int l = 0; l < kSweepBlockPlants; ++l) {
            const int i = b * kSweepBlockPlants + l;
            const bool c = i < N && sweep_counts(x[i]);
            w[l] = c ? x[i] : 0.0;
            if (c) {
                cnt += 1;
                mn = x[i] < mn ? x[i] : mn;
                if (x[i] > mx) { mx = x[i]; arg = i; }   // ascending i, strictly: the smallest index on a tie
            }
        }
        for (int width = kSweepBlockPlants; width > 1; width >>= 1)   // level 0 adds 2j and 2j + 1, level 1 the results pairwise, ...
            for (int j = 0; j < width / 2; ++j) w[j] = w[2 * j] + w[2 * j + 1];
        total = b == 0 ? w[0] : total + w[0];
    }
    out[PIME_SWEEP_SUM] = total; out[PIME_SWEEP_MIN] = mn; out[PIME_SWEEP_MAX] = mx; out[PIME_SWEEP_ARGMAX] = (double)arg;
    out[PIME_SWEEP_FINITE] = (double)cnt;
}

// a host pair's signals, if asked: actions / outputs [n_steps][P * N], column col
struct HostTraceSink {
    double *actions, *outputs;
    size_t PN, col;
    void step(int t, double u, double y) const {
        if (actions) actions[(size_t)t * PN + col] = u;
        if (outputs) outputs[(size_t)t * PN + col] = y;
    }
};

// the rows of sweep row `r` of R (a gain row, a perturbation row, a disturbance row, an excitation row), ROWS per segment: vals into pairs
// [n_seg][ROWS][R][N] (if asked) and, reduced, into summary [R][n_seg][ROWS][PIME_SWEEP_STATS]
inline void host_reduce_rows(const double* vals, int n_seg, int ROWS, int N, int r, int R, double* pairs, double* summary) {
    const int cells = n_seg * ROWS;
    for (int cell = 0; cell < cells; ++cell) {
        const double* x = vals + (size_t)cell * N;
        if (pairs) {
            double* q = pairs + ((size_t)cell * R + r) * N;
            for (int i = 0; i < N; ++i) q[i] = x[i];
        }
        host_reduce_row(x, N, summary + ((size_t)r * cells + cell) * PIME_SWEEP_STATS);
    }
}

}  // namespace pime
