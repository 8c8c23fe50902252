// libpime_margin_host.so (include/pime_margin_host.h): the pair function of pime_margin_sweep -- margin_sweep.hpp, the source the
// kernel runs -- compiled for the host under the prior controller alone (MarginNoPolicy), in float64 and float32 state, no handle;
// the summary's order (blocks of 64 plants, the balanced pairwise tree inside a block, the blocks in ascending order) written as a
// plain loop.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the loop perturbations can be checked on a machine without a GPU, and the GPU
// tests have a float64 result to be bit-equal to.
#include <vector>

#include "env_handle.hpp"
#include "margin_sweep.hpp"
#include "pime_margin_host.h"

namespace pime {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {
// a host pair keeps its rows and, if asked, its signals: vals [n_seg][ROWS][N] column i; actions / outputs [n_steps][P * N] column col
struct MarginHostSink {
    double* vals;
    double *actions, *outputs;
    int N, i;
    size_t PN, col;
    void step(int t, double u, double y) const {
        if (actions) actions[(size_t)t * PN + col] = u;
        if (outputs) outputs[(size_t)t * PN + col] = y;
    }
    void operator()(int seg, const SegMetrics& M) const {
        double v[PIME_METRIC_ROWS];
        sweep_rows(M, v);
        for (int row = 0; row < PIME_METRIC_ROWS; ++row) vals[((size_t)seg * PIME_METRIC_ROWS + row) * N + i] = v[row];
    }
};

// one row over the N plants, into out[PIME_SWEEP_STATS]: the order pime_prior_sweep documents
void margin_host_reduce(const double* x, int N, double* out) {
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

template <typename S>
void margin_host_run(const pime_env_cfg* cfg, const PhParams& ph, const WtParams& wt, const pime_sweep_lanes* lanes, int N,
                     const double* priorK, const double* perturb, int P, const MarginNoise& nz, const SweepSchedule& s, double* pairs,
                     double* summary, double* actions, double* outputs) {
    const bool is_ph = cfg->kind == PIME_ENV_PH;
    std::vector<S> table;
    if (is_ph) {
        table.resize((size_t)cfg->ph_table_len);
        for (size_t k = 0; k < table.size(); ++k) table[k] = (S)cfg->ph_table[k];
    }
    const int n_seg = sweep_segments(s.n_steps, s.seg_len);
    std::vector<double> vals((size_t)n_seg * PIME_METRIC_ROWS * N);
    for (int p = 0; p < P; ++p) {
        const MarginRow row = margin_row(perturb + (size_t)p * PIME_PERTURB_COLS);
        for (int i = 0; i < N; ++i) {
            MarginHostSink sink{vals.data(), actions, outputs, N, i, (size_t)P * N, (size_t)p * N + i};
            const uint32_t gid = cfg->env_offset + (uint32_t)i;   // the PLANT's global lane keys both noises
            if (is_ph) {
                PhLane<S> E{};
                E.x = lanes->ph_x[i]; E.A = lanes->ph_A[i]; E.B = lanes->ph_B[i]; E.C = lanes->ph_C[i];
                E.I = (S)lanes->I[i]; E.r = (S)lanes->r[i]; E.t = lanes->t[i]; E.episode = lanes->episode[i];
                E.last_a = ph.has_punish && lanes->ph_last_a ? (S)lanes->ph_last_a[i] : S(0);
                const double K[3] = {priorK[0], priorK[1], priorK[2]};
                margin_ph_pair<S>(ph, table.data(), gid, E, K, row, nz, s, MarginNoPolicy{}, sink);
            } else {
                WtLane<S> W{};
                W.h1 = (S)lanes->wt_h1[i]; W.h2 = (S)lanes->wt_h2[i]; W.r = (S)lanes->r[i]; W.I = (S)lanes->I[i];
                W.a1 = (S)lanes->wt_a1[i]; W.a2 = (S)lanes->wt_a2[i]; W.kp = (S)lanes->wt_kp[i];
                W.t = lanes->t[i]; W.episode = lanes->episode[i];
                const double K[4] = {priorK[0], priorK[1], priorK[2], priorK[3]};
                margin_wt_pair<S>(wt, gid, W, K, row, nz, s, MarginNoPolicy{}, sink);
            }
        }
        for (int cell = 0; cell < n_seg * PIME_METRIC_ROWS; ++cell) {
            const double* x = vals.data() + (size_t)cell * N;
            if (pairs) {
                double* q = pairs + ((size_t)cell * P + p) * N;
                for (int i = 0; i < N; ++i) q[i] = x[i];
            }
            margin_host_reduce(x, N, summary + ((size_t)p * n_seg * PIME_METRIC_ROWS + cell) * PIME_SWEEP_STATS);
        }
    }
}
}  // namespace
}  // namespace pime

using namespace pime;

extern "C" {

const char* pime_margin_host_last_error(void) { return g_err; }

int pime_margin_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* priorK,
                           const double* perturb, int32_t P, uint64_t noise_seed, uint32_t noise_epoch, int32_t n_steps,
                           int32_t seg_len, const double* setpoints, int32_t n_setpoints, double band, int32_t tail, double* pairs,
                           double* summary, double* actions, double* outputs) {
    const char* fn = "pime_margin_sweep_host";
    if (int rc = check_cfg(cfg)) return rc;
    PIME_REQUIRE(lanes != nullptr && N >= 1, "%s: NULL lanes or N = %d", fn, N);
    const bool is_ph = cfg->kind == PIME_ENV_PH;
    PIME_REQUIRE(cfg->state_mode == PIME_STATE_F64 || cfg->state_mode == PIME_STATE_MIXED, "%s: not served for state_mode %d", fn,
                 cfg->state_mode);
    PIME_REQUIRE(is_ph || cfg->num_stack == 0, "%s: not served for the Stacking observation", fn);
    PIME_REQUIRE(lanes->r && lanes->I && lanes->t && lanes->episode, "%s: a lane array (r, I, t, episode) is NULL", fn);
    if (is_ph) PIME_REQUIRE(lanes->ph_x && lanes->ph_A && lanes->ph_B && lanes->ph_C, "%s: a pH lane array is NULL", fn);
    else PIME_REQUIRE(lanes->wt_h1 && lanes->wt_h2 && lanes->wt_a1 && lanes->wt_a2 && lanes->wt_kp, "%s: a tank lane array is NULL", fn);
    if (int rc = check_margin_args(fn, N, priorK, perturb, P, n_steps, seg_len, setpoints, n_setpoints, band, tail, summary)) return rc;
    PhParams ph{};
    WtParams wt{};
    pime_env_cfg c = *cfg;
    c.n_envs = N;
    fill_params(c, is_ph ? 3 : 4, ph, wt);
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    const MarginNoise nz{noise_seed, noise_epoch};
    if (cfg->state_mode == PIME_STATE_F64) margin_host_run<double>(cfg, ph, wt, lanes, N, priorK, perturb, P, nz, s, pairs, summary, actions, outputs);
    else margin_host_run<float>(cfg, ph, wt, lanes, N, priorK, perturb, P, nz, s, pairs, summary, actions, outputs);
    return PIME_OK;
}

}  // extern "C"
