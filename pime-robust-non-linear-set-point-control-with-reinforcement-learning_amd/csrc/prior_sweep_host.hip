// libpime_sweep_host.so (include/pime_sweep_host.h): the pair function of pime_prior_sweep -- prior_sweep.hpp, the source the kernel
// runs -- compiled for the host, float64 state, no handle; the summary's order (blocks of 64 plants, the balanced pairwise tree
// inside a block, the blocks in ascending order) written as a plain loop.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the arithmetic of the sweep can be checked on a machine without a GPU, and the
// GPU tests have a float64 result to be bit-equal to.
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

namespace {
// a host pair keeps its rows: vals [n_seg][ROWS][N], column i
struct SweepHostSink {
    double* vals;
    int N, i;
    void operator()(int seg, const SegMetrics& M) const {
        double v[PIME_METRIC_ROWS];
        sweep_rows(M, v);
        for (int row = 0; row < PIME_METRIC_ROWS; ++row) vals[((size_t)seg * PIME_METRIC_ROWS + row) * N + i] = v[row];
    }
};

// one row over the N plants, into out[PIME_SWEEP_STATS]
void sweep_host_reduce(const double* x, int N, double* out) {
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
}  // namespace
}  // namespace pime

using namespace pime;

extern "C" {

const char* pime_sweep_host_last_error(void) { return g_err; }

int pime_prior_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* gains, int32_t G,
                          int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints, double band, int32_t tail,
                          double* pairs, double* summary) {
    const char* fn = "pime_prior_sweep_host";
    if (int rc = check_cfg(cfg)) return rc;
    PIME_REQUIRE(lanes != nullptr && N >= 1, "%s: NULL lanes or N = %d", fn, N);
    const bool is_ph = cfg->kind == PIME_ENV_PH;
    PIME_REQUIRE(is_ph || cfg->num_stack == 0, "%s: not served for the Stacking observation", fn);
    PIME_REQUIRE(lanes->r && lanes->I && lanes->t && lanes->episode, "%s: a lane array (r, I, t, episode) is NULL", fn);
    if (is_ph) PIME_REQUIRE(lanes->ph_x && lanes->ph_A && lanes->ph_B && lanes->ph_C, "%s: a pH lane array is NULL", fn);
    else PIME_REQUIRE(lanes->wt_h1 && lanes->wt_h2 && lanes->wt_a1 && lanes->wt_a2 && lanes->wt_kp, "%s: a tank lane array is NULL", fn);
    if (int rc = check_sweep_args(fn, N, gains, G, n_steps, seg_len, setpoints, n_setpoints, band, tail, summary)) return rc;
    PhParams ph{};
    WtParams wt{};
    pime_env_cfg c = *cfg;
    c.n_envs = N;
    fill_params(c, is_ph ? 3 : 4, ph, wt);
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    const int n_seg = sweep_segments(n_steps, seg_len);
    std::vector<double> vals((size_t)n_seg * PIME_METRIC_ROWS * N);
    for (int g = 0; g < G; ++g) {
        for (int i = 0; i < N; ++i) {
            SweepHostSink sink{vals.data(), N, i};
            if (is_ph) {
                PhLane<double> E{};
                E.x = lanes->ph_x[i]; E.A = lanes->ph_A[i]; E.B = lanes->ph_B[i]; E.C = lanes->ph_C[i];
                E.I = lanes->I[i]; E.r = lanes->r[i]; E.t = lanes->t[i]; E.episode = lanes->episode[i];
                E.last_a = ph.has_punish && lanes->ph_last_a ? lanes->ph_last_a[i] : 0.0;
                const double K[3] = {gains[3 * (size_t)g], gains[3 * (size_t)g + 1], gains[3 * (size_t)g + 2]};
                sweep_ph_pair<double>(ph, cfg->ph_table, E, K, s, sink);
            } else {
                WtLane<double> W{};
                W.h1 = lanes->wt_h1[i]; W.h2 = lanes->wt_h2[i]; W.r = lanes->r[i]; W.I = lanes->I[i];
                W.a1 = lanes->wt_a1[i]; W.a2 = lanes->wt_a2[i]; W.kp = lanes->wt_kp[i];
                W.t = lanes->t[i]; W.episode = lanes->episode[i];
                const double K[4] = {gains[4 * (size_t)g], gains[4 * (size_t)g + 1], gains[4 * (size_t)g + 2], gains[4 * (size_t)g + 3]};
                sweep_wt_pair<double>(wt, cfg->env_offset + (uint32_t)i, W, K, s, sink);   // the PLANT's global lane keys the noise
            }
        }
        for (int cell = 0; cell < n_seg * PIME_METRIC_ROWS; ++cell) {
            const double* x = vals.data() + (size_t)cell * N;
            if (pairs) {
                double* q = pairs + ((size_t)cell * G + g) * N;
                for (int i = 0; i < N; ++i) q[i] = x[i];
            }
            sweep_host_reduce(x, N, summary + ((size_t)g * n_seg * PIME_METRIC_ROWS + cell) * PIME_SWEEP_STATS);
        }
    }
    return PIME_OK;
}

}  // extern "C"
