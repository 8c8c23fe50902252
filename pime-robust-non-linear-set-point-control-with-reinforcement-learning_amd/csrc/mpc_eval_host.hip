// libpime_mpc_host.so (include/pime_mpc_host.h): the closed loop of pime_mpc_eval -- mpc_eval.hpp, the source the kernel runs --
// compiled for the host in float64 and float32 state, no handle; the 64 candidates of a pass in a plain loop c = 0 .. 63 under the
// same choice function (mpc_prefer).
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the controller can be checked on a machine without a GPU, the GPU tests have a
// float64 result to be bit-equal to, and the optimality bar of the checker is measured on its float32 build.
#include <vector>

#include "env_handle.hpp"
#include "mpc_eval.hpp"
#include "pime_mpc_host.h"

namespace pime {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {
struct MpcHostSearch {
    double* pass_costs;   // this step's [passes][N] column i, or nullptr
    int N, i;
    template <typename F>
    MpcBest argmin(const F& f) const {
        MpcBest b{f(0), 0};
        for (int c = 1; c < kMpcCandidates; ++c) {
            const double J = f(c);
            if (mpc_prefer(J, c, b.J, b.c)) b = MpcBest{J, c};
        }
        return b;
    }
    void chosen(int pass, double J) const {
        if (pass_costs) pass_costs[(size_t)pass * N + i] = J;
    }
};

struct MpcHostSink {
    MpcHostSearch* search;
    double *metrics, *actions, *outputs, *pass_costs;
    int N, i, passes;
    void step(int t, double u, double y) const {
        if (actions) actions[(size_t)t * N + i] = u;
        if (outputs) outputs[(size_t)t * N + i] = y;
        if (pass_costs) search->pass_costs = pass_costs + (size_t)(t + 1) * passes * N;   // the next step's block
    }
    void operator()(int seg, const SegMetrics& M) const { M.store(metrics, seg, N, i); }
};

template <typename S>
void mpc_host_run(const pime_env_cfg* cfg, const PhParams& ph, const WtParams& wt, const pime_sweep_lanes* lanes, int N, const double* model,
                  const SweepSchedule& s, const MpcConfig& m, double* metrics, double* actions, double* outputs, double* pass_costs) {
    const bool is_ph = cfg->kind == PIME_ENV_PH;
    std::vector<S> table;
    if (is_ph) {
        table.resize((size_t)cfg->ph_table_len);
        for (size_t k = 0; k < table.size(); ++k) table[k] = (S)cfg->ph_table[k];
    }
    for (int i = 0; i < N; ++i) {
        MpcHostSearch search{pass_costs, N, i};
        MpcHostSink sink{&search, metrics, actions, outputs, pass_costs, N, i, m.passes};
        if (is_ph) {
            PhLane<S> E{};
            E.x = lanes->ph_x[i]; E.A = lanes->ph_A[i]; E.B = lanes->ph_B[i]; E.C = lanes->ph_C[i];
            E.I = (S)lanes->I[i]; E.r = (S)lanes->r[i]; E.t = lanes->t[i]; E.episode = lanes->episode[i];
            E.last_a = ph.has_punish && lanes->ph_last_a ? (S)lanes->ph_last_a[i] : S(0);
            mpc_ph_plant<S>(ph, table.data(), E, s, m, search, sink);
        } else {
            WtLane<S> W{};
            W.h1 = (S)lanes->wt_h1[i]; W.h2 = (S)lanes->wt_h2[i]; W.r = (S)lanes->r[i]; W.I = (S)lanes->I[i];
            W.a1 = (S)lanes->wt_a1[i]; W.a2 = (S)lanes->wt_a2[i]; W.kp = (S)lanes->wt_kp[i];
            W.t = lanes->t[i]; W.episode = lanes->episode[i];
            const bool has_model = model != nullptr;
            const S m1 = has_model ? (S)model[(size_t)i * 3] : S(0), m2 = has_model ? (S)model[(size_t)i * 3 + 1] : S(0),
                    mk = has_model ? (S)model[(size_t)i * 3 + 2] : S(0);
            mpc_wt_plant<S>(wt, cfg->env_offset + (uint32_t)i, W, has_model, m1, m2, mk, s, m, search, sink);   // the plant's global lane
        }
    }
}
}  // namespace
}  // namespace pime

using namespace pime;

extern "C" {

const char* pime_mpc_host_last_error(void) { return g_err; }

int pime_mpc_eval_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* model_plants, int32_t horizon,
                       int32_t passes, double rho, int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints,
                       double band, int32_t tail, double* metrics, double* actions, double* outputs, double* pass_costs) {
    const char* fn = "pime_mpc_eval_host";
    if (int rc = check_cfg(cfg)) return rc;
    PIME_REQUIRE(lanes != nullptr && N >= 1, "%s: NULL lanes or N = %d", fn, N);
    const bool is_ph = cfg->kind == PIME_ENV_PH;
    PIME_REQUIRE(cfg->state_mode == PIME_STATE_F64 || cfg->state_mode == PIME_STATE_MIXED, "%s: not served for state_mode %d", fn,
                 cfg->state_mode);
    PIME_REQUIRE(is_ph || cfg->num_stack == 0, "%s: not served for the Stacking observation", fn);
    PIME_REQUIRE(lanes->r && lanes->I && lanes->t && lanes->episode, "%s: a lane array (r, I, t, episode) is NULL", fn);
    if (is_ph) PIME_REQUIRE(lanes->ph_x && lanes->ph_A && lanes->ph_B && lanes->ph_C, "%s: a pH lane array is NULL", fn);
    else PIME_REQUIRE(lanes->wt_h1 && lanes->wt_h2 && lanes->wt_a1 && lanes->wt_a2 && lanes->wt_kp, "%s: a tank lane array is NULL", fn);
    if (int rc = check_mpc_args(fn, is_ph, model_plants, horizon, passes, rho, n_steps, seg_len, setpoints, n_setpoints, band, tail, metrics))
        return rc;
    PhParams ph{};
    WtParams wt{};
    pime_env_cfg c = *cfg;
    c.n_envs = N;
    fill_params(c, is_ph ? 3 : 4, ph, wt);
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    const MpcConfig m{horizon, passes, rho};
    if (cfg->state_mode == PIME_STATE_F64) mpc_host_run<double>(cfg, ph, wt, lanes, N, model_plants, s, m, metrics, actions, outputs, pass_costs);
    else mpc_host_run<float>(cfg, ph, wt, lanes, N, model_plants, s, m, metrics, actions, outputs, pass_costs);
    return PIME_OK;
}

}  // extern "C"
