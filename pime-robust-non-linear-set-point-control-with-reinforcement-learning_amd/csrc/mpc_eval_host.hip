// libpime_mpc_host.so (include/pime_mpc_host.h): the closed loop of pime_mpc_eval -- mpc_eval.hpp, the source the kernel runs --
// compiled for the host in float64 and float32 state, no handle; the 64 candidates of a pass in a plain loop c = 0 .. 63 under the
// same choice function (mpc_prefer).
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the controller can be checked on a machine without a GPU, the GPU tests have a
// float64 result to be bit-equal to, and the optimality bar of the checker is measured on its float32 build.
#include "host_grid.hpp"
#include "mpc_eval.hpp"
#include "pime_mpc_host.h"

namespace pime {
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
void mpc_host_run(const pime_env_cfg* cfg, const HostGrid& g, const pime_sweep_lanes* lanes, int N, const double* model,
                  const SweepSchedule& s, const MpcConfig& m, double* metrics, double* actions, double* outputs, double* pass_costs) {
    const std::vector<S> table = host_table<S>(cfg);
    for (int i = 0; i < N; ++i) {
        MpcHostSearch search{pass_costs, N, i};
        MpcHostSink sink{&search, metrics, actions, outputs, pass_costs, N, i, m.passes};
        if (g.is_ph) {
            mpc_ph_plant<S>(g.ph, table.data(), host_ph_lane<S>(g.ph, lanes, i), s, m, search, sink);
        } else {
            const bool has_model = model != nullptr;
            const S m1 = has_model ? (S)model[(size_t)i * 3] : S(0), m2 = has_model ? (S)model[(size_t)i * 3 + 1] : S(0),
                    mk = has_model ? (S)model[(size_t)i * 3 + 2] : S(0);
            mpc_wt_plant<S>(g.wt, cfg->env_offset + (uint32_t)i, host_wt_lane<S>(lanes, i), has_model, m1, m2, mk, s, m, search,
                            sink);   // the plant's global lane
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
    HostGrid g{};
    if (int rc = host_grid_open(fn, cfg, lanes, N, true, g)) return rc;
    if (int rc = check_mpc_args(fn, g.is_ph, model_plants, horizon, passes, rho, n_steps, seg_len, setpoints, n_setpoints, band, tail, metrics))
        return rc;
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    const MpcConfig m{horizon, passes, rho};
    if (cfg->state_mode == PIME_STATE_F64) mpc_host_run<double>(cfg, g, lanes, N, model_plants, s, m, metrics, actions, outputs, pass_costs);
    else mpc_host_run<float>(cfg, g, lanes, N, model_plants, s, m, metrics, actions, outputs, pass_costs);
    return PIME_OK;
}

}  // extern "C"
