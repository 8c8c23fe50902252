// libpime_actuator_host.so (include/pime_actuator_host.h): the pair function of pime_actuator_sweep -- actuator_sweep.hpp, the source
// the kernel runs -- compiled for the host under the prior controller alone (PriorOnlyPolicy), in float64 and float32 state, no
// handle; the opening checks, the lanes and the summary's order are host_grid.hpp's.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the actuator chain can be checked on a machine without a GPU, and the GPU tests
// have a float64 result to be bit-equal to.
#include "host_grid.hpp"
#include "actuator_sweep.hpp"
#include "pime_actuator_host.h"

namespace pime {
namespace {
// a host pair keeps its sixteen rows -- vals [n_seg][kActAllRows][N], column i -- and, if asked, its three signals
struct ActHostSink : HostTraceSink {
    double* commands;
    double* vals;
    int N, i;
    void command(int t, double a_c) const {
        if (commands) commands[(size_t)t * PN + col] = a_c;
    }
    void operator()(int seg, const SegMetrics& M, const ActMetrics& Q) const {
        double v[kActAllRows];
        act_rows(M, Q, v);
        for (int row = 0; row < kActAllRows; ++row) vals[((size_t)seg * kActAllRows + row) * N + i] = v[row];
    }
};

template <typename S>
void act_host_run(const pime_env_cfg* cfg, const HostGrid& g, const pime_sweep_lanes* lanes, int N, const double* priorK,
                  const double* actuator, int P, const SweepSchedule& s, double* pairs, double* summary, double* actions, double* commands,
                  double* outputs) {
    const std::vector<S> table = host_table<S>(cfg);
    const int n_seg = sweep_segments(s.n_steps, s.seg_len);
    std::vector<double> vals((size_t)n_seg * kActAllRows * N);
    for (int p = 0; p < P; ++p) {
        const ActRow row = act_row(actuator + (size_t)p * PIME_ACT_COLS);
        for (int i = 0; i < N; ++i) {
            ActHostSink sink{{actions, outputs, (size_t)P * N, (size_t)p * N + i}, commands, vals.data(), N, i};
            if (g.is_ph) {
                const double K[3] = {priorK[0], priorK[1], priorK[2]};
                act_ph_pair<S>(g.ph, table.data(), host_ph_lane<S>(g.ph, lanes, i), K, row, s, PriorOnlyPolicy{}, sink);
            } else {
                const double K[4] = {priorK[0], priorK[1], priorK[2], priorK[3]};
                const uint32_t gid = cfg->env_offset + (uint32_t)i;   // the PLANT's global lane keys the process noise
                act_wt_pair<S>(g.wt, gid, host_wt_lane<S>(lanes, i), K, row, s, PriorOnlyPolicy{}, sink);
            }
        }
        host_reduce_rows(vals.data(), n_seg, kActAllRows, N, p, P, pairs, summary);
    }
}
}  // namespace
}  // namespace pime

using namespace pime;

extern "C" {

const char* pime_actuator_host_last_error(void) { return g_err; }

int pime_actuator_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* priorK,
                             const double* actuator, int32_t P, int32_t n_steps, int32_t seg_len, const double* setpoints,
                             int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary, double* actions,
                             double* commands, double* outputs) {
    const char* fn = "pime_actuator_sweep_host";
    HostGrid g{};
    if (int rc = host_grid_open(fn, cfg, lanes, N, true, g)) return rc;
    if (int rc = check_row_grid_args(fn, N, priorK, actuator, "actuator", P, n_steps, seg_len, setpoints, n_setpoints, band, tail, summary)) return rc;
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    if (cfg->state_mode == PIME_STATE_F64)
        act_host_run<double>(cfg, g, lanes, N, priorK, actuator, P, s, pairs, summary, actions, commands, outputs);
    else
        act_host_run<float>(cfg, g, lanes, N, priorK, actuator, P, s, pairs, summary, actions, commands, outputs);
    return PIME_OK;
}

}  // extern "C"
