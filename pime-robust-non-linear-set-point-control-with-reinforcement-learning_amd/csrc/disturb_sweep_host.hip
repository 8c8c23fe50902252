// libpime_disturb_host.so (include/pime_disturb_host.h): the pair function of pime_disturb_sweep -- disturb_sweep.hpp, the source the
// kernel runs -- compiled for the host under the prior controller alone (PriorOnlyPolicy), in float64 and float32 state, no handle;
// the opening checks, the lanes and the summary's order are host_grid.hpp's.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the disturbance protocol can be checked on a machine without a GPU, and the GPU
// tests have a float64 result to be bit-equal to.
#include "host_grid.hpp"
#include "disturb_sweep.hpp"
#include "pime_disturb_host.h"

namespace pime {
namespace {
// a host pair keeps its fifteen rows -- vals [n_seg][kDisturbAllRows][N], column i -- and, if asked, its signals
struct DisturbHostSink : HostTraceSink {
    double* vals;
    int N, i;
    void operator()(int seg, const SegMetrics& M, const DistMetrics& Q) const {
        double v[kDisturbAllRows];
        disturb_rows(M, Q, v);
        for (int row = 0; row < kDisturbAllRows; ++row) vals[((size_t)seg * kDisturbAllRows + row) * N + i] = v[row];
    }
};

template <typename S>
void disturb_host_run(const pime_env_cfg* cfg, const HostGrid& g, const pime_sweep_lanes* lanes, int N, const double* ph_qww,
                      const double* ph_qc, const double* priorK, const double* disturb, int P, const SweepSchedule& s, double* pairs,
                      double* summary, double* actions, double* outputs) {
    const std::vector<S> table = host_table<S>(cfg);
    const int n_seg = sweep_segments(s.n_steps, s.seg_len);
    std::vector<double> vals((size_t)n_seg * kDisturbAllRows * N);
    for (int p = 0; p < P; ++p) {
        const DisturbRow row = disturb_row(disturb + (size_t)p * PIME_DISTURB_COLS);
        for (int i = 0; i < N; ++i) {
            DisturbHostSink sink{{actions, outputs, (size_t)P * N, (size_t)p * N + i}, vals.data(), N, i};
            if (g.is_ph) {
                const double K[3] = {priorK[0], priorK[1], priorK[2]};
                PhLane<S> E = host_ph_lane<S>(g.ph, lanes, i);
                E.qww = ph_qww[i]; E.qc = ph_qc[i];
                disturb_ph_pair<S>(g.ph, table.data(), E, K, row, s, PriorOnlyPolicy{}, sink);
            } else {
                const double K[4] = {priorK[0], priorK[1], priorK[2], priorK[3]};
                const uint32_t gid = cfg->env_offset + (uint32_t)i;   // the PLANT's global lane keys the process noise
                disturb_wt_pair<S>(g.wt, gid, host_wt_lane<S>(lanes, i), K, row, s, PriorOnlyPolicy{}, sink);
            }
        }
        host_reduce_rows(vals.data(), n_seg, kDisturbAllRows, N, p, P, pairs, summary);
    }
}
}  // namespace
}  // namespace pime

using namespace pime;

extern "C" {

const char* pime_disturb_host_last_error(void) { return g_err; }

int pime_disturb_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* ph_qww, const double* ph_qc,
                            const double* priorK, const double* disturb, int32_t P, int32_t n_steps, int32_t seg_len,
                            const double* setpoints, int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary,
                            double* actions, double* outputs) {
    const char* fn = "pime_disturb_sweep_host";
    HostGrid g{};
    if (int rc = host_grid_open(fn, cfg, lanes, N, true, g)) return rc;
    if (g.is_ph) PIME_REQUIRE(ph_qww != nullptr && ph_qc != nullptr, "%s: ph_qww or ph_qc is NULL", fn);
    if (int rc = check_row_grid_args(fn, N, priorK, disturb, "disturb", P, n_steps, seg_len, setpoints, n_setpoints, band, tail, summary)) return rc;
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    if (cfg->state_mode == PIME_STATE_F64)
        disturb_host_run<double>(cfg, g, lanes, N, ph_qww, ph_qc, priorK, disturb, P, s, pairs, summary, actions, outputs);
    else
        disturb_host_run<float>(cfg, g, lanes, N, ph_qww, ph_qc, priorK, disturb, P, s, pairs, summary, actions, outputs);
    return PIME_OK;
}

}  // extern "C"
