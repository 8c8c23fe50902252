// libpime_margin_host.so (include/pime_margin_host.h): the pair function of pime_margin_sweep -- margin_sweep.hpp, the source the
// kernel runs -- compiled for the host under the prior controller alone (PriorOnlyPolicy), in float64 and float32 state, no handle;
// the opening checks, the lanes and the summary's order are host_grid.hpp's.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the loop perturbations can be checked on a machine without a GPU, and the GPU
// tests have a float64 result to be bit-equal to.
#include "host_grid.hpp"
#include "margin_sweep.hpp"
#include "pime_margin_host.h"

namespace pime {
namespace {
// a host pair keeps its rows and, if asked, its signals
struct MarginHostSink : HostRowSink, HostTraceSink {};

template <typename S>
void margin_host_run(const pime_env_cfg* cfg, const HostGrid& g, const pime_sweep_lanes* lanes, int N, const double* priorK,
                     const double* perturb, int P, const MarginNoise& nz, const SweepSchedule& s, double* pairs, double* summary,
                     double* actions, double* outputs) {
    const std::vector<S> table = host_table<S>(cfg);
    const int n_seg = sweep_segments(s.n_steps, s.seg_len);
    std::vector<double> vals((size_t)n_seg * PIME_METRIC_ROWS * N);
    for (int p = 0; p < P; ++p) {
        const MarginRow row = margin_row(perturb + (size_t)p * PIME_PERTURB_COLS);
        for (int i = 0; i < N; ++i) {
            MarginHostSink sink{{vals.data(), N, i}, {actions, outputs, (size_t)P * N, (size_t)p * N + i}};
            const uint32_t gid = cfg->env_offset + (uint32_t)i;   // the PLANT's global lane keys both noises
            if (g.is_ph) {
                const double K[3] = {priorK[0], priorK[1], priorK[2]};
                margin_ph_pair<S>(g.ph, table.data(), gid, host_ph_lane<S>(g.ph, lanes, i), K, row, nz, s, PriorOnlyPolicy{}, sink);
            } else {
                const double K[4] = {priorK[0], priorK[1], priorK[2], priorK[3]};
                margin_wt_pair<S>(g.wt, gid, host_wt_lane<S>(lanes, i), K, row, nz, s, PriorOnlyPolicy{}, sink);
            }
        }
        host_reduce_rows(vals.data(), n_seg, PIME_METRIC_ROWS, N, p, P, pairs, summary);
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
    HostGrid g{};
    if (int rc = host_grid_open(fn, cfg, lanes, N, true, g)) return rc;
    if (int rc = check_row_grid_args(fn, N, priorK, perturb, "perturb", P, n_steps, seg_len, setpoints, n_setpoints, band, tail, summary)) return rc;
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    const MarginNoise nz{noise_seed, noise_epoch};
    if (cfg->state_mode == PIME_STATE_F64) margin_host_run<double>(cfg, g, lanes, N, priorK, perturb, P, nz, s, pairs, summary, actions, outputs);
    else margin_host_run<float>(cfg, g, lanes, N, priorK, perturb, P, nz, s, pairs, summary, actions, outputs);
    return PIME_OK;
}

}  // extern "C"
