// libpime_sweep_host.so (include/pime_sweep_host.h): the pair function of pime_prior_sweep -- prior_sweep.hpp, the source the kernel
// runs -- compiled for the host, float64 state, no handle; the opening checks, the lanes and the summary's order are host_grid.hpp's.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the arithmetic of the sweep can be checked on a machine without a GPU, and the
// GPU tests have a float64 result to be bit-equal to.
#include "host_grid.hpp"

using namespace pime;

extern "C" {

const char* pime_sweep_host_last_error(void) { return g_err; }

int pime_prior_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* gains, int32_t G,
                          int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints, double band, int32_t tail,
                          double* pairs, double* summary) {
    const char* fn = "pime_prior_sweep_host";
    HostGrid g{};
    if (int rc = host_grid_open(fn, cfg, lanes, N, false, g)) return rc;   // (no state-mode check: always float64 lanes)
    if (int rc = check_sweep_args(fn, N, gains, G, n_steps, seg_len, setpoints, n_setpoints, band, tail, summary)) return rc;
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    const int n_seg = sweep_segments(n_steps, seg_len);
    std::vector<double> vals((size_t)n_seg * PIME_METRIC_ROWS * N);
    for (int r = 0; r < G; ++r) {
        for (int i = 0; i < N; ++i) {
            HostRowSink sink{vals.data(), N, i};
            if (g.is_ph) {
                const double K[3] = {gains[3 * (size_t)r], gains[3 * (size_t)r + 1], gains[3 * (size_t)r + 2]};
                sweep_ph_pair<double>(g.ph, cfg->ph_table, host_ph_lane<double>(g.ph, lanes, i), K, s, sink);
            } else {
                const double K[4] = {gains[4 * (size_t)r], gains[4 * (size_t)r + 1], gains[4 * (size_t)r + 2], gains[4 * (size_t)r + 3]};
                sweep_wt_pair<double>(g.wt, cfg->env_offset + (uint32_t)i, host_wt_lane<double>(lanes, i), K, s, sink);   // the PLANT's global lane keys the noise
            }
        }
        host_reduce_rows(vals.data(), n_seg, PIME_METRIC_ROWS, N, r, G, pairs, summary);
    }
    return PIME_OK;
}

}  // extern "C"
