// libpime_freq_host.so (include/pime_freq_host.h): the pair function of pime_freq_sweep -- freq_sweep.hpp, the source the kernel runs
// -- compiled for the host under the prior controller alone (PriorOnlyPolicy), in float64 and float32 state, no handle; the opening
// checks, the lanes and the summary's order are host_grid.hpp's.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the excitation protocol can be checked on a machine without a GPU, and the GPU
// tests have a float64 result to be bit-equal to.
#include "host_grid.hpp"
#include "freq_sweep.hpp"
#include "pime_freq_host.h"

namespace pime {
namespace {
// a host pair keeps its sixteen rows -- vals [n_seg][kFreqAllRows][N], column i -- and, if asked, its signals
struct FreqHostSink : HostTraceSink {
    double* vals;
    int N, i;
    void operator()(int seg, const SegMetrics& M, const FreqMetrics& Q) const {
        double v[kFreqAllRows];
        freq_rows(M, Q, v);
        for (int row = 0; row < kFreqAllRows; ++row) vals[((size_t)seg * kFreqAllRows + row) * N + i] = v[row];
    }
};

template <typename S>
void freq_host_run(const pime_env_cfg* cfg, const HostGrid& g, const pime_sweep_lanes* lanes, int N, const double* priorK,
                   const double* excite, const double* wave, int wave_len, int P, const SweepSchedule& s, double* pairs, double* summary,
                   double* actions, double* outputs) {
    const std::vector<S> table = host_table<S>(cfg);
    const int n_seg = sweep_segments(s.n_steps, s.seg_len);
    std::vector<double> vals((size_t)n_seg * kFreqAllRows * N);
    for (int p = 0; p < P; ++p) {
        const FreqRow row = freq_row(excite + (size_t)p * PIME_FREQ_COLS);
        const double* w = wave + (size_t)p * wave_len * 2;
        for (int i = 0; i < N; ++i) {
            FreqHostSink sink{{actions, outputs, (size_t)P * N, (size_t)p * N + i}, vals.data(), N, i};
            if (g.is_ph) {
                const double K[3] = {priorK[0], priorK[1], priorK[2]};
                freq_ph_pair<S>(g.ph, table.data(), host_ph_lane<S>(g.ph, lanes, i), K, row, w, s, PriorOnlyPolicy{}, sink);
            } else {
                const double K[4] = {priorK[0], priorK[1], priorK[2], priorK[3]};
                const uint32_t gid = cfg->env_offset + (uint32_t)i;   // the PLANT's global lane keys the process noise
                freq_wt_pair<S>(g.wt, gid, host_wt_lane<S>(lanes, i), K, row, w, s, PriorOnlyPolicy{}, sink);
            }
        }
        host_reduce_rows(vals.data(), n_seg, kFreqAllRows, N, p, P, pairs, summary);
    }
}
}  // namespace
}  // namespace pime

using namespace pime;

extern "C" {

const char* pime_freq_host_last_error(void) { return g_err; }

int pime_freq_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* priorK, const double* excite,
                         const double* wave, int32_t wave_len, int32_t P, int32_t n_steps, int32_t seg_len, const double* setpoints,
                         int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary, double* actions,
                         double* outputs) {
    const char* fn = "pime_freq_sweep_host";
    HostGrid g{};
    if (int rc = host_grid_open(fn, cfg, lanes, N, true, g)) return rc;
    if (int rc = check_row_grid_args(fn, N, priorK, excite, "excite", P, n_steps, seg_len, setpoints, n_setpoints, band, tail, summary)) return rc;
    if (int rc = check_freq_wave(fn, wave, wave_len, n_steps, seg_len)) return rc;
    SweepSchedule s{};
    fill_sweep_schedule(s, n_steps, seg_len, setpoints, n_setpoints, band, tail);
    if (cfg->state_mode == PIME_STATE_F64)
        freq_host_run<double>(cfg, g, lanes, N, priorK, excite, wave, wave_len, P, s, pairs, summary, actions, outputs);
    else
        freq_host_run<float>(cfg, g, lanes, N, priorK, excite, wave, wave_len, P, s, pairs, summary, actions, outputs);
    return PIME_OK;
}

}  // extern "C"
