// libpime_replay_host.so (include/pime_replay_host.h): the lane function of pime_env_replay_error -- replay_error.hpp, the source the
// kernel runs -- compiled for the host, float64 state, no handle.
//
// NOT part of the product path: libpime_hip.so has no CPU fallback and the pime_amd package never loads this library.  Like the CPU
// twins (cpu_twins.hip) it is test infrastructure: the arithmetic of the replay can be checked on a machine without a GPU, and the
// GPU tests have a float64 result to be bit-equal to.
#include <thread>
#include <vector>

#include "host_grid.hpp"
#include "pime_replay_host.h"
#include "replay_error.hpp"

using namespace pime;

extern "C" {

const char* pime_replay_host_last_error(void) { return g_err; }

int pime_replay_error_host(const pime_env_cfg* cfg, const double* plants, int32_t N, const pime_replay_records* rec, int32_t mode,
                           int32_t skip, double* err, double* sim, int32_t threads) {
    const char* fn = "pime_replay_error_host";
    if (int rc = check_cfg(cfg)) return rc;
    PIME_REQUIRE(plants != nullptr && N >= 1, "%s: NULL plants or N = %d", fn, N);
    const bool is_ph = cfg->kind == PIME_ENV_PH;
    if (int rc = check_replay_args(fn, is_ph, rec, mode, skip, err)) return rc;
    PhParams ph{};
    WtParams wt{};
    pime_env_cfg c = *cfg;
    c.n_envs = N;
    fill_params(c, is_ph ? 3 : 4, ph, wt);
    wt.num_stack = 0;   // the plant is the same under either observation
    ReplayRecords r{rec->action, rec->output, rec->state0, rec->E, rec->T};
    auto body = [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i) {
            double A = 0, B = 0, C = 0;
            if (is_ph) {   // the zero-order hold of a resampling reset (ph_lane_reset), from injected draws
                PhLane<double> L{};
                L.episode = -1;
                PhParams q = ph;
                q.resample_every = 1;
                const double draws[4] = {plants[2 * (size_t)i], plants[2 * (size_t)i + 1], 0.0, 0.0};
                float o[3];
                ph_lane_reset<double>(q, cfg->ph_table, 0u, draws, L, o);
                A = L.A; B = L.B; C = L.C;
            }
            for (int e = 0; e < r.E; ++e) {
                ReplayErr acc;
                if (is_ph)
                    replay_ph_lane<double>(ph, cfg->ph_table, A, B, C, r, e, skip, acc, sim ? sim + i : nullptr, N);
                else if (mode == PIME_REPLAY_PREDICT)
                    replay_wt_lane<double, PIME_REPLAY_PREDICT>(wt, plants[3 * (size_t)i], plants[3 * (size_t)i + 1],
                                                                plants[3 * (size_t)i + 2], r, e, skip, acc, sim ? sim + i : nullptr, N);
                else
                    replay_wt_lane<double, PIME_REPLAY_SIMULATE>(wt, plants[3 * (size_t)i], plants[3 * (size_t)i + 1],
                                                                 plants[3 * (size_t)i + 2], r, e, skip, acc, sim ? sim + i : nullptr, N);
                acc.store(err, e, N, i);
            }
        }
    };
    int nt = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
    if (nt > N) nt = N;
    if (nt <= 1) { body(0, N); return PIME_OK; }
    const int per = (N + nt - 1) / nt;   // contiguous chunks of lanes; lanes are independent, so the result does not depend on nt
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) {
        const int lo = t * per, hi = lo + per < N ? lo + per : N;
        if (lo < hi) pool.emplace_back(body, lo, hi);
    }
    for (auto& th : pool) th.join();
    return PIME_OK;
}

}  // extern "C"
