/*
 * pime_replay_host.h -- C ABI of libpime_replay_host.so: the lane function of pime_env_replay_error (csrc/replay_error.hpp, the
 * very source the kernel runs) compiled for the host, float64 state.
 *
 * TEST INFRASTRUCTURE, like libpime_cpu.so: libpime_hip.so has no CPU path and the pime_amd package never loads this library.
 * It lets the arithmetic of the replay -- the step, the gaps, the order of the sums -- be checked on a machine without a GPU, and
 * gives the GPU tests a float64 result to be bit-equal to.
 */
#ifndef PIME_REPLAY_HOST_H
#define PIME_REPLAY_HOST_H

#include "pime_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* pime_env_replay_error without a handle.  Every pointer is a HOST pointer, rec's included.
 *   cfg      the env configuration (kind, the plant constants, pH: the titration table); state_mode is ignored: the state is
 *            float64 (PIME_STATE_F64 semantics)
 *   plants   float64[N, P]: pH P = 2 (qww_V, qc_V), through the zero-order hold of a resampling reset (ph.py:114-121);
 *            water tank P = 3 (a1, a2, Kp)
 *   mode, skip, err [E][PIME_REPLAY_ROWS][N], sim [E][T][C][N] or NULL: as pime_env_replay_error
 *   threads  host threads over the lanes (results do not depend on it)
 * Returns PIME_OK or PIME_ERR_ARG (the cases of pime_env_replay_error, and NULL cfg / plants, N < 1) with a message in
 * pime_replay_host_last_error(). */
int pime_replay_error_host(const pime_env_cfg* cfg, const double* plants, int32_t N, const pime_replay_records* rec, int32_t mode,
                           int32_t skip, double* err, double* sim, int32_t threads);
const char* pime_replay_host_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
