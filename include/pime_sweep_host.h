/*
 * pime_sweep_host.h -- C ABI of libpime_sweep_host.so: the pair function of pime_prior_sweep (csrc/prior_sweep.hpp, the very source
 * the kernel runs) compiled for the host, float64 state, with the summary's order written as a plain loop.
 *
 * TEST INFRASTRUCTURE, like libpime_cpu.so and libpime_replay_host.so: libpime_hip.so has no CPU path and the pime_amd package never
 * loads this library.  It lets the arithmetic of the sweep -- the pair loop, the common random numbers, the order of the sums -- be
 * checked on a machine without a GPU, and gives the GPU tests a float64 result to be bit-equal to.
 */
#ifndef PIME_SWEEP_HOST_H
#define PIME_SWEEP_HOST_H

#include "pime_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* The lane state a handle would hold, as HOST arrays of N words each (what pime_env_read_field returns per field). */
typedef struct pime_sweep_lanes {
    const double *ph_x, *ph_A, *ph_B, *ph_C;     /* pH */
    const double *ph_last_a;                     /* pH, or NULL: zeros (read only when a punish term is configured) */
    const double *wt_h1, *wt_h2, *wt_a1, *wt_a2, *wt_kp; /* water tank */
    const double *r, *I;                         /* both */
    const int32_t *t, *episode;                  /* both */
} pime_sweep_lanes;

/* pime_prior_sweep without a handle.  Every pointer is a HOST pointer; there is no workspace.
 *   cfg      the env configuration (kind, the plant constants, seed, env_offset, pH: the titration table); state_mode is ignored: the
 *            state is float64 (PIME_STATE_F64 semantics); num_stack must be 0
 *   lanes, N the lane state the pairs start from
 *   gains .. summary: as pime_prior_sweep
 * Returns PIME_OK or PIME_ERR_ARG (the cases of pime_prior_sweep, and NULL cfg / lanes / a lane array, N < 1) with a message in
 * pime_sweep_host_last_error(). */
int pime_prior_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* gains, int32_t G,
                          int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints, double band, int32_t tail,
                          double* pairs, double* summary);
const char* pime_sweep_host_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
