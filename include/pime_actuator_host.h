/*
 * pime_actuator_host.h -- C ABI of libpime_actuator_host.so: the pair function of pime_actuator_sweep (csrc/actuator_sweep.hpp, the
 * very source the kernel runs) compiled for the host under the prior controller alone, in float64 and in float32 state, with the
 * summary's order written as a plain loop.
 *
 * TEST INFRASTRUCTURE, like libpime_cpu.so, libpime_replay_host.so, libpime_sweep_host.so, libpime_mpc_host.so,
 * libpime_margin_host.so, libpime_disturb_host.so and libpime_freq_host.so: libpime_hip.so has no CPU path and the pime_amd package
 * never loads this library.  It lets the actuator chain -- the decode of a row, the sensor quantum, the order of the four stages, the
 * actuator rows, the order of the sums -- be checked on a machine without a GPU, and gives the GPU tests a float64 result to be
 * bit-equal to.
 */
#ifndef PIME_ACTUATOR_HOST_H
#define PIME_ACTUATOR_HOST_H

#include "pime_sweep_host.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* pime_actuator_sweep(kind = -1) without a handle.  Every pointer is a HOST pointer; there is no workspace.
 *   cfg        the env configuration (kind, the plant constants, seed, env_offset, pH: the titration table, float64); num_stack must
 *              be 0.  cfg->state_mode selects the state's precision: PIME_STATE_F64 float64, PIME_STATE_MIXED float32 (the lane words
 *              and the table are rounded to float32 as a MIXED handle holds them; the float32 roots and Box-Muller functions are
 *              libm's, an ulp or so from the device's hardware ones); anything else is refused
 *   lanes, N   the lane state the pairs start from (pime_sweep_lanes of pime_sweep_host.h)
 *   priorK .. outputs: as pime_actuator_sweep
 * Returns PIME_OK or PIME_ERR_ARG (the cases of pime_actuator_sweep, and NULL cfg / lanes / a lane array, N < 1) with a message in
 * pime_actuator_host_last_error(). */
int pime_actuator_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* priorK,
                             const double* actuator, int32_t P, int32_t n_steps, int32_t seg_len, const double* setpoints,
                             int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary, double* actions,
                             double* commands, double* outputs);
const char* pime_actuator_host_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
