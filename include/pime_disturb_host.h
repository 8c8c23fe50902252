/*
 * pime_disturb_host.h -- C ABI of libpime_disturb_host.so: the pair function of pime_disturb_sweep (csrc/disturb_sweep.hpp, the very
 * source the kernel runs) compiled for the host under the prior controller alone, in float64 and in float32 state, with the summary's
 * order written as a plain loop.
 *
 * TEST INFRASTRUCTURE, like libpime_cpu.so, libpime_replay_host.so, libpime_sweep_host.so, libpime_mpc_host.so and
 * libpime_margin_host.so: libpime_hip.so has no CPU path and the pime_amd package never loads this library.  It lets the disturbance
 * protocol -- the onset and the length of a row, the load in front of the actuator, the plant switch, the rejection rows, the order
 * of the sums -- be checked on a machine without a GPU, and gives the GPU tests a float64 result to be bit-equal to.
 */
#ifndef PIME_DISTURB_HOST_H
#define PIME_DISTURB_HOST_H

#include "pime_sweep_host.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* pime_disturb_sweep(kind = -1) without a handle.  Every pointer is a HOST pointer; there is no workspace.
 *   cfg        the env configuration (kind, the plant constants, seed, env_offset, pH: the titration table, float64); num_stack must
 *              be 0.  cfg->state_mode selects the state's precision: PIME_STATE_F64 float64, PIME_STATE_MIXED float32 (the lane words
 *              and the table are rounded to float32 as a MIXED handle holds them; the float32 roots and Box-Muller functions are
 *              libm's, an ulp or so from the device's hardware ones); anything else is refused
 *   lanes, N   the lane state the pairs start from (pime_sweep_lanes of pime_sweep_host.h)
 *   ph_qww, ph_qc   pH: float64[N], the lanes' stored qww_V and qc_V, from which a disturbed plant is rebuilt (pime_sweep_lanes does
 *              not hold them); NULL for the tank
 *   priorK .. outputs: as pime_disturb_sweep
 * Returns PIME_OK or PIME_ERR_ARG (the cases of pime_disturb_sweep, and NULL cfg / lanes / a lane array / ph_qww or ph_qc on pH,
 * N < 1) with a message in pime_disturb_host_last_error(). */
int pime_disturb_sweep_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* ph_qww, const double* ph_qc,
                            const double* priorK, const double* disturb, int32_t P, int32_t n_steps, int32_t seg_len,
                            const double* setpoints, int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary,
                            double* actions, double* outputs);
const char* pime_disturb_host_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
