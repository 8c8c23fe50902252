/*
 * pime_mpc_host.h -- C ABI of libpime_mpc_host.so: the closed loop of pime_mpc_eval (csrc/mpc_eval.hpp, the very source the kernel
 * runs) compiled for the host, in float64 and in float32 state, the 64 candidates of a pass in a plain loop c = 0 .. 63 and the same
 * choice function.
 *
 * TEST INFRASTRUCTURE, like libpime_cpu.so, libpime_replay_host.so and libpime_sweep_host.so: libpime_hip.so has no CPU path and the
 * pime_amd package never loads this library.  It lets the controller -- candidates, cost, choice, the true plant's loop -- be checked
 * on a machine without a GPU, gives the GPU tests a float64 result to be bit-equal to, and is the source of the optimality bar of
 * tests/mpc_eval.py (profiles/mpc_eval_bars.txt).
 */
#ifndef PIME_MPC_HOST_H
#define PIME_MPC_HOST_H

#include "pime_sweep_host.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* pime_mpc_eval without a handle.  Every pointer is a HOST pointer.
 *   cfg        the env configuration (kind, the plant constants, seed, env_offset, pH: the titration table, float64); num_stack must
 *              be 0.  cfg->state_mode selects the state's precision: PIME_STATE_F64 float64, PIME_STATE_MIXED float32 (the lane words
 *              and the table are rounded to float32 as a MIXED handle holds them; the float32 roots and Box-Muller functions are
 *              libm's, an ulp or so from the device's hardware ones); anything else is refused
 *   lanes, N   the lane state the plants start from (pime_sweep_lanes of pime_sweep_host.h)
 *   model_plants .. outputs: as pime_mpc_eval
 *   pass_costs float64[n_steps, passes, N] or NULL: the cost of the winner of every pass of every step (host only)
 * Returns PIME_OK or PIME_ERR_ARG (the cases of pime_mpc_eval, and NULL cfg / lanes / a lane array, N < 1) with a message in
 * pime_mpc_host_last_error(). */
int pime_mpc_eval_host(const pime_env_cfg* cfg, const pime_sweep_lanes* lanes, int32_t N, const double* model_plants, int32_t horizon,
                       int32_t passes, double rho, int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints,
                       double band, int32_t tail, double* metrics, double* actions, double* outputs, double* pass_costs);
const char* pime_mpc_host_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
