/*
 * pime_hip.h -- C ABI of libpime_hip.so, the MI355X (gfx950) implementation of the vectorised
 * set-point-control hot path.
 *
 * The reference (ruoqizzz/PIME-..., 100 % Python) has no FFI: its boundary for this path is the Python duck
 * type consumed by elegantrl/env.py:PreprocessEnv and the agents.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference root); INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add to bind them.
 *
 * Conventions
 *  - plain C types only; every buffer is caller-owned.  Pointers marked [dev] are device pointers on the
 *    handle's device (e.g. torch tensor .data_ptr()), [host] are host pointers.
 *  - every launch goes to the caller-supplied HIP stream (pime_stream = hipStream_t; pass torch's current
 *    stream) and returns without synchronising, so calls are hipGraph-capturable.  Functions documented as
 *    "synchronous" (field I/O, create/destroy) synchronise that stream themselves.
 *  - return value: 0 = PIME_OK, negative = error class; pime_last_error() returns a thread-local message.
 *    No C++ exception crosses the ABI.
 *  - a handle is single-writer: one host thread, one stream at a time.  Different handles are independent.
 *  - there is NO CPU fallback: without a usable gfx950 device pime_env_create() fails with PIME_ERR_DEVICE.
 */
#ifndef PIME_HIP_H
#define PIME_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define PIME_ABI_VERSION 26 /* (still 26 with the prior-gain sweep: pime_prior_sweep* ADD symbols, nothing that was there changes) */

typedef struct pime_env pime_env; /* opaque: SoA env state + titration LUT replica, resident in HBM */
typedef void* pime_stream;        /* hipStream_t */

enum pime_status {
    PIME_OK = 0,
    PIME_ERR_ARG = -1,    /* bad argument / shape / enum */
    PIME_ERR_DEVICE = -2, /* no usable gfx950 device, or HIP runtime error */
    PIME_ERR_ALLOC = -3,
    PIME_ERR_STATE = -4   /* call sequence error (e.g. step before reset) */
};

enum pime_kind { PIME_ENV_PH = 0, PIME_ENV_WT = 1 };
/* PIME_STATE_F64: every state word float64 (reference precision).  PIME_STATE_MIXED: float32 state; the pH
 * reaction-invariant x and the discretised plant (A,B,C) stay float64 so the LUT index is the reference's.
 * PIME_STATE_MIXED16 (BASELINE.json config 5 "fp16 state" = SURVEY.md §8(d) cfg 5): as MIXED with the integrated error I STORED
 * as IEEE binary16 and, through the *_h entry points, observations and rewards written as binary16 (48 instead of 68 bytes of
 * algorithmic traffic per pH env-step); all arithmetic stays float32 / float64.  What it costs in accuracy is stated with
 * pime_env_step_h.  Through the float entry points such a handle writes float32 rows whose I is the stored binary16 word, the value the
 * next step continues from and pime_env_observe returns. */
enum pime_state_mode { PIME_STATE_F64 = 0, PIME_STATE_MIXED = 1, PIME_STATE_MIXED16 = 2 };
enum pime_reward { PIME_REWARD_DISTANCE = 0, PIME_REWARD_SQUARE = 1, PIME_REWARD_SPARSE = 2 };
enum pime_dtype { PIME_F32 = 0, PIME_F64 = 1 };

/* state fields for pime_env_read_field / pime_env_write_field */
enum pime_field {
    /* pH  (gym_control/envs/ph.py attributes: state, integrator, r, y, dsys.A/B/C, qww_V, qc_V, _episode_steps) */
    PIME_PH_X = 0, PIME_PH_I = 1, PIME_PH_R = 2, PIME_PH_Y = 3, PIME_PH_A = 4, PIME_PH_B = 5, PIME_PH_C = 6,
    PIME_PH_QWW_V = 7, PIME_PH_QC_V = 8, PIME_PH_T = 9, PIME_PH_EPISODE = 10,
    /* water tank (nonlinear_watertank.py attributes: h1, h2, r, integrator, a1, a2, Kp, _episode_steps) */
    PIME_WT_H1 = 32, PIME_WT_H2 = 33, PIME_WT_R = 34, PIME_WT_I = 35, PIME_WT_A1 = 36, PIME_WT_A2 = 37,
    PIME_WT_KP = 38, PIME_WT_T = 39, PIME_WT_EPISODE = 40,
    /* Stacking variant only, read-only: the ring slot of a lane's OLDEST frame (0 after every reset, then one further per step,
     * modulo num_stack) */
    PIME_WT_HEAD = 41
};

/* Titration chemistry, gym_control/envs/ph.py:32-37 */
typedef struct pime_ph_chem {
    double kw, kchem, ka, MNaOH, MHA, MNH3;
} pime_ph_chem;

typedef struct pime_env_cfg {
    int32_t kind;            /* pime_kind */
    int32_t n_envs;          /* instances advanced per launch (this rank's slice) */
    int32_t device_id;       /* HIP device ordinal */
    int32_t state_mode;      /* pime_state_mode */
    int32_t max_steps;       /* pH: gym TimeLimit (gym_control/__init__.py:6) ; WT: max_step (:55) */
    int32_t reward_type;     /* pime_reward */
    int32_t integral_bound;  /* 1: clip I to +-integral_max (ph.py:341, nonlinear_watertank.py:825); 0: _NoBound (ph.py:470) */
    int32_t num_stack;       /* WT only. 0: Integrator obs [h1,h2,r,I]; S>=1: Stacking obs, 3*S floats (:1056-1208) */
    int32_t resample_every;  /* n: redraw the ensemble params on every n-th reset; 0 = never (if_reset_all False) */
    uint32_t env_offset;     /* global id of lane 0 (rank * n_envs under data-parallel sharding); Philox counter word */
    uint64_t seed;           /* Philox key */
    double integral_max, integral_punish, action_punish, action_change_punish, distance_threshold;
    double range_lo[3], range_hi[3]; /* ensemble ranges: pH (qww_V, qc_V, -) ; WT (a1, a2, Kp) */
    double init_lo[2], init_hi[2];   /* [0]: initial state range (pH x0 / WT h1,h2) ; [1]: goal r range */
    /* pH plant */
    double ph_sample_t, ph_u_low, ph_u_high, ph_table_scale; /* T=20 s; action map [0,1.5]; 1e5 = 1/MHCl step */
    const double* ph_table;  /* [host] ph_table_len float64 entries (pime_ph_table_build); copied at create */
    int32_t ph_table_len;
    /* water-tank plant */
    int32_t wt_n_discrete;
    double wt_A1, wt_A2, wt_G, wt_dt, wt_noise_scale, wt_z1, wt_pmax;
} pime_env_cfg;

/* -- library --------------------------------------------------------------------------------------------- */
int pime_abi_version(void);
const char* pime_last_error(void);
/* number of visible gfx950 devices (0 on a CPU-only host); never throws */
int pime_device_count(void);

/* -- titration LUT ----------------------------------------------------------------------------------------
 * replaces: PH1D.__init__ table loop, gym_control/envs/ph.py:72-84 (13 s of Python per gym.make).
 * Sequential warm-started Newton => host code, fp64, ~10 ms.  out: [host] n entries, entry i for
 * MHCl = i * mhcl_step.  chem == NULL selects ph.py:32-37. */
int pime_ph_table_build(const pime_ph_chem* chem, double mhcl_step, int32_t n, double* out);

/* -- env handle -------------------------------------------------------------------------------------------
 * pime_env_cfg_default fills the registered configuration of
 *   kind PH: 'PH1DChangingParamUniformGoalIntegrator-SqaureDistance-v35' (gym_control/__init__.py:3-14)
 *   kind WT: 'NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2' (:50-69)
 * (ph_table left NULL: the caller supplies it). */
int pime_env_cfg_default(int32_t kind, pime_env_cfg* cfg);
/* replaces: gym.make(id) -> env constructor (ph.py:353-407, nonlinear_watertank.py:830-888). synchronous. */
pime_env* pime_env_create(const pime_env_cfg* cfg);
void pime_env_destroy(pime_env* env);
/* Stream capture and device frees.  hipFree under an open stream capture aborts the process, and Python finalises handles whenever
 * its garbage collector pleases.  Bracket every capture (torch.cuda.graph, hipStreamBeginCapture) with pime_capture_begin / _end:
 * while the depth is non-zero pime_env_destroy and
 * pime_oneshot_destroy park their device memory instead of freeing it; pime_capture_end (at depth 0), pime_env_create and the
 * destroy calls outside a capture drain the queue.  pime_deferred_releases: pointers parked right now. */
void pime_capture_begin(void);
void pime_capture_end(void);
void pime_capture_leave(void);   /* pime_capture_end without the drain (a finaliser inside a capture the library was not told about) */
int pime_deferred_releases(void);
int32_t pime_env_obs_dim(const pime_env* env);
int32_t pime_env_num_envs(const pime_env* env);
/* number of float64 draws one reset consumes per lane: pH 4 (qww_V, qc_V, x0, r), WT 6 (a1, a2, Kp, h1, h2, r) */
int32_t pime_env_reset_draw_width(const pime_env* env);

/* replaces: env.reset() -> reset_all()/reset_r(), ph.py:412-445 ; nonlinear_watertank.py:902-939,1166-1208.
 *   mask  [dev] uint8[N] or NULL (= all lanes)
 *   draws [dev] float64[N, width] final values in the reference's draw order (seed-for-seed replay of the
 *         MT19937 streams, generated host side) or NULL (= in-kernel Philox4x32-10)
 *   obs   [dev] float32[N, obs_dim] written for the reset lanes (float32 = PreprocessEnv cast, env.py:46) */
int pime_env_reset(pime_env* env, const uint8_t* mask, const double* draws, float* obs, pime_stream stream);

/* replaces: PreprocessEnv.step_type -> TimeLimit.step -> env.step(action), ph.py:320-348,448-478 ;
 * nonlinear_watertank.py:800-826,1118-1147.
 *   action       [dev] N env actions, float32 or float64 (action_dtype = pime_dtype)
 *   noise        [dev] WT: float64[N,2] already-scaled normals added to h1,h2 (:810-811) or NULL (= Philox)
 *   auto_reset   1: a lane that reports done is reset in the same launch and its obs row is the first
 *                observation of the next episode (vector-env convention; the reference calls reset() itself)
 *   reset_draws  [dev] as pime_env_reset's draws, consumed only by lanes that auto-reset; or NULL
 *   obs [dev] float32[N, obs_dim]; reward [dev] float32[N]; done [dev] uint8[N] */
int pime_env_step(pime_env* env, const void* action, int32_t action_dtype, const double* noise,
                  int32_t auto_reset, const double* reset_draws, float* obs, float* reward, uint8_t* done,
                  pime_stream stream);

/* The same step with the residual-policy action composition fused into the kernel prologue.
 * replaces: elegantrl/agent_residual.py:61  env.step(np.tanh(action) + state @ self.priorK)
 *   a_pre   [dev] float32[N] pre-tanh residual action (mean + sigma*eps)
 *   obs_in  [dev] float32[N, obs_dim] the observation the policy saw
 *   priorK  [host] float64[obs_dim] (= -env.K); copied into the launch arguments */
int pime_env_step_residual(pime_env* env, const float* a_pre, const float* obs_in, const double* priorK,
                           const double* noise, int32_t auto_reset, const double* reset_draws, float* obs,
                           float* reward, uint8_t* done, pime_stream stream);

/* The same three calls with binary16 observation / reward buffers ([dev] uint16_t = IEEE binary16 bits, torch.float16), for
 * handles in PIME_STATE_MIXED16 mode (PIME_ERR_ARG otherwise).  obs_in of the residual form is the binary16 observation the
 * policy saw.  Accuracy: every stored word is the float32 value rounded to nearest binary16 (relative 2^-11 = 4.9e-4: pH 11 ->
 * +-0.004, reward -64 -> +-0.03); the dynamics (x, the LUT index, h1, h2) are untouched, but the integrated error accumulates one
 * binary16 rounding per step (|I| <= 25: <= 0.008 per step, random-walk growth), and with it the prior PI controller's action. */
int pime_env_reset_h(pime_env* env, const uint8_t* mask, const double* draws, uint16_t* obs, pime_stream stream);
int pime_env_step_h(pime_env* env, const float* action, const double* noise, int32_t auto_reset, const double* reset_draws,
                    uint16_t* obs, uint16_t* reward, uint8_t* done, pime_stream stream);
int pime_env_step_residual_h(pime_env* env, const float* a_pre, const uint16_t* obs_in, const double* priorK,
                             const double* noise, int32_t auto_reset, const double* reset_draws, uint16_t* obs,
                             uint16_t* reward, uint8_t* done, pime_stream stream);

/* replaces: attribute reads/writes on the env object (set_state/set_r/set_params/get_changable_parameters/
 * reset_changable_parameters: ph.py:233-270, nonlinear_watertank.py:205-212,896-900).  synchronous.
 *   out/in [host] float64[N]; mask [host] uint8[N] or NULL.  Writing PIME_PH_QWW_V / PIME_PH_QC_V rebuilds the
 *   lane's ZOH plant (A,B,C) as update_system does (ph.py:114-121).  PIME_PH_Y is read-only. */
int pime_env_read_field(pime_env* env, int32_t field, double* out, pime_stream stream);
int pime_env_write_field(pime_env* env, int32_t field, const double* in, const uint8_t* mask, pime_stream stream);
/* run-time changes the evaluation harness makes on a live env (utils/test.py:1062-1064, utils/robust_test.py:17) */
int pime_env_set_punish(pime_env* env, double integral_punish, double action_punish, double action_change_punish);
int pime_env_set_max_steps(pime_env* env, int32_t max_steps);
int pime_env_set_resample_every(pime_env* env, int32_t n);
/* writes the current observation of every lane (what _get_observe() returns) */
int pime_env_observe(pime_env* env, float* obs, pime_stream stream);

/* -- trajectory post-processing ---------------------------------------------------------------------------
 * replaces: AgentPPO.compute_reward_gae / compute_reward_adv, elegantrl/agent.py:666-708 (a Python loop over
 * device scalars).  Time-major [T, N] float32 buffers, one thread per lane, reverse scan over T.
 * Outputs are un-normalised; the buffer-global (adv-mean)/(std+1e-5) stays with the caller (agent.py:707). */
int pime_gae_scan(const float* reward, const float* mask, const float* value, int32_t T, int32_t N, float lambda,
                  int32_t use_gae, float* r_sum, float* adv, pime_stream stream);

/* -- batched MLP forwards on the f32 matrix cores -----------------------------------------------------------
 * (v_mfma_f32_32x32x2_f32: exact float32, the reference's precision.)  Two steps so that the weight permutation
 * is paid once per weight version, not once per call: pime_mlp_pack re-lays the nn.Linear tensors into the image
 * the kernel keeps in LDS; pime_mlp_forward runs the whole net per 32-row tile with activations in registers.
 *
 *   kind PIME_MLP_CRITIC         replaces CriticAdv.forward over the buffer, elegantrl/agent.py:619-620 with
 *                                net.py:274-277 (D -> md ReLU -> md ReLU -> md ReLU -> 1)
 *                                params[8]  = net.0 W,b ; net.2 W,b ; net.4 W,b ; net.6 W,b
 *   kind PIME_MLP_PLAIN_ACTOR    replaces ActorResidualPPO / ActorPPO mean, net_residual.py:19-22,45-48
 *                                (same shape, Tanh); params[8] as above
 *   kind PIME_MLP_MODULAR_ACTOR  replaces ActorResidualIntegratorModularPPO mean, net_residual.py:153-160,172-176
 *                                params[12] = other_net.0 W,b ; other_net.2 W,b ; integrator_net.0 W,b ;
 *                                integrator_net.2 W,b ; net.0 W,b ; net.2 W,b ; Di = integrator_dim (trailing
 *                                columns of x), 1 <= Di < D.  The other kinds ignore Di.
 *   kind PIME_MLP_SAC_ACTOR      replaces ActorSAC's net_state + net_a_avg / net_a_std, elegantrl/net.py:197-205 (width 64 / 128): params =
 *                                ten tensors in module order (net_state.0/2/4, net_a_avg, net_a_std: W, b); ReLU, Hardswish, Hardswish
 *                                body; the image carries both head rows; pime_mlp_forward returns the mean head BEFORE its tanh
 * All weights are [dev] float32 in nn.Linear layout ([out, in] row-major).  1 <= D <= 32, M >= 1.  Widths: 64 and 128 (every kind: the
 * whole net stays in the 160 KB LDS of a persistent workgroup, csrc/mlp_mfma.hip) and 256 (every kind but PIME_MLP_SAC_ACTOR, which is
 * refused there -- the width run_watertank_changing.sh trains: ResidualPPO on the 30-float Stacking10 observation :20-27,
 * ResidualIntegratorModularPPO on the Integrator observation :11-18 -- on 16-sample tiles of v_mfma_f32_16x16x4_f32 with the weight images streamed through LDS in
 * k-slices, csrc/mlp16.hip; the modular actor's md -> md/2 tower layers are rectangular chain layers there).  Anything else returns
 * PIME_ERR_ARG (pime_mlp_packed_floats: 0) with a message and launches nothing; tests/mlp_cases.py: served pins the set.
 * A NaN in a row of x gives a NaN in that row of out (the ReLU kinds included) and touches no other row.
 * out [dev] float32[M] is the scalar head (value, or pre-tanh action mean without noise and prior term). */
enum pime_mlp_kind { PIME_MLP_CRITIC = 0, PIME_MLP_PLAIN_ACTOR = 1, PIME_MLP_MODULAR_ACTOR = 2, PIME_MLP_SAC_ACTOR = 3 };
/* floats in the packed image (0 and an error message if the shape is unsupported) */
int64_t pime_mlp_packed_floats(int32_t kind, int32_t D, int32_t Di, int32_t md);
int pime_mlp_pack(int32_t kind, int32_t D, int32_t Di, int32_t md, const float* const* params, float* packed,
                  pime_stream stream);
int pime_mlp_forward(int32_t kind, const float* x, int32_t M, int32_t D, int32_t Di, int32_t md, const float* packed,
                     float* out, pime_stream stream);

/* -- fused PPO minibatch gradients ------------------------------------------------------------------------------
 * replaces, per optimizer step of AgentPPO.update_net (elegantrl/agent.py:629-657): the minibatch gather (:632-636),
 * compute_logprob of the residual actors (net_residual.py:48-54,182-190), the clipped surrogate + entropy proxy
 * (:637-645), CriticAdv forward + SmoothL1 (:648-649), the united loss (:652) and `obj_united.backward()` (:654-655)
 * -- i.e. everything between drawing the indices and `optimizer.step()` (pime_adam_step or torch.optim.Adam).
 * Three launches (csrc/ppo_fused.hip): one kernel per net that forms forward, loss gradient, backward chain and the
 * weight gradients of a 256-sample group per workgroup and stores them as a per-workgroup slab, and one reduction of the
 * slabs in a fixed order (bit-for-bit reproducible gradients) that also applies the critic scale.  Observations too wide
 * for that kernel's LDS map use the older net + dW + scale kernels (csrc/ppo_train.hip, float atomics).
 *
 * pime_ppo_net describes one net: the same (kind, D, Di, md, params) as pime_mlp_pack; `grads` are the .grad tensors in
 * the same order and are ACCUMULATED into (zero them first); img_fwd = pime_mlp_pack image,
 * img_bwd = pime_ppo_pack_bwd image (both must be re-packed after the weights change); workspace =
 * pime_ppo_workspace_floats(kind, B, md) floats.  action_dim must be 1. */
typedef struct pime_ppo_net {
    int32_t kind, D, Di, md;
    const float* const* params;   /* [host] array of [dev] pointers, W,b pairs */
    float* const* grads;          /* [host] array of [dev] pointers, same order */
    const float* a_std_log;       /* [dev] actor only: the [1,1] log-std parameter */
    float* g_a_std_log;           /* [dev] actor only: its gradient (accumulated) */
    const float* img_fwd;         /* [dev] */
    const float* img_bwd;         /* [dev] */
    float* workspace;             /* [dev] */
} pime_ppo_net;

typedef struct pime_ppo_batch {
    const float* state;           /* [dev] float32[L, D] trajectory observations */
    const float* action;          /* [dev] float32[L] pre-tanh actions that were taken */
    const float* logprob;         /* [dev] float32[L] their log-probabilities under the old policy */
    const float* adv;             /* [dev] float32[L] normalised advantages */
    const float* r_sum;           /* [dev] float32[L] reward sums (critic targets) */
    const int64_t* indices;       /* [dev] int64[B] minibatch rows (torch.randint) */
    int32_t B;
    int32_t flags;                /* PIME_PPO_* bits, 0 = accumulate into the gradient tensors */
    int64_t* index_row;           /* [dev] int64[1] or NULL.  Not NULL: `indices` is a table int64[rows, B], this call uses
                                   * row index_row[0] and then advances it by one -- the minibatches of a whole update can be
                                   * drawn by one torch.randint and a captured HIP graph replayed per optimizer step */
    float* dp_moments;            /* [dev] float32[4] or NULL.  Not NULL (data-parallel callers): the critic's gradient is left
                                   * UNSCALED and dp_moments[0..2] = sum r_sum[indices], sum of squares, B are written -- the caller
                                   * all-reduces them with the gradients (they sit behind the flat gradient buffer) and
                                   * pime_adam_step_dp applies 1 / (std over the UNION minibatch + 1e-5), which is what agent.py:652
                                   * means when the minibatch is spread over several ranks.  Slab nets only (PIME_ERR_ARG if the
                                   * critic takes the split pipeline) */
} pime_ppo_batch;
/* the call OVERWRITES the gradient tensors (and g_a_std_log) instead of adding to them: saves the caller's zeroing launch */
#define PIME_PPO_OVERWRITE_GRADS 1

/* floats of img_fwd / img_bwd of a pime_ppo_net (filled by pime_ppo_repack; img_bwd alone by pime_ppo_pack_bwd).  The forward
 * image of the gradient path is NOT always pime_mlp_pack's: nets of width 64 / 128 whose observation is too wide for the
 * LDS-resident gradient kernel (the stacked water tank, 30 floats) take the streamed 16-tile family here. */
int64_t pime_ppo_fwd_image_floats(int32_t kind, int32_t D, int32_t Di, int32_t md);
int64_t pime_ppo_bwd_image_floats(int32_t kind, int32_t D, int32_t Di, int32_t md);
/* The leading part of img_bwd that is a permutation of the parameters (what pime_ppo_image_map covers).  Equal to
 * pime_ppo_bwd_image_floats unless the process runs with PIME_GRAD_BF16X3=1 (opt-in; widths 128 / 256 on the 16-tile family --
 * PIME_MLP16=1 routes width 128 there): the streamed layers of the gradient kernels then run on bf16 matrix instructions with every
 * f32 operand split into hi + mid + lo bf16 pieces (six v_mfma_f32_16x16x32_bf16 per product block; error at the f32 rounding level,
 * not bit-equal to the f32 MFMA chain), and the three bf16 planes of those layers' weights follow the f32 image.  The library
 * re-splits them itself after every optimizer step it applies (pime_ppo_minibatch_step, pime_adam_step_images / _dp) and in
 * pime_ppo_repack / pime_ppo_pack_bwd. */
int64_t pime_ppo_bwd_image_f32_floats(int32_t kind, int32_t D, int32_t Di, int32_t md);
int64_t pime_ppo_workspace_floats(int32_t kind, int32_t B, int32_t md);
/* Workgroups (= gradient slabs per net) of the LDS-resident fused gradient kernels for a minibatch of B: one per 256-sample group
 * up to a cap; beyond it a workgroup takes several groups and accumulates them in its slab. */
int32_t pime_ppo_fused_grid(int32_t B);
/* 1 if pime_ppo_minibatch_grad / _step serve an actor of this kind and a critic of the same width on the same D-float state with
 * the pair kernel (a group's actor and critic in one workgroup), 0 if another kernel serves them. */
int pime_ppo_pair_fits(int32_t actor_kind, int32_t D, int32_t Di, int32_t md);
/* Workgroups (= gradient slabs) of the streamed 16-tile family for a net of this shape and a minibatch of B: one per 64-sample
 * group up to a cap that depends on the net's LDS map; 0 (and an error text) for a shape the family has no kernel for. */
int32_t pime_ppo_grid16(int32_t kind, int32_t B, int32_t md, int32_t D, int32_t Di);
/* Host-only: which kernels pime_ppo_minibatch_grad / _step run for an actor of this kind and width beside a critic of width
 * critic_md on the same D-float state -- computed by the function that the two calls themselves dispatch on.  route[0] / route[1]:
 * the actor's / the critic's family (PIME_PPO_FAMILY_*); route[2]: the launch form (PIME_PPO_LAUNCH_*) of the nets on the
 * LDS-resident family.  The answer follows the process's PIME_MLP16 setting, as the calls do. */
#define PIME_PPO_FAMILY_16TILE 0 /* streamed 16-tile kernels (csrc/mlp16.hip), per-workgroup slabs */
#define PIME_PPO_FAMILY_LDS 1    /* LDS-resident fused kernels (csrc/ppo_fused.hip), per-workgroup slabs */
#define PIME_PPO_FAMILY_SPLIT 2  /* net + dW pipeline (csrc/ppo_train.hip), float atomics */
#define PIME_PPO_FAMILY_NONE 3   /* no kernel (the LDS map of the 16-tile kernel does not fit): the query and the calls return an error */
#define PIME_PPO_LAUNCH_SINGLE 0 /* every net in a launch of its own */
#define PIME_PPO_LAUNCH_DUAL 1   /* ppo_fused_dual_kernel: one launch, one workgroup per net and group */
#define PIME_PPO_LAUNCH_PAIR 2   /* ppo_fused_pair_kernel: one launch, a group's actor and critic in one workgroup */
int pime_ppo_route(int32_t actor_kind, int32_t D, int32_t Di, int32_t actor_md, int32_t critic_md, int32_t* route);
int pime_ppo_pack_bwd(int32_t kind, int32_t D, int32_t Di, int32_t md, const float* const* params, float* image,
                      pime_stream stream);
/* Re-packs img_fwd and img_bwd of both nets from their `params` in ONE launch (after every optimizer step; the four
 * separate pack launches cost ~20 us of a ~400 us step). */
int pime_ppo_repack(const pime_ppo_net* actor, const pime_ppo_net* critic, pime_stream stream);
/* critic_scale: [dev] float32[1], WRITTEN: 1 / (r_sum[indices].std() + 1e-5) with torch's unbiased std (agent.py:652);
 *               the critic's gradients are multiplied by it (in the slab reduction)
 * moments:      [dev] float64[2], WRITTEN: sum and sum of squares of the minibatch targets r_sum[indices]
 * loss_sums:    [dev] float32[6], ACCUMULATED over calls (zero them per update): [0] sum(-min(surr1,surr2)),
 *               [1] sum(exp(logp)*logp), [2] sum(smooth_l1), [3] sum of the calls' critic_scale, [4] sum over calls of
 *               (the call's smooth_l1 sum * its critic_scale) -- the critic part of the logged united loss, agent.py:652 --
 *               [5] scratch (value of [2] after the previous call) */
int pime_ppo_minibatch_grad(const pime_ppo_net* actor, const pime_ppo_net* critic, const pime_ppo_batch* batch,
                            float ratio_clip, float lambda_entropy, float* critic_scale, double* moments,
                            float* loss_sums, pime_stream stream);

/* The same call with the optimizer step fused into its last launch (the slab reduction): gradients of the minibatch, then
 * torch.optim.Adam's update of every parameter (pime_adam_step semantics) -- one launch and one launch boundary less per
 * optimizer step.  replaces agent.py:632-657 (gather ... backward ... optimizer.step()).  param / grad are the two flat tensors
 * every pime_ppo_net params / grads pointer is a view into, at equal offsets; gradients of parameters outside them (frozen ones
 * routed to a scratch tensor) are left without an update.  Not available when a net takes the split pipeline (PIME_ERR_ARG);
 * data-parallel callers, who all-reduce the gradients first, use pime_ppo_minibatch_grad + pime_adam_step. */
typedef struct pime_adam {
    float* param;       /* [dev] float32[n] */
    float* grad;        /* [dev] float32[n] */
    float* exp_avg;     /* [dev] float32[n] */
    float* exp_avg_sq;  /* [dev] float32[n] */
    float* step;        /* [dev] float32[2], as pime_adam_step */
    int64_t n;
    float lr, beta1, beta2, eps;
    const int32_t* image_map;   /* [dev] int32[2 n] from pime_ppo_image_map, or NULL.  Not NULL: the launch that updates a
                                 * parameter also writes its new value into the nets' img_fwd / img_bwd, so that NO
                                 * pime_ppo_repack is needed after the step (one launch less per optimizer step) */
    const float* dp_moments;    /* pime_adam_step_dp: [dev] float32[4], the rank-AVERAGED words pime_ppo_batch.dp_moments wrote */
    int64_t critic_offset;      /* pime_adam_step_dp: flat elements [critic_offset, n) are the critic's */
    int32_t dp_world;           /* pime_adam_step_dp: ranks the all-reduce averaged over */
} pime_adam;
/* For every element j of the flat parameter tensor: image_map[2j] = its position in its net's img_fwd, image_map[2j+1] = its
 * position in img_bwd, each with the net in bits 28..29 (0 critic, 1 actor; -1: not in that image, e.g. hidden-layer biases in the
 * transposed image).  The images are permutations of
 * the parameters (plus zero padding); the map is derived by running the library's own pack kernels on index-coded parameters, so it
 * follows whichever kernel family serves each net.  Allocates and frees scratch memory and synchronises the stream: call it once
 * per (nets, flat tensor), outside any graph capture.  PIME_ERR_ARG if a parameter straddles the flat tensor's ends. */
int pime_ppo_image_map(const pime_ppo_net* actor, const pime_ppo_net* critic, const float* flat_param, int64_t n,
                       int32_t* image_map, pime_stream stream);
int pime_ppo_minibatch_step(const pime_ppo_net* actor, const pime_ppo_net* critic, const pime_ppo_batch* batch,
                            float ratio_clip, float lambda_entropy, float* critic_scale, double* moments,
                            float* loss_sums, const pime_adam* opt, pime_stream stream);

/* -- fused rollout ---------------------------------------------------------------------------------------------
 * replaces: the whole per-step loop of AgentResidual*.explore_env for one episode chunk (elegantrl/agent_residual.py:
 * 52-69: select_action -> env.step(np.tanh(action) + state @ priorK) -> buffer.append_buffer), as ONE launch: policy
 * forward (packed actor image, pime_mlp_pack), exploration noise (in-kernel Philox stream 2 keyed by noise_seed,
 * counter (lane, noise_epoch, t)), residual composition, env step with in-kernel auto-reset, trajectory writes.
 * pH or water-tank (Integrator observation) env handle in PIME_STATE_MIXED mode with Philox draws;
 * kind = PIME_MLP_PLAIN_ACTOR | PIME_MLP_MODULAR_ACTOR.
 *   state  [dev] float32[n_steps+1, N, obs_dim]: slot 0 must hold the current observation on entry (pime_env_reset /
 *          pime_env_observe), slots 1..n_steps are written;  action (pre-tanh), noise, reward [dev] float32[n_steps, N];
 *          done [dev] uint8[n_steps, N];  priorK [host] float64[obs_dim]. */
/* 1 if pime_rollout serves this env handle with this actor (PIME_STATE_MIXED / MIXED16, pH or water-tank Integrator / Stacking
 * observation, width 64 / 128 with the actor image resident in LDS, width 256 with the images streamed -- float32 rows only),
 * else 0: the caller then steps the env launch by launch (pime_mlp_forward + pime_env_step_residual). */
int pime_rollout_supported(const pime_env* env, int32_t kind, int32_t md);
int pime_rollout(pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const float* a_std_log,
                 const double* priorK, int32_t n_steps, uint64_t noise_seed, uint32_t noise_epoch, float* state,
                 float* action, float* noise, float* reward, uint8_t* done, pime_stream stream);
/* The same launch for a handle in PIME_STATE_MIXED16 mode (BASELINE.json config 5, "fp16 state"; pH or Integrator water tank):
 * state [dev] binary16[n_steps+1, N, obs_dim] and reward [dev] binary16[n_steps, N] (torch.float16); action and noise stay
 * float32 (they feed the log-probabilities of the update).  Semantics of a chain of pime_env_step_residual_h calls: the policy
 * and the prior term see the binary16 observation, the integrated error is rounded to binary16 after every step (its storage
 * format in this mode), x / h1 / h2 / the plant never are.  replaces agent_residual.py:52-69 as pime_rollout does. */
int pime_rollout_h(pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const float* a_std_log,
                   const double* priorK, int32_t n_steps, uint64_t noise_seed, uint32_t noise_epoch, uint16_t* state,
                   float* action, float* noise, uint16_t* reward, uint8_t* done, pime_stream stream);

/* -- fused evaluation ---------------------------------------------------------------------------------------------
 * replaces: get_episode_return (elegantrl/run.py:600-619: max_step x [act(s) -> env.step], summed rewards) on every lane, and the
 * set-point step-response protocols (utils/test.py:1369-1407 pH, :209-349 water tank; utils/robust_test.py:4-46), as ONE launch:
 * n_steps steps of every lane under the DETERMINISTIC residual policy a_env = tanh(mean(s)) + s @ priorK -- no exploration noise,
 * no auto-reset, no per-step host round trip -- with the env state in registers.  Handles in PIME_STATE_MIXED or PIME_STATE_F64
 * mode (the latter reproduces the reference's float64 protocol records to 1e-11), pH or Integrator water tank, Philox draws.
 *   kind         PIME_MLP_PLAIN_ACTOR | PIME_MLP_MODULAR_ACTOR | PIME_MLP_SAC_ACTOR (ActorSAC.forward = tanh(net_a_avg), net.py:197-199)
 *                | PIME_MLP_CRITIC (the TD3 Actor, net.py:96-110: a_env = tanh(net(s)) + s @ priorK)
 *                with packed_actor = its pime_mlp_pack image (width 64 / 128; 256 except ActorSAC), or -1:
 *                the prior controller alone (get_linear_action, ph.py:227-231), packed_actor ignored
 *   seg_len      0: plain episode.  > 0: every seg_len steps (from step 0) a protocol segment starts: set-point r =
 *                setpoints[segment], integrated error 0, step counter 0, plant state kept -- what the protocols' `env.reset();
 *                set_state(last); set_r(r)` leaves (:1377-1381); setpoints [host] float64[n_setpoints <= 16]
 *   ret          [dev] float64[N] or NULL: += the launch's per-lane sum of (float32) rewards, as run.py:613 accumulates them
 *   trace        [dev] float64[n_steps, 6, N] or NULL, per step and lane: pH (y, r, I BEFORE the step; action, reward, x after it: the
 *                protocol's per-step records, utils/test.py:1388-1396), water tank (h1, h2, r, I after the step; reward; action)
 * Leaves every lane n_steps further; the caller resets the env before it rolls out again.
 * pime_rollout_eval_supported: 0 = not served; 1 = served (widths 64 / 128 in either state mode; width 256 -- the streamed rollout
 * kernel's evaluation mode, csrc/mlp16.hip -- in PIME_STATE_MIXED on the pH / Integrator observation, trace and schedule included);
 * 2 = returns and trace, but no set-point schedule (a Stacking1 / 4 / 10 observation at width 256 under PIME_MLP_PLAIN_ACTOR or
 * PIME_MLP_CRITIC: seg_len must be 0).  Stacking observations at widths 64 / 128 are not served; PIME_MLP_SAC_ACTOR is not
 * served at width 256 (it has no image there). */
int pime_rollout_eval_supported(const pime_env* env, int32_t kind, int32_t md);
int pime_rollout_eval(pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const double* priorK, int32_t n_steps,
                      int32_t seg_len, const double* setpoints, int32_t n_setpoints, double* ret, double* trace,
                      pime_stream stream);

/* -- fused step-response metrics ----------------------------------------------------------------------------------
 * pime_rollout_eval that also reduces the step response WHILE IT RUNS: per lane and set-point segment the control indices one
 * reads off a response, accumulated in registers and written once per segment, so a plant grid needs no float64 trace
 * (48 bytes per lane and step, reduced on the host).  Served exactly where pime_rollout_eval_supported answers 1; where it
 * answers 2 (Stacking at width 256) seg_len must be 0.  kind / md / packed_actor / priorK / n_steps / seg_len / setpoints / ret /
 * trace are pime_rollout_eval's, and ret and trace hold exactly what that call leaves; both may be NULL.
 *   A SEGMENT is the seg_len steps between two set-point boundaries; seg_len == 0: the whole launch is one segment on each
 *   lane's own set-point; a last segment cut short by n_steps is reported over the steps it had.  Per lane and segment with
 *   steps k = 0 .. L-1, everything in double, summed in ascending k:
 *     y_k      the controlled output AFTER step k, widened from the state's precision (pH: the titration-table value at the new
 *              x -- what the trace's next row holds in column 0; water tank: h2 after the step)
 *     r        the segment's set-point as the lane state holds it;  e_k = r - y_k
 *     y_start  the output before the segment's first step;  a_k  the env action as the trace records it
 *   metrics      [dev] float64[n_segments, PIME_METRIC_ROWS, N], n_segments = ceil(n_steps / seg_len) (1 when seg_len == 0); rows:
 *     PIME_METRIC_IAE         sum |e_k|
 *     PIME_METRIC_ISE         sum e_k^2
 *     PIME_METRIC_ITAE        sum (k + 1) |e_k|
 *     PIME_METRIC_OVERSHOOT   max(0, max_k d (y_k - r)),  d = +1 if r >= y_start else -1
 *     PIME_METRIC_SETTLING    1 + the largest k with |e_k| > band; 0 if there is none; L = not inside the band at the last step
 *     PIME_METRIC_SSE         steady-state error: mean of e_k over the last min(tail, L) steps (summed ascending, divided once)
 *     PIME_METRIC_RETURN      sum of the float32 rewards widened, as ret accumulates them
 *     PIME_METRIC_ACTION_VAR  sum over k >= 1 of |a_k - a_{k-1}| inside the segment (no term across a boundary)
 *   band         settling band, finite and >= 0;   tail: steady-state window in steps, >= 1
 * PIME_ERR_ARG with a message naming the argument: NULL metrics, negative / NaN / infinite band, tail < 1, and
 * pime_rollout_eval's own checks.  pime_rollout_eval_metrics_rows() == PIME_METRIC_ROWS. */
enum pime_metric {
    PIME_METRIC_IAE = 0, PIME_METRIC_ISE = 1, PIME_METRIC_ITAE = 2, PIME_METRIC_OVERSHOOT = 3, PIME_METRIC_SETTLING = 4,
    PIME_METRIC_SSE = 5, PIME_METRIC_RETURN = 6, PIME_METRIC_ACTION_VAR = 7, PIME_METRIC_ROWS = 8
};
int pime_rollout_eval_metrics_rows(void);
int pime_rollout_eval_metrics(pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const double* priorK,
                              int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints,
                              double band, int32_t tail, double* ret, double* trace, double* metrics, pime_stream stream);

/* -- fused response band ------------------------------------------------------------------------------------------
 * pime_rollout_eval_metrics that also reduces every step ACROSS lanes: the step response of a whole plant ensemble as a band --
 * per step and lane group the sum, sum of squares, minimum and maximum of four signals, and a histogram of the controlled output
 * -- without the float64 trace.  Served exactly where pime_rollout_eval_supported answers 1 or 2 (2: seg_len must be 0).  Every
 * argument up to `metrics` is pime_rollout_eval_metrics'; ret, trace and metrics hold exactly what that call leaves for the same
 * launch.  ret, trace and hist may be NULL; metrics, stats and workspace may not.
 *   SIGNALS of lane i at launch step t, the values the metrics of that step are built from:
 *     PIME_BAND_Y   y_k, the controlled output after the step        PIME_BAND_E   r - y_k, with the set-point the lane holds
 *     PIME_BAND_A   the env action as the trace records it           PIME_BAND_R   the float32 reward widened to double
 *   GROUPS: lane i of the handle (the local index 0 .. N-1, not the global lane id) belongs to group i / group_lanes;
 *     G = ceil(N / group_lanes).  group_lanes is a positive multiple of 16, or >= N (one group).  The last group may be short.
 *   stats        [dev] float64[n_steps, PIME_BAND_ROWS, G], row = 4 * signal + stat, over the lanes of the group, in double:
 *     PIME_BAND_SUM    sum x          PIME_BAND_SUMSQ  sum x * x (each product rounded before it is added)
 *     PIME_BAND_MIN    min x          PIME_BAND_MAX    max x
 *     Every lane counts once.  The order of the additions is fixed (per 16-lane tile four mirrored folds, then the group's tiles in
 *     ascending order within sixteen interleaved chunks, then the chunks in ascending order): two launches from equal state
 *     give bit-equal stats.  No floating-point atomics.
 *   hist         [dev] uint32[n_steps, G, bins] or NULL: counts of Y.  1 <= bins <= 256, finite lo < hi;
 *     scale = (double)bins / (hi - lo);  bin = 0 if !(y >= lo); bins - 1 if y >= hi; else min((int)floor((y - lo) * scale), bins - 1).
 *     The call zeroes hist on the stream (capture-safe) and counts with integer atomics: exact, order-free.
 *     bins, lo and hi are ignored when hist is NULL.
 *   workspace    [dev] pime_rollout_eval_band_workspace_bytes(env, kind, md, n_steps, group_lanes) bytes (-1: bad arguments), any
 *     content; the layout is private (one 128-byte partial per 16-lane tile and step: at most 8 bytes per lane and step plus one
 *     tile).  Every byte the call reads from it was written by the same call.
 * PIME_ERR_ARG with a message naming the argument: NULL metrics / stats / workspace, group_lanes that is neither a positive
 * multiple of 16 nor >= N, bins outside 1 .. 256, lo >= hi or not finite, and pime_rollout_eval_metrics' own checks.
 * pime_rollout_eval_band_rows() == PIME_BAND_ROWS. */
enum pime_band_signal { PIME_BAND_Y = 0, PIME_BAND_E = 1, PIME_BAND_A = 2, PIME_BAND_R = 3, PIME_BAND_SIGNALS = 4 };
enum pime_band_stat { PIME_BAND_SUM = 0, PIME_BAND_SUMSQ = 1, PIME_BAND_MIN = 2, PIME_BAND_MAX = 3, PIME_BAND_STATS = 4, PIME_BAND_ROWS = 16 };
int pime_rollout_eval_band_rows(void);
int64_t pime_rollout_eval_band_workspace_bytes(const pime_env* env, int32_t kind, int32_t md, int32_t n_steps, int32_t group_lanes);
int pime_rollout_eval_band(pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const double* priorK,
                           int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints, double band, int32_t tail,
                           double* ret, double* trace, double* metrics, int32_t group_lanes, double* stats, uint32_t* hist,
                           int32_t bins, double lo, double hi, void* workspace, pime_stream stream);

/* -- fused replay of recorded runs (plant identification) ----------------------------------------------------------------------
 * Scores PLANTS against measured data: every lane of the handle is a candidate plant, every record a run of T steps with the env
 * action that was applied and the outputs that were measured.  ONE launch runs every (lane, record) pair through the product's own
 * lane step (csrc/env_device.hpp: a replayed step is bit for bit the arithmetic of pime_env_step) with the lane in registers and
 * reduces the output error while the record runs -- instead of one pime_env_step per recorded step and record (and, for one-step
 * prediction, a synchronous pime_env_write_field per step) on a handle that the run advances.  Process noise is zero whatever
 * wt_noise_scale says; no reset ever happens and T may exceed max_steps; rewards, r and the integrated error play no part.
 *   rec (all float64, [dev], shared by all lanes)
 *     action   [E, T]         the env action exactly as env.step received it (pH clips it to [-1, 1] as the env does; the water
 *                             tank does not clip)
 *     output   [E, T + 1, C]  the measured outputs, row 0 before the first step; C = pime_env_replay_channels: pH 1 (y), water
 *                             tank 2 (h1, h2).  The tank's state at row 0 is output[e][0][:] rounded to the state's precision.
 *     state0   [E] or NULL    pH only: the reaction-invariant x at row 0.  NULL: x is hidden, and each (plant, record) pair derives
 *                             x0 = k0 / (C_plant * ph_table_scale), k0 = the smallest table index whose entry is <= output[e][0][0]
 *                             (binary search; the table is strictly decreasing; compared in the precision the handle holds the
 *                             table in), clamped to the table
 *   mode  PIME_REPLAY_SIMULATE  free run from row 0
 *         PIME_REPLAY_PREDICT   one-step-ahead prediction, water tank only: before step t the state is set to the measured
 *                               output[e][t][:] rounded to the state's precision (a NaN word keeps the simulated one)
 *   skip  burn-in: the steps t < skip run but their error is not counted (the transient of a wrong x0 decays as A^t)
 *   err   [dev] float64[E, PIME_REPLAY_ROWS, N], per record and lane, over t = skip .. T-1 in ascending order and per step channel
 *         0 before channel 1:  d = (double)sim_c - output[e][t+1][c];  SSE_c += d * d (the product rounded before it is added);
 *         MAX_c = max(MAX_c, |d|);  COUNT = the number of terms that entered SSE0 + SSE1.  A NaN measurement is a gap: no term,
 *         not counted.  The channel-1 rows are 0 for pH.
 *   sim   [dev] float64[E, T, C, N] or NULL: the simulated outputs after each step (every step, the burn-in included)
 * The call READS the handle and never writes it: per lane pH (A, B, C) / water tank (a1, a2, Kp), from the configuration the plant
 * constants and the table; state, step and episode counters and frame rings are bit-unchanged.  Asynchronous on the caller's
 * stream, capturable, no allocation, no synchronisation, no atomics; a pair's result does not depend on N, E or the grid.
 * Served (pime_env_replay_supported == 1): pH (SIMULATE) and the Integrator water tank (both modes) in PIME_STATE_F64 and
 * PIME_STATE_MIXED.  PIME_STATE_MIXED16 handles and the tank's Stacking observation are REFUSED (0, and the call returns
 * PIME_ERR_ARG): the plant is the same there, so identify on a MIXED Integrator handle.
 * PIME_ERR_ARG before any launch, with a message: E < 1, T < 1, skip < 0 or >= T, NULL action / output / err, state0 on a tank
 * handle, PREDICT on pH, an unknown mode, a handle that is not served.  pime_env_replay_rows() == PIME_REPLAY_ROWS. */
enum pime_replay_mode { PIME_REPLAY_SIMULATE = 0, PIME_REPLAY_PREDICT = 1 };
enum pime_replay_row { PIME_REPLAY_SSE0 = 0, PIME_REPLAY_MAX0 = 1, PIME_REPLAY_SSE1 = 2, PIME_REPLAY_MAX1 = 3, PIME_REPLAY_COUNT = 4,
                       PIME_REPLAY_ROWS = 5 };
typedef struct pime_replay_records {
    const double* action;   /* [dev] float64[E, T] */
    const double* output;   /* [dev] float64[E, T + 1, C] */
    const double* state0;   /* [dev] float64[E] (pH) or NULL */
    int32_t E, T;
} pime_replay_records;
int pime_env_replay_channels(const pime_env* env);   /* C: 1 pH, 2 water tank; 0: NULL handle */
int pime_env_replay_rows(void);
int pime_env_replay_supported(const pime_env* env, int32_t mode);
int pime_env_replay_error(pime_env* env, const pime_replay_records* rec, int32_t mode, int32_t skip, double* err, double* sim,
                          pime_stream stream);

/* -- prior-gain sweep (csrc/prior_sweep.hip) ----------------------------------------------------------------------
 * Which prior gain is best over a whole ensemble of plants, and how bad is it on its worst plant?  ONE call runs every (gain row g,
 * plant lane i) pair of a [G, D] grid of prior gains over the N lanes of the handle under the prior controller alone, a_env =
 * sum_j (double)obs[j] * gains[g][j] (ascending j from 0.0), and reduces each pair's step response to the rows of
 * pime_rollout_eval_metrics and each row ACROSS the plants -- instead of G launches of pime_rollout_eval_metrics(kind = -1), G
 * metric tables and a host-side reduction.  A pair runs exactly that entry point's loop (set-point boundaries every seg_len steps,
 * the lane step, the metrics with the same band and tail) on a register copy of lane i as the handle holds it; the process noise
 * of the water tank is keyed on the plant's global lane (env_offset + i), never on the pair: every gain sees the same disturbance
 * on a given plant (common random numbers).
 *   gains    [dev] float64[G, D], D = the observation width (pH 3, tank 4), in the kernels' sign: priorK = -K of the env classes
 *   n_steps, seg_len, setpoints [host], n_setpoints, band, tail: as pime_rollout_eval_metrics (same checks, same messages)
 *   pairs    [dev] float64[n_segments, PIME_METRIC_ROWS, G, N] or NULL: pairs[:, :, g, :] is bit for bit the `metrics` of
 *            pime_rollout_eval_metrics(kind = -1, priorK = gains[g]) from the same lane state.  NULL is the normal use and does not
 *            change a bit of summary.
 *   summary  [dev] float64[G, n_segments, PIME_METRIC_ROWS, PIME_SWEEP_STATS]: each row over the N plants; a value counts if it is
 *            finite:
 *     PIME_SWEEP_SUM     the sum of the counted values in this order: plants form blocks of 64 consecutive indices (absent plants
 *                        and uncounted values contribute +0.0); inside a block the balanced pairwise tree over the index bits (level
 *                        0 adds elements 2j and 2j + 1, level 1 the results pairwise, .. six levels); the block sums are added
 *                        sequentially in ascending block order, starting from block 0's sum
 *     PIME_SWEEP_MIN, PIME_SWEEP_MAX   over the counted values; +inf / -inf if there is none
 *     PIME_SWEEP_ARGMAX  the plant index of the maximum, as a double; the smallest index on a tie; -1 if no value counts
 *     PIME_SWEEP_FINITE  the number of counted values
 *   workspace [dev] pime_prior_sweep_workspace_bytes(env, G, n_steps, seg_len) bytes (-1: bad arguments); private layout, every
 *            byte read was written by the same call
 * The handle is READ and never written (state, counters, observations bit-unchanged), but must have been reset.  Asynchronous on
 * the caller's stream, capturable, no allocation, no synchronisation, no atomics: two calls give the same bits.
 * Served (pime_prior_sweep_supported == 1): pH and the Integrator water tank in PIME_STATE_F64 and PIME_STATE_MIXED.
 * PIME_STATE_MIXED16 handles and the tank's Stacking observation are REFUSED (0, and the call returns PIME_ERR_ARG).
 * PIME_ERR_ARG before any launch, with a message naming the argument: G < 1, G * N > 2^31 - 1, NULL gains / summary / workspace,
 * and the schedule / band / tail cases of pime_rollout_eval_metrics.  pime_prior_sweep_stats() == PIME_SWEEP_STATS. */
enum pime_sweep_stat { PIME_SWEEP_SUM = 0, PIME_SWEEP_MIN = 1, PIME_SWEEP_MAX = 2, PIME_SWEEP_ARGMAX = 3, PIME_SWEEP_FINITE = 4,
                       PIME_SWEEP_STATS = 5 };
int pime_prior_sweep_supported(const pime_env* env);
int64_t pime_prior_sweep_workspace_bytes(const pime_env* env, int32_t G, int32_t n_steps, int32_t seg_len);
int pime_prior_sweep_stats(void);
int pime_prior_sweep(const pime_env* env, const double* gains, int32_t G, int32_t n_steps, int32_t seg_len, const double* setpoints,
                     int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary, void* workspace,
                     pime_stream stream);

/* -- receding-horizon benchmark controller (csrc/mpc_eval.hip) -------------------------------------------------------
 * How good could ANY controller be on each plant of the handle?  ONE launch runs every lane's plant in closed loop with a non-linear
 * receding-horizon controller on the plant's own model and reduces its step response to the rows of pime_rollout_eval_metrics. All
 * controller arithmetic is float64; no product is contracted into a sum.  One plant at one control step:
 *   CANDIDATES  64 per pass, c = 0 .. 63.  step_0 = 2.0 / 63.0, step_p = step_{p-1} / 32.0.
 *     pass 0       u_c = clip(-1.0 + (double)c * step_0, -1, 1)
 *     pass p >= 1  u_c = clip(u* + (double)(c - 32) * step_p, -1, 1), u* the winner of pass p - 1 (candidate 32 is u* itself: a pass
 *                  never makes the cost worse).  clip(v, lo, hi) = min(max(v, lo), hi).  1 <= passes <= 3.
 *   MODEL ROLLOUT of candidate c: a register copy of the lane as it stands (the tank's h1, h2 are measured: the model state is the
 *     true state; pH: the lane's x), the tank's (a1, a2, Kp) replaced by model_plants[i][:] rounded to the state's precision where
 *     given, stepped `horizon` times (1 .. 64) by the lane step of pime_env_step with the constant action u_c and BOTH process-noise
 *     normals 0.0, under the set-point the lane holds now (no preview across a segment boundary); the TimeLimit flag is ignored and
 *     the copy's t, I, last action and reward are discarded.
 *   COST  J_c = (sum_{k = 1 .. horizon} (y_k - r) * (y_k - r)) + rho * ((u_c - u_prev) * (u_c - u_prev)): the sum sequential in
 *     ascending k from 0.0; y_k the controlled output after model step k widened to double (tank: h2; pH: the looked-up pH in the
 *     state's precision -- for float32 state the observation's value); r the lane's set-point widened to double; u_prev the action
 *     applied at the previous step of the launch (0.0 at its first step; it survives a segment boundary).  rho finite, >= 0.
 *   CHOICE  the smallest J_c; on a tie the smaller c; a non-finite cost loses to any finite one; if none is finite, c = 0.  The
 *     winner of the last pass, u*, is the applied action.
 *   TRUE PLANT  the loop of pime_prior_sweep / pime_rollout_eval_metrics(kind = -1) with a_env = u* in place of obs @ K (no prior
 *     term): the set-point boundaries every seg_len steps (r set, I and t zeroed, a new episode beyond the first), the tank's process
 *     noise keyed on the plant's global lane env_offset + i, the same lane step and the same metric definitions -- so a plant's rows
 *     are directly comparable with those entry points' on the same handle.
 *   model_plants [dev] float64[N, 3] (a1, a2, Kp) or NULL (every plant on its own model); water tank only
 *   n_steps, seg_len, setpoints [host], n_setpoints, band, tail: as pime_rollout_eval_metrics (same checks, same messages)
 *   metrics  [dev] float64[n_segments, PIME_METRIC_ROWS, N], the layout of pime_rollout_eval_metrics
 *   actions  [dev] float64[n_steps, N] or NULL: the applied u*          outputs  [dev] float64[n_steps, N] or NULL: y after the step
 *            NULL is the normal use and does not change a bit of metrics.
 * One wave per plant, the lane index is the candidate index, the argmin is a six-level xor butterfly under the CHOICE rule (a strict
 * total order: every lane ends with the same winner).  The handle is READ and never written (state, counters, observations
 * bit-unchanged), but must have been reset.  Asynchronous on the caller's stream, capturable, no allocation, no synchronisation, no
 * atomics: two calls give the same bits; a plant's rows do not depend on the other lanes or on N.
 * Served (pime_mpc_eval_supported == 1): pH and the Integrator water tank in PIME_STATE_F64 and PIME_STATE_MIXED.
 * PIME_STATE_MIXED16 handles and the tank's Stacking observation are REFUSED (0, and the call returns PIME_ERR_ARG).
 * PIME_ERR_ARG before any launch, with a message naming the argument: a handle that is not served, horizon outside 1 .. 64, passes
 * outside 1 .. 3, rho negative or not finite, NULL metrics, model_plants on a pH handle (its state x is not measured), and the
 * schedule / band / tail cases of pime_rollout_eval_metrics. */
int pime_mpc_eval_supported(const pime_env* env);
int pime_mpc_eval(const pime_env* env, const double* model_plants, int32_t horizon, int32_t passes, double rho, int32_t n_steps,
                  int32_t seg_len, const double* setpoints, int32_t n_setpoints, double band, int32_t tail, double* metrics,
                  double* actions, double* outputs, pime_stream stream);

/* -- loop-perturbation sweep (csrc/margin_sweep.hip) ----------------------------------------------------------------
 * How much dead time, how much loop-gain error and how much sensor noise does the closed loop tolerate -- under the residual policy
 * and under the prior controller alone?  The entry points above perturb the PLANT and leave the LOOP ideal; this one perturbs the
 * loop.  ONE call runs every (perturbation row p, plant lane i) pair of a [P, 3] grid `perturb` -- a row is (g, d, sigma), columns
 * enum pime_perturb_col -- over the N lanes of the handle.  A pair runs the loop of pime_rollout_eval_metrics (set-point boundaries
 * every seg_len steps, the lane step, the metrics with the same band and tail) on a register copy of lane i as the handle holds it,
 * with three things inserted at launch step t:
 *   MEASUREMENT  obs_m = obs, except for the measured plant outputs -- pH column 0 (y), tank columns 0 and 1 (h1, h2) -- where
 *     obs_m[j] = obs[j] + (float)sigma * n_j in float32.  (n_0, n_1) is the Box-Muller pair of philox_pair(noise_seed, env_offset + i,
 *     noise_epoch, t, stream 3): radius sqrt(-2 log(1 - ua)), angle 2 pi ub, the cosine branch for column 0 and the sine branch for
 *     column 1, computed in double and rounded to float32.  The key is the plant, never the pair: every row meets the same noise
 *     sequence, scaled (common random numbers, as the tank's process noise in pime_prior_sweep).  sigma == 0: the observation is used
 *     as it is and nothing is drawn.  The set-point column and the integrator column are the ENV'S OWN: the env integrates the true
 *     error and the controller reads that integral unperturbed (a controller-side integrator of the measured error is not modelled).
 *   CONTROLLER  a_c = tanh(mean(obs_m)) + obs_m @ priorK as pime_rollout_eval forms it (the prior term in double, ascending j from
 *     0.0); kind = -1: the prior controller alone.
 *   ACTUATOR  a_env(t) = g * a_c(t - d), a_c(s) = 0.0 for s < 0: a delay line of PIME_MARGIN_MAX_DELAY doubles, NOT cleared at a
 *     segment boundary (the actuator knows nothing of set-points).  d = rint(perturb[p][1]) clamped into 0 .. PIME_MARGIN_MAX_DELAY
 *     (NaN: 0).  The metrics' action row and `actions` hold the APPLIED a_env.
 * With (g, d, sigma) = (1, 0, 0) a pair is bit for bit a lane of pime_rollout_eval_metrics from the same lane state.
 *   kind, md, packed_actor, priorK: as pime_rollout_eval (priorK [host] float64[D])
 *   perturb  [dev] float64[P, PIME_PERTURB_COLS]
 *   noise_seed, noise_epoch: the key of the measurement noise
 *   n_steps, seg_len, setpoints [host], n_setpoints, band, tail: as pime_rollout_eval_metrics (same checks, same messages)
 *   pairs    [dev] float64[n_segments, PIME_METRIC_ROWS, P, N] or NULL
 *   summary  [dev] float64[P, n_segments, PIME_METRIC_ROWS, PIME_SWEEP_STATS]: each row over the N plants, EXACTLY the statistics and
 *            the addition order of pime_prior_sweep's summary (blocks of 64 plants, the pairwise tree, the blocks in sequence, the
 *            smaller index on a tie)
 *   actions  [dev] float64[n_steps, P, N] or NULL: the applied a_env     outputs  [dev] float64[n_steps, P, N] or NULL: y after the step
 *            NULL pairs / actions / outputs is the normal use and does not change a bit of summary.
 *   workspace [dev] pime_margin_sweep_workspace_bytes(env, P, n_steps, seg_len) bytes (-1: bad arguments); private layout, every byte
 *            read was written by the same call
 * Persistent 256-thread workgroups stage the actor's image into LDS once and walk quads of 16-lane tiles (one tile of ONE row per
 * wave: g, d and sigma are wave-uniform; the prior alone runs 64 distinct pairs per wave); a finishing launch reduces the rows per
 * perturbation.  The handle is READ and never written (state, counters, observations bit-unchanged), but must have been reset.
 * Asynchronous on the caller's stream, capturable, no allocation, no synchronisation, no floating-point atomics: two calls give the
 * same bits; a pair's result does not depend on P, N or its position in the grid.
 * Served (pime_margin_sweep_supported == 1): pH and the Integrator water tank in PIME_STATE_F64 and PIME_STATE_MIXED, kind = -1 or one
 * of the four policy kinds of pime_rollout_eval at width 64 or 128.  Width 256 (the streamed family), PIME_STATE_MIXED16 handles and
 * the tank's Stacking observation are REFUSED (0, and the call returns PIME_ERR_ARG).
 * PIME_ERR_ARG before any launch, with a message naming the argument: the refused classes, P < 1, P * N > 2^31 - 1, NULL perturb /
 * summary / workspace / priorK (and packed_actor with a policy), and the schedule / band / tail cases of pime_rollout_eval_metrics. */
enum pime_perturb_col { PIME_PERTURB_GAIN = 0, PIME_PERTURB_DELAY = 1, PIME_PERTURB_SIGMA = 2, PIME_PERTURB_COLS = 3 };
enum { PIME_MARGIN_MAX_DELAY = 8 };
int pime_margin_sweep_supported(const pime_env* env, int32_t kind, int32_t md);
int64_t pime_margin_sweep_workspace_bytes(const pime_env* env, int32_t P, int32_t n_steps, int32_t seg_len);
int pime_margin_sweep(const pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const double* priorK,
                      const double* perturb, int32_t P, uint64_t noise_seed, uint32_t noise_epoch, int32_t n_steps, int32_t seg_len,
                      const double* setpoints, int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary,
                      double* actions, double* outputs, void* workspace, pime_stream stream);

/* -- disturbance-rejection sweep (csrc/disturb_sweep.hip) ------------------------------------------------------------
 * How well does the closed loop REJECT a disturbance -- a load at the plant input, a step of the plant's parameters -- under the
 * residual policy and under the prior controller alone?  The entry points above excite the loop through set-point steps only.  ONE
 * call runs every (disturbance row p, plant lane i) pair of a [P, 6] grid `disturb` -- columns enum pime_disturb_col -- over the N
 * lanes of the handle.  A pair runs the loop of pime_rollout_eval_metrics (set-point boundaries every seg_len steps, the lane step, the
 * metrics with the same band and tail) on a register copy of lane i as the handle holds it.  With k the step WITHIN the segment:
 *   ONSET k0, LENGTH L   k0 = rint(disturb[p][0]) clamped into 0 .. 2^30 (NaN: never); L = rint(disturb[p][1]) clamped likewise (NaN:
 *     0).  The row is ACTIVE at k iff k >= k0 && (L == 0 || k < k0 + L): L == 0 lasts to the end of the segment, L > 0 is a pulse cut at
 *     the segment's end.  Every segment starts on the nominal plant again and the row comes back at its step k0.
 *   LOAD d_u   while active a_env = a_c + d_u (one double addition, normalised action units) IN FRONT of the actuator: pH's
 *     clip(a, -1, 1) sees the sum, the tank does not clip.  While inactive a_env = a_c with no addition at all.
 *   M0, M1, M2   while active the lane steps on a disturbed parameter set formed once per pair.  Tank: a1' = (S)((double)a1 * M0),
 *     a2' with M1, Kp' with M2 (S the state's precision).  pH: q = qww_V * M0, e = -q * sample_t, A' = exp(e), B' = -expm1(e) / q,
 *     C' = qc_V * M1 in double from the lane's STORED qww_V and qc_V, as a resampling reset forms them; M2 is ignored.  A parameter
 *     whose multiplier is exactly 1.0 is the lane's own stored word, never recomputed (M0 == 1 keeps the stored A and B, M1 == 1 the
 *     stored C).
 *   CONTROLLER  a_c = tanh(mean(obs)) + obs @ priorK as pime_rollout_eval forms it; kind = -1: the prior controller alone.  The
 *     metrics' action row and `actions` hold the CONTROLLER's output a_c (controller effort); the applied action is a_c + d_u.
 * Rows PIME_METRIC_ROWS + enum pime_disturb_row of a pair and segment, over the window k >= k0 of that segment (sums sequential in
 * ascending k from 0.0, e_k = r - y_k with y_k the controlled output after step k):
 *   E0           r - y of the output step k0 starts from (k0 == 0: the segment's start): had the loop settled?
 *   PEAK         max |e_k|            PEAK_STEP  k - k0 + 1 of the first step that attains it
 *   RECOVERY     1 + (the last window step with |e_k| > band) - k0, 0 if there is none; the window's length: not recovered
 *   IAE          sum |e_k|            ITAE       sum (double)(k - k0 + 1) * |e_k|
 *   ACTION_PEAK  max |a_c(k) - a_c(k0 - 1)|, a_c(-1) := 0.0
 * A segment with k0 >= its steps holds NaN in all seven; the summary does not count them.  With d_u = 0 and unit multipliers, for
 * any ONSET and LENGTH, the first PIME_METRIC_ROWS rows are bit for bit a lane of pime_rollout_eval_metrics from the same lane state.
 *   kind, md, packed_actor, priorK: as pime_rollout_eval (priorK [host] float64[D])
 *   disturb  [dev] float64[P, PIME_DISTURB_COLS]
 *   n_steps, seg_len, setpoints [host], n_setpoints, band, tail: as pime_rollout_eval_metrics (same checks, same messages)
 *   pairs    [dev] float64[n_segments, PIME_METRIC_ROWS + PIME_DISTURB_ROWS, P, N] or NULL
 *   summary  [dev] float64[P, n_segments, PIME_METRIC_ROWS + PIME_DISTURB_ROWS, PIME_SWEEP_STATS]: each row over the N plants, EXACTLY
 *            the statistics and the addition order of pime_prior_sweep's summary
 *   actions  [dev] float64[n_steps, P, N] or NULL: a_c                   outputs  [dev] float64[n_steps, P, N] or NULL: y after the step
 *            NULL pairs / actions / outputs is the normal use and does not change a bit of summary.
 *   workspace [dev] pime_disturb_sweep_workspace_bytes(env, P, n_steps, seg_len) bytes (-1: bad arguments); private layout, every
 *            byte read was written by the same call
 * The tiling is pime_margin_sweep's (one 16-lane tile of ONE row per wave: the row is wave-uniform; the prior alone runs 64 distinct
 * pairs per wave; a finishing launch reduces the rows per disturbance).  The handle is READ and never written (state, counters,
 * observations bit-unchanged), but must have been reset.  Asynchronous on the caller's stream, capturable, no allocation, no
 * synchronisation, no atomics: two calls give the same bits; a pair's result does not depend on P, N or its position in the grid.
 * Served (pime_disturb_sweep_supported == 1): exactly the classes of pime_margin_sweep.  Width 256, PIME_STATE_MIXED16 handles and the
 * tank's Stacking observation are REFUSED (0, and the call returns PIME_ERR_ARG).
 * PIME_ERR_ARG before any launch, with a message naming the argument: the refused classes, P < 1, P * N > 2^31 - 1, NULL disturb /
 * summary / workspace / priorK (and packed_actor with a policy), and the schedule / band / tail cases of pime_rollout_eval_metrics. */
enum pime_disturb_col { PIME_DISTURB_ONSET = 0, PIME_DISTURB_LENGTH = 1, PIME_DISTURB_LOAD = 2, PIME_DISTURB_M0 = 3, PIME_DISTURB_M1 = 4,
                        PIME_DISTURB_M2 = 5, PIME_DISTURB_COLS = 6 };
enum pime_disturb_row { PIME_DISTURB_E0 = 0, PIME_DISTURB_PEAK = 1, PIME_DISTURB_PEAK_STEP = 2, PIME_DISTURB_RECOVERY = 3,
                        PIME_DISTURB_IAE = 4, PIME_DISTURB_ITAE = 5, PIME_DISTURB_ACTION_PEAK = 6, PIME_DISTURB_ROWS = 7 };
int pime_disturb_sweep_supported(const pime_env* env, int32_t kind, int32_t md);
int64_t pime_disturb_sweep_workspace_bytes(const pime_env* env, int32_t P, int32_t n_steps, int32_t seg_len);
int pime_disturb_sweep(const pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const double* priorK,
                       const double* disturb, int32_t P, int32_t n_steps, int32_t seg_len, const double* setpoints,
                       int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary, double* actions,
                       double* outputs, void* workspace, pime_stream stream);

/* -- frequency-response sweep (csrc/freq_sweep.hip) -----------------------------------------------------------------
 * What is the loop's transfer function -- its gain margin, phase margin, peak sensitivity and bandwidth -- under the residual
 * policy and under the prior controller alone?  The entry points above are time-domain experiments; this one excites the loop with a
 * tabulated waveform and correlates the response with it (a lock-in).  ONE call runs every (excitation row p, plant lane i) pair of a
 * [P, 3] grid `excite` -- columns enum pime_freq_col -- over the N lanes of the handle.  A pair runs the loop of
 * pime_rollout_eval_metrics (set-point boundaries every seg_len steps, the lane step, the metrics with the same band and tail) on a
 * register copy of lane i as the handle holds it.  With k the step WITHIN the segment and (c_k, s_k) = wave[p][k] (the table is
 * indexed by k: the excitation restarts with every segment), the excitation of step k is e_k = A * s_k, one double multiplication,
 * applied at EVERY step of the segment at the row's POINT (rint, clamped into 0 .. 2, NaN: 0; enum pime_freq_point):
 *   SETPOINT     the lane's set-point word of step k is (S)(sp + e_k) (S the state's precision, sp the segment's set-point; without a
 *     schedule the lane's stored word) and the observation's set-point column follows it: the env integrates the error against the
 *     modulated set-point, as for a real reference change.  The metrics keep the segment's nominal set-point.  Measures the
 *     complementary sensitivity T.
 *   LOAD         a_env = a_c + e_k, one double addition IN FRONT of the actuator (pH's clip(a, -1, 1) sees the sum, the tank does not
 *     clip): the classical loop-breaking measurement.  a_c and a_env carry the same step index: L = -A_c / (A_c + E) at the
 *     fundamental.
 *   MEASUREMENT  the controller reads obs[c] + (float)e_k in float32 on the controlled output's column (pH: 0, y; tank: 1, h2); the
 *     env integrates the TRUE error, as in pime_margin_sweep.  Measures the noise sensitivity.
 * A == 0.0: nothing is added and no word is rewritten -- for any POINT, ONSET and table the first PIME_METRIC_ROWS rows are bit for
 * bit a lane of pime_rollout_eval_metrics from the same lane state.  The metrics' action row and `actions` hold the CONTROLLER's
 * output a_c, `outputs` y after the step.
 * Rows PIME_METRIC_ROWS + enum pime_freq_row of a pair and segment, over the window k >= k0 (ONSET, decoded as pime_disturb_sweep's:
 * rint clamped into 0 .. 2^30, NaN: never; the steps before k0 let the loop reach its periodic state).  Sums are sequential double
 * additions in ascending k from 0.0, each product rounded before it is added:
 *   YC  sum y_k c_k      YS  sum y_k s_k      UC  sum a_c,k c_k      US  sum a_c,k s_k
 *   Y0  sum y_k          U0  sum a_c,k        Y2  sum y_k^2          U2  sum a_c,k^2
 * A segment with k0 >= its steps holds NaN in all eight; the summary does not count them.
 *   kind, md, packed_actor, priorK: as pime_rollout_eval (priorK [host] float64[D])
 *   excite   [dev] float64[P, PIME_FREQ_COLS]
 *   wave     [dev] float64[P, wave_len, 2]: (c_k, s_k) per row and segment step; wave_len must be seg_len, or n_steps when seg_len == 0.
 *            Any waveform: the table comes from the caller (a sinusoid with an integer number of cycles in the window makes c and s
 *            orthogonal over it), so every stored row is reproducible from the traces bit for bit.
 *   n_steps, seg_len, setpoints [host], n_setpoints, band, tail: as pime_rollout_eval_metrics (same checks, same messages)
 *   pairs    [dev] float64[n_segments, PIME_METRIC_ROWS + PIME_FREQ_ROWS, P, N] or NULL
 *   summary  [dev] float64[P, n_segments, PIME_METRIC_ROWS + PIME_FREQ_ROWS, PIME_SWEEP_STATS]: each row over the N plants, EXACTLY the
 *            statistics and the addition order of pime_prior_sweep's summary
 *   actions  [dev] float64[n_steps, P, N] or NULL: a_c                   outputs  [dev] float64[n_steps, P, N] or NULL: y after the step
 *            NULL pairs / actions / outputs is the normal use and does not change a bit of summary.
 *   workspace [dev] pime_freq_sweep_workspace_bytes(env, P, n_steps, seg_len) bytes (-1: bad arguments); private layout, every byte
 *            read was written by the same call
 * The tiling is pime_margin_sweep's (one 16-lane tile of ONE row per wave: the row and its table are wave-uniform; the prior alone
 * runs 64 distinct pairs per wave; a finishing launch reduces the rows per excitation).  The handle is READ and never written, but
 * must have been reset.  Asynchronous on the caller's stream, capturable, no allocation, no synchronisation, no atomics: two calls give
 * the same bits; a pair's result does not depend on P, N or its position in the grid.
 * Served (pime_freq_sweep_supported == 1): exactly the classes of pime_margin_sweep.  Width 256, PIME_STATE_MIXED16 handles and the
 * tank's Stacking observation are REFUSED (0, and the call returns PIME_ERR_ARG).
 * PIME_ERR_ARG before any launch, with a message naming the argument: the cases of pime_disturb_sweep (with `excite` for `disturb`),
 * NULL wave, and wave_len other than seg_len (n_steps when seg_len == 0). */
enum pime_freq_col { PIME_FREQ_POINT = 0, PIME_FREQ_AMPLITUDE = 1, PIME_FREQ_ONSET = 2, PIME_FREQ_COLS = 3 };
enum pime_freq_point { PIME_FREQ_SETPOINT = 0, PIME_FREQ_LOAD = 1, PIME_FREQ_MEASUREMENT = 2 };
enum pime_freq_row { PIME_FREQ_YC = 0, PIME_FREQ_YS = 1, PIME_FREQ_UC = 2, PIME_FREQ_US = 3, PIME_FREQ_Y0 = 4, PIME_FREQ_U0 = 5,
                     PIME_FREQ_Y2 = 6, PIME_FREQ_U2 = 7, PIME_FREQ_ROWS = 8 };
int pime_freq_sweep_supported(const pime_env* env, int32_t kind, int32_t md);
int64_t pime_freq_sweep_workspace_bytes(const pime_env* env, int32_t P, int32_t n_steps, int32_t seg_len);
int pime_freq_sweep(const pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const double* priorK, const double* excite,
                    const double* wave, int32_t wave_len, int32_t P, int32_t n_steps, int32_t seg_len, const double* setpoints,
                    int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary, double* actions, double* outputs,
                    void* workspace, pime_stream stream);

/* -- actuator-limits sweep (csrc/actuator_sweep.hip) ------------------------------------------------------------------
 * What do a REAL actuator and a real sensor -- saturation, a slew-rate limit, a dead-band, a DAC quantum, an ADC quantum -- do to the
 * closed loop under the residual policy and under the prior controller alone: wind-up overshoot, limit cycles ("hunting")?  The entry
 * points above hand the plant the controller's real number and the controller the plant's outputs at full precision.  ONE call runs
 * every (actuator row p, plant lane i) pair of a [P, 6] grid `actuator` -- columns enum pime_act_col -- over the N lanes of the
 * handle.  Everything not said here is pime_disturb_sweep's: the loop of pime_rollout_eval_metrics on a register copy of lane i, the
 * schedule, band and tail, pairs / summary / workspace and a NULL pairs, the tiling, the handle READ and never written, no allocation,
 * capturable, two calls give the same bits, the served classes, the refusals.
 * The rows live on the device, so they are DECODED, not validated.  All columns are in normalised action units except QY:
 *   LO, HI     saturation limits.                                        off: -inf / +inf, or NaN (the stage runs iff LO > -inf || HI < inf)
 *   RATE       the largest move per sample period.                       off: anything not 0 < RATE < inf
 *   DEADBAND   hold if the command is within it of the present position. off: anything not > 0
 *   QU         the actuator's quantum (a DAC step).                      off: anything not > 0
 *   QY         the sensor's quantum (an ADC step), observation units.    off: anything not > 0
 * Per launch step t:
 *   SENSOR      obs_m = obs; with QY on, for the measured plant outputs only (pH: column 0; tank: columns 0 and 1, as in
 *     pime_margin_sweep) obs_m[j] = (float)(QY * rint((double)obs[j] / QY)).  The set-point and integrator columns are the env's own.
 *   CONTROLLER  a_c from obs_m as pime_disturb_sweep forms it from obs; kind = -1: the prior controller alone.
 *   ACTUATOR    in double, on v = a_c and the previous APPLIED action u_prev -- 0.0 before the launch's first step, NOT cleared at a
 *     segment boundary (like pime_margin_sweep's delay line) -- the stages in this fixed order, each only if it is on:
 *       dead-band   if (fabs(v - u_prev) <= DEADBAND) v = u_prev;
 *       slew        v = u_prev + clip(v - u_prev, -RATE, RATE);
 *       quantise    v = QU * rint(v / QU);
 *       clamp       v = clip(v, LO, HI);
 *     with clip(x, lo, hi): x < lo ? lo : x, then x > hi ? hi : x (a NaN limit never binds), rint to nearest-even.  The clamp comes
 *     last, so a limit holds exactly.  u = v; the lane steps on u (pH's own clip(a, -1, 1) still sees it); u_prev = u.
 * A stage that is off performs no arithmetic and rewrites no word: a row with all six columns off is bit for bit a lane of
 * pime_rollout_eval_metrics from the same lane state (a -0.0 stays -0.0).  The metrics' action row and `actions` hold the APPLIED u (as
 * in pime_margin_sweep), `commands` the controller's a_c, `outputs` y after the step.
 * Rows PIME_METRIC_ROWS + enum pime_act_row of a pair and segment, over ALL steps of the segment; each can be recomputed from the
 * three traces (the chain re-run on `commands`):
 *   SAT_STEPS    steps where the clamp changed v          RATE_STEPS   steps where the slew limit bound (clip(d) != d)
 *   HOLD_STEPS   steps the dead-band held                 GAP_PEAK     max |a_c - u|
 *   GAP_IAE      sum |a_c - u|, sequential from 0.0 in ascending step
 *   REVERSALS    sign changes between successive NON-ZERO moves u_k - u_{k-1}; the last move's sign is forgotten at the segment's
 *                start, the segment's first move is measured from the u_prev it inherited
 *   TAIL_Y_P2P   max - min of y over the segment's last `tail` steps (the window of PIME_METRIC_SSE): the limit cycle's amplitude
 *   TAIL_U_P2P   max - min of u over the same steps
 * Counts are exact integers stored as double.  Every segment has steps, so no row is NaN by construction.
 *   kind, md, packed_actor, priorK: as pime_rollout_eval (priorK [host] float64[D])
 *   actuator [dev] float64[P, PIME_ACT_COLS]
 *   n_steps, seg_len, setpoints [host], n_setpoints, band, tail: as pime_rollout_eval_metrics (same checks, same messages)
 *   pairs    [dev] float64[n_segments, PIME_METRIC_ROWS + PIME_ACT_ROWS, P, N] or NULL
 *   summary  [dev] float64[P, n_segments, PIME_METRIC_ROWS + PIME_ACT_ROWS, PIME_SWEEP_STATS]: pime_prior_sweep's statistics and order
 *   actions  [dev] float64[n_steps, P, N] or NULL: u        commands [dev] float64[n_steps, P, N] or NULL: a_c
 *   outputs  [dev] float64[n_steps, P, N] or NULL: y after the step.  NULL pairs / actions / commands / outputs is the normal use and
 *            does not change a bit of summary.
 *   workspace [dev] pime_actuator_sweep_workspace_bytes(env, P, n_steps, seg_len) bytes (-1: bad arguments); private layout, every
 *            byte read was written by the same call
 * Served (pime_actuator_sweep_supported == 1): exactly the classes of pime_margin_sweep.  Width 256, PIME_STATE_MIXED16 handles and the
 * tank's Stacking observation are REFUSED (0, and the call returns PIME_ERR_ARG).
 * PIME_ERR_ARG before any launch, with a message naming the argument: the cases of pime_disturb_sweep (with `actuator` for `disturb`). */
enum pime_act_col { PIME_ACT_LO = 0, PIME_ACT_HI = 1, PIME_ACT_RATE = 2, PIME_ACT_DEADBAND = 3, PIME_ACT_QU = 4, PIME_ACT_QY = 5,
                    PIME_ACT_COLS = 6 };
enum pime_act_row { PIME_ACT_SAT_STEPS = 0, PIME_ACT_RATE_STEPS = 1, PIME_ACT_HOLD_STEPS = 2, PIME_ACT_GAP_PEAK = 3, PIME_ACT_GAP_IAE = 4,
                    PIME_ACT_REVERSALS = 5, PIME_ACT_TAIL_Y_P2P = 6, PIME_ACT_TAIL_U_P2P = 7, PIME_ACT_ROWS = 8 };
int pime_actuator_sweep_supported(const pime_env* env, int32_t kind, int32_t md);
int64_t pime_actuator_sweep_workspace_bytes(const pime_env* env, int32_t P, int32_t n_steps, int32_t seg_len);
int pime_actuator_sweep(const pime_env* env, int32_t kind, int32_t md, const float* packed_actor, const double* priorK,
                        const double* actuator, int32_t P, int32_t n_steps, int32_t seg_len, const double* setpoints,
                        int32_t n_setpoints, double band, int32_t tail, double* pairs, double* summary, double* actions,
                        double* commands, double* outputs, void* workspace, pime_stream stream);

/* -- policy sweep (csrc/policy_sweep.hip) -----------------------------------------------------------------------------
 * Which of my controllers -- the snapshots of one training run, the seeds of one configuration -- is best on its WORST plant?  The
 * sweeps above take one packed actor and one priorK; this one adds the policy as the grid's axis.  ONE call runs every (policy row p,
 * plant lane i) pair of P packed actors over the N lanes of the handle.  A pair runs the loop of pime_rollout_eval_metrics (set-point
 * boundaries every seg_len steps, the lane step, the metrics with the same band and tail) on a register copy of lane i as the handle
 * holds it, under a_env = tanh(mean_p(obs)) + obs @ priorK[p] as pime_rollout_eval forms it (the prior term in double, ascending j
 * from 0.0): row p uses image p and its own prior gain.  A pair of row p is bit for bit a lane of pime_rollout_eval_metrics(kind, md,
 * image p, priorK[p]) from the same lane state; the tank's process noise is keyed on the plant's global lane, so every policy meets
 * the same disturbance (common random numbers, as every gain of pime_prior_sweep does).
 *   kind, md      one class for all P images: one of the four policy kinds of pime_rollout_eval at width 64 or 128.  kind = -1 is
 *                 REFUSED: under the prior controller alone a grid of gains is pime_prior_sweep.
 *   packed_actors [dev] P images of pime_mlp_packed_floats(kind, D, Di, md) floats (pime_mlp_pack), image p at packed_actors +
 *                 p * image_stride; 16-byte aligned
 *   image_stride  floats between two images: >= the packed size and a multiple of 4; the padding is never read
 *   priorK        [dev] float64[P, D] -- on the DEVICE, unlike the single-policy calls: it is read with the row
 *   n_steps, seg_len, setpoints [host], n_setpoints, band, tail: as pime_rollout_eval_metrics (same checks, same messages)
 *   pairs    [dev] float64[n_segments, PIME_METRIC_ROWS, P, N] or NULL
 *   summary  [dev] float64[P, n_segments, PIME_METRIC_ROWS, PIME_SWEEP_STATS]: each row over the N plants, EXACTLY the statistics and
 *            the addition order of pime_prior_sweep's summary
 *   actions  [dev] float64[n_steps, P, N] or NULL: a_env                 outputs  [dev] float64[n_steps, P, N] or NULL: y after the step
 *            NULL pairs / actions / outputs is the normal use and does not change a bit of summary.
 *   workspace [dev] pime_policy_sweep_workspace_bytes(env, P, n_steps, seg_len) bytes (-1: bad arguments); private layout, every byte
 *            read was written by the same call
 * A tile is 16 plants of one row; a 256-thread workgroup takes a quad of four tiles of the SAME row, and persistent workgroups each
 * walk a contiguous range of quads, so the image in LDS is re-staged only when the row changes; a finishing launch (the row grid's)
 * reduces the rows per policy.  The handle is READ and never written (state, counters, observations bit-unchanged), but must have been
 * reset.  Asynchronous on the caller's stream, capturable, no allocation, no synchronisation, no atomics: two calls give the same
 * bits; a pair's result does not depend on P, N or its position in the grid.
 * Served (pime_policy_sweep_supported == 1): the classes of pime_margin_sweep WITH a policy (32: pH and the Integrator water tank,
 * PIME_STATE_F64 and PIME_STATE_MIXED, four kinds, widths 64 and 128).  kind = -1, width 256, PIME_STATE_MIXED16 handles and the
 * tank's Stacking observation are REFUSED (0, and the call returns PIME_ERR_ARG).
 * PIME_ERR_ARG before any launch, with a message naming the argument: the refused classes, P < 1, P * N > 2^31 - 1, NULL
 * packed_actors / summary / priorK / workspace, an image_stride below the packed size or not a multiple of 4, a base that is not
 * 16-byte aligned, and the schedule / band / tail cases of pime_rollout_eval_metrics. */
int pime_policy_sweep_supported(const pime_env* env, int32_t kind, int32_t md);
int64_t pime_policy_sweep_workspace_bytes(const pime_env* env, int32_t P, int32_t n_steps, int32_t seg_len);
int pime_policy_sweep(const pime_env* env, int32_t kind, int32_t md, const float* packed_actors, int64_t image_stride,
                      const double* priorK, int32_t P, int32_t n_steps, int32_t seg_len, const double* setpoints, int32_t n_setpoints,
                      double band, int32_t tail, double* pairs, double* summary, double* actions, double* outputs, void* workspace,
                      pime_stream stream);

/* -- fused off-policy exploration-----------------------------------------------------------------------------------
 * replaces, per lock-step of the vectorised off-policy agents: AgentBase.explore_env's body (elegantrl/agent.py:54-70) with
 * AgentTD3.select_action (:300-306: a = (act(s) + N(0, explore_noise)).clamp(-1, 1)), env.step, and ReplayBuffer.append_buffer
 * (replay.py:290-300) -- as ONE launch for n_steps lock-steps of every lane: deterministic actor forward on the matrix cores,
 * clipped exploration noise (Philox stream 2, counter (lane, noise_epoch, t)), env action a_env = a + s @ priorK (priorK zeros:
 * plain TD3), env step with in-kernel auto-reset, transition written into the device ring.  The running episodes CONTINUE (no
 * reset in front).  Handle in PIME_STATE_MIXED mode, Philox draws; pH, Integrator water tank, or the water tank's Stacking
 * observation with num_stack 1 / 4 / 10 (there the handle's frame ring is rewritten when the launch ends, so pime_env_step /
 * pime_env_observe continue from it).  Widths 64 / 128: the LDS-resident image (csrc/rollout_offpolicy.hip); width 256: the
 * streamed kernel (csrc/mlp16.hip).  Anything else (another num_stack, PIME_STATE_F64 / MIXED16): PIME_ERR_ARG.
 *   packed_actor  pime_mlp_pack image of kind PIME_MLP_CRITIC built from the TD3 Actor's tensors (net.py:96-110 has CriticAdv's
 *                 shape and ReLUs; the kernel applies the tanh), width md = 64 / 128 / 256
 *   obs           [dev] float32[N, obs_dim]: in = the lanes' current observation, out = the observation after the last step
 *   ring_state    [dev] float32[slots, N, obs_dim]; ring_other [dev] float32[slots, N, 3] = (reward * reward_scale, mask = 0 if done
 *                 else gamma, action); slots slot0 .. slot0 + n_steps - 1 (mod slots) are written: the successor of (slot, lane) is
 *                 (slot + 1, lane), where replay.py:344-351 uses row i + 1 */
int pime_rollout_offpolicy_supported(const pime_env* env, int32_t md);
int pime_rollout_offpolicy(pime_env* env, int32_t md, const float* packed_actor, const double* priorK, float explore_noise,
                           float gamma, float reward_scale, int32_t n_steps, uint64_t noise_seed, uint32_t noise_epoch,
                           float* obs, float* ring_state, float* ring_other, int32_t slot0, int32_t slots, pime_stream stream);
/* The same launch for AgentSAC -- replaces AgentBase.explore_env's body (elegantrl/agent.py:54-70) with AgentSAC.select_action
 * (:425-431) and ActorSAC.get_action (net.py:201-205): a = tanh(avg + exp(clamp(log_std, -20, 2)) * eps), eps the SAME Philox
 * stream-2 draw (counter (lane, noise_epoch, t)); the ring stores the squashed action.  packed_actor: pime_mlp_pack image of kind
 * PIME_MLP_SAC_ACTOR, width 64 / 128, pH or Integrator water tank only; everything else as pime_rollout_offpolicy. */
int pime_rollout_offpolicy_sac_supported(const pime_env* env, int32_t md);
int pime_rollout_offpolicy_sac(pime_env* env, int32_t md, const float* packed_actor, const double* priorK, float gamma,
                               float reward_scale, int32_t n_steps, uint64_t noise_seed, uint32_t noise_epoch, float* obs,
                               float* ring_state, float* ring_other, int32_t slot0, int32_t slots, pime_stream stream);

/* -- fused TD3 optimizer step ---------------------------------------------------------------------------------------
 * replaces, per iteration of AgentTD3.update_net's loop (elegantrl/agent.py:314-331): get_obj_critic_raw (:361-370 -- the gather of
 * buffer.sample_batch's rows (replay.py:344-351), act_target.get_action with clamped smoothing noise (net.py:107-110),
 * min(cri_target.get_q1_q2), q_label, cri.get_q1_q2, SmoothL1 x 2), obj_critic.backward(), cri_optimizer.step(), the delayed
 * soft_update(cri_target) (:116-124), obj_actor = -cri_target(state, act(state)).mean() (:323-324), obj_actor.backward(),
 * act_optimizer.step() and the delayed soft_update(act_target): FOUR launches (csrc/td3_fused.hip) -- critic gradients
 * (one 16-sample tile per workgroup, its four or eight waves splitting every layer's output features), slab reduction + Adam + soft
 * update of the critic, actor gradients (through the TARGET critic's first head, as the reference has it), the same for the actor.
 * Nets: Actor (net.py:96-110: D -> md ReLU -> md ReLU -> md ReLU -> 1, tanh) and CriticTwin (net.py:305-332: D+1 -> md ReLU -> md
 * ReLU, two linear heads), action_dim 1, 1 <= D <= 31, md 64 | 128 | 256 (width 256: the md x md weights streamed in k-slices,
 * the Stacking observations' first layers in eight k-steps).  The weights are read where they live: every net is ONE flat
 * float32 tensor in nn.Module parameter order with each tensor starting on a multiple of 4 floats (pime_td3_param_offsets;
 * padding words zero) -- no packed images, nothing to re-pack after a step. */
typedef struct pime_td3_net {
    float* param;        /* [dev] float32[pime_td3_param_floats]: the online net */
    float* target;       /* [dev] same layout: the target net (soft-updated in place) */
    float* grad;         /* [dev] same layout, WRITTEN: this step's gradient (the reference's .grad after backward()) */
    float* exp_avg;      /* [dev] Adam state, same layout; zero at construction */
    float* exp_avg_sq;
    const float* step;   /* [dev] float32[1]: optimizer steps applied BEFORE table row 0; a call is Adam step number step[0] + row + 1.
                          * The CALLER adds the number of steps behind an update (one stream-ordered add per update_net) */
    float lr, beta1, beta2, eps;
} pime_td3_net;
typedef struct pime_td3_batch {
    const float* state;      /* [dev] float32[rows, D]: replay states (ReplayBuffer.buf_state / VecReplayBuffer.buf_state) */
    const float* other;      /* [dev] float32[rows, 3]: reward * scale, mask, action (buf_other) */
    const int64_t* idx;      /* [dev] int64[table_rows, B]: the sampled rows of every optimizer step of an update */
    const int64_t* nxt;      /* [dev] int64[table_rows, B]: their successors (idx + 1 in the flat ring, idx + N lanes in the vector ring) */
    const float* noise;      /* [dev] float32[table_rows, B] standard normal draws of the smoothing noise (torch.randn_like), or NULL:
                              * drawn in the kernel -- Philox4x32-10 keyed by noise_seed, counter (batch position, noise_epoch,
                              * table row, stream 3), Box-Muller cosine branch in float32 */
    int64_t row;             /* the table row of THIS optimizer step.  A launch argument, not device state: every node of a captured
                              * update graph carries its own row, so no launch has to advance a shared cursor */
    const int64_t* epoch;    /* [dev] int64[1] or NULL: added to noise_epoch (the host bumps it once per update, so that a captured
                              * HIP graph draws fresh noise in every replay) */
    int32_t B;
    uint64_t noise_seed;
    uint32_t noise_epoch;
    float policy_noise, noise_clip;   /* 0.2, 0.5 (agent.py:281, net.py:109) */
} pime_td3_batch;
int pime_td3_supported(int32_t D, int32_t action_dim, int32_t md);
/* which: 0 actor, 1 critic.  offsets [8]: float offset of every parameter tensor (W, b pairs in module order) */
int64_t pime_td3_param_floats(int32_t which, int32_t D, int32_t md);
int pime_td3_param_offsets(int32_t which, int32_t D, int32_t md, int32_t* offsets);
int64_t pime_td3_workspace_floats(int32_t D, int32_t md, int32_t B);
/* soft_mode: 0 no soft target update, 1 soft update, 2 soft update when row % update_freq == 0 (the reference's delayed update).
 * phases: bit 0 = critic gradients, bit 1 = critic apply (slab reduction, Adam, soft update), bit 2 = actor gradients, bit 3 = actor
 *         apply; 15 = the whole step.  The launches of consecutive calls sharing a workspace run in stream order: the actor gradients
 *         of a row read the state rows that the critic gradients of the same row gathered into the workspace, and the critic
 *         gradients of the next row overwrite them.
 *         Data-parallel callers split the two apply launches around their all-reduce (mean) of the net's `grad` tensor: 16 = critic slab
 *         reduction ONLY (grad = this rank's gradient, loss words), 32 = critic Adam (+ soft update) FROM `grad` (no slabs read); 64 / 128
 *         the same for the actor.  One optimizer step on G ranks: phases 1|16, all-reduce critic grad, phases 32|4|64, all-reduce actor
 *         grad, phases 128 (order inside a call: 1, 2|16, 32, 4, 8|64, 128; 2 with 16 or 8 with 64 is PIME_ERR_ARG).
 * loss [dev] float32[4] or NULL: [0] += obj_actor, [1] += obj_critic of this step (zero them per update), [2], [3] = this step's values.
 * workspace [dev] float32[pime_td3_workspace_floats]. */
int pime_td3_step(int32_t D, int32_t md, const pime_td3_net* actor, const pime_td3_net* critic, const pime_td3_batch* batch,
                  float tau, int32_t update_freq, int32_t soft_mode, int32_t phases, float* workspace, float* loss,
                  pime_stream stream);

/* -- fused SAC optimizer step ---------------------------------------------------------------------------------------
 * replaces, per iteration of AgentSAC.update_net's loop (elegantrl/agent.py:442-468): get_obj_critic_raw (:519-527 -- the gather of
 * buffer.sample_batch's rows (replay.py:344-351), act.get_action_logprob(next_s) on the ONLINE actor (net.py:207-239),
 * min(cri_target.get_q1_q2) + next_logprob * alpha, q_label, cri.get_q1_q2, SmoothL1 x 2), obj_critic.backward(),
 * cri_optimizer.step(), soft_update(cri_target) on every step (:116-124), act.get_action_logprob(state), obj_alpha and
 * alpha_optimizer.step() (:452-458), alpha = exp(alpha_log) (:461), obj_actor = -(min(cri_target.get_q1_q2(state, a_pg)) +
 * logprob * alpha).mean() (:463), obj_actor.backward(), act_optimizer.step(): FOUR launches (csrc/sac_fused.hip) -- critic gradients
 * (which also leave the batch sum of the policy-gradient sample's logprob), slab reduction + Adam + soft update of the critic +
 * the temperature's Adam step, actor gradients (through BOTH heads of the target critic, min per sample, with the new alpha), slab
 * reduction + Adam of the actor.  "logprob" is the reference's NEGATIVE log-density, kept with its sign.
 * Nets: ActorSAC (net.py:175-239, non-DenseNet: D -> md ReLU -> md Hardswish -> md Hardswish, heads net_a_avg / net_a_std) and
 * CriticTwin (net.py:305-332), action_dim 1, 1 <= D <= 7, md 64 | 128.  Both are read where they live: ONE flat float32 tensor per net
 * in nn.Module parameter order, each tensor on a multiple of 4 floats, padding words zero (the actor: pime_sac_param_offsets, ten
 * tensors; the critic: pime_td3_param_offsets(1, ...)).  The nets are described by pime_td3_net; the actor's `target` is unused and
 * may be NULL (SAC has no actor target). */
typedef struct pime_sac_temperature {
    float* alpha_log;     /* [dev] float32[1]: the trainable log-temperature (agent.py:408), stepped by the critic's apply launch */
    float* exp_avg;       /* [dev] float32[1]: its Adam moments; zero at construction */
    float* exp_avg_sq;
    float lr, beta1, beta2, eps;   /* the step number is the nets': pime_td3_net.step[0] + row + 1 */
    float target_entropy;          /* agent.py:403,407: 1.0 * log(action_dim) = 0 */
} pime_sac_temperature;
typedef struct pime_sac_batch {
    const float* state;        /* [dev] float32[rows, D]: replay states */
    const float* other;        /* [dev] float32[rows, 3]: reward * scale, mask, action */
    const int64_t* idx;        /* [dev] int64[table_rows, B]: the sampled rows of every optimizer step of an update */
    const int64_t* nxt;        /* [dev] int64[table_rows, B]: their successors */
    const float* noise_next;   /* [dev] float32[table_rows, B]: the standard normal draws of the next-state sample (the first */
    const float* noise_pg;     /*   torch.randn_like of an iteration) and of the policy-gradient sample (the second); or BOTH NULL: drawn
                                *   in the kernels -- Philox4x32-10 keyed by noise_seed, counter (batch position, noise_epoch, table row,
                                *   stream 4 / 5), Box-Muller cosine branch in float32 */
    int64_t row;               /* the table row of THIS optimizer step: a launch argument, so that an update's steps sit in one graph */
    const int64_t* epoch;      /* [dev] int64[1] or NULL: added to noise_epoch (bumped by the host once per update) */
    int32_t B;
    uint64_t noise_seed;
    uint32_t noise_epoch;
} pime_sac_batch;
int pime_sac_supported(int32_t D, int32_t action_dim, int32_t md);
/* the actor's flat size, and offsets [10]: float offset of every parameter tensor (W, b pairs in module order) */
int64_t pime_sac_param_floats(int32_t D, int32_t md);
int pime_sac_param_offsets(int32_t D, int32_t md, int32_t* offsets);
int64_t pime_sac_workspace_floats(int32_t D, int32_t md, int32_t B);
/* phases: bit 0 = critic gradients, bit 1 = critic apply (slab reduction, Adam, soft update with tau, temperature step), bit 2 = actor
 *         gradients, bit 3 = actor apply; 15 = the whole step.  Launches of consecutive calls sharing a workspace run in stream order.
 * loss [dev] float32[8] or NULL: [0] += obj_actor, [1] += obj_critic, [2] += obj_alpha, [3] += alpha of this step (zero them per
 *         update), [4..7] = this step's values.
 * workspace [dev] float32[pime_sac_workspace_floats].  Two calls on the same inputs give the same bits (fixed summation order). */
int pime_sac_step(int32_t D, int32_t md, const pime_td3_net* actor, const pime_td3_net* critic, const pime_sac_temperature* temp,
                  const pime_sac_batch* batch, float tau, int32_t phases, float* workspace, float* loss, pime_stream stream);

/* replaces: self.optimizer.step() of the single Adam over both nets (elegantrl/agent.py:565-566,656-657; no weight
 * decay, no amsgrad) when every parameter lives in ONE flat tensor.  All [dev] float32[n]; step [dev] float32[2], zeroed
 * by the caller at construction: step[0] is the step counter, incremented by the call on the device (so the launch can be
 * replayed from a HIP graph), step[1] is this optimizer's arrival counter (scratch).  One optimizer = one stream at a time;
 * different optimizers are independent. */
int pime_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, float* step, pime_stream stream);
/* pime_adam_step for the nets of a PPO agent, with opt->image_map set: every new parameter value is also written into the nets'
 * packed images, so no pime_ppo_repack follows.  For data-parallel callers, whose all-reduce sits between pime_ppo_minibatch_grad
 * and the optimizer step (single-GPU callers get the same from pime_ppo_minibatch_step in one launch less). */
int pime_adam_step_images(const pime_adam* opt, const pime_ppo_net* actor, const pime_ppo_net* critic, pime_stream stream);

/* The optimizer step of a data-parallel rank, behind the all-reduce (AVG) of [flat gradients | dp_moments]: the critic's elements
 * grad[critic_offset .. n) are first multiplied by 1 / (std + 1e-5), std = torch's unbiased std of the dp_world * B targets of the
 * UNION minibatch, recovered from the averaged moments (agent.py:652: `obj_critic / (r_sum.std() + 1e-5)`; actor and critic
 * parameters are disjoint and the united loss is linear in that factor, so scaling the averaged critic gradient is exact), written
 * back into grad, then torch.optim.Adam as pime_adam_step.  image_map may be NULL (then pime_ppo_repack follows). */
int pime_adam_step_dp(const pime_adam* opt, const pime_ppo_net* actor, const pime_ppo_net* critic, pime_stream stream);

/* -- one-shot all-reduce of the flat gradient buffer over peer-mapped memory ---------------------------------------------
 * replaces: nothing in the reference (one process; elegantrl/run.py:232-247 is an unused mp.Pipe) -- it is the hand-written
 * alternative to the RCCL all-reduce of SURVEY.md section 8(e) for the 270 KB gradient message: every rank writes its vector into
 * every peer's inbox (hipIpc-mapped, one write per xGMI link, all links at once), raises a flag, waits for its peers' flags and
 * sums the rows in rank order: one latency step, bit-identical results on every rank.  csrc/allreduce.hip has the protocol.
 * Life cycle, per rank (one process per GPU): create -> export the 64-byte handle -> exchange the handles of all ranks (any
 * transport: torch.distributed all_gather) -> connect -> allreduce_mean per optimizer step (one launch on the caller's stream,
 * HIP-graph capturable) -> destroy.  world <= 8.  A peer that never arrives does not hang the device: the kernel gives up after
 * ~2 s and pime_oneshot_status() returns non-zero -- which the caller must treat as fatal. */
typedef struct pime_oneshot pime_oneshot;
pime_oneshot* pime_oneshot_create(int32_t rank, int32_t world, int64_t n_floats, int32_t device);
int pime_oneshot_export(pime_oneshot* h, void* handle_out /* [host] 64 bytes */);
int pime_oneshot_connect(pime_oneshot* h, const void* handles /* [host] world x 64 bytes, rank order */);
/* data [dev] float32[n_floats]: replaced by the mean over the ranks */
int pime_oneshot_allreduce_mean(pime_oneshot* h, float* data, pime_stream stream);
/* 0: every call so far completed.  Non-zero: a peer's rows did not arrive within ~2 s (1) or the local grid barrier timed out (2) --
 * the launch then left `data` partly or wholly UN-averaged: treat it as fatal (the replicas have diverged); the Python side checks it
 * at the end of every update and raises on every rank.  Synchronises the device. */
int pime_oneshot_status(pime_oneshot* h);
/* info [host] int32[5]: [0] 1 = the region is fine-grained memory (required between DIFFERENT devices), 0 = the runtime fell back to
 * coarse-grained memory (valid only between processes sharing one device); [1] device ordinal; [2..4] PCI domain / bus / device. */
int pime_oneshot_info(pime_oneshot* h, int32_t* info);
void pime_oneshot_destroy(pime_oneshot* h);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PIME_HIP_H */
