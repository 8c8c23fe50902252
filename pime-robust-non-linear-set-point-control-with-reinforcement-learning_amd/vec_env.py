"""Vectorised pH-process and water-tank envs: N independent instances advanced by one HIP launch per step.

This is the build's extension of the reference's one-instance envs (SURVEY.md §8b "vectorised extension"); the
per-instance semantics are the reference's (/root/reference/gym_control/envs/ph.py,
nonlinear_watertank.py) and live in csrc/env_kernels.hip.  Everything here is host-side plumbing: handle
ownership, tensor allocation, and the *draw sources* that decide where an episode's random numbers come from:

  PhiloxDraws      in-kernel Philox4x32-10 keyed by (seed, global env id, episode, slot)   -- throughput mode
  Mt19937Draws     per-env emulation of the reference's two MT19937 streams, env i seeded with base+i,
                   generated on the host and injected into the kernels                    -- seed-for-seed mode
  (the 1-instance facades in gym_control/ inject draws taken from the *global* np.random exactly where the
   reference takes them)

There is no CPU implementation: constructing an env without a gfx950 device raises `native.PimeError`.
"""
import ctypes as C

import numpy as np
import torch

from . import gym_compat, native

_STATE_MODES = {"f64": native.STATE_F64, "mixed": native.STATE_MIXED, "mixed16": native.STATE_MIXED16}


# ------------------------------------------------------------------------------------------------ draw sources
class PhiloxDraws:
    """Counter-based in-kernel draws; nothing to do on the host."""
    injects = False

    def reset_draws(self, env, lanes):
        return None

    def step_noise(self, env):
        return None

    def reseed(self, base):
        raise native.PimeError("Philox mode is keyed at construction: pass seed= to the env")


class Mt19937Draws:
    """Reference-compatible streams: env i behaves like the reference env after
    `env.seed(base+i); np.random.seed(base+i)` (train.py:105-106).

    pH  : ensemble params from the global stream (ph.py:410), x0 then r from gym's np_random (ph.py:420,424).
    WT  : everything from the global stream (nonlinear_watertank.py:891-893,912-913,271-272), including the two
          per-step normals, in call order.
    """
    injects = True

    def __init__(self, base_seed, num_envs, env_offset=0):
        self.num_envs = num_envs
        self.env_offset = env_offset
        self.reseed(base_seed)

    def reseed(self, base):
        ids = [int(base) + self.env_offset + i for i in range(self.num_envs)]
        self.global_rs = [np.random.RandomState(s) for s in ids]
        self.env_rs = [gym_compat.np_random(s)[0] for s in ids]

    def reset_draws(self, env, lanes):
        out = np.zeros((self.num_envs, env.draw_width), dtype=np.float64)
        for i in lanes:
            out[i] = env._draw_episode(self.global_rs[i], self.env_rs[i])
        return out

    def step_noise(self, env):
        if not env.has_step_noise:
            return None
        out = np.empty((self.num_envs, 2), dtype=np.float64)
        s = env.noise_scale
        for i, rs in enumerate(self.global_rs):
            out[i, 0] = rs.normal(loc=0., scale=s)  # get_noise(): nonlinear_watertank.py:271-272, h1 then h2
            out[i, 1] = rs.normal(loc=0., scale=s)
        return out


class CallbackDraws:
    """Draws supplied by callables (used by the 1-instance facades to read the process-global np.random)."""
    injects = True

    def __init__(self, episode_fn, noise_fn=None):
        self.episode_fn, self.noise_fn = episode_fn, noise_fn

    def reset_draws(self, env, lanes):
        out = np.zeros((env.num_envs, env.draw_width), dtype=np.float64)
        for i in lanes:
            out[i] = self.episode_fn(i)
        return out

    def step_noise(self, env):
        if not env.has_step_noise or self.noise_fn is None:
            return None
        return np.asarray([self.noise_fn(i) for i in range(env.num_envs)], dtype=np.float64).reshape(-1, 2)

    def reseed(self, base):
        pass


# ------------------------------------------------------------------------------------------------ base class
# image kinds the fused evaluation kernels take as a policy ("critic": the TD3 Actor, whose image has CriticAdv's shape and ReLUs)
def check_perturb(perturb):
    """The rows of `VecControlEnv.margin_sweep` as float64 [P, 3], or ValueError: the shape, a non-finite gain, a delay that is not an
    integer in 0 .. native.MARGIN_MAX_DELAY, a sigma that is negative or not finite."""
    rows = np.asarray(perturb.detach().cpu().numpy() if torch.is_tensor(perturb) else perturb, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != native.PERTURB_COLS or rows.shape[0] < 1:
        raise ValueError(f"margin_sweep: perturb {tuple(rows.shape)} must be [P >= 1, {native.PERTURB_COLS}]")
    g, d, sg = rows[:, 0], rows[:, 1], rows[:, 2]
    if not np.all(np.isfinite(g)):
        raise ValueError("margin_sweep: a gain is not finite")
    if not np.all(np.isfinite(d)) or np.any(d != np.rint(d)) or np.any(d < 0) or np.any(d > native.MARGIN_MAX_DELAY):
        raise ValueError(f"margin_sweep: a delay is not an integer in 0 .. {native.MARGIN_MAX_DELAY}")
    if not np.all(np.isfinite(sg)) or np.any(sg < 0):
        raise ValueError("margin_sweep: a sigma is negative or not finite")
    return np.ascontiguousarray(rows)


def check_disturb(rows, is_ph):
    """The rows of `VecControlEnv.disturbance_sweep` as float64 [P, 6] (columns native.DISTURB_COL_NAMES), or ValueError: the shape, an
    onset or a length that is not a non-negative integer, a load that is not finite, a multiplier that is not finite and > 0, M2 != 1
    on pH (it has two plant parameters)."""
    rows = np.asarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != native.DISTURB_COLS or rows.shape[0] < 1:
        raise ValueError(f"disturbance_sweep: rows {tuple(rows.shape)} must be [P >= 1, {native.DISTURB_COLS}]")
    for j, name in ((0, "onset"), (1, "length")):
        v = rows[:, j]
        if not np.all(np.isfinite(v)) or np.any(v != np.rint(v)) or np.any(v < 0):
            raise ValueError(f"disturbance_sweep: {name} must be a non-negative integer")
    if not np.all(np.isfinite(rows[:, 2])):
        raise ValueError("disturbance_sweep: a load is not finite")
    m = rows[:, 3:6]
    if not np.all(np.isfinite(m)) or np.any(m <= 0):
        raise ValueError("disturbance_sweep: a multiplier is not finite and > 0")
    if is_ph and np.any(rows[:, 5] != 1.0):
        raise ValueError("disturbance_sweep: m2 must be 1 on pH (two plant parameters: qww_V, qc_V)")
    return np.ascontiguousarray(rows)


def check_actuator(rows):
    """The rows of `VecControlEnv.actuator_sweep` as float64 [P, 6] (columns native.ACT_COL_NAMES), or ValueError: the shape, a limit
    that is NaN, lo > hi, a rate, dead-band or quantum that is NaN or negative, a quantum that is infinite.  Off is spelled lo = -inf,
    hi = +inf, rate = inf (or 0) and 0 for the dead-band and the quanta."""
    rows = np.asarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != native.ACT_COLS or rows.shape[0] < 1:
        raise ValueError(f"actuator_sweep: rows {tuple(rows.shape)} must be [P >= 1, {native.ACT_COLS}]")
    lo, hi = rows[:, 0], rows[:, 1]
    if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(lo > hi):
        raise ValueError("actuator_sweep: a limit is NaN or lo > hi")
    for j, name in ((2, "rate"), (3, "deadband"), (4, "qu"), (5, "qy")):
        v = rows[:, j]
        if np.any(np.isnan(v)) or np.any(v < 0) or (j >= 4 and np.any(np.isinf(v))):
            raise ValueError(f"actuator_sweep: {name} is NaN, negative or an infinite quantum")
    return np.ascontiguousarray(rows)


def check_excite(rows, wave, L):
    """The rows and the table of `VecControlEnv.frequency_sweep` as float64 [P, 3] (columns native.FREQ_COL_NAMES) and [P, L, 2], or
    ValueError: a shape, a point that is not 0, 1 or 2, an amplitude that is not finite, an onset that is not a non-negative integer,
    a table entry that is not finite."""
    rows = np.asarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows, dtype=np.float64)
    wave = np.asarray(wave.detach().cpu().numpy() if torch.is_tensor(wave) else wave, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != native.FREQ_COLS or rows.shape[0] < 1:
        raise ValueError(f"frequency_sweep: rows {tuple(rows.shape)} must be [P >= 1, {native.FREQ_COLS}]")
    if wave.shape != (rows.shape[0], int(L), 2):
        raise ValueError(f"frequency_sweep: wave {tuple(wave.shape)} must be [P = {rows.shape[0]}, L = {int(L)}, 2]")
    pt, amp, k0 = rows[:, 0], rows[:, 1], rows[:, 2]
    if not np.all(np.isin(pt, tuple(float(v) for v in native.FREQ_POINTS.values()))):
        raise ValueError(f"frequency_sweep: point must be one of {native.FREQ_POINTS}")
    if not np.all(np.isfinite(amp)):
        raise ValueError("frequency_sweep: an amplitude is not finite")
    if not np.all(np.isfinite(k0)) or np.any(k0 != np.rint(k0)) or np.any(k0 < 0):
        raise ValueError("frequency_sweep: onset must be a non-negative integer")
    if not np.all(np.isfinite(wave)):
        raise ValueError("frequency_sweep: a wave entry is not finite")
    return np.ascontiguousarray(rows), np.ascontiguousarray(wave)


_EVAL_KINDS ={"modular_actor": native.MLP_MODULAR_ACTOR, "plain_actor": native.MLP_PLAIN_ACTOR, "sac_actor": native.MLP_SAC_ACTOR,
               "critic": native.MLP_CRITIC}


class VecControlEnv:
    """Common host logic of the two env families.  Tensors returned by reset/step live on `device`."""
    kind = None
    field_prefix = ""
    draw_width = 0
    has_step_noise = False
    action_dim = 1
    if_discrete = False

    def __init__(self, cfg, device, draws, K):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise native.PimeError(f"pime_amd envs run on a gfx950 GPU only (got device '{device}'); there is no "
                                   "CPU fallback")
        if self.device.index is None:  # "cuda" -> the concrete ordinal, so tensor.device comparisons are exact
            self.device = torch.device("cuda", torch.cuda.current_device())
        cfg.device_id = self.device.index
        self._lib = native.lib()
        with torch.cuda.device(self.device):
            self._h = C.c_void_p(self._lib.pime_env_create(C.byref(cfg)))
        if not self._h:
            raise native.PimeError(f"pime_env_create failed: {native.last_error()}")
        self.cfg = cfg
        self.num_envs = int(cfg.n_envs)
        self.state_dim = self.obs_dim = int(self._lib.pime_env_obs_dim(self._h))
        self.max_step = int(cfg.max_steps)
        self.draws = draws
        self.K = np.asarray(K, dtype=np.float64)
        self.action_max = 1.0
        self.target_return = 2 ** 16
        N, D = self.num_envs, self.obs_dim
        self.obs = torch.zeros((N, D), dtype=torch.float32, device=self.device)
        self.reward = torch.zeros((N,), dtype=torch.float32, device=self.device)
        self.done = torch.zeros((N,), dtype=torch.uint8, device=self.device)
        # Host mirror of the per-lane step counter (episodes are fixed length, so the host can tell which lanes end
        # without reading the device).  While every lane is at the same step -- the normal case -- it is ONE integer;
        # a masked reset or a write to the `t` field switches to a per-lane array.
        self._t_all = 0
        self._t_lanes = None
        self._was_reset = False
        self.reset_count = 0   # host-initiated resets so far: lets a caller that caches observations across calls (the
        #                        off-policy agents) notice that someone else -- the evaluator -- reset the env in between

    def clone(self, **overrides):
        """A second, independent env of the same configuration (own handle, own state slab): `copy.deepcopy` for an env whose
        state lives in HBM.  Used to give an off-policy run its own evaluation env (run.py: the evaluator resets the env it is
        given, which must not be the one whose running episodes the agent continues)."""
        env = type(self)(**{**self._ctor, **overrides})
        for k in ("env_name", "target_return"):
            if hasattr(self, k):
                setattr(env, k, getattr(self, k))
        return env

    # -- lifetime ------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            native.destroy_handle(self._lib.pime_env_destroy, self._h)   # parked, not freed, while a stream capture is open
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev64(self, host):
        return None if host is None else torch.as_tensor(np.ascontiguousarray(host), dtype=torch.float64).to(
            self.device, non_blocking=False)

    # -- gym-like API --------------------------------------------------------------------------------------
    def seed(self, seed=None):
        """Env i uses seed+i.  Only meaningful for injected (MT19937) draws; Philox is keyed at construction."""
        if seed is not None and self.draws.injects:
            self.draws.reseed(seed)
        return [seed]

    def reset(self, mask=None, out=None):
        """Reset the lanes selected by `mask` (bool/uint8 [N], host or device; None = all).  Returns obs [N, D]."""
        obs = self.obs if out is None else out
        if mask is None:
            lanes, mask_dev = range(self.num_envs), None
            self._t_all, self._t_lanes = 0, None
        else:
            m = torch.as_tensor(mask).to(torch.uint8)
            lanes = np.nonzero(m.cpu().numpy())[0]
            mask_dev = m.to(self.device)
            self._lane_steps()[lanes] = 0
        draws = self._dev64(self.draws.reset_draws(self, lanes)) if self.draws.injects else None
        native.check(self._lib.pime_env_reset(self._h, native.ptr(mask_dev), native.ptr(draws), native.ptr(obs),
                                              self._stream()), "pime_env_reset")
        self._was_reset = True
        self.reset_count += 1
        return obs

    def _lane_steps(self):
        """Per-lane view of the step mirror (materialised on first need)."""
        if self._t_lanes is None:
            self._t_lanes = np.full(self.num_envs, self._t_all, dtype=np.int64)
        return self._t_lanes

    def _pre_step(self, auto_reset):
        noise = self._dev64(self.draws.step_noise(self)) if self.draws.injects else None
        if self._t_lanes is None:                      # lock-step fast path: O(1) host work per launch
            self._t_all += 1
            ending = range(self.num_envs) if self._t_all >= self.max_step else ()
            if auto_reset and len(ending):
                self._t_all = 0
        else:
            self._t_lanes += 1
            ending = np.nonzero(self._t_lanes >= self.max_step)[0]
            if auto_reset and len(ending):
                self._t_lanes[ending] = 0
                if not self._t_lanes.any():
                    self._t_all, self._t_lanes = 0, None   # back in lock-step
        reset_draws = None
        if auto_reset and len(ending) and self.draws.injects:
            reset_draws = self._dev64(self.draws.reset_draws(self, ending))
        return noise, reset_draws

    def step(self, action, auto_reset=True, out_obs=None, out_reward=None, out_done=None):
        """action: [N] or [N,1] tensor (float32 or float64) of env actions.  Returns (obs, reward, done)."""
        a = action.reshape(-1)
        if a.dtype not in (torch.float32, torch.float64):
            a = a.to(torch.float32)
        a = a.contiguous()
        assert a.numel() == self.num_envs and a.device == self.device, "action must be an [N] tensor on the env device"
        obs = self.obs if out_obs is None else out_obs
        rew = self.reward if out_reward is None else out_reward
        done = self.done if out_done is None else out_done
        noise, reset_draws = self._pre_step(auto_reset)
        native.check(self._lib.pime_env_step(self._h, native.ptr(a), native.F32 if a.dtype == torch.float32 else native.F64,
                                             native.ptr(noise), int(auto_reset), native.ptr(reset_draws), native.ptr(obs),
                                             native.ptr(rew), native.ptr(done), self._stream()), "pime_env_step")
        return obs, rew, done

    def step_residual(self, a_pre, obs_in, priorK=None, auto_reset=True, out_obs=None, out_reward=None, out_done=None):
        """env.step(tanh(a_pre) + obs_in @ priorK) with the composition fused into the kernel
        (elegantrl/agent_residual.py:61).  a_pre [N] float32, obs_in [N, D] float32 (may alias nothing written)."""
        a = a_pre.reshape(-1).to(torch.float32).contiguous()
        obs_in = obs_in.contiguous()
        assert obs_in.dtype == torch.float32 and tuple(obs_in.shape) == (self.num_envs, self.obs_dim)
        k = np.ascontiguousarray(-self.K if priorK is None else np.asarray(priorK, dtype=np.float64).reshape(-1))
        assert k.size == self.obs_dim
        obs = self.obs if out_obs is None else out_obs
        assert obs.data_ptr() != obs_in.data_ptr(), "obs_in and the output obs must not alias"
        rew = self.reward if out_reward is None else out_reward
        done = self.done if out_done is None else out_done
        noise, reset_draws = self._pre_step(auto_reset)
        native.check(self._lib.pime_env_step_residual(self._h, native.ptr(a), native.ptr(obs_in), native.ptr(k),
                                                      native.ptr(noise), int(auto_reset), native.ptr(reset_draws),
                                                      native.ptr(obs), native.ptr(rew), native.ptr(done), self._stream()),
                     "pime_env_step_residual")
        return obs, rew, done

    # -- binary16 observation / reward buffers (state_mode "mixed16": BASELINE.json config 5) -----------------------------
    def _half_buffers(self):
        if getattr(self, "_obs_h", None) is None:
            if self.cfg.state_mode != native.STATE_MIXED16:
                raise native.PimeError("binary16 observations need state_mode='mixed16'")
            N, D = self.num_envs, self.obs_dim
            self._obs_h = torch.zeros((N, D), dtype=torch.float16, device=self.device)
            self._reward_h = torch.zeros((N,), dtype=torch.float16, device=self.device)
        return self._obs_h, self._reward_h

    def reset_h(self, mask=None, out=None):
        """`reset` writing float16 observations (pime_env_reset_h)."""
        obs = self._half_buffers()[0] if out is None else out
        assert obs.dtype == torch.float16
        if mask is None:
            lanes, mask_dev = range(self.num_envs), None
            self._t_all, self._t_lanes = 0, None
        else:
            m = torch.as_tensor(mask).to(torch.uint8)
            lanes = np.nonzero(m.cpu().numpy())[0]
            mask_dev = m.to(self.device)
            self._lane_steps()[lanes] = 0
        draws = self._dev64(self.draws.reset_draws(self, lanes)) if self.draws.injects else None
        native.check(self._lib.pime_env_reset_h(self._h, native.ptr(mask_dev), native.ptr(draws), native.ptr(obs),
                                                self._stream()), "pime_env_reset_h")
        self._was_reset = True
        self.reset_count += 1
        return obs

    def step_h(self, action, auto_reset=True, out_obs=None, out_reward=None, out_done=None):
        """`step` with float16 observation / reward buffers (pime_env_step_h); action float32 [N]."""
        a = action.reshape(-1).to(torch.float32).contiguous()
        obs_h, rew_h = self._half_buffers()
        obs = obs_h if out_obs is None else out_obs
        rew = rew_h if out_reward is None else out_reward
        done = self.done if out_done is None else out_done
        noise, reset_draws = self._pre_step(auto_reset)
        native.check(self._lib.pime_env_step_h(self._h, native.ptr(a), native.ptr(noise), int(auto_reset), native.ptr(reset_draws),
                                               native.ptr(obs), native.ptr(rew), native.ptr(done), self._stream()),
                     "pime_env_step_h")
        return obs, rew, done

    def step_residual_h(self, a_pre, obs_in, priorK=None, auto_reset=True, out_obs=None, out_reward=None, out_done=None):
        """`step_residual` with float16 buffers: obs_in is the float16 observation the policy saw (pime_env_step_residual_h)."""
        a = a_pre.reshape(-1).to(torch.float32).contiguous()
        obs_in = obs_in.contiguous()
        assert obs_in.dtype == torch.float16 and tuple(obs_in.shape) == (self.num_envs, self.obs_dim)
        k = np.ascontiguousarray(-self.K if priorK is None else np.asarray(priorK, dtype=np.float64).reshape(-1))
        obs_h, rew_h = self._half_buffers()
        obs = obs_h if out_obs is None else out_obs
        assert obs.data_ptr() != obs_in.data_ptr(), "obs_in and the output obs must not alias"
        rew = rew_h if out_reward is None else out_reward
        done = self.done if out_done is None else out_done
        noise, reset_draws = self._pre_step(auto_reset)
        native.check(self._lib.pime_env_step_residual_h(self._h, native.ptr(a), native.ptr(obs_in), native.ptr(k),
                                                        native.ptr(noise), int(auto_reset), native.ptr(reset_draws),
                                                        native.ptr(obs), native.ptr(rew), native.ptr(done), self._stream()),
                     "pime_env_step_residual_h")
        return obs, rew, done

    @property
    def fresh(self):
        """True when every lane is at step 0 of an episode (just reset, or auto-reset by the last step)."""
        return self._was_reset and (self._t_all == 0 if self._t_lanes is None else not self._t_lanes.any())

    def observe(self, out=None):
        obs = self.obs if out is None else out
        native.check(self._lib.pime_env_observe(self._h, native.ptr(obs), self._stream()), "pime_env_observe")
        return obs

    @property
    def supports_fused_rollout(self):
        """The one-launch-per-episode rollout kernel needs mixed-precision state (float32 words, or binary16 storage: "mixed16")
        and in-kernel (Philox) draws; which observation / actor shapes it serves is the library's answer (`rollout_supported`)."""
        return self.cfg.state_mode in (native.STATE_MIXED, native.STATE_MIXED16) and not self.draws.injects

    @property
    def trajectory_dtype(self):
        """dtype of the observation / reward rows this env hands to a trajectory buffer: float16 in state_mode "mixed16"
        (BASELINE.json config 5 "fp16 state"), else float32."""
        return torch.float16 if self.cfg.state_mode == native.STATE_MIXED16 else torch.float32

    def rollout_supported(self, packed_actor):
        """Does the fused rollout kernel serve this env with this packed actor (kind / width)?  (pime_rollout_supported)"""
        kind = native.MLP_MODULAR_ACTOR if packed_actor.kind == "modular_actor" else native.MLP_PLAIN_ACTOR
        return self.supports_fused_rollout and bool(self._lib.pime_rollout_supported(self._h, kind, int(packed_actor.md)))

    def rollout(self, packed_actor, a_std_log, priorK, n_steps, noise_seed, noise_epoch, state, action, noise, reward, done):
        """Advance every lane `n_steps` steps under the packed residual policy in ONE launch (csrc/rollout.hip):
        state [n_steps+1, N, D] (slot 0 = current observation), action / noise / reward [n_steps, N], done uint8.
        Requires whole episodes from a fresh env (every lane at step 0), like AgentResidual*.explore_env collects."""
        assert self.fresh and n_steps % self.max_step == 0, "fused rollout advances whole episodes from a fresh env"
        for t_ in (state, action, noise, reward, done):
            assert t_.is_contiguous() and t_.device == self.device
        k = np.ascontiguousarray(np.asarray(priorK, dtype=np.float64).reshape(-1))
        assert k.size == self.obs_dim and packed_actor.D == self.obs_dim
        assert state.dtype == reward.dtype == self.trajectory_dtype and action.dtype == noise.dtype == torch.float32
        fn = self._lib.pime_rollout_h if state.dtype == torch.float16 else self._lib.pime_rollout
        native.check(fn(
            self._h, native.MLP_MODULAR_ACTOR if packed_actor.kind == "modular_actor" else native.MLP_PLAIN_ACTOR,
            packed_actor.md, native.ptr(packed_actor.packed), native.ptr(a_std_log), native.ptr(k), int(n_steps),
            C.c_uint64(noise_seed), C.c_uint32(noise_epoch), native.ptr(state), native.ptr(action), native.ptr(noise),
            native.ptr(reward), native.ptr(done), self._stream()), "pime_rollout")
        # whole episodes with in-kernel auto-reset: every lane is back at step 0 of a new episode

    def offpolicy_rollout_supported(self, packed_actor):
        """Does the fused off-policy exploration kernel serve this env with this packed actor?  (The TD3 Actor: widths 64 / 128 /
        256 on pH, the Integrator tank and Stacking1 / 4 / 10; ActorSAC: widths 64 / 128 on pH and the Integrator tank.)"""
        if self.cfg.state_mode != native.STATE_MIXED or self.draws.injects or packed_actor.D != self.obs_dim:
            return False
        if packed_actor.kind == "sac_actor":   # ActorSAC: the re-parameterised sample instead of mean + clipped noise
            return bool(self._lib.pime_rollout_offpolicy_sac_supported(self._h, int(packed_actor.md)))
        return packed_actor.kind == "critic" and bool(self._lib.pime_rollout_offpolicy_supported(self._h, int(packed_actor.md)))

    def rollout_offpolicy(self, packed_actor, priorK, explore_noise, gamma, reward_scale, n_steps, noise_seed, noise_epoch, obs,
                          ring_state, ring_other, slot0):
        """`n_steps` lock-steps of every lane under the deterministic actor + clipped exploration noise in ONE launch, the
        transitions written into the device ring from slot `slot0` on (csrc/rollout_offpolicy.hip); `obs` [N, D] is read (the
        lanes' current observation) and overwritten with the observation after the last step.  The running episodes continue."""
        for t_ in (obs, ring_state, ring_other):
            assert t_.is_contiguous() and t_.device == self.device and t_.dtype == torch.float32
        slots = ring_state.shape[0]
        assert ring_state.shape == (slots, self.num_envs, self.obs_dim) and ring_other.shape == (slots, self.num_envs, 3)
        k = np.ascontiguousarray(np.asarray(priorK, dtype=np.float64).reshape(-1))
        assert k.size == self.obs_dim and self._was_reset
        if packed_actor.kind == "sac_actor":   # (explore_noise unused: the actor's own log-std head scales the draw)
            native.check(self._lib.pime_rollout_offpolicy_sac(
                self._h, int(packed_actor.md), native.ptr(packed_actor.packed), native.ptr(k), C.c_float(gamma), C.c_float(reward_scale),
                int(n_steps), C.c_uint64(noise_seed), C.c_uint32(noise_epoch), native.ptr(obs), native.ptr(ring_state),
                native.ptr(ring_other), int(slot0), int(slots), self._stream()), "pime_rollout_offpolicy_sac")
        else:
            native.check(self._lib.pime_rollout_offpolicy(
                self._h, int(packed_actor.md), native.ptr(packed_actor.packed), native.ptr(k), C.c_float(explore_noise), C.c_float(gamma),
                C.c_float(reward_scale), int(n_steps), C.c_uint64(noise_seed), C.c_uint32(noise_epoch), native.ptr(obs),
                native.ptr(ring_state), native.ptr(ring_other), int(slot0), int(slots), self._stream()), "pime_rollout_offpolicy")
        if self._t_lanes is None:     # host mirror of the step counters: auto-reset wraps them at max_step
            self._t_all = (self._t_all + n_steps) % self.max_step
        else:
            self._t_lanes = (self._t_lanes + n_steps) % self.max_step

    def eval_supported(self, packed_actor=None, trace=False, schedule=False):
        """Does the fused evaluation kernel serve this env (with this packed actor, or the prior controller alone)?
        (pime_rollout_eval_supported: 1 = everything, 2 = returns and trace but no set-point schedule -- a Stacking observation
        at width 256; float64 or mixed state, in-kernel draws).  A packed TD3 Actor (kind "critic") evaluates as tanh(net(s)).  `schedule`: the caller wants a set-point schedule."""
        if self.draws.injects:
            return False
        if packed_actor is None:
            level = self._lib.pime_rollout_eval_supported(self._h, -1, 0)
        else:
            if packed_actor.kind not in _EVAL_KINDS or packed_actor.D != self.obs_dim:
                return False
            kind = _EVAL_KINDS[packed_actor.kind]
            level = self._lib.pime_rollout_eval_supported(self._h, kind, int(packed_actor.md))
        return level == 1 or (level == 2 and not schedule)

    # -- the arguments the plant-grid calls share (rollout_eval*, prior_sweep, mpc_eval, margin_sweep) -------------
    def _prior_row(self, priorK):
        """priorK as the native calls read it: one contiguous float64 row of obs_dim gains."""
        k = np.ascontiguousarray(np.asarray(priorK, dtype=np.float64).reshape(-1))
        assert k.size == self.obs_dim
        return k

    @staticmethod
    def _actor_triple(packed_actor):
        """(kind, md, img) of a packed actor; None = the prior controller alone."""
        if packed_actor is None:
            return -1, 0, None
        return _EVAL_KINDS[packed_actor.kind], int(packed_actor.md), packed_actor.packed

    @staticmethod
    def _schedule(setpoints, n_steps, seg_len):
        """(sp, its pointer or None, its length, n_segments) of a set-point schedule; the caller keeps sp alive over the call."""
        sp = np.ascontiguousarray(np.asarray(setpoints if setpoints is not None else [], dtype=np.float64))
        n_seg = max(-(-int(n_steps) // int(seg_len)) if seg_len > 0 else 1, 1)
        return sp, native.ptr(sp) if sp.size else None, int(sp.size), n_seg

    def _lanes_advanced(self, n_steps):
        """After a call that stepped every lane n_steps without auto-reset: the lanes sit somewhere inside an episode, so the next
        rollout must reset first."""
        self._was_reset = False
        if self._t_lanes is None:
            self._t_all += n_steps
        else:
            self._t_lanes += n_steps

    def rollout_eval(self, packed_actor, priorK, n_steps, setpoints=None, seg_len=0, want_trace=False, ret=None):
        """`n_steps` steps of every lane under the deterministic residual policy in ONE launch (csrc/rollout_eval.hip; no
        exploration noise, no auto-reset): returns (ret float64 [N] = per-lane sum of rewards, accumulated into `ret` if given,
        trace float64 [n_steps, 6, N] or None).  packed_actor None = the prior controller alone.  setpoints / seg_len: a
        step-response schedule (see include/pime_hip.h).  The lanes are left mid-episode: reset before the next rollout."""
        k = self._prior_row(priorK)
        if ret is None:
            ret = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        trace = torch.empty((n_steps, 6, self.num_envs), dtype=torch.float64, device=self.device) if want_trace else None
        sp, sp_ptr, n_sp, _ = self._schedule(setpoints, n_steps, seg_len)
        kind, md, img = self._actor_triple(packed_actor)
        native.check(self._lib.pime_rollout_eval(self._h, kind, md, native.ptr(img), native.ptr(k), int(n_steps), int(seg_len),
                                                 sp_ptr, n_sp, native.ptr(ret), native.ptr(trace), self._stream()),
                     "pime_rollout_eval")
        self._lanes_advanced(n_steps)
        return ret, trace

    def rollout_eval_metrics(self, packed_actor, priorK, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, want_trace=False,
                             ret=None):
        """`rollout_eval` that also reduces the step response on the device (pime_rollout_eval_metrics): returns (ret, metrics,
        trace) with metrics float64 [n_segments, 8, N] -- per set-point segment and lane the rows native.METRIC_NAMES (IAE, ISE,
        ITAE, overshoot, settling step for `band`, steady-state error over the last `tail` steps, return, action variation;
        definitions in include/pime_hip.h).  n_segments = ceil(n_steps / seg_len), 1 without a schedule.  ret and trace (None
        unless `want_trace`) are what `rollout_eval` returns for the same launch."""
        k = self._prior_row(priorK)
        if ret is None:
            ret = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        sp, sp_ptr, n_sp, n_seg = self._schedule(setpoints, n_steps, seg_len)
        metrics = torch.empty((n_seg, native.METRIC_ROWS, self.num_envs), dtype=torch.float64, device=self.device)
        trace = torch.empty((n_steps, 6, self.num_envs), dtype=torch.float64, device=self.device) if want_trace else None
        kind, md, img = self._actor_triple(packed_actor)
        native.check(self._lib.pime_rollout_eval_metrics(
            self._h, kind, md, native.ptr(img), native.ptr(k), int(n_steps), int(seg_len), sp_ptr, n_sp, float(band), int(tail),
            native.ptr(ret), native.ptr(trace), native.ptr(metrics), self._stream()), "pime_rollout_eval_metrics")
        self._lanes_advanced(n_steps)
        return ret, metrics, trace

    def rollout_eval_band(self, packed_actor, priorK, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, group_lanes=None,
                          hist=None, want_trace=False, ret=None):
        """`rollout_eval_metrics` that also reduces every step across lanes (pime_rollout_eval_band): returns (ret, metrics, stats,
        hist, trace).  stats float64 [n_steps, 16, G]: row 4 * signal + stat over native.BAND_SIGNALS (controlled output y, error
        r - y, env action, reward) x native.BAND_STATS (sum, sum of squares, min, max) of the lanes of each group of `group_lanes`
        consecutive lanes (a positive multiple of 16; None: all lanes as one group), G = ceil(N / group_lanes).  hist: None, or
        (bins, lo, hi) -> uint32 counts [n_steps, G, bins] of y (stored in an int32 tensor; definitions in include/pime_hip.h).
        ret, metrics and trace are what `rollout_eval_metrics` returns for the same launch."""
        k = self._prior_row(priorK)
        if ret is None:
            ret = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        n_steps, seg_len = int(n_steps), int(seg_len)
        group_lanes = self.num_envs if group_lanes is None else int(group_lanes)
        kind, md, img = self._actor_triple(packed_actor)
        ws_bytes = int(self._lib.pime_rollout_eval_band_workspace_bytes(self._h, kind, md, n_steps, group_lanes))
        if ws_bytes < 0:
            raise native.PimeError(f"pime_rollout_eval_band_workspace_bytes: {native.last_error()}")
        groups = -(-self.num_envs // group_lanes) if group_lanes < self.num_envs else 1
        sp, sp_ptr, n_sp, n_seg = self._schedule(setpoints, n_steps, seg_len)
        metrics = torch.empty((n_seg, native.METRIC_ROWS, self.num_envs), dtype=torch.float64, device=self.device)
        stats = torch.empty((n_steps, native.BAND_ROWS, groups), dtype=torch.float64, device=self.device)
        workspace = torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device)
        trace = torch.empty((n_steps, 6, self.num_envs), dtype=torch.float64, device=self.device) if want_trace else None
        bins, lo, hi = (0, 0.0, 0.0) if hist is None else (int(hist[0]), float(hist[1]), float(hist[2]))
        counts = None if hist is None else torch.empty((n_steps, groups, max(bins, 0)), dtype=torch.int32, device=self.device)
        native.check(self._lib.pime_rollout_eval_band(
            self._h, kind, md, native.ptr(img), native.ptr(k), n_steps, seg_len, sp_ptr, n_sp, float(band), int(tail),
            native.ptr(ret), native.ptr(trace), native.ptr(metrics), group_lanes, native.ptr(stats), native.ptr(counts), bins, lo, hi,
            native.ptr(workspace), self._stream()), "pime_rollout_eval_band")
        self._lanes_advanced(n_steps)
        return ret, metrics, stats, counts, trace

    # -- replay of recorded runs (plant identification) ----------------------------------------------------------
    def replay_supported(self, mode="simulate"):
        """Does `replay_error` serve this env in this mode?  (pime_env_replay_supported: pH -- simulate only -- and the Integrator
        tank, float64 or mixed state.)"""
        return mode in native.REPLAY_MODES and bool(self._lib.pime_env_replay_supported(self._h, native.REPLAY_MODES[mode]))

    def replay_error(self, records, mode="simulate", skip=0, want_sim=False):
        """Every lane's plant run over every recorded run in ONE launch (pime_env_replay_error, csrc/replay_error.hip), the output
        error reduced on the device: returns (err float64 [E, 5, N] -- rows native.REPLAY_ROW_NAMES: per output channel the sum of
        squared errors and the largest absolute error over the steps >= `skip`, and the number of terms -- and sim float64
        [E, T, C, N], the simulated outputs after each step, or None).  records: dict with "action" [E, T] (the env actions as
        env.step received them), "output" [E, T + 1, C] (the measured outputs, row 0 before the first step; C = 1 pH, 2 tank; NaN = a
        gap) and, pH only, optionally "state0" [E] (the hidden x at row 0; without it x0 is derived from the first measurement);
        host arrays or device tensors.  mode "simulate": free run; "predict" (tank): every step from the measured state.  The env
        itself is read, never advanced: state, counters and observations are untouched (definitions in include/pime_hip.h)."""
        if mode not in native.REPLAY_MODES:
            raise native.PimeError(f"replay_error: unknown mode {mode!r} ({sorted(native.REPLAY_MODES)})")
        dev = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float64).to(self.device).contiguous()
        action, output, state0 = dev(records["action"]), dev(records["output"]), dev(records.get("state0"))
        C_out = int(self._lib.pime_env_replay_channels(self._h))
        if action.dim() != 2 or output.dim() != 3 or tuple(output.shape) != (action.shape[0], action.shape[1] + 1, C_out):
            raise native.PimeError(f"replay_error: action {tuple(action.shape)} must be [E, T] and output {tuple(output.shape)} "
                                   f"[E, T + 1, {C_out}]")
        E, T = int(action.shape[0]), int(action.shape[1])
        if state0 is not None and tuple(state0.shape) != (E,):
            raise native.PimeError(f"replay_error: state0 {tuple(state0.shape)} must be [E]")
        rec = native.ReplayRecords(action.data_ptr(), output.data_ptr(), None if state0 is None else state0.data_ptr(), E, T)
        err = torch.empty((E, native.REPLAY_ROWS, self.num_envs), dtype=torch.float64, device=self.device)
        sim = torch.empty((E, T, C_out, self.num_envs), dtype=torch.float64, device=self.device) if want_sim else None
        native.check(self._lib.pime_env_replay_error(self._h, C.byref(rec), native.REPLAY_MODES[mode], int(skip), native.ptr(err),
                                                     native.ptr(sim), self._stream()), "pime_env_replay_error")
        return err, sim

    # -- prior-gain sweep (robust tuning of the prior controller) --------------------------------------------------
    def prior_sweep_supported(self):
        """Does `prior_sweep` serve this env?  (pime_prior_sweep_supported: pH and the Integrator tank, float64 or mixed state,
        in-kernel draws.)"""
        return not self.draws.injects and bool(self._lib.pime_prior_sweep_supported(self._h))

    def prior_sweep(self, gains, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, want_pairs=False):
        """A grid of prior gains over every lane's plant in ONE call (pime_prior_sweep, csrc/prior_sweep.hip): every (gain row,
        lane) pair runs `n_steps` steps under the prior controller alone, a_env = obs @ gains[g] -- gains float64 [G, D] in the
        KERNELS' sign, priorK = -env.K -- from the lane state as it stands, and its step response is reduced to the rows of
        `rollout_eval_metrics` and each row across the lanes.  Returns summary float64 [G, n_segments, 8, 5] -- per gain, segment
        and metric row (native.METRIC_NAMES) the stats native.SWEEP_STATS over the lanes: sum, min, max, argmax (the lane of the
        maximum), finite (the number of finite values, the only ones that count) -- and, with `want_pairs`, (summary, pairs) with
        pairs float64 [n_segments, 8, G, N], the metrics of every pair.  setpoints / seg_len / band / tail: as
        `rollout_eval_metrics`.  The tank's process noise is keyed on the lane, so every gain meets the same disturbance on a plant.
        The env itself is read, never advanced (definitions in include/pime_hip.h)."""
        g = torch.as_tensor(gains, dtype=torch.float64).to(self.device).contiguous()
        if g.dim() != 2 or g.shape[1] != self.obs_dim or g.shape[0] < 1:
            raise native.PimeError(f"prior_sweep: gains {tuple(g.shape)} must be [G >= 1, {self.obs_dim}]")
        G, n_steps, seg_len = int(g.shape[0]), int(n_steps), int(seg_len)
        ws_bytes = int(self._lib.pime_prior_sweep_workspace_bytes(self._h, G, n_steps, seg_len))
        if ws_bytes < 0:
            raise native.PimeError(f"pime_prior_sweep_workspace_bytes: {native.last_error()}")
        sp, sp_ptr, n_sp, n_seg = self._schedule(setpoints, n_steps, seg_len)
        summary = torch.empty((G, n_seg, native.METRIC_ROWS, len(native.SWEEP_STATS)), dtype=torch.float64, device=self.device)
        pairs = torch.empty((n_seg, native.METRIC_ROWS, G, self.num_envs), dtype=torch.float64, device=self.device) if want_pairs else None
        # the workspace lives for this call only; it comes from torch's allocator, so under a capture (native.capture_guard around
        # torch.cuda.graph, as for every capture of this package) it is a block of the graph's private pool and dropping it frees nothing
        workspace = torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device)
        native.check(self._lib.pime_prior_sweep(
            self._h, native.ptr(g), G, n_steps, seg_len, sp_ptr, n_sp, float(band), int(tail), native.ptr(pairs), native.ptr(summary),
            native.ptr(workspace), self._stream()), "pime_prior_sweep")
        del workspace
        return (summary, pairs) if want_pairs else summary

    # -- receding-horizon benchmark controller ---------------------------------------------------------------------
    def mpc_supported(self):
        """Does `mpc_eval` serve this env?  (pime_mpc_eval_supported: pH and the Integrator tank, float64 or mixed state, in-kernel
        draws.)"""
        return not self.draws.injects and bool(self._lib.pime_mpc_eval_supported(self._h))

    def mpc_eval(self, horizon, passes=2, rho=0.0, model_plants=None, n_steps=1, seg_len=0, setpoints=None, band=0.05, tail=10,
                 trace=False):
        """Every lane's plant in closed loop with a non-linear receding-horizon controller on its own model, in ONE launch
        (pime_mpc_eval, csrc/mpc_eval.hip): per control step 64 constant-action candidates per pass (`passes` 1 .. 3, each pass 32 x
        finer around the last winner) are rolled `horizon` (1 .. 64) noise-free lane steps forward, the one with the smallest
        sum (y - r)^2 + rho (u - u_prev)^2 is applied to the true plant.  model_plants: None (the lane's own plant) or float64 [N, 3]
        (a1, a2, Kp), tank only: the plant the candidates are rolled on.  Returns metrics float64 [n_segments, 8, N] -- the rows of
        `rollout_eval_metrics`, comparable with it and with `prior_sweep` on the same lane state -- or, with `trace`, (metrics,
        actions, outputs), float64 [n_steps, N]: the applied action and the controlled output after each step.  setpoints / seg_len /
        band / tail: as `rollout_eval_metrics`.  The env itself is read, never advanced (definitions in include/pime_hip.h)."""
        n_steps, seg_len = int(n_steps), int(seg_len)
        model = None
        if model_plants is not None:
            model = torch.as_tensor(model_plants, dtype=torch.float64).to(self.device).contiguous()
            if tuple(model.shape) != (self.num_envs, 3):
                raise native.PimeError(f"mpc_eval: model_plants {tuple(model.shape)} must be [{self.num_envs}, 3]")
        sp, sp_ptr, n_sp, n_seg = self._schedule(setpoints, n_steps, seg_len)
        metrics = torch.empty((n_seg, native.METRIC_ROWS, self.num_envs), dtype=torch.float64, device=self.device)
        actions = torch.empty((max(n_steps, 0), self.num_envs), dtype=torch.float64, device=self.device) if trace else None
        outputs = torch.empty((max(n_steps, 0), self.num_envs), dtype=torch.float64, device=self.device) if trace else None
        native.check(self._lib.pime_mpc_eval(
            self._h, native.ptr(model), int(horizon), int(passes), float(rho), n_steps, seg_len, sp_ptr, n_sp, float(band), int(tail),
            native.ptr(metrics), native.ptr(actions), native.ptr(outputs), self._stream()), "pime_mpc_eval")
        return (metrics, actions, outputs) if trace else metrics

    # -- the row-grid sweeps: what margin_sweep, disturbance_sweep and frequency_sweep share ---------------------------------------------
    def _row_grid_supported(self, supported, packed_actor):
        """`supported` (pime_margin_sweep_supported, pime_disturb_sweep_supported) for this env with this packed actor, or with the
        prior controller alone."""
        if self.draws.injects:
            return False
        if packed_actor is None:
            return bool(supported(self._h, -1, 0))
        if packed_actor.kind not in _EVAL_KINDS or packed_actor.D != self.obs_dim:
            return False
        return bool(supported(self._h, _EVAL_KINDS[packed_actor.kind], int(packed_actor.md)))

    def _row_grid_sweep(self, fn, R, packed_actor, priorK, rows, own, n_steps, setpoints, seg_len, band, tail, want_pairs, want_trace,
                        before=(), commands=False):
        """The native call `fn` on the validated device tensor `rows` [P, columns]: R metric rows per pair and segment, `own` the
        call's own arguments between P and n_steps, `before` those between the rows and P, `commands` a third trace between actions
        and outputs (pime_actuator_sweep).  Returns what the public method documents."""
        k = self._prior_row(priorK)
        P, n_steps, seg_len = int(rows.shape[0]), int(n_steps), int(seg_len)
        ws_bytes = int(getattr(self._lib, fn + "_workspace_bytes")(self._h, P, n_steps, seg_len))
        if ws_bytes < 0:
            raise native.PimeError(f"{fn}_workspace_bytes: {native.last_error()}")
        kind, md, img = self._actor_triple(packed_actor)
        N = self.num_envs
        sp, sp_ptr, n_sp, n_seg = self._schedule(setpoints, n_steps, seg_len)
        summary = torch.empty((P, n_seg, R, len(native.SWEEP_STATS)), dtype=torch.float64, device=self.device)
        pairs = torch.empty((n_seg, R, P, N), dtype=torch.float64, device=self.device) if want_pairs else None
        actions = torch.empty((max(n_steps, 0), P, N), dtype=torch.float64, device=self.device) if want_trace else None
        outputs = torch.empty((max(n_steps, 0), P, N), dtype=torch.float64, device=self.device) if want_trace else None
        # (the workspace lives for this call only and comes from torch's allocator: see prior_sweep)
        cmds = torch.empty((max(n_steps, 0), P, N), dtype=torch.float64, device=self.device) if commands and want_trace else None
        third = (native.ptr(cmds),) if commands else ()
        workspace = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=self.device)
        native.check(getattr(self._lib, fn)(
            self._h, kind, md, native.ptr(img), native.ptr(k), native.ptr(rows), *before, P, *own, n_steps, seg_len, sp_ptr, n_sp, float(band),
            int(tail), native.ptr(pairs), native.ptr(summary), native.ptr(actions), *third, native.ptr(outputs), native.ptr(workspace),
            self._stream()), fn)
        del workspace
        if not (want_pairs or want_trace):
            return summary
        out = {"summary": summary, "pairs": pairs, "actions": actions, "outputs": outputs}
        if commands:
            out["commands"] = cmds
        return out

    # -- loop-perturbation sweep (delay, gain and sensor-noise margins) ---------------------------------------------
    def margin_supported(self, packed_actor=None):
        """Does `margin_sweep` serve this env (with this packed actor, or the prior controller alone)?
        (pime_margin_sweep_supported: pH and the Integrator tank, float64 or mixed state, in-kernel draws; actor widths 64 / 128.)"""
        return self._row_grid_supported(self._lib.pime_margin_sweep_supported, packed_actor)

    def margin_sweep(self, packed_actor, priorK, perturb, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, noise_seed=0,
                     noise_epoch=0, want_pairs=False, want_trace=False):
        """A grid of LOOP perturbations over every lane's plant in ONE call (pime_margin_sweep, csrc/margin_sweep.hip): every
        (perturbation row, lane) pair runs the loop of `rollout_eval_metrics` from the lane state as it stands with the row's
        (gain g, dead time d in sample periods, sensor-noise scale sigma) -- perturb float64 [P, 3], columns native.PERTURB_NAMES:
        the controller reads the plant outputs plus sigma x a standard normal keyed on the LANE (every row meets the same noise
        sequence, scaled), the plant receives g x the controller's output of d steps ago (0 before the first).  packed_actor None =
        the prior controller alone.  Returns summary float64 [P, n_segments, 8, 5] -- per row, segment and metric row
        (native.METRIC_NAMES) the stats native.SWEEP_STATS over the lanes, exactly as `prior_sweep` -- or, with `want_pairs` and /
        or `want_trace`, a dict with "summary", "pairs" float64 [n_segments, 8, P, N] and "actions", "outputs" float64
        [n_steps, P, N] (the APPLIED action and the controlled output after each step).  ValueError for a row with a non-finite
        gain, a delay that is not an integer in 0 .. native.MARGIN_MAX_DELAY, or a sigma that is negative or not finite (`check_perturb`;
        inside a stream capture pass a float64 device tensor validated beforehand).  The env itself is read, never advanced
        (definitions in include/pime_hip.h)."""
        if torch.is_tensor(perturb) and perturb.is_cuda and torch.cuda.is_current_stream_capturing():
            # a capture can neither read the rows back nor upload them: a float64 [P, 3] device tensor the caller validated
            # (check_perturb) before the capture; the kernel itself rounds and clamps the delay
            pt = perturb
            if pt.dtype != torch.float64 or pt.dim() != 2 or pt.shape[1] != native.PERTURB_COLS or pt.shape[0] < 1 or not pt.is_contiguous():
                raise ValueError(f"margin_sweep: under capture perturb must be a contiguous float64 [P >= 1, {native.PERTURB_COLS}] device tensor")
        else:
            pt = torch.as_tensor(check_perturb(perturb), dtype=torch.float64).to(self.device).contiguous()
        return self._row_grid_sweep("pime_margin_sweep", native.METRIC_ROWS, packed_actor, priorK, pt,
                                    (C.c_uint64(int(noise_seed)), C.c_uint32(int(noise_epoch))), n_steps, setpoints, seg_len, band, tail,
                                    want_pairs, want_trace)

    # -- disturbance-rejection sweep (load and plant-parameter steps) -------------------------------------------------
    def disturbance_supported(self, packed_actor=None):
        """Does `disturbance_sweep` serve this env (with this packed actor, or the prior controller alone)?
        (pime_disturb_sweep_supported: the classes of `margin_sweep`.)"""
        return self._row_grid_supported(self._lib.pime_disturb_sweep_supported, packed_actor)

    def disturbance_sweep(self, packed_actor, priorK, rows, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, want_pairs=False,
                          want_trace=False):
        """A grid of DISTURBANCES over every lane's plant in ONE call (pime_disturb_sweep, csrc/disturb_sweep.hip): every (row, lane)
        pair runs the loop of `rollout_eval_metrics` from the lane state as it stands; from step `onset` of every segment, for
        `length` steps (0: to the segment's end), `load` is added to the controller's output in front of the actuator and the plant's
        parameters are multiplied by m0, m1, m2 (pH: qww_V, qc_V; tank: a1, a2, Kp) -- rows float64 [P, 6], columns
        native.DISTURB_COL_NAMES.  packed_actor None = the prior controller alone.  Returns summary float64 [P, n_segments, 15, 5]
        -- per row, segment and metric row (native.METRIC_NAMES, then native.DISTURB_ROW_NAMES over the steps from the onset: the
        error the onset met, peak error and its step, recovery step for `band`, IAE, ITAE, the largest move of the controller's
        output) the stats native.SWEEP_STATS over the lanes, exactly as `prior_sweep`; a segment the row never starts in holds NaN and
        is not counted -- or, with `want_pairs` and / or `want_trace`, a dict with "summary", "pairs" float64 [n_segments, 15, P, N]
        and "actions", "outputs" float64 [n_steps, P, N] (the CONTROLLER's output -- the applied action is that plus the load while
        the row is active -- and the controlled output after each step).  ValueError for a bad row (`check_disturb`); a device tensor
        is taken as given, so a capture works.  The env itself is read, never advanced (definitions in include/pime_hip.h)."""
        if torch.is_tensor(rows) and rows.is_cuda:
            dt = rows
            if dt.dtype != torch.float64 or dt.dim() != 2 or dt.shape[1] != native.DISTURB_COLS or dt.shape[0] < 1 or not dt.is_contiguous():
                raise ValueError(f"disturbance_sweep: a device tensor of rows must be contiguous float64 [P >= 1, {native.DISTURB_COLS}]")
        else:
            dt = torch.as_tensor(check_disturb(rows, self.kind == native.ENV_PH), dtype=torch.float64).to(self.device).contiguous()
        return self._row_grid_sweep("pime_disturb_sweep", native.METRIC_ROWS + native.DISTURB_ROWS, packed_actor, priorK, dt, (), n_steps,
                                    setpoints, seg_len, band, tail, want_pairs, want_trace)

    # -- frequency-response sweep (tabulated excitation and lock-in rows) ------------------------------------------------
    def frequency_supported(self, packed_actor=None):
        """Does `frequency_sweep` serve this env (with this packed actor, or the prior controller alone)?
        (pime_freq_sweep_supported: the classes of `margin_sweep`.)"""
        return self._row_grid_supported(self._lib.pime_freq_sweep_supported, packed_actor)

    def frequency_sweep(self, packed_actor, priorK, rows, wave, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, want_pairs=False,
                        want_trace=False):
        """A grid of EXCITATIONS over every lane's plant in ONE call (pime_freq_sweep, csrc/freq_sweep.hip): every (row, lane) pair
        runs the loop of `rollout_eval_metrics` from the lane state as it stands while amplitude x s_k is added at every step k of every
        segment at the row's point (native.FREQ_POINTS: the set-point, the controller's output in front of the actuator, the measured
        output the controller reads) -- rows float64 [P, 3], columns native.FREQ_COL_NAMES; wave float64 [P, L, 2] holds (c_k, s_k)
        per row and segment step, L = seg_len (n_steps when seg_len is 0): `protocols.excitation_grid` makes both.  packed_actor None =
        the prior controller alone.  Returns summary float64 [P, n_segments, 16, 5] -- per row, segment and metric row
        (native.METRIC_NAMES, then native.FREQ_ROW_NAMES: the sums of y c, y s, a_c c, a_c s, y, a_c, y^2 and a_c^2 over the steps from
        `onset`) the stats native.SWEEP_STATS over the lanes, exactly as `prior_sweep`; a segment that never reaches the onset holds
        NaN and is not counted -- or, with `want_pairs` and / or `want_trace`, a dict with "summary", "pairs" float64
        [n_segments, 16, P, N] and "actions", "outputs" float64 [n_steps, P, N] (the CONTROLLER's output and the controlled output
        after each step).  ValueError for a bad row or table (`check_excite`); device tensors are taken as given apart from their
        shapes, so a capture works.  The env itself is read, never advanced (definitions in include/pime_hip.h)."""
        n_steps, seg_len = int(n_steps), int(seg_len)
        L = seg_len if seg_len > 0 else n_steps
        if torch.is_tensor(rows) and rows.is_cuda and torch.is_tensor(wave) and wave.is_cuda:
            rt, wt = rows, wave
            if rt.dtype != torch.float64 or rt.dim() != 2 or rt.shape[1] != native.FREQ_COLS or rt.shape[0] < 1 or not rt.is_contiguous():
                raise ValueError(f"frequency_sweep: a device tensor of rows must be contiguous float64 [P >= 1, {native.FREQ_COLS}]")
            if wt.dtype != torch.float64 or tuple(wt.shape) != (rt.shape[0], L, 2) or not wt.is_contiguous():
                raise ValueError(f"frequency_sweep: a device tensor of wave must be contiguous float64 [P, {L}, 2]")
        else:
            r, w = check_excite(rows, wave, L)
            rt = torch.as_tensor(r, dtype=torch.float64).to(self.device).contiguous()
            wt = torch.as_tensor(w, dtype=torch.float64).to(self.device).contiguous()
        return self._row_grid_sweep("pime_freq_sweep", native.METRIC_ROWS + native.FREQ_ROWS, packed_actor, priorK, rt, (), n_steps,
                                    setpoints, seg_len, band, tail, want_pairs, want_trace, before=(native.ptr(wt), L))

    # -- actuator-limits sweep (saturation, slew, dead-band, DAC and ADC quanta) ------------------------------------------
    def actuator_supported(self, packed_actor=None):
        """Does `actuator_sweep` serve this env (with this packed actor, or the prior controller alone)?
        (pime_actuator_sweep_supported: the classes of `margin_sweep`.)"""
        return self._row_grid_supported(self._lib.pime_actuator_sweep_supported, packed_actor)

    def actuator_sweep(self, packed_actor, priorK, rows, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, want_pairs=False,
                       want_trace=False):
        """A grid of ACTUATOR and SENSOR limits over every lane's plant in ONE call (pime_actuator_sweep, csrc/actuator_sweep.hip):
        every (row, lane) pair runs the loop of `rollout_eval_metrics` from the lane state as it stands, the controller reading the
        measured plant outputs on the sensor's quantum `qy` and its command passing, in this order, a dead-band (`deadband`: hold
        within it of the present position), a slew limit (`rate` per step), the actuator's quantum `qu` and the clamp [`lo`, `hi`] --
        rows float64 [P, 6], columns native.ACT_COL_NAMES; a stage is OFF for lo = -inf / hi = +inf (or NaN) and for a rate (other
        than 0 < rate < inf), dead-band or quantum that is not > 0, and a row with every stage off is bit for bit
        `rollout_eval_metrics`.  packed_actor None = the prior controller alone.  Returns summary float64 [P, n_segments, 16, 5] --
        per row, segment and metric row (native.METRIC_NAMES on the APPLIED action, then native.ACT_ROW_NAMES: the steps the clamp,
        the slew limit and the dead-band acted on, the peak and the sum of |command - applied|, the reversals of the applied action,
        the peak-to-peak of the output and of the applied action over the last `tail` steps) the stats native.SWEEP_STATS over the
        lanes, exactly as `prior_sweep` -- or, with `want_pairs` and / or `want_trace`, a dict with "summary", "pairs" float64
        [n_segments, 16, P, N] and "actions", "commands", "outputs" float64 [n_steps, P, N] (the applied action, the controller's
        command and the controlled output after each step).  ValueError for a bad row (`check_actuator`); a device tensor is taken
        as given (the kernel decodes, it does not validate), so a capture works.  The env itself is read, never advanced
        (definitions in include/pime_hip.h)."""
        if torch.is_tensor(rows) and rows.is_cuda:
            at = rows
            if at.dtype != torch.float64 or at.dim() != 2 or at.shape[1] != native.ACT_COLS or at.shape[0] < 1 or not at.is_contiguous():
                raise ValueError(f"actuator_sweep: a device tensor of rows must be contiguous float64 [P >= 1, {native.ACT_COLS}]")
        else:
            at = torch.as_tensor(check_actuator(rows), dtype=torch.float64).to(self.device).contiguous()
        return self._row_grid_sweep("pime_actuator_sweep", native.METRIC_ROWS + native.ACT_ROWS, packed_actor, priorK, at, (), n_steps,
                                    setpoints, seg_len, band, tail, want_pairs, want_trace, commands=True)

    # -- policy sweep (many actors, each with its own prior gain, over the lanes' plants) ----------------------------------
    def policy_supported(self, policies):
        """Does `policy_sweep` serve this env with this `ops.PackedPolicies` stack?  (pime_policy_sweep_supported: the classes of
        `margin_sweep` WITH a policy -- pH and the Integrator tank, float64 or mixed state, in-kernel draws, actor widths 64 / 128;
        the prior controller alone is `prior_sweep`.)"""
        if self.draws.injects or policies is None or len(policies) < 1:
            return False
        if policies.kind not in _EVAL_KINDS or policies.D != self.obs_dim or policies.packed.device != self.obs.device:
            return False
        return bool(self._lib.pime_policy_sweep_supported(self._h, _EVAL_KINDS[policies.kind], int(policies.md)))

    def policy_sweep(self, policies, n_steps, setpoints=None, seg_len=0, band=0.05, tail=10, want_pairs=False, want_trace=False):
        """A grid of POLICIES over every lane's plant in ONE call (pime_policy_sweep, csrc/policy_sweep.hip): every (policy row, lane)
        pair runs the loop of `rollout_eval_metrics` from the lane state as it stands under row p's packed actor and row p's prior
        gain -- policies: an `ops.PackedPolicies` stack of P actors of one class.  Row p is bit for bit what `rollout_eval_metrics`
        with that actor and gain writes from the same lane state, and every policy meets the same process noise (it is keyed on the
        lane).  Returns summary float64 [P, n_segments, 8, 5] -- per policy, segment and metric row (native.METRIC_NAMES) the stats
        native.SWEEP_STATS over the lanes, exactly as `prior_sweep` -- or, with `want_pairs` and / or `want_trace`, a dict with
        "summary", "pairs" float64 [n_segments, 8, P, N] and "actions", "outputs" float64 [n_steps, P, N] (the action and the
        controlled output after each step).  native.PimeError for a stack `policy_supported` refuses (injected draws among them).
        Nothing is uploaded or read back, so a capture works.  The env itself is read, never advanced (definitions in
        include/pime_hip.h)."""
        fn = "pime_policy_sweep"
        if self.draws.injects:
            raise native.PimeError(f"{fn}: injected draws are not served (in-kernel Philox draws only)")
        if policies is None or len(policies) < 1:
            raise native.PimeError(f"{fn}: P = {0 if policies is None else len(policies)} (>= 1)")
        if policies.kind not in _EVAL_KINDS or policies.D != self.obs_dim:
            raise native.PimeError(f"{fn}: a stack of kind {policies.kind!r} on {policies.D} observation columns is not served on "
                                   f"this env ({self.obs_dim} columns)")
        P, n_steps, seg_len = len(policies), int(n_steps), int(seg_len)
        ws_bytes = int(self._lib.pime_policy_sweep_workspace_bytes(self._h, P, n_steps, seg_len))
        if ws_bytes < 0:
            raise native.PimeError(f"{fn}_workspace_bytes: {native.last_error()}")
        N = self.num_envs
        sp, sp_ptr, n_sp, n_seg = self._schedule(setpoints, n_steps, seg_len)
        images, gains = policies.packed, policies.K
        summary = torch.empty((P, n_seg, native.METRIC_ROWS, len(native.SWEEP_STATS)), dtype=torch.float64, device=self.device)
        pairs = torch.empty((n_seg, native.METRIC_ROWS, P, N), dtype=torch.float64, device=self.device) if want_pairs else None
        actions = torch.empty((max(n_steps, 0), P, N), dtype=torch.float64, device=self.device) if want_trace else None
        outputs = torch.empty((max(n_steps, 0), P, N), dtype=torch.float64, device=self.device) if want_trace else None
        # (the workspace lives for this call only and comes from torch's allocator: see prior_sweep)
        workspace = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=self.device)
        native.check(self._lib.pime_policy_sweep(
            self._h, _EVAL_KINDS[policies.kind], int(policies.md), native.ptr(images), int(policies.stride), native.ptr(gains), P, n_steps,
            seg_len, sp_ptr, n_sp, float(band), int(tail), native.ptr(pairs), native.ptr(summary), native.ptr(actions), native.ptr(outputs),
            native.ptr(workspace), self._stream()), fn)
        del workspace
        if not (want_pairs or want_trace):
            return summary
        return {"summary": summary, "pairs": pairs, "actions": actions, "outputs": outputs}

    # -- state access (float64 numpy on the host; synchronous) -------------------------------------------------
    def get_field(self, name):
        out = np.empty(self.num_envs, dtype=np.float64)
        native.check(self._lib.pime_env_read_field(self._h, native.FIELD[self.field_prefix + name], native.ptr(out),
                                                   self._stream()), f"read_field({name})")
        return out

    def set_field(self, name, values, mask=None):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float64), (self.num_envs,)))
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=np.uint8))
        native.check(self._lib.pime_env_write_field(self._h, native.FIELD[self.field_prefix + name], native.ptr(v),
                                                    native.ptr(m), self._stream()), f"write_field({name})")
        if name == "t":
            t = self._lane_steps()
            t[:] = v.astype(np.int64) if mask is None else np.where(m.astype(bool), v, t)

    def set_reset_all(self, if_reset_all, every=1):
        """if_reset_all False keeps the ensemble params across resets (ph.py:111-112; attribute
        nonlinear_watertank.py:861).  `every` = n of "resample every n episodes" (README step 4)."""
        self.if_reset_all = bool(if_reset_all)
        native.check(self._lib.pime_env_set_resample_every(self._h, int(every) if if_reset_all else 0))

    def set_max_step(self, n):
        self.max_step = int(n)
        native.check(self._lib.pime_env_set_max_steps(self._h, int(n)))

    def get_linear_action(self, state):
        """Prior controller -state @ K (ph.py:227-231; nonlinear_watertank.py:755-759 clips to the action box)."""
        k = torch.as_tensor(self.K, dtype=state.dtype, device=state.device)
        return -(state @ k)


# ------------------------------------------------------------------------------------------------ pH
_PH_TABLE_CACHE = {}


def ph_table(n=100000, step=1e-5, chem=None):
    """Titration LUT (cached per configuration); built by the native library in ~10 ms (reference: 13 s)."""
    key = (n, step, None if chem is None else tuple(sorted(chem.items())))
    if key not in _PH_TABLE_CACHE:
        _PH_TABLE_CACHE[key] = native.ph_table_build(n, step, chem)
    return _PH_TABLE_CACHE[key]


class VecPH(VecControlEnv):
    """N x PH1DChangingParamUniformGoalIntegrator[_NoBound] behind gym's TimeLimit (registered id ...-v35)."""
    kind = native.ENV_PH
    field_prefix = "ph_"
    draw_width = 4
    n_integrator = 1
    dim = 1

    def __init__(self, num_envs, device="cuda", state_mode="mixed", seed=0, env_offset=0, draws="philox",
                 reward_type="square_distance", max_episode_steps=50, integral_bound=True, resample_every=1,
                 qww_V=(0.005, 0.015), qc_V=(0.0015, 0.0025), P_control_K=(-0.02, 0.02, 0.035),
                 MHCl_step=1e-5, MHCl_len=100000, chem=None, action_punishment=0., action_change_punishment=0.,
                 integral_punish=0., sample_t=20.0, distance_threshold=0.05):
        self._ctor = {k: v for k, v in locals().items() if k not in ("self", "__class__")}
        cfg = native.EnvCfg()
        native.check(native.lib().pime_env_cfg_default(native.ENV_PH, C.byref(cfg)))
        self.table = ph_table(MHCl_len, MHCl_step, chem)
        cfg.n_envs = num_envs
        cfg.state_mode = _STATE_MODES[state_mode]
        cfg.max_steps = max_episode_steps
        cfg.reward_type = native.REWARD[reward_type]
        cfg.integral_bound = int(bool(integral_bound))
        cfg.resample_every = resample_every
        cfg.env_offset = env_offset
        cfg.seed = seed
        cfg.integral_punish, cfg.action_punish, cfg.action_change_punish = integral_punish, action_punishment, \
            action_change_punishment
        cfg.distance_threshold = distance_threshold
        cfg.range_lo[0], cfg.range_hi[0] = qww_V
        cfg.range_lo[1], cfg.range_hi[1] = qc_V
        cfg.ph_sample_t = sample_t
        cfg.ph_table_scale = 1.0 / MHCl_step
        cfg.ph_table = self.table.ctypes.data_as(C.POINTER(C.c_double))
        cfg.ph_table_len = len(self.table)
        self.qww_Vrange, self.qc_Vrange = tuple(qww_V), tuple(qc_V)
        self.reward_type = reward_type
        self.if_reset_all = resample_every > 0
        if draws == "philox":
            draws = PhiloxDraws()
        elif draws == "mt19937":
            draws = Mt19937Draws(seed, num_envs, env_offset)
        super().__init__(cfg, device, draws, P_control_K)

    def _draw_episode(self, global_rs, env_rs):
        # reset_all: sample_parameters (2 global uniforms, ph.py:410,413) then x0, r from np_random (:420,:424).
        # With if_reset_all False the reference does not touch the global stream (reset_r, :428-439).
        if self.if_reset_all:
            qww, qc = global_rs.uniform(*self.qww_Vrange), global_rs.uniform(*self.qc_Vrange)
        else:
            qww = qc = 0.0
        x0 = env_rs.uniform(low=0, high=50)
        r = env_rs.uniform(3., 11.)
        return qww, qc, x0, r

    def get_changable_parameters(self):
        return self.get_field("qww_V"), self.get_field("qc_V")

    def set_params(self, qww_V, qc_V, mask=None):
        """Unlike the reference's set_params (ph.py:263-265, which forgets update_system -- SURVEY.md App. C.3),
        this rebuilds the discretised plant."""
        self.set_field("qww_V", qww_V, mask)
        self.set_field("qc_V", qc_V, mask)

    reset_changable_parameters = set_params


# ------------------------------------------------------------------------------------------------ water tank
class VecWaterTank(VecControlEnv):
    """N x NonLinearWaterTankChangingParamUniformGoalIntegrator (num_stack=0) or ...GoalStacking (num_stack=S)."""
    kind = native.ENV_WT
    field_prefix = "wt_"
    draw_width = 6
    has_step_noise = True

    def __init__(self, num_envs, device="cuda", state_mode="mixed", seed=0, env_offset=0, draws="philox",
                 reward_type="square_distance", max_step=200, num_stack=0, resample_every=1,
                 a1=(0.0015, 0.0024), a2=(0.0015, 0.0024), Kp=(0.07, 0.17), A1=1, A2=1, G=980, sample_t=2, n_discrete=20,
                 noise_scale=0.01, z1=1, P_max_action=10.0, P_control_K=None, integral_punish=0.,
                 distance_threshold=0.05):
        self._ctor = {k: v for k, v in locals().items() if k not in ("self", "__class__")}
        cfg = native.EnvCfg()
        native.check(native.lib().pime_env_cfg_default(native.ENV_WT, C.byref(cfg)))
        cfg.n_envs = num_envs
        cfg.state_mode = _STATE_MODES[state_mode]
        cfg.max_steps = max_step
        cfg.reward_type = native.REWARD[reward_type]
        cfg.num_stack = num_stack
        cfg.resample_every = resample_every
        cfg.env_offset = env_offset
        cfg.seed = seed
        cfg.integral_punish = integral_punish
        cfg.distance_threshold = distance_threshold
        for j, rng in enumerate((a1, a2, Kp)):
            cfg.range_lo[j], cfg.range_hi[j] = rng
        cfg.wt_A1, cfg.wt_A2, cfg.wt_G = A1, A2, G
        cfg.wt_n_discrete = n_discrete
        cfg.wt_dt = sample_t / n_discrete
        cfg.wt_noise_scale = noise_scale
        cfg.wt_z1 = z1
        cfg.wt_pmax = P_max_action
        self.a1_range, self.a2_range, self.Kp_range = tuple(a1), tuple(a2), tuple(Kp)
        self.noise_scale = noise_scale
        self.num_stack = num_stack
        self.reward_type = reward_type
        self.if_reset_all = resample_every > 0
        if num_stack == 0:
            self.n_integrator = 1
        if P_control_K is None:
            if num_stack == 0:
                P_control_K = [0., 0.4, -0.4, 0.]            # gym_control/__init__.py:67
            else:
                P_control_K = np.zeros(3 * num_stack)       # :71-73
                P_control_K[-3:] = [0., 0.4, -0.4]
        if draws == "philox":
            draws = PhiloxDraws()
        elif draws == "mt19937":
            draws = Mt19937Draws(seed, num_envs, env_offset)
        super().__init__(cfg, device, draws, P_control_K)

    def _draw_episode(self, global_rs, env_rs):
        # reset_all: sample_parameters (:890-894) then uniform(0,10,2) and uniform(0,10) (:912-913), one stream
        if self.if_reset_all:
            a1 = global_rs.uniform(self.a1_range[0], self.a1_range[1])
            a2 = global_rs.uniform(self.a2_range[0], self.a2_range[1])
            kp = global_rs.uniform(self.Kp_range[0], self.Kp_range[1])
        else:
            a1 = a2 = kp = 0.0
        h1, h2 = tuple(global_rs.uniform(0., 10., 2))
        r = global_rs.uniform(0., 10.)
        return a1, a2, kp, h1, h2, r

    def get_changable_parameters(self):
        return self.get_field("a1"), self.get_field("a2"), self.get_field("Kp")

    def reset_changable_parameters(self, a1, a2, Kp, mask=None):
        self.set_field("a1", a1, mask)
        self.set_field("a2", a2, mask)
        self.set_field("Kp", Kp, mask)
