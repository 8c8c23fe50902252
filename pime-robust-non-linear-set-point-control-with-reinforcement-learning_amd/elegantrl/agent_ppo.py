"""AgentPPO: the on-policy agent, the residual PPO agents' parent (interface of the reference's elegantrl/agent.py:543-712).  What
differs from the reference is listed in agent.py; the optimizer steps of `update_net` on the fused HIP gradient path are
ppo_update.py's."""
import numpy as np
import torch

from . import logger, ppo_update
from .agent_base import AgentBase
from .net import ActorPPO, CriticAdv
from .replay import TrajectoryBuffer


class AgentPPO(AgentBase):
    def __init__(self, backend=None, device=None):
        super().__init__(backend, device)
        self.ratio_clip = 0.2
        self.lambda_entropy = 0.02
        self.lambda_gae_adv = 0.97
        self.if_use_gae = True
        self.if_on_policy = True
        self.if_use_dn = False
        self.noise = None
        self.optimizer = None
        self.compute_reward = None
        self._packed = {}
        self.noise_hook = None  # tests: callable(t, shape) -> exploration noise tensor (else torch.randn)
        self.use_fused_update = True
        self.use_hip_graphs = True
        self.use_graph_collective = True  # data parallel: capture the RCCL all-reduce INSIDE that one graph
        self.use_update_graph = True      # ... and, once that graph exists, all n_steps optimizer steps of an update as ONE graph
        self.use_fused_rollout = True
        self.launch_timer = None  # optional callable(name, thunk) that brackets the thunk with HIP events

    # ---- construction ------------------------------------------------------------------------------------
    def _build_nets(self, net_dim, state_dim, action_dim):
        self.cri = CriticAdv(state_dim, net_dim, self.if_use_dn).to(self.device)
        self.act = ActorPPO(net_dim, state_dim, action_dim, self.if_use_dn).to(self.device)

    def init(self, net_dim, state_dim, action_dim, if_per=False):
        assert if_per is False, "on-policy agents do not use prioritised replay"
        self._pick_device()
        self.compute_reward = self.compute_reward_gae if self.if_use_gae else self.compute_reward_adv
        self._build_nets(net_dim, state_dim, action_dim)
        self._make_optimizer()
        self.criterion = torch.nn.SmoothL1Loss()

    def _make_optimizer(self):
        # ONE Adam over both nets (agent.py:565-566); rebuilt whenever the reference rebuilds it
        fused = self._packed.get("fused")
        if fused and fused.params_are(self):
            # the parameters already live in the fused path's flat tensor: a fresh optimizer there (fresh moments and step
            # count, as a rebuilt torch Adam has), and the captured graphs -- which replay the OLD optimizer's buffers -- go
            self.optimizer = fused.make_optimizer(self.learning_rate)
            ppo_update.drop(fused)
            self.weights_changed()
            return
        groups = [{"params": self.act.parameters(), "lr": self.learning_rate},
                  {"params": self.cri.parameters(), "lr": self.learning_rate}]
        # fused=True: one multi-tensor kernel per step on the GPU instead of ~10 foreach launches
        # capturable=True: the step counter lives on the device, so the step can be replayed from a HIP graph
        self.optimizer = torch.optim.Adam(groups, fused=True, capturable=True) if self.device.type == "cuda" \
            else torch.optim.Adam(groups)
        self.weights_changed()

    def init_actor_zero(self):
        """Zero the policy's output layer so the initial policy is the prior controller alone (agent.py:569-574)."""
        with torch.no_grad():
            self.act.net[-1].bias.fill_(0.)
            self.act.net[-1].weight.fill_(0.)
        self._make_optimizer()

    def frozen_transfer(self):
        self.cri.frozen_transfer()
        self.act.frozen_transfer()

    # ---- acting ------------------------------------------------------------------------------------------
    def select_action(self, state, if_deterministic=False):
        states = torch.as_tensor(np.asarray(state)[None], dtype=torch.float32, device=self.device)
        with torch.no_grad():
            if if_deterministic:
                return self.act(states)[0].cpu().numpy(), None
            actions, noises = self.act.get_action_noise(states)
        return actions[0].cpu().numpy(), noises[0].cpu().numpy()

    def _env_action(self, state, action):
        """What is sent to a one-instance env for the sampled pre-tanh `action` (agent.py:599)."""
        return np.tanh(action)

    def _packed_for(self, name):
        if name not in self._packed:
            self._packed[name] = self.backend.packed(getattr(self, name))
        return self._packed[name]

    def policy_mean(self, states):
        """a_avg for a [M, D] batch without autograd: fused MFMA forward when the shape is supported."""
        pk = self._packed_for("act")
        if pk is not None:
            return pk(states).unsqueeze(1)
        with torch.no_grad():
            return self.act.mean(states)

    def state_value(self, states):
        pk = self._packed_for("cri")
        if pk is not None:
            return pk(states)
        with torch.no_grad():
            out = [self.cri(states[i:i + 2 ** 16])[:, 0] for i in range(0, states.shape[0], 2 ** 16)]
        return torch.cat(out)

    def explore_env(self, env, buffer, target_step, reward_scale, gamma):
        if hasattr(env, "num_envs"):
            return self.explore_vec_env(env, buffer, target_step, reward_scale, gamma)
        # one-instance env: whole episodes until >= target_step transitions (agent.py:591-609)
        buffer.empty_buffer_before_explore()
        actual_step = 0
        while actual_step < target_step:
            state = env.reset()
            for _ in range(env.max_step):
                action, noise = self.select_action(state)
                next_state, reward, done, _ = env.step(self._env_action(state, action))
                actual_step += 1
                buffer.append_buffer(state, (reward * reward_scale, 0.0 if done else gamma, *action, *noise))
                if done:
                    break
                state = next_state
        return actual_step

    def _rollout_priorK(self):
        """Prior-controller gain of the fused rollout: none for plain PPO (the env sees tanh(a_pre), agent.py:599)."""
        return np.zeros(self.act.state_dim)

    def _fused_rollout_ok(self, env):
        if not (self.use_fused_rollout and getattr(env, "supports_fused_rollout", False)) or self.noise_hook is not None:
            return False
        if not hasattr(self, "_rollout_seed"):
            self._rollout_seed = int(torch.initial_seed()) & (2 ** 63 - 1)   # exploration stream follows torch's seed
            self._rollout_epoch = 0
        pk = self._packed_for("act")
        return pk is not None and self.act.state_dim == env.obs_dim and env.rollout_supported(pk)

    def fused_eval_policy(self, env):
        """(packed actor, priorK) if the fused evaluation kernel can run this agent's deterministic policy on `env`
        (run.py:600-619 as one launch, csrc/rollout_eval.hip), else None -> the evaluator steps the env launch by launch."""
        if not self.use_fused_rollout or not hasattr(env, "eval_supported"):
            return None
        pk = self._packed_for("act")
        if pk is None or not env.eval_supported(pk):
            return None
        return pk, self._rollout_priorK()

    def _vec_env_step(self, env, a_pre, obs, out_obs, out_reward, out_done):
        """Plain PPO: the env sees tanh(a_pre) (agent.py:599)."""
        step = env.step_h if out_obs.dtype == torch.float16 else env.step
        return step(torch.tanh(a_pre), auto_reset=True, out_obs=out_obs, out_reward=out_reward, out_done=out_done)

    def explore_vec_env(self, env, buffer, target_step, reward_scale, gamma):
        """Lock-step rollout of all lanes for whole episodes until >= target_step transitions are stored.
        Every tensor stays in HBM; per step: policy mean (fused forward) + noise + ONE env launch that also
        applies tanh + prior and writes obs/reward/done into the trajectory slots."""
        assert isinstance(buffer, TrajectoryBuffer) and buffer.num_envs == env.num_envs
        buffer.empty_buffer_before_explore()
        N, T_max = env.num_envs, buffer.horizon
        episodes = max(1, -(-target_step // (N * env.max_step)))
        assert episodes * env.max_step <= T_max, "TrajectoryBuffer horizon too short for target_step"
        std = None
        t = 0
        fused = self._fused_rollout_ok(env)
        # Every lane sits at the start of an episode either because nothing ran yet (-> reset) or because the last
        # step of the previous rollout auto-reset it inside the kernel (-> just read the observation back).
        half = buffer.state.dtype == torch.float16   # env in state_mode "mixed16": binary16 observation / reward rows
        assert buffer.state.dtype == getattr(env, "trajectory_dtype", torch.float32), "buffer / env row dtype mismatch"
        if half:
            if env.fresh:
                buffer.state[0].copy_(env.observe())   # float32 -> binary16: the rounding the *_h kernels apply
            else:
                env.reset_h(out=buffer.state[0])
        elif env.fresh:
            env.observe(out=buffer.state[0])
        else:
            env.reset(out=buffer.state[0])
        for ep in range(episodes):
            if fused:  # one launch per episode: policy forward + noise + env step + buffer writes (csrc/rollout.hip)
                n = env.max_step
                self._rollout_epoch += 1
                env.rollout(self._packed_for("act"), self.act.a_std_log.detach(), self._rollout_priorK(), n,
                            self._rollout_seed, self._rollout_epoch, buffer.state[t:t + n + 1], buffer.action[t:t + n],
                            buffer.noise[t:t + n], buffer.reward[t:t + n], buffer.done[t:t + n])
                t += n
                continue
            for _ in range(env.max_step):
                obs = buffer.state[t]
                with torch.no_grad():
                    if std is None:
                        std = self.act.a_std_log.detach().exp()
                    a_avg = self.policy_mean(obs.float() if half else obs)
                    noise = torch.randn_like(a_avg) if self.noise_hook is None else self.noise_hook(t, a_avg.shape)
                    a_pre = a_avg + noise * std
                    buffer.action[t] = a_pre
                    buffer.noise[t] = noise
                self._vec_env_step(env, a_pre, obs, buffer.state[t + 1], buffer.reward[t], buffer.done[t])
                t += 1
        with torch.no_grad():
            if reward_scale != 1.0:
                buffer.reward[:t] *= reward_scale
            buffer.mask[:t] = (1.0 - buffer.done[:t].to(torch.float32)) * gamma  # 0.0 if done else gamma
        buffer.length = t
        return t * N

    # ---- learning ----------------------------------------------------------------------------------------
    def _trajectory_views(self, buffer):
        """(reward, mask, action, noise, state) flattened in storage order plus the [T, N] shape for the scan."""
        buffer.update_now_len_before_sample()
        if isinstance(buffer, TrajectoryBuffer):
            T, N = buffer.length, buffer.num_envs
        else:
            T, N = buffer.now_len, 1  # flat time-ordered ring: one lane
        rew, mask, action, noise, state = buffer.sample_all()
        return T, N, rew, mask, action, noise, state

    def update_net(self, buffer, _target_step, batch_size, repeat_times=4):
        T, N, buf_reward, buf_mask, buf_action, buf_noise, buf_state = self._trajectory_views(buffer)
        buf_len = T * N
        dev = buf_state.device
        with torch.no_grad():
            buf_value = self.state_value(buf_state)                                # agent.py:619-620
            buf_logprob = self.act.old_logprob(buf_noise)                          # :621
            buf_r_sum, buf_advantage = self.compute_reward(buf_len, buf_reward, buf_mask, buf_value, shape=(T, N))

        n_steps = int(repeat_times * buf_len / batch_size)                         # :629
        fused = self._fused_grad(batch_size)
        if fused is not None:
            return self._update_fused(fused, n_steps, buf_len, batch_size, repeat_times, buf_state, buf_action,
                                      buf_r_sum, buf_logprob, buf_advantage)
        sums = torch.zeros(4, device=dev)  # united, actor, critic, entropy
        obj_actor = obj_critic = torch.zeros((), device=dev)
        params = [p for g in self.optimizer.param_groups for p in g["params"]]
        for step in range(n_steps):
            indices = self._minibatch_indices(step, buf_len, batch_size, dev)
            state = buf_state[indices]
            action = buf_action[indices]
            r_sum = buf_r_sum[indices]
            logprob = buf_logprob[indices]
            advantage = buf_advantage[indices]

            new_logprob = self.act.compute_logprob(state, action)
            ratio = (new_logprob - logprob).exp()
            surrogate = torch.min(advantage * ratio,
                                  advantage * ratio.clamp(1 - self.ratio_clip, 1 + self.ratio_clip))
            obj_entropy = (new_logprob.exp() * new_logprob).mean()                 # ElegantRL's entropy proxy (:643)
            obj_actor = -surrogate.mean() + obj_entropy * self.lambda_entropy
            value = self.cri(state).squeeze(1)
            obj_critic = self.criterion(value, r_sum)
            if self.dp is None:
                obj_united = obj_actor + obj_critic / (r_sum.std() + 1e-5)         # :652
                self.optimizer.zero_grad(set_to_none=False)
                obj_united.backward()
            else:
                # Data parallel: the minibatch of :652 is the UNION of the ranks' minibatches.  Actor and critic parameters are
                # disjoint and the united loss is linear in the critic's factor, so: back-propagate actor + UNSCALED critic, let
                # the one flat all-reduce of the step also carry (sum r, sum r^2, count), then scale the averaged critic gradient
                # by 1 / (std of the union + 1e-5) -- the same weights as one rank stepping on the concatenated minibatch.
                self.optimizer.zero_grad(set_to_none=False)
                (obj_actor + obj_critic).backward()
                r64 = r_sum.detach().double()
                mom = self.dp.average_gradients(params, extra=torch.stack([r64.sum(), (r64 * r64).sum(),
                                                                           torch.tensor(float(r64.numel()), dtype=torch.float64)]).float())
                G = float(self.dp.world)
                n_tot, s1, s2 = G * mom[2].double(), G * mom[0].double(), G * mom[1].double()
                var = ((s2 - s1 * s1 / n_tot) / (n_tot - 1.0)).clamp_min(0.0)
                scale = (1.0 / (var.sqrt().float() + 1e-5))
                obj_united = obj_actor + obj_critic * scale                        # (logged: this rank's terms, the union's scale)
                cri_params = {id(p) for p in self.cri.parameters()}
                with torch.no_grad():
                    for p in params:
                        if id(p) in cri_params and p.grad is not None:
                            p.grad.mul_(scale)
            self.optimizer.step()
            sums += torch.stack([obj_united.detach(), obj_actor.detach(), obj_critic.detach(), obj_entropy.detach()])
        self.weights_changed()
        self._n_updates += int(repeat_times)
        if n_steps:
            mean = (sums / n_steps).tolist()                                       # the only host sync of the update
            self._log_losses(*mean)
        return float(obj_actor.detach()), float(obj_critic.detach())

    def _minibatch_indices(self, step, buf_len, batch_size, dev, out=None):
        if self.index_hook is not None:
            return self.index_hook(step, buf_len, batch_size).to(dev)
        if out is not None:   # same draws, written where the captured graph reads them (saves a copy launch per step)
            return torch.randint(buf_len, size=(batch_size,), device=dev, out=out)
        return torch.randint(buf_len, size=(batch_size,), device=dev)              # agent.py:630

    @staticmethod
    def _log_losses(united, actor, critic, entropy):
        logger.record("train/united_loss", united)
        logger.record("train/actor_loss", actor)
        logger.record("train/critic_loss", critic)
        logger.record("train/entropy_losses", entropy)

    def _fused_grad(self, batch_size):
        """The fused HIP gradient path when the backend offers it for these nets (width 64/128, action_dim 1, GPU);
        otherwise None and the update runs through torch autograd on the same device."""
        if not self.use_fused_update or not hasattr(self.backend, "fused_ppo"):
            return None
        f = self._packed.get("fused")
        if f is None or f.max_batch < batch_size:
            f = self.backend.fused_ppo(self.act, self.cri, batch_size)
            self._packed["fused"] = f
            if f:  # parameters now live in one flat tensor: give Adam that tensor (fresh state, as after init)
                self.optimizer = f.make_optimizer(self.learning_rate)
        return f if f else None

    def _update_fused(self, fused, n_steps, buf_len, batch_size, repeat_times, buf_state, buf_action, buf_r_sum,
                      buf_logprob, buf_advantage):
        """The optimizer steps on the fused HIP gradient path: ppo_update.FusedPPOUpdate (`fused.static`) holds the update's buffers
        where the kernels read them and launches, captures or replays the steps; the loss sums come back in one host read."""
        fused.loss_sums.zero_()
        st = ppo_update.FusedPPOUpdate.of(fused, buf_len, batch_size, buf_state.shape[1], buf_state.device)
        st.load(self, n_steps, buf_state, buf_action, buf_r_sum, buf_logprob, buf_advantage)
        last = st.run(n_steps)
        self._packed = {"fused": fused}  # packed forward images of the value pass / rollout are stale now
        self._n_updates += int(repeat_times)
        if not n_steps:
            return 0.0, 0.0
        tot = fused.loss_sums.tolist()                                             # the only host sync of the update
        if self.dp is not None:
            self.dp.check()   # a timed-out one-shot all-reduce left gradients un-averaged: fatal, here where the stream is drained
        lst = last.tolist()
        B = float(batch_size)
        ent, cri = tot[1] / (n_steps * B), tot[2] / (n_steps * B)
        act = tot[0] / (n_steps * B) + self.lambda_entropy * ent
        self._log_losses(act + tot[4] / (n_steps * B), act, cri, ent)   # mean over steps of (actor + critic * scale), agent.py:652
        obj_a = (tot[0] - lst[0]) / B + self.lambda_entropy * (tot[1] - lst[1]) / B
        obj_c = (tot[2] - lst[2]) / B
        return obj_a, obj_c

    def _normalise_advantage(self, adv):
        """(adv - mean) / (std + 1e-5) over the WHOLE buffer with torch's unbiased std (agent.py:707); under data
        parallelism the buffer is the union of all ranks' slices -> all-reduce (count, sum, sum of squares)."""
        if self.dp is None:
            return (adv - adv.mean()) / (adv.std() + 1e-5)
        a64 = adv.double()
        m = torch.stack([torch.tensor(float(adv.numel()), dtype=torch.float64, device=adv.device), a64.sum(),
                         (a64 * a64).sum()])
        self.dp.all_reduce_sum(m)
        n, s, ss = m[0], m[1], m[2]
        mean = s / n
        var = (ss - n * mean * mean) / (n - 1)
        return ((a64 - mean) / (var.clamp_min(0).sqrt() + 1e-5)).float()

    def compute_reward_gae(self, buf_len, buf_reward, buf_mask, buf_value, shape=None):
        """r_sum and GAE advantage, ElegantRL's recursion (agent.py:685-708), as one reverse scan per env lane."""
        T, N = shape if shape is not None else (buf_len, 1)
        value = buf_value.reshape(-1)
        r_sum, adv = self.backend.gae(buf_reward.reshape(T, N), buf_mask.reshape(T, N), value.reshape(T, N),
                                      self.lambda_gae_adv, True)
        return r_sum.reshape(-1), self._normalise_advantage(adv.reshape(-1))

    def compute_reward_adv(self, buf_len, buf_reward, buf_mask, buf_value, shape=None):
        T, N = shape if shape is not None else (buf_len, 1)
        value = buf_value.reshape(-1)
        r_sum, adv = self.backend.gae(buf_reward.reshape(T, N), buf_mask.reshape(T, N), value.reshape(T, N), 0.0, False)
        return r_sum.reshape(-1), self._normalise_advantage(adv.reshape(-1))
