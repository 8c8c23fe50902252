"""AgentSAC: soft actor-critic with automatic temperature (interface of the reference's elegantrl/agent.py:397-478,519-527).

One iteration of `update_net`, in the reference's order:
  1. critic: next_a, next_lp = act.get_action_logprob(next_s) on the ONLINE actor, q_label = r + mask * (min(cri_target(next_s,
     next_a)) + next_lp * alpha), SmoothL1 on both heads, Adam, soft update of cri_target on EVERY step (there is no actor target);
  2. temperature: a_pg, lp = act.get_action_logprob(state), obj_alpha = (alpha_log * (lp - target_entropy).detach()).mean(), Adam
     on the scalar alpha_log;
  3. actor: alpha = exp(alpha_log) AFTER step 2, obj_actor = -(min(cri_target.get_q1_q2(state, a_pg)) + lp * alpha).mean() through
     the target critic AFTER step 1's soft update, Adam.
"logprob" is the reference's name for the NEGATIVE log-density (net.py:207-239); it is used with that sign throughout.

Three paths, chosen like AgentTD3 chooses:
  * CPU tensors (one-instance env + flat ReplayBuffer): the reference's loop op for op on the PyTorch modules
    (tests/test_sac_golden_cpu.py pins it against the reference's own weights);
  * GPU, a shape `pime_sac_step` serves (width 64 / 128, state_dim 1..7, action_dim 1): four hand-written launches per optimizer
    step (csrc/sac_fused.hip), the index tables of the whole update drawn at once, one HIP graph per `update_net` from the
    second call on, one host read at the end;
  * GPU, any other shape: the modules, with the one-time RuntimeWarning of backend.py.
Exploration on a vectorised env is ONE launch per call where `pime_rollout_offpolicy_sac` serves the env and the actor (pH /
water-tank Integrator observation, width 64 / 128), evaluation one launch per episode (`fused_eval_policy`); otherwise all lanes
step in lock-step, one policy forward per step.

The exploration loop, the packed-actor cache, the table and capture-or-replay stages of the fused update are agent_offpolicy.py's
AgentOffPolicy, shared with AgentTD3; this file holds what is SAC's own."""
import os

import numpy as np
import torch

from . import logger
from .agent_offpolicy import AgentOffPolicy
from .net import ActorSAC, CriticTwin
from .replay import VecReplayBuffer


class AgentSAC(AgentOffPolicy):
    _fused_name = "fused_sac"

    def __init__(self, backend=None, device=None):
        super().__init__(backend, device)
        self.target_entropy = 1.0   # * log(action_dim) in init (agent.py:403,407)
        self.alpha_log = None
        self.alpha_optimizer = None
        self.use_fused_update = os.environ.get("PIME_SAC_FUSED", "1") == "1"   # the optimizer step on the hand-written kernels

    # data parallelism is not built for SAC: refuse the object instead of training un-averaged replicas
    @property
    def dp(self):
        return None

    @dp.setter
    def dp(self, value):
        if value is not None:
            raise NotImplementedError("AgentSAC has no data-parallel path: run it on one GPU (train.py without torchrun)")

    def init(self, net_dim, state_dim, action_dim, if_per=False):
        assert not if_per, "prioritised replay is not on the residual-control path"
        self._pick_device()
        from copy import deepcopy
        self.target_entropy *= np.log(action_dim)
        self.alpha_log = torch.tensor((-np.log(action_dim) * np.e,), dtype=torch.float32, requires_grad=True, device=self.device)
        self.cri = CriticTwin(net_dim, state_dim, action_dim).to(self.device)
        self.cri_target = deepcopy(self.cri)
        self.act = ActorSAC(net_dim, state_dim, action_dim).to(self.device)
        self._make_optimizers()
        self.criterion = torch.nn.SmoothL1Loss()
        self.get_obj_critic = self.get_obj_critic_raw

    def _make_optimizers(self):
        self.alpha_optimizer = torch.optim.Adam((self.alpha_log,), self.learning_rate)
        self.cri_optimizer = torch.optim.Adam(self.cri.parameters(), lr=self.learning_rate)
        self.act_optimizer = torch.optim.Adam(self.act.parameters(), lr=self.learning_rate)
        self._fused_sac = None   # its Adam moments belong to the optimizers just replaced
        self._packed_act = None

    def fused_eval_policy(self, env):
        """(packed actor, priorK = zeros) if the fused evaluation kernel can run tanh(net_a_avg(s)) on `env` as one launch per
        episode (csrc/rollout_eval.hip), else None -> the evaluator steps the env launch by launch."""
        if not hasattr(env, "eval_supported"):
            return None
        pk = self._packed_actor()
        if pk is None or not env.eval_supported(pk):
            return None
        return pk.repack(), self._rollout_priorK()

    def _rollout_sigma(self):
        return 0.0   # the fused kernel draws the re-parameterised sample itself: no Gaussian on top

    def _explore_actions(self, obs):
        a = self.act.get_action(obs)   # the buffer stores the squashed action, which is what the env receives
        return a, a

    def select_action(self, state, if_deterministic=False):
        states = torch.as_tensor(np.asarray(state)[None], dtype=torch.float32, device=self.device)
        with torch.no_grad():
            action = self.act(states)[0] if if_deterministic else self.act.get_action(states)[0]
        return action.cpu().numpy()

    def explore_env(self, env, buffer, target_step, reward_scale, gamma):
        if hasattr(env, "num_envs"):
            return self.explore_vec_env(env, buffer, target_step, reward_scale, gamma)
        return super().explore_env(env, buffer, target_step, reward_scale, gamma)   # agent.py:54-70 with get_action

    def get_obj_critic_raw(self, buffer, batch_size, alpha, draws=None):
        """agent.py:519-527.  draws: (idx, nxt, noise_next) of an injected minibatch, or None: sampled here."""
        with torch.no_grad():
            if draws is None:
                reward, mask, action, state, next_s = buffer.sample_batch(batch_size)
                next_a, next_logprob = self.act.get_action_logprob(next_s)
            else:
                idx, nxt, noise = draws
                r_m_a = buffer.buf_other[idx]
                reward, mask, action, state, next_s = r_m_a[:, 0:1], r_m_a[:, 1:2], r_m_a[:, 2:], buffer.buf_state[idx], buffer.buf_state[nxt]
                next_a, next_logprob = self.act.get_action_logprob(next_s, noise.reshape(-1, 1))
            next_q = torch.min(*self.cri_target.get_q1_q2(next_s, next_a))
            q_label = reward + mask * (next_q + next_logprob * alpha)
        q1, q2 = self.cri.get_q1_q2(state, action)
        return self.criterion(q1, q_label) + self.criterion(q2, q_label), state

    def _one_update(self, buffer, batch_size, alpha, draws=None):
        """One iteration of the reference's loop (agent.py:442-468); returns (obj_actor, obj_critic, obj_alpha, alpha) detached."""
        obj_critic, state = self.get_obj_critic(buffer, batch_size, alpha, None if draws is None else draws[:3])
        self.cri_optimizer.zero_grad()
        obj_critic.backward()
        self.cri_optimizer.step()
        self.soft_update(self.cri_target, self.cri, self.soft_update_tau)

        action_pg, logprob = self.act.get_action_logprob(state, None if draws is None else draws[3].reshape(-1, 1))
        obj_alpha = (self.alpha_log * (logprob - self.target_entropy).detach()).mean()
        self.alpha_optimizer.zero_grad()
        obj_alpha.backward()
        self.alpha_optimizer.step()

        alpha = self.alpha_log.exp().detach()
        obj_actor = -(torch.min(*self.cri_target.get_q1_q2(state, action_pg)) + logprob * alpha).mean()
        self.act_optimizer.zero_grad()
        obj_actor.backward()
        self.act_optimizer.step()
        return obj_actor.detach(), obj_critic.detach(), obj_alpha.detach(), alpha

    def _log(self, n_steps, sums):
        logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        if n_steps:
            logger.record("train/ent_coef", sums[3] / n_steps)
            logger.record("train/ent_coef_loss", sums[2] / n_steps)
            logger.record("train/actor_loss", sums[0] / n_steps)
            logger.record("train/critic_loss", sums[1] / n_steps)

    def update_net(self, buffer, target_step, batch_size, repeat_times):
        buffer.update_now_len_before_sample()
        dev = self.device
        vec = isinstance(buffer, VecReplayBuffer)
        n_steps = int(target_step * repeat_times) if not vec else max(1, int(target_step // buffer.num_envs * repeat_times))
        n_updates = int(target_step if not vec else n_steps)
        fused = self._fused_step(batch_size) if n_steps else None
        if fused is not None:
            return self._update_fused(fused, buffer, n_steps, batch_size, n_updates)
        alpha = self.alpha_log.exp().detach()
        sums = torch.zeros(4, device=dev)
        last = torch.zeros(4, device=dev)
        tables = None
        if self.draw_hook is not None:
            tables = [torch.as_tensor(np.asarray(t)).to(dev) for t in self.draw_hook(n_steps, batch_size)]
            tables = [tables[0].long(), tables[1].long(), tables[2].float().reshape(n_steps, -1), tables[3].float().reshape(n_steps, -1)]
        for k in range(n_steps):
            draws = None if tables is None else tuple(t[k] for t in tables)
            out = self._one_update(buffer, batch_size, alpha, draws)
            alpha = out[3]
            last = torch.stack([o.reshape(()) for o in out])
            sums += last
        self._n_updates += n_updates
        self._log(n_steps, sums.tolist())
        last = last.tolist()
        return last[0], last[1]

    def _update_fused(self, f, buffer, n_steps, batch_size, n_updates):
        """update_net on the fused step (AgentOffPolicy._draw_tables / _run_update): the two normal draws per sample come from Philox
        streams 4 and 5 inside the kernels (`draw_hook` injects tables instead) and the whole update -- n_steps x 4 launches -- is ONE
        HIP graph.  The temperature lives on the device; the only host synchronisation is the read of the loss words at the end."""
        idx, nxt, noise = self._draw_tables(f, buffer, n_steps, batch_size, 2)
        noise_next, noise_pg = noise or (None, None)

        def run():
            for k in range(n_steps):   # the row is a launch argument: every node of the captured graph carries its own
                f.step(buffer.buf_state, buffer.buf_other, idx, nxt, noise_next, noise_pg, self.soft_update_tau, self.target_entropy,
                       noise_seed=self._noise_seed, row=k)

        key = (buffer.buf_state.data_ptr(), buffer.buf_other.data_ptr(), noise is None, self.soft_update_tau, float(self.target_entropy))
        tot = self._run_update(f, run, key, "sac", n_steps, n_updates)
        self._log(n_steps, tot[:4])
        return tot[4], tot[5]
