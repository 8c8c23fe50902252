"""AgentSAC: soft actor-critic with automatic temperature (interface of /root/reference/elegantrl/agent.py:397-478,519-527).

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
step in lock-step, one policy forward per step."""
import os

import numpy as np
import torch

from . import logger
from .agent import AgentBase, _no_gc
from .net import ActorSAC, CriticTwin
from .replay import VecReplayBuffer


class AgentSAC(AgentBase):
    def __init__(self, backend=None, device=None):
        super().__init__(backend, device)
        self.target_entropy = 1.0   # * log(action_dim) in init (agent.py:403,407)
        self.alpha_log = None
        self.alpha_optimizer = None
        self.use_hip_graphs = True
        self.use_fused_update = os.environ.get("PIME_SAC_FUSED", "1") == "1"   # the optimizer step on the hand-written kernels
        self.use_fused_rollout = True   # vectorised env: a whole explore call / evaluation episode as ONE launch
        self._packed_act = None
        self.draw_hook = None   # tests: callable(n_steps, batch) -> (idx, nxt, noise_next, noise_pg) tables of a whole update
        self._fused_sac = None
        self._obs = None

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

    def _fused_step(self, batch_size):
        """ops.FusedSAC serving the current nets, or None -> the PyTorch modules (_one_update)."""
        if not self.use_fused_update or self.device.type != "cuda" or not hasattr(self.backend, "fused_sac"):
            return None
        f = self._fused_sac
        if f is False:
            return None
        if f is None or not f.wraps(self):
            f = self._fused_sac = self.backend.fused_sac(self, batch_size)
            if f is False:
                return None
        f.ensure_batch(batch_size)
        return f

    def _packed_actor(self):
        """ops.PackedMLP image of the actor (kind "sac_actor": body + both head rows) for the fused exploration / evaluation kernels,
        re-packed on every call (the weights change with every update_net); None when its shape has no fused forward."""
        if not self.use_fused_rollout or not hasattr(self.backend, "packed") or getattr(self.act, "action_dim", 1) != 1:
            return None
        if self._packed_act is None:
            self._packed_act = self.backend.packed(self.act) or False
        if self._packed_act is False:
            return None
        return self._packed_act.repack()

    def _fused_explore(self, env):
        """The packed actor if pime_rollout_offpolicy_sac serves `env` with it, else None -> lock-step by lock-step launches."""
        if not hasattr(env, "offpolicy_rollout_supported"):
            return None
        pk = self._packed_actor()
        if pk is None or not env.offpolicy_rollout_supported(pk):
            return None
        if not hasattr(self, "_rollout_seed"):
            self._rollout_seed = int(torch.initial_seed()) & (2 ** 63 - 1)   # exploration stream follows torch's seed
            self._rollout_epoch = 0
        return pk

    def fused_eval_policy(self, env):
        """(packed actor, priorK = zeros) if the fused evaluation kernel can run tanh(net_a_avg(s)) on `env` as one launch per
        episode (csrc/rollout_eval.hip), else None -> the evaluator steps the env launch by launch."""
        if not hasattr(env, "eval_supported"):
            return None
        pk = self._packed_actor()
        if pk is None or not env.eval_supported(pk):
            return None
        return pk, np.zeros(self.act.state_dim)

    def select_action(self, state, if_deterministic=False):
        states = torch.as_tensor(np.asarray(state)[None], dtype=torch.float32, device=self.device)
        with torch.no_grad():
            action = self.act(states)[0] if if_deterministic else self.act.get_action(states)[0]
        return action.cpu().numpy()

    def explore_env(self, env, buffer, target_step, reward_scale, gamma):
        if hasattr(env, "num_envs"):
            return self.explore_vec_env(env, buffer, target_step, reward_scale, gamma)
        return super().explore_env(env, buffer, target_step, reward_scale, gamma)   # agent.py:54-70 with get_action

    def explore_vec_env(self, env, buffer, target_step, reward_scale, gamma):
        """target_step transitions = target_step / N lock-steps of all N lanes, continuing the running episodes (AgentTD3's loop
        with the stochastic actor); the buffer stores the squashed action."""
        assert isinstance(buffer, VecReplayBuffer) and buffer.num_envs == env.num_envs
        N = env.num_envs
        steps = max(1, target_step // N)
        if buffer.stored_slots + steps < 2:
            steps = 2   # sampling needs one stored lock-step WITH a successor
        if self._obs is not None and getattr(self, "_obs_epoch", None) != (id(env), env.reset_count):
            buffer.cut_last_step()   # someone else reset this env since the last call (AgentTD3.explore_vec_env)
            self._obs = None
        if self._obs is None:
            self._obs = env.reset().clone()
            self._next_obs = torch.empty_like(self._obs)
            self._obs_epoch = (id(env), env.reset_count)
        pk = self._fused_explore(env)
        if pk is not None:   # ONE launch for the whole call: actor forward, re-parameterised sample, env step, ring writes
            done_steps = 0
            while done_steps < steps:
                n = min(steps - done_steps, buffer.slots)
                self._rollout_epoch += 1
                env.rollout_offpolicy(pk, np.zeros(self.act.state_dim), 0.0, gamma, reward_scale, n, self._rollout_seed,
                                      self._rollout_epoch, self._obs, buffer.state, buffer.other, buffer.next_slot)
                buffer.advance(n)
                done_steps += n
            return steps * N
        for _ in range(steps):
            obs = self._obs
            with torch.no_grad():
                a = self.act.get_action(obs)
            _, rew, done = env.step(a, auto_reset=True, out_obs=self._next_obs)
            with torch.no_grad():
                mask = (1.0 - done.to(torch.float32)) * gamma
                buffer.append_step(obs, rew * reward_scale if reward_scale != 1.0 else rew, mask, a)
            self._obs, self._next_obs = self._next_obs, self._obs
        return steps * N

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
        """update_net on the fused step: the sampled rows of ALL n_steps optimizer steps are drawn at once into an index table that
        the kernels read by row (a launch argument), the two normal draws per sample come from Philox streams 4 and 5 inside the
        kernels (`draw_hook` injects tables instead), and from the second call on the whole update -- n_steps x 4 launches -- is ONE
        HIP graph.  The temperature lives on the device; the only host synchronisation is the read of the loss words at the end."""
        dev = self.device
        vec = isinstance(buffer, VecReplayBuffer)
        st = getattr(f, "tables", None)
        if st is None or st["shape"] != (n_steps, batch_size):
            i64 = dict(dtype=torch.int64, device=dev)
            st = f.tables = {"shape": (n_steps, batch_size), "idx": torch.zeros((n_steps, batch_size), **i64),
                             "nxt": torch.zeros((n_steps, batch_size), **i64), "noise": None, "graph": None, "key": None, "warm": False}
        idx, nxt = st["idx"], st["nxt"]
        if self.draw_hook is not None:
            h_idx, h_nxt, h_n1, h_n2 = self.draw_hook(n_steps, batch_size)
            idx.copy_(torch.as_tensor(np.asarray(h_idx)).to(dev)); nxt.copy_(torch.as_tensor(np.asarray(h_nxt)).to(dev))
            if st["noise"] is None:
                st["noise"] = torch.zeros((2, n_steps, batch_size), dtype=torch.float32, device=dev)
            st["noise"][0].copy_(torch.as_tensor(np.asarray(h_n1)).to(dev).reshape(n_steps, batch_size))
            st["noise"][1].copy_(torch.as_tensor(np.asarray(h_n2)).to(dev).reshape(n_steps, batch_size))
        elif vec:   # VecReplayBuffer.sample_indices for the whole table: uniform over the rows that have a successor
            assert buffer.stored_slots >= 2, "need two stored steps before sampling"
            N = buffer.num_envs
            u = torch.randint(2 ** 62, (n_steps, batch_size), device=dev) % buffer._bounds[0]   # bounds live on the device (replay.py)
            lane = u % N
            slot = (u // N + buffer._bounds[1]) % buffer.slots
            torch.add(slot * N, lane, out=idx)
            torch.add(((slot + 1) % buffer.slots) * N, lane, out=nxt)
        else:       # ReplayBuffer.sample_batch: rows [0, now_len - 1), successor = the next row
            torch.randint(buffer.now_len - 1, (n_steps, batch_size), device=dev, out=idx)
            torch.add(idx, 1, out=nxt)
        noise = st["noise"] if self.draw_hook is not None else None
        if not hasattr(self, "_noise_seed"):
            self._noise_seed = (int(torch.initial_seed()) ^ 0x5DEECE66D) & (2 ** 63 - 1)   # the draws follow torch's seed
        f.loss.zero_()
        f.begin_update()   # table row 0; the noise epoch advances (a captured graph draws fresh noise in every replay)

        def run():
            for k in range(n_steps):   # the row is a launch argument: every node of the captured graph carries its own
                f.step(buffer.buf_state, buffer.buf_other, idx, nxt, None if noise is None else noise[0],
                       None if noise is None else noise[1], self.soft_update_tau, self.target_entropy, noise_seed=self._noise_seed, row=k)

        key = (buffer.buf_state.data_ptr(), buffer.buf_other.data_ptr(), noise is None, self.soft_update_tau, float(self.target_entropy))
        if self.use_hip_graphs and st["warm"] and (st["graph"] is None or st["key"] != key):
            try:
                torch.cuda.synchronize(dev)
                g = torch.cuda.CUDAGraph()
                with _no_gc(), torch.cuda.graph(g, capture_error_mode="thread_local"):
                    run()
                st["graph"], st["key"] = g, key
            except RuntimeError as exc:
                print(f"| HIP graph capture of the SAC update failed ({exc}); continuing with eager launches")
                self.use_hip_graphs = False
                torch.cuda.synchronize(dev)
                st["graph"] = None
        go = st["graph"].replay if (self.use_hip_graphs and st["graph"] is not None and st["key"] == key) else run
        go()
        st["warm"] = True
        f.row = n_steps        # (begin_update of the next call moves them into the optimizers' step base)
        self._n_updates += n_updates
        tot = f.loss.tolist()   # the update's only host synchronisation
        self._log(n_steps, tot[:4])
        return tot[4], tot[5]
