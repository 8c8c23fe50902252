"""AgentOffPolicy and AgentTD3 (interface of the reference's elegantrl/agent.py:276-394).  AgentOffPolicy is not in the reference:
it is the host path that AgentTD3 and AgentSAC (agent_sac.py) share."""
import os

import numpy as np
import torch

from . import logger
from .agent_base import AgentBase
from .graphs import capture, capture_on_every_rank, collective_in_graph
from .net import Actor, CriticTwin
from .replay import VecReplayBuffer


class AgentOffPolicy(AgentBase):
    """The host path AgentTD3 and AgentSAC share: exploration of a vectorised env into a `VecReplayBuffer` (one fused launch per
    call where the library serves the env and the actor -- `env.offpolicy_rollout_supported`: the TD3 Actor at width 64 / 128 / 256
    on pH, the Integrator tank and Stacking1 / 4 / 10, ActorSAC at width 64 / 128 on pH and the Integrator tank -- or lock-step by
    lock-step), and `update_net` on a fused optimizer step (ops.FusedTD3 / ops.FusedSAC): the tables of a
    whole update drawn at once, the update captured as ONE HIP graph from the second call on, one host read at the end.

    An agent names its fused step (`_fused_name`: the backend's factory and, with a leading underscore, the cache attribute) and
    supplies `_explore_actions`, `_rollout_sigma`, `_rollout_priorK` and the `f.step` closure of its `_update_fused`."""
    _fused_name = None   # "fused_td3" / "fused_sac"

    def __init__(self, backend=None, device=None):
        super().__init__(backend, device)
        self.use_hip_graphs = True
        self.use_graph_collective = True   # data parallel: capture the all-reduces inside the update's graph
        self.use_fused_rollout = True      # vectorised env: a whole explore call / evaluation episode as ONE launch
        self.draw_hook = None      # tests: callable(n_steps, batch) -> (idx, nxt, noise table(s)) of a whole update (injected draws)
        self.launch_timer = None   # bench.py: callable(name, fn) timing one update's launches with HIP events
        setattr(self, "_" + self._fused_name, None)   # None: not built yet; False: no fused step for these nets
        self._obs = None
        self._packed_act = None

    def _fused_step(self, batch_size):
        """The fused optimizer step (ops.FusedTD3 / ops.FusedSAC) serving the current nets, or None -> the PyTorch modules
        (_one_update)."""
        if not self.use_fused_update or self.device.type != "cuda" or not hasattr(self.backend, self._fused_name):
            return None
        f = getattr(self, "_" + self._fused_name)
        if f is False:
            return None
        if f is None or not f.wraps(self):
            f = getattr(self.backend, self._fused_name)(self, batch_size)
            setattr(self, "_" + self._fused_name, f)
            if f is False:
                return None
        f.ensure_batch(batch_size)
        return f

    # ---- exploration -------------------------------------------------------------------------------------
    def _rollout_priorK(self):
        """float64 prior gain of the fused exploration kernel's composition a_env = a + s @ priorK (zeros: no prior controller)."""
        return np.zeros(self.act.state_dim)

    def _rollout_sigma(self):
        """Standard deviation of the clipped Gaussian the fused exploration kernel adds to the actor's output."""
        raise NotImplementedError

    def _explore_actions(self, obs):
        """(stored action, env action) of one lock-step for the observation batch `obs`."""
        raise NotImplementedError

    def _packed_actor(self):
        """ops.PackedMLP image of the actor for the fused exploration / evaluation kernels (its caller re-packs it: the weights change
        with every update_net); None when its shape has no fused forward."""
        if not self.use_fused_rollout or not hasattr(self.backend, "packed") or getattr(self.act, "action_dim", 1) != 1:
            return None
        if self._packed_act is None:
            self._packed_act = self.backend.packed(self.act) or False
        return self._packed_act or None

    def _fused_explore(self, env):
        """The freshly re-packed actor if the fused exploration kernel serves `env` with it, else None -> lock-step by lock-step
        launches."""
        if not hasattr(env, "offpolicy_rollout_supported"):
            return None
        pk = self._packed_actor()
        if pk is None or not env.offpolicy_rollout_supported(pk):
            return None
        if not hasattr(self, "_rollout_seed"):
            self._rollout_seed = int(torch.initial_seed()) & (2 ** 63 - 1)   # exploration stream follows torch's seed
            self._rollout_epoch = 0
        return pk.repack()

    def explore_vec_env(self, env, buffer, target_step, reward_scale, gamma):
        """target_step transitions = target_step / N lock-steps of all N lanes, continuing the running episodes; finished
        lanes are reset inside the env kernel and their next row holds the new episode's first observation."""
        assert isinstance(buffer, VecReplayBuffer) and buffer.num_envs == env.num_envs
        N = env.num_envs
        steps = max(1, target_step // N)
        if buffer.stored_slots + steps < 2:
            steps = 2   # sampling needs one stored lock-step WITH a successor (replay.py: row i and row i + N)
        if self._obs is not None and getattr(self, "_obs_epoch", None) != (id(env), env.reset_count):
            # someone else reset this env since the last call (the evaluator, when it shares the training env): the cached
            # observation is stale and the lanes sit in a post-evaluation state.  Start new episodes, and cut the newest
            # stored lock-step off from what follows it (its successor slot will hold a reset observation).
            buffer.cut_last_step()
            self._obs = None
        if self._obs is None:
            self._obs = env.reset().clone()
            self._next_obs = torch.empty_like(self._obs)
            self._obs_epoch = (id(env), env.reset_count)
        pk = self._fused_explore(env)
        if pk is not None:   # ONE launch for the whole call: actor forward, noise, composition, env step, ring writes
            done_steps = 0
            while done_steps < steps:
                n = min(steps - done_steps, buffer.slots)
                self._rollout_epoch += 1
                env.rollout_offpolicy(pk, self._rollout_priorK(), self._rollout_sigma(), gamma, reward_scale, n, self._rollout_seed,
                                      self._rollout_epoch, self._obs, buffer.state, buffer.other, buffer.next_slot)
                buffer.advance(n)
                done_steps += n
            return steps * N
        for _ in range(steps):
            obs = self._obs
            with torch.no_grad():
                a, a_env = self._explore_actions(obs)
            _, rew, done = env.step(a_env, auto_reset=True, out_obs=self._next_obs)
            with torch.no_grad():
                mask = (1.0 - done.to(torch.float32)) * gamma
                buffer.append_step(obs, rew * reward_scale if reward_scale != 1.0 else rew, mask, a)
            self._obs, self._next_obs = self._next_obs, self._obs
        return steps * N

    # ---- update_net on the fused step --------------------------------------------------------------------
    def _draw_tables(self, f, buffer, n_steps, batch_size, n_noise):
        """First stage of an update on the fused step `f`: the sampled rows of ALL n_steps optimizer steps drawn at once into the
        index tables idx / nxt (int64 [n_steps, batch_size]) that the kernels read by row; `draw_hook` injects them instead, with
        n_noise tables of normal draws.  Then table row 0 and the next noise epoch.  Returns (idx, nxt, the list of noise tables or
        None: Philox in the kernels)."""
        dev = self.device
        st = f.tables
        if st is None or st["shape"] != (n_steps, batch_size):
            i64 = dict(dtype=torch.int64, device=dev)
            st = f.tables = {"shape": (n_steps, batch_size), "idx": torch.zeros((n_steps, batch_size), **i64),
                             "nxt": torch.zeros((n_steps, batch_size), **i64), "noise": None, "graph": None, "key": None, "warm": False}
        idx, nxt, noise = st["idx"], st["nxt"], None
        if self.draw_hook is not None:
            h_idx, h_nxt, *h_noise = self.draw_hook(n_steps, batch_size)
            assert len(h_noise) == n_noise
            idx.copy_(torch.as_tensor(h_idx).to(dev)); nxt.copy_(torch.as_tensor(h_nxt).to(dev))
            if st["noise"] is None:
                st["noise"] = torch.zeros((n_noise, n_steps, batch_size), dtype=torch.float32, device=dev)
            for dst, h in zip(st["noise"], h_noise):
                dst.copy_(torch.as_tensor(h).to(dev).reshape(n_steps, batch_size))
            noise = list(st["noise"])
        elif isinstance(buffer, VecReplayBuffer):   # its sample_indices for the whole table: uniform over the rows that have a successor
            assert buffer.stored_slots >= 2, "need two stored steps before sampling"
            N = buffer.num_envs
            u = torch.randint(2 ** 62, (n_steps, batch_size), device=dev) % buffer._bounds[0]   # bounds live on the device (replay.py)
            lane = u % N
            slot = (u // N + buffer._bounds[1]) % buffer.slots                   # slots in age order start at the oldest
            torch.add(slot * N, lane, out=idx)
            torch.add(((slot + 1) % buffer.slots) * N, lane, out=nxt)            # successor: same lane, next slot
        else:       # ReplayBuffer.sample_batch (replay.py:344-351): rows [0, now_len - 1), successor = the next row
            torch.randint(buffer.now_len - 1, (n_steps, batch_size), device=dev, out=idx)
            torch.add(idx, 1, out=nxt)
        if not hasattr(self, "_noise_seed"):
            self._noise_seed = (int(torch.initial_seed()) ^ 0x5DEECE66D) & (2 ** 63 - 1)   # the kernels' draws follow torch's seed
        f.loss.zero_()
        f.begin_update()   # table row 0; the noise epoch advances (a captured graph draws fresh noise in every replay)
        return idx, nxt, noise

    def _run_update(self, f, run, key, name, n_steps, n_updates):
        """Second stage: `run` launches every optimizer step of the update on the current stream.  After the first (warm, eager)
        update it is captured as ONE HIP graph, replayed while `key` -- everything the graph bakes in besides f's own tensors --
        stays the same.  Returns f.loss as a list: the update's only host synchronisation."""
        dev, st = self.device, f.tables
        # data parallel: the all-reduces of every step are captured inside the update's graph where the communicator allows it
        # (RCCL: yes; gloo and a refused capture: eager launches, decided for all ranks together)
        can_graph = self.use_hip_graphs and (self.dp is None or collective_in_graph(self))
        if can_graph and st["warm"] and (st["graph"] is None or st["key"] != key):
            st["graph"], refused = capture_on_every_rank(self.dp, dev, run)   # (the ranks must agree on the launch form)
            if st["graph"] is not None:
                st["key"] = key
            elif self.dp is not None:
                print(f"| all-reduce inside the {name.upper()} update's HIP graph refused on a rank ({refused}); every rank launches eagerly")
                self.use_graph_collective, can_graph = False, False
            else:
                print(f"| HIP graph capture of the {name.upper()} update failed ({refused}); continuing with eager launches")
                self.use_hip_graphs = can_graph = False
        go = st["graph"].replay if (can_graph and st["graph"] is not None and st["key"] == key) else run
        if self.launch_timer is not None:
            self.launch_timer(name + "_update", go)
        else:
            go()
        st["warm"] = True
        f.row = n_steps        # (begin_update of the next call moves them into the optimizers' step base)
        self._n_updates += n_updates
        tot = f.loss.tolist()
        if self.dp is not None:
            self.dp.check()     # a timed-out one-shot all-reduce left gradients un-averaged: fatal, here where the stream is drained
        return tot


# ================================================================================================= TD3
class AgentTD3(AgentOffPolicy):
    """Twin-delayed DDPG (agent.py:276-394): twin critics, target policy smoothing, delayed soft target updates.

    One-instance env + flat ring buffer: the reference's loop, op for op (pinned against the reference's weights by
    tests/test_td3_golden_cpu.py).  Vectorised env (`env.num_envs`) + `VecReplayBuffer`: all lanes step in lock-step through
    the HIP env kernel, transitions stay in HBM, and `update_net` runs target_step / num_envs * repeat_times optimizer steps
    (the reference's "one gradient step per env step" counted per LOCK-STEP, not per lane).  On the GPU an optimizer step is
    four hand-written launches (`pime_td3_step`, csrc/td3_fused.hip: critic gradients, slab reduction + Adam + delayed soft
    update, actor gradients through the target critic, the same for the actor), a whole update_net one HIP graph
    (AgentOffPolicy); shapes the kernels do not serve (state_dim > 31, widths other than 64 / 128 / 256) and CPU tensors run
    the same arithmetic as PyTorch modules (`_one_update`).  Exploration of a vectorised env is ONE launch per call
    (`pime_rollout_offpolicy`) at width 64 / 128 / 256 on pH, the Integrator tank and the Stacking1 / 4 / 10 tank; an evaluation
    episode is ONE launch (`fused_eval_policy` -> `pime_rollout_eval`) at width 64 / 128 / 256 on pH and the Integrator tank and
    at width 256 on Stacking1 / 4 / 10; elsewhere all lanes step in lock-step, one policy forward per step."""
    _fused_name = "fused_td3"

    def __init__(self, backend=None, device=None):
        super().__init__(backend, device)
        self.explore_noise = 0.1
        self.policy_noise = 0.2
        self.update_freq = 2
        self.use_fused_update = os.environ.get("PIME_TD3_FUSED", "1") == "1"   # the optimizer step on the hand-written kernels
        self._graphs = None

    def init(self, net_dim, state_dim, action_dim, if_per=False):
        assert not if_per, "prioritised replay is not on the residual-control path"
        self._pick_device()
        from copy import deepcopy
        self.cri = CriticTwin(net_dim, state_dim, action_dim).to(self.device)
        self.cri_target = deepcopy(self.cri)
        self.act = Actor(net_dim, state_dim, action_dim).to(self.device)
        self.act_target = deepcopy(self.act)
        self._make_optimizers()
        self.criterion = torch.nn.SmoothL1Loss()
        self.get_obj_critic = self.get_obj_critic_raw

    def _make_optimizers(self):
        kw = dict(fused=True, capturable=True) if self.device.type == "cuda" else {}
        self.cri_optimizer = torch.optim.Adam(self.cri.parameters(), lr=self.learning_rate, **kw)
        self.act_optimizer = torch.optim.Adam(self.act.parameters(), lr=self.learning_rate, **kw)
        self._graphs = None
        self._packed_act = None
        self._fused_td3 = None   # its Adam moments belong to the optimizers just replaced

    def weights_changed(self):
        super().weights_changed()
        self._graphs = None   # (the fused step reads the parameters where they live: nothing of it goes stale)

    def _prior_term(self, states):
        """Prior-controller part of the env action (none for plain TD3)."""
        return None

    def _rollout_sigma(self):
        return self.explore_noise

    def fused_eval_policy(self, env):
        """(packed actor, priorK) if the fused evaluation kernel can run a_env = tanh(net(s)) + s @ priorK on `env` as one launch
        per episode -- what the evaluator's module path computes (`self.act`, or AgentResidualTD3.eval_policy) -- else None -> the
        evaluator steps the env launch by launch.  priorK: zeros for plain TD3, the prior gain for the residual agent."""
        if not hasattr(env, "eval_supported"):
            return None
        pk = self._packed_actor()
        if pk is None or not env.eval_supported(pk):
            return None
        return pk.repack(), self._rollout_priorK()

    def _explore_actions(self, obs):
        a = self.act(obs)
        a = (a + torch.randn_like(a) * self.explore_noise).clamp(-1, 1)   # agent.py:305
        prior = self._prior_term(obs)
        return a, (a if prior is None else a + prior)

    def select_action(self, state, if_deterministic=False):
        states = torch.as_tensor(np.asarray(state)[None], dtype=torch.float32, device=self.device)
        with torch.no_grad():
            action = self.act(states)[0]
            if not if_deterministic:
                action = (action + torch.randn_like(action) * self.explore_noise).clamp(-1, 1)
        return action.cpu().numpy()

    def _env_action(self, state, action):
        """What a one-instance env receives for the stored `action` (the residual agents add the prior term)."""
        return action

    def explore_env(self, env, buffer, target_step, reward_scale, gamma):
        if hasattr(env, "num_envs"):
            return self.explore_vec_env(env, buffer, target_step, reward_scale, gamma)
        for _ in range(target_step):   # agent.py:54-70, continuing from self.state
            action = self.select_action(self.state)
            next_s, reward, done, _ = env.step(self._env_action(self.state, action))
            buffer.append_buffer(self.state, (reward * reward_scale, 0.0 if done else gamma, *action))
            self.state = env.reset() if done else next_s
        return target_step

    def get_obj_critic_raw(self, buffer, batch_size):
        with torch.no_grad():
            reward, mask, action, state, next_s = buffer.sample_batch(batch_size)
            next_a = self.act_target.get_action(next_s, self.policy_noise)
            next_q = torch.min(*self.cri_target.get_q1_q2(next_s, next_a))
            q_label = reward + mask * next_q
        q1, q2 = self.cri.get_q1_q2(state, action)
        return self.criterion(q1, q_label) + self.criterion(q2, q_label), state

    def _one_update(self, buffer, batch_size, soft):
        """One iteration of the reference's loop (agent.py:314-331).  Data parallel (the reference has no collective): every rank
        samples its own minibatch from its own lanes and the gradients of BOTH backward passes are averaged before their optimizer
        step -- the two means over batch_size samples become the means over the union of the ranks' minibatches, so G ranks make the
        step of one rank on a G x batch_size minibatch (tests/test_dist_gloo.py) and the replicas stay identical.  Two all-reduces per
        step: the actor's objective needs the critic's step applied."""
        obj_critic, state = self.get_obj_critic(buffer, batch_size)
        self.cri_optimizer.zero_grad(set_to_none=False)
        obj_critic.backward()
        if self.dp is not None:
            self.dp.average_gradients([p for p in self.cri.parameters() if p.grad is not None])
        self.cri_optimizer.step()
        if soft:
            self.soft_update(self.cri_target, self.cri, self.soft_update_tau)
        obj_actor = -self.cri_target(state, self.act(state)).mean()
        self.act_optimizer.zero_grad(set_to_none=False)
        obj_actor.backward()
        if self.dp is not None:
            self.dp.average_gradients([p for p in self.act.parameters() if p.grad is not None])
        self.act_optimizer.step()
        if soft:
            self.soft_update(self.act_target, self.act, self.soft_update_tau)
        return obj_actor.detach(), obj_critic.detach()

    def update_net(self, buffer, target_step, batch_size, repeat_times):
        buffer.update_now_len_before_sample()
        dev = self.device
        vec = isinstance(buffer, VecReplayBuffer)
        n_steps = int(target_step * repeat_times) if not vec else max(1, int(target_step // buffer.num_envs * repeat_times))
        fused = self._fused_step(batch_size) if n_steps else None
        if fused is not None:
            return self._update_fused(fused, buffer, n_steps, batch_size, int(target_step if not vec else n_steps))
        sums = torch.zeros(2, device=dev)
        obj_actor = obj_critic = torch.zeros((), device=dev)
        use_graphs = vec and self.use_hip_graphs and dev.type == "cuda" and self.dp is None   # (the all-reduces run eagerly)
        graphs = self._graphs if use_graphs else None
        key = (id(buffer), batch_size)
        for i in range(n_steps):
            soft = i % self.update_freq == 0
            if use_graphs and (i >= 2 or (graphs and graphs.get("key") == key)):
                # the step's launch sequence is fixed once Adam's state exists (two eager steps): capture it twice (with /
                # without the delayed soft update) and replay.  The sampler reads its index bounds from the device
                # (VecReplayBuffer._bounds), so the two graphs serve every later call as well.
                if graphs is None or graphs.get("key") != key:
                    graphs = self._capture_updates(buffer, batch_size, key)
                    self._graphs = graphs
                if graphs:
                    g = graphs[soft]
                    g["graph"].replay()
                    sums += g["out"]
                    obj_actor, obj_critic = g["out"][0], g["out"][1]
                    continue
            obj_actor, obj_critic = self._one_update(buffer, batch_size, soft)
            sums += torch.stack([obj_actor, obj_critic])
        self._n_updates += int(target_step if not vec else n_steps)
        if n_steps:
            mean = (sums / n_steps).tolist()
            logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
            logger.record("train/actor_loss", mean[0])
            logger.record("train/critic_loss", mean[1])
        return float(obj_actor), float(obj_critic) / 2

    def _update_fused(self, f, buffer, n_steps, batch_size, n_updates):
        """update_net on the fused step (AgentOffPolicy._draw_tables / _run_update): the smoothing noise is drawn inside the critic
        kernel (Philox stream 3; `draw_hook` injects a table instead) and the whole update -- n_steps x 4 launches -- is ONE HIP
        graph.  The only host synchronisation is the read of the four loss words at the end."""
        idx, nxt, noise = self._draw_tables(f, buffer, n_steps, batch_size, 1)
        noise = None if noise is None else noise[0]

        def one(k, phases):   # the row is a launch argument: every node of the captured graph carries its own
            f.step(buffer.buf_state, buffer.buf_other, idx, nxt, noise, self.soft_update_tau, self.update_freq, self.policy_noise,
                   noise_seed=self._noise_seed, row=k, phases=phases)

        def run():
            """Every optimizer step's launches, in order, on the current stream."""
            if self.dp is not None:
                # data parallel: a net's slab reduction leaves THIS rank's gradient, the ranks average it, Adam (+ the delayed soft
                # update) is applied from the averaged tensor -- five launches and two all-reduces per step (ops.FusedTD3.step_dp); G
                # ranks with their own minibatches make the step of one rank on the union minibatch
                for k in range(n_steps):
                    one(k, 1 | 16)
                    self.dp.all_reduce_mean(f.cri_grad)
                    one(k, 32 | 4 | 64)
                    self.dp.all_reduce_mean(f.act_grad)
                    one(k, 128)
                return
            for k in range(n_steps):
                one(k, 15)

        key = (buffer.buf_state.data_ptr(), buffer.buf_other.data_ptr(), noise is None, self.soft_update_tau, self.update_freq,
               self.policy_noise, self.dp is not None)
        tot = self._run_update(f, run, key, "td3", n_steps, n_updates)
        logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        logger.record("train/actor_loss", tot[0] / n_steps)
        logger.record("train/critic_loss", tot[1] / n_steps)
        return tot[2], tot[3] / 2

    def _capture_updates(self, buffer, batch_size, key):
        out = {"key": key}
        try:
            for soft in (True, False):
                res = torch.zeros(2, device=self.device)

                def one_update():
                    oa, oc = self._one_update(buffer, batch_size, soft)
                    res.copy_(torch.stack([oa, oc]))
                out[soft] = {"graph": capture(self.device, one_update), "out": res}
            return out
        except RuntimeError as exc:   # keep training on eager launches
            print(f"| HIP graph capture of the TD3 update failed ({exc}); continuing with eager launches")
            self.use_hip_graphs = False
            torch.cuda.synchronize(self.device)
            return {}
