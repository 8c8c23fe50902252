"""AgentBase: what every agent has (interface of the reference's elegantrl/agent.py:15-124) -- device and backend, the
one-instance exploration loop, checkpoints, the soft target update."""
import os

import numpy as np
import torch

from ..backend import HipBackend


class AgentBase:
    def __init__(self, backend=None, device=None):
        self.learning_rate = 1e-4
        self.soft_update_tau = 2 ** -8
        self.state = None
        self.device = torch.device(device) if device is not None else None
        self.backend = backend if backend is not None else HipBackend()
        self.act = self.act_target = None
        self.cri = self.cri_target = None
        self.act_optimizer = self.cri_optimizer = None
        self.criterion = None
        self.get_obj_critic = None
        self.if_on_policy = False
        self._n_updates = 0
        self.dp = None          # pime_amd.dist.DataParallel when training sharded
        self.index_hook = None  # tests: callable(step, buf_len, batch_size) -> LongTensor of minibatch indices
        self.index_table_hook = None  # tests: callable(n_steps, buf_len, batch_size) -> LongTensor [n_steps, batch_size], the
        #                               whole update's minibatches at once (keeps the one-graph-per-step path, unlike index_hook)

    def _pick_device(self):
        if self.device is None:
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.backend.check_device(self.device)
        return self.device

    def select_action(self, state):
        states = torch.as_tensor(np.asarray(state)[None], dtype=torch.float32, device=self.device)
        with torch.no_grad():
            return self.act(states)[0].cpu().numpy()

    def explore_env(self, env, buffer, target_step, reward_scale, gamma):
        """Off-policy default: `target_step` transitions continuing from self.state (agent.py:54-70)."""
        for _ in range(target_step):
            action = self.select_action(self.state)
            next_s, reward, done, _ = env.step(action)
            buffer.append_buffer(self.state, (reward * reward_scale, 0.0 if done else gamma, *action))
            self.state = env.reset() if done else next_s
        return target_step

    def update_net(self, buffer, target_step, batch_size, repeat_times):
        raise NotImplementedError

    def save_load_model(self, cwd, if_save):
        """actor.pth / critic.pth state_dicts, the reference's checkpoint layout (agent.py:86-114).  Loading uses
        weights_only=True: nothing in the file is executed."""
        paths = {"act": os.path.join(cwd, "actor.pth"), "cri": os.path.join(cwd, "critic.pth")}
        for name, path in paths.items():
            net = getattr(self, name)
            if net is None:
                continue
            if if_save:
                torch.save(net.state_dict(), path)
            elif os.path.exists(path):
                net.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
                print(f"Loaded {name}:", cwd)
            else:
                print(f"FileNotFound when load {name}: {cwd}")
        if not if_save:
            self.weights_changed()

    def weights_changed(self):
        """Invalidate packed (kernel-layout) copies of the weights."""
        fused = getattr(self, "_packed", {}).get("fused")
        self._packed = {}
        if fused and fused.params_are(self):   # (False = "no fused kernel for these nets", remembered below)
            fused.repack()
            self._packed["fused"] = fused

    @staticmethod
    def soft_update(target_net, current_net, tau):
        """target <- (1 - tau) target + tau current (agent.py:116-124), as two multi-tensor launches per net on the GPU (the
        per-parameter loop is ~40 small launches per delayed update of a TD3 agent)."""
        with torch.no_grad():
            tar, cur = list(target_net.parameters()), list(current_net.parameters())
            if tar and tar[0].is_cuda:
                torch._foreach_mul_(tar, 1 - tau)
                torch._foreach_add_(tar, cur, alpha=tau)
                return
            for t, c in zip(tar, cur):
                t.mul_(1 - tau).add_(c, alpha=tau)
