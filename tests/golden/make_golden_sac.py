#!/usr/bin/env python3
"""Generate tests/golden/sac_update*.npz by running the UNMODIFIED reference AgentSAC: net_dim 128 on the water-tank Integrator
observation (state_dim 4), batch 4 096, FOUR iterations of update_net on a flat ring.

Container-only, like make_golden.py (whose reference import, shims and save() this reuses; that file and golden_meta.json are left
as they are).  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sac.py

Three files, each under 1 MiB.  What they pin (prefix "sac:"):
  sac_update.npz
    * state [4200, 4], other [4200, 3]: a flat ring of random transitions (reward * scale, mask, action), float32;
    * indices [4, 4096]: the rows torch.randint sampled in each iteration (successors are index + 1: flat ring);
    * noise_next, noise_pg [4, 4096]: the two torch.randn_like draws of each iteration, in call order (get_obj_critic_raw's on
      next_s first, the policy-gradient sample on state second; elegantrl/agent.py:522,452);
    * obj: (obj_actor, obj_critic) as update_net returns them (the fourth iteration's); alpha_log: [initial, after step 1, after
      step 4]; grad1:alpha_log: the temperature's .grad at step 1;
    * hyper: net_dim, state_dim, batch, iterations, learning_rate, soft_update_tau, target_entropy.
  sac_update_nets0.npz
    * act0.*, cri0.*: the initial online ActorSAC / CriticTwin of AgentSAC.init(128, 4, 1) under torch.manual_seed(41) (the target
      critic is the reference's own deepcopy, so it is not stored twice);
    * grad1:cri.*, grad1:act.*: the critic's .grad after obj_critic.backward() and the actor's after obj_actor.backward() of the
      first iteration.
  sac_update_steps.npz
    * act_step1.*, cri_step1.*, cri_target_step1.*; act_step4.*, cri_step4.*, cri_target_step4.*: the nets after the first and the
      fourth iteration.  Step 2 is the first whose critic objective sees an alpha != 1 and a target critic that differs from
      the online one."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference and the shims on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

MD, D, B, N, ITERS = 128, 4, 4096, 4200, 4


def golden_sac_update():
    from elegantrl.agent import AgentSAC
    from elegantrl.replay import ReplayBuffer
    out = {}
    torch.manual_seed(41)
    agent = AgentSAC()
    agent.init(MD, D, 1)
    rng = np.random.RandomState(17)
    buf = ReplayBuffer(max_len=N + 8, state_dim=D, action_dim=1, if_on_policy=False, if_per=False, if_gpu=True)
    state = (rng.rand(N, D) * 10 - np.array([0, 0, 0, 5.])).astype(np.float32)   # tank levels, goal, integrator
    other = np.stack([-rng.rand(N) * 5, np.where(rng.rand(N) < 0.02, 0.0, 0.99), np.tanh(rng.randn(N))], axis=1).astype(np.float32)
    buf.extend_buffer(torch.as_tensor(state), torch.as_tensor(other))
    out.update(mg._sd_to_np("sac:act0", agent.act.state_dict()))
    out.update(mg._sd_to_np("sac:cri0", agent.cri.state_dict()))
    alpha_logs = [agent.alpha_log.item()]
    idx_log, noise_log, steps = [], [], {"cri": 0, "act": 0, "alpha": 0}
    orig_randint, orig_randn_like = torch.randint, torch.randn_like
    orig = {"cri": agent.cri_optimizer.step, "act": agent.act_optimizer.step, "alpha": agent.alpha_optimizer.step}

    def rec_randint(*a, **k):
        v = orig_randint(*a, **k)
        idx_log.append(v.numpy().astype(np.int32))
        return v

    def rec_randn_like(t, **k):
        v = orig_randn_like(t, **k)
        noise_log.append(v.detach().numpy().reshape(-1).copy())
        return v

    def snapshot(tag):
        out.update(mg._sd_to_np(f"sac:act_{tag}", agent.act.state_dict()))
        out.update(mg._sd_to_np(f"sac:cri_{tag}", agent.cri.state_dict()))
        out.update(mg._sd_to_np(f"sac:cri_target_{tag}", agent.cri_target.state_dict()))
        alpha_logs.append(agent.alpha_log.item())

    def rec_step(which):
        def step(*a, **k):
            steps[which] += 1
            if steps[which] == 1:
                if which == "alpha":
                    out["sac:grad1:alpha_log"] = agent.alpha_log.grad.detach().numpy().copy()
                else:
                    for name, p_ in getattr(agent, which).named_parameters():
                        out[f"sac:grad1:{which}.{name}"] = p_.grad.detach().numpy().copy()
            r = orig[which](*a, **k)
            if which == "act" and steps[which] == 1:
                snapshot("step1")
            return r
        return step

    torch.randint, torch.randn_like = rec_randint, rec_randn_like
    agent.cri_optimizer.step, agent.act_optimizer.step, agent.alpha_optimizer.step = rec_step("cri"), rec_step("act"), rec_step("alpha")
    torch.manual_seed(79)
    try:
        obj_a, obj_c = agent.update_net(buf, ITERS, B, 1)
    finally:
        torch.randint, torch.randn_like = orig_randint, orig_randn_like
    assert steps == {"cri": ITERS, "act": ITERS, "alpha": ITERS} and len(idx_log) == ITERS and len(noise_log) == 2 * ITERS
    snapshot("step4")
    out["sac:state"], out["sac:other"] = state, other
    out["sac:indices"] = np.array(idx_log)
    out["sac:noise_next"] = np.array(noise_log[0::2], dtype=np.float32)
    out["sac:noise_pg"] = np.array(noise_log[1::2], dtype=np.float32)
    out["sac:obj"] = np.array([obj_a, obj_c])
    out["sac:alpha_log"] = np.array(alpha_logs, dtype=np.float64)
    out["sac:hyper"] = np.array([MD, D, B, ITERS, agent.learning_rate, agent.soft_update_tau, agent.target_entropy])
    parts = {"sac_update_nets0.npz": ("sac:act0.", "sac:cri0.", "sac:grad1:cri.", "sac:grad1:act."),
             "sac_update_steps.npz": ("sac:act_step", "sac:cri_step", "sac:cri_target_step")}
    for name, prefixes in parts.items():
        mg.save(name, **{k: out.pop(k) for k in list(out) if k.startswith(prefixes)})
    mg.save("sac_update.npz", **out)


if __name__ == "__main__":
    golden_sac_update()
