#!/usr/bin/env python3
"""Generate tests/golden/td3_update_256*.npz by running the UNMODIFIED reference AgentTD3 at the shape its water-tank script trains:
net_dim 256 on the Stacking10 observation (state_dim 30).

Container-only, like make_golden.py (whose reference import, shims and save() this reuses; that file and golden_meta.json are left
as they are).  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_td3_wide.py

The fixture is four files, each under 1 MiB (about 2.9 MB in all): td3_update_256.npz (the ring, the draws, objectives and
hyper-parameters), td3_update_256_nets0.npz, td3_update_256_grad1.npz and td3_update_256_step1.npz.  What it pins (prefix "td3w:"):
  * state [4200, 30], other [4200, 3]: a flat ring of random transitions (reward * scale, mask, action), float32;
  * act0.*, cri0.*: the initial online Actor / CriticTwin (elegantrl/net.py) of AgentTD3.init(256, 30, 1) under torch.manual_seed(41);
    the targets are the reference's own deepcopy of them, so they are not stored twice;
  * indices [1, 4096], noise [1, 4096]: the rows torch.randint sampled and the smoothing-noise draws (torch.randn_like) of the one
    optimizer step of update_net(target_step 1, batch 4 096, repeat 1) -- successors are index + 1 (flat ring);
  * grad1:cri.*, grad1:act.*: the critic's .grad after obj_critic.backward() and the actor's after obj_actor.backward()
    (elegantrl/agent.py:317,326) -- the reference's own first-step gradients at batch 4 096;
  * act_step1.*, cri_step1.*: the online nets after that step's Adam updates (the targets after the soft update are left out to
    keep the file under 3 MB);
  * obj: the step's (obj_actor, obj_critic) as update_net returns them; hyper: net_dim, state_dim, batch, lr, tau, policy_noise,
    update_freq."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference and the shims on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

MD, D, B, N = 256, 30, 4096, 4200


def golden_td3_update_256():
    from elegantrl.agent import AgentTD3
    from elegantrl.replay import ReplayBuffer
    out = {}
    torch.manual_seed(41)
    agent = AgentTD3()
    agent.init(MD, D, 1)
    rng = np.random.RandomState(17)
    buf = ReplayBuffer(max_len=N + 8, state_dim=D, action_dim=1, if_on_policy=False, if_per=False, if_gpu=True)
    # Stacking10: ten (level, goal, error) triples of the tank
    state = (rng.rand(N, D) * np.tile([10., 10., 10.], D // 3) - np.tile([0., 0., 5.], D // 3)).astype(np.float32)
    other = np.stack([-rng.rand(N) * 5, np.where(rng.rand(N) < 0.02, 0.0, 0.99), np.tanh(rng.randn(N))], axis=1).astype(np.float32)
    buf.extend_buffer(torch.as_tensor(state), torch.as_tensor(other))
    out.update(mg._sd_to_np("td3w:act0", agent.act.state_dict()))
    out.update(mg._sd_to_np("td3w:cri0", agent.cri.state_dict()))
    idx_log, noise_log, steps = [], [], {"cri": 0, "act": 0}
    orig_randint, orig_randn_like = torch.randint, torch.randn_like
    orig_cri_step, orig_act_step = agent.cri_optimizer.step, agent.act_optimizer.step

    def rec_randint(*a, **k):
        v = orig_randint(*a, **k)
        idx_log.append(v.numpy().astype(np.int32))
        return v

    def rec_randn_like(t, **k):
        v = orig_randn_like(t, **k)
        noise_log.append(v.numpy().reshape(-1).copy())
        return v

    def rec_cri_step(*a, **k):
        for name, p_ in agent.cri.named_parameters():
            out[f"td3w:grad1:cri.{name}"] = p_.grad.detach().numpy().copy()
        steps["cri"] += 1
        return orig_cri_step(*a, **k)

    def rec_act_step(*a, **k):
        for name, p_ in agent.act.named_parameters():
            out[f"td3w:grad1:act.{name}"] = p_.grad.detach().numpy().copy()
        steps["act"] += 1
        return orig_act_step(*a, **k)

    torch.randint, torch.randn_like = rec_randint, rec_randn_like
    agent.cri_optimizer.step, agent.act_optimizer.step = rec_cri_step, rec_act_step
    torch.manual_seed(79)
    try:
        obj_a, obj_c = agent.update_net(buf, 1, B, 1)
    finally:
        torch.randint, torch.randn_like = orig_randint, orig_randn_like
    assert steps == {"cri": 1, "act": 1} and len(idx_log) == 1 and len(noise_log) == 1
    out.update(mg._sd_to_np("td3w:act_step1", agent.act.state_dict()))
    out.update(mg._sd_to_np("td3w:cri_step1", agent.cri.state_dict()))
    out["td3w:state"], out["td3w:other"] = state, other
    out["td3w:indices"], out["td3w:noise"] = np.array(idx_log), np.array(noise_log, dtype=np.float32)
    out["td3w:obj"] = np.array([obj_a, obj_c])
    out["td3w:hyper"] = np.array([MD, D, B, agent.learning_rate, agent.soft_update_tau, agent.policy_noise, agent.update_freq])
    parts = {"td3_update_256_nets0.npz": ("td3w:act0.", "td3w:cri0."), "td3_update_256_grad1.npz": ("td3w:grad1:",),
             "td3_update_256_step1.npz": ("td3w:act_step1.", "td3w:cri_step1.")}
    for name, prefixes in parts.items():
        mg.save(name, **{k: out.pop(k) for k in list(out) if k.startswith(prefixes)})
    mg.save("td3_update_256.npz", **out)


if __name__ == "__main__":
    golden_td3_update_256()
