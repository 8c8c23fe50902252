#!/usr/bin/env python3
"""SAC optimizer steps and exploration in ONE process, beside the fused TD3 step at the same shapes on the same device:

  * AgentSAC.update_net on the fused step (csrc/sac_fused.hip) and AgentTD3.update_net on its fused step (csrc/td3_fused.hip) at
    (128, 4) and (64, 3), batch 4 096: a synthetic vector replay ring (no env), two warm-up calls (eager, then the capture of the
    update's graph), then REPS calls of STEPS = 200 optimizer steps, each one graph replay timed with HIP events; the algorithmic
    flop ratio SAC / TD3 from the layer sizes next to the measured time ratio;
  * the PyTorch-module SAC step on the same inputs (what a user gets without the kernels), and the ratio;
  * one AgentSAC.explore_vec_env call of 200 lock-steps on 4 096 water-tank lanes: the fused launch against launch by launch.
One JSON line each.

    python tools/sac_bench.py [out.jsonl]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pime_amd.elegantrl.agent import AgentTD3  # noqa: E402
from pime_amd.elegantrl.agent_sac import AgentSAC  # noqa: E402
from pime_amd.elegantrl.replay import VecReplayBuffer  # noqa: E402

DEV, N, SLOTS, STEPS, REPS = "cuda:0", 4096, 32, 200, 5


def td3_macs(m, D):
    """Multiply-adds per sample of one TD3 optimizer step (tools/td3_wide_bench.py: td3_gflop)."""
    critic = (D * m + 2 * m * m + m) + 2 * ((D + 1) * m + m * m + 2 * m) + (2 * m * m + (D + 1) * m + 2 * m)
    actor = (D * m + 2 * m * m + m) + ((D + 1) * m + m * m + m) + (m * m + m) + (m + 4 * m * m + D * m)
    return critic + actor


def sac_macs(m, D):
    """The same count for SAC: two actor forwards with two heads in the critic launch (next-state sample, policy-gradient sample),
    both target heads and the two-head backward in the actor launch."""
    actor_fwd = D * m + 2 * m * m + 2 * m
    critic = 2 * actor_fwd + 2 * ((D + 1) * m + m * m + 2 * m) + (2 * m * m + (D + 1) * m + 2 * m)
    actor = actor_fwd + ((D + 1) * m + m * m + 2 * m) + (m * m + m) + (2 * m + 2 * m + 4 * m * m + D * m)
    return critic + actor


def ring(D):
    buf = VecReplayBuffer(SLOTS * N, N, D, 1, DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    buf.state.copy_(torch.rand(buf.state.shape, device=DEV, generator=g) * 10 - 5)
    buf.other[..., 0].copy_(-torch.rand(buf.other.shape[:-1], device=DEV, generator=g) * 5)
    buf.other[..., 1].fill_(0.99)
    buf.other[..., 2].copy_(torch.rand(buf.other.shape[:-1], device=DEV, generator=g) * 2 - 1)
    buf.next_slot, buf.if_full = 0, True
    return buf


def measure(algo, md, D, B, fused, steps=STEPS):
    torch.manual_seed(0)
    ag = (AgentSAC if algo == "sac" else AgentTD3)(device=DEV)
    ag.init(md, D, 1)
    ag.use_fused_update = fused
    buf = ring(D)
    for _ in range(2):
        ag.update_net(buf, steps * N, B, 1)
    torch.cuda.synchronize()
    f = ag._fused_sac if algo == "sac" else ag._fused_td3
    assert (f not in (None, False)) == fused, "the path asked for is not the one that ran"
    times = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ag.update_net(buf, steps * N, B, 1)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e3 / steps)
    us = sorted(times)[len(times) // 2]
    macs = (sac_macs if algo == "sac" else td3_macs)(md, D)
    return {"what": f"{algo}_update_net", "path": "fused" if fused else "module", "md": md, "D": D, "B": B, "steps_per_call": steps,
            "us_per_step": round(us, 1), "us_per_step_all": [round(t, 1) for t in times], "kflop_per_sample": round(2 * macs / 1e3, 1),
            "gflop_per_step": round(2.0 * B * macs / 1e9, 3)}


def explore(fused, lock_steps=200):
    from pime_amd import gym_control
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, N, device=DEV, state_mode="mixed", seed=1, reward_type="distance")
    torch.manual_seed(0)
    ag = AgentSAC(device=DEV)
    ag.use_fused_rollout = fused
    ag.init(128, env.state_dim, 1)
    buf = VecReplayBuffer(4 * lock_steps * N, N, env.state_dim, 1, DEV)
    ag.explore_env(env, buf, lock_steps * N, 1.0, 0.99)   # warm-up (image pack, first launch)
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ag.explore_env(env, buf, lock_steps * N, 1.0, 0.99)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    assert (ag._fused_explore(env) is not None) == fused
    env.close()
    return {"what": "sac_explore_vec_env", "path": "fused" if fused else "lock_step", "lanes": N, "lock_steps": lock_steps,
            "ms_per_call": round(sorted(times)[1], 3), "ms_per_call_all": [round(t, 3) for t in times]}


def main():
    rows = []
    for md, D in ((128, 4), (64, 3)):
        sac, td3 = measure("sac", md, D, 4096, True), measure("td3", md, D, 4096, True)
        rows += [sac, td3, {"what": "sac_vs_td3_fused", "md": md, "D": D, "time_ratio": round(sac["us_per_step"] / td3["us_per_step"], 3),
                            "flop_ratio": round(sac_macs(md, D) / td3_macs(md, D), 3)}]
    mod = measure("sac", 128, 4, 4096, False, steps=20)
    rows += [mod, {"what": "sac_fused_vs_module", "md": 128, "D": 4, "speedup": round(mod["us_per_step"] / rows[0]["us_per_step"], 1)}]
    ef, es = explore(True), explore(False)
    rows += [ef, es, {"what": "sac_explore_fused_vs_lock_step", "speedup": round(es["ms_per_call"] / ef["ms_per_call"], 1)}]
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
