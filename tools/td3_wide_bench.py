#!/usr/bin/env python3
"""TD3 optimizer steps at width 256 on the Stacking10 observation, in ONE process: the fused step (csrc/td3_fused.hip) and the module
path (AgentTD3._one_update, PIME_TD3_FUSED=0's route) at (256, 30, 4096), and the fused step at (128, 30, 4096) and (128, 4, 4096).
Each is AgentTD3.update_net on a synthetic vector replay ring (no env): two warm-up calls (eager, then the capture of the update's
graphs), then REPS calls of STEPS optimizer steps timed with HIP events.  One JSON line per shape: us per step, GFLOP per step from the
layer shapes, and the fraction of the f32 matrix peak.

Then the other half of a TD3 iteration at that shape, on the Stacking10 water tank itself (4 096 lanes, 200-step episodes, residual TD3
at width 256): one `explore_env` call of 200 lock-steps and one evaluation episode (`get_episode_return_vec`: reset, 200 steps, the
returns copied to the host), each with `use_fused_rollout` True (ONE launch: pime_rollout_offpolicy / pime_rollout_eval) and False (lock-step
by lock-step: torch actor, noise, clamp, prior term, pime_env_step, ring copies).  Same timing: two warm-up calls, REPS calls between
HIP events, the median.  One JSON line per (what, path): ms per call.

    python tools/td3_wide_bench.py [out.jsonl] [all|step|rollout]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pime_amd import gym_control  # noqa: E402
from pime_amd.elegantrl.agent import AgentTD3  # noqa: E402
from pime_amd.elegantrl.agent_residual import AgentResidualTD3  # noqa: E402
from pime_amd.elegantrl.replay import VecReplayBuffer  # noqa: E402
from pime_amd.elegantrl.run import Evaluator, get_episode_return_vec  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3   # bench.py's constant
DEV, N, SLOTS, STEPS, REPS = "cuda:0", 4096, 32, 20, 5


def td3_gflop(md, D, B):
    """Multiply-adds of one optimizer step from the layer shapes (forward, backward, weight gradients; heads included), x 2."""
    m = md
    critic = (D * m + 2 * m * m + m) + 2 * ((D + 1) * m + m * m + 2 * m) + (2 * m * m + (D + 1) * m + 2 * m)
    actor = (D * m + 2 * m * m + m) + ((D + 1) * m + m * m + m) + (m * m + m) + (m + 4 * m * m + D * m)
    return 2.0 * B * (critic + actor) / 1e9


def measure(md, D, B, fused):
    torch.manual_seed(0)
    ag = AgentTD3(device=DEV)
    ag.init(md, D, 1)
    ag.use_fused_update = fused
    buf = VecReplayBuffer(SLOTS * N, N, D, 1, DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    buf.state.copy_(torch.rand(buf.state.shape, device=DEV, generator=g) * 10 - 5)
    buf.other[..., 0].copy_(-torch.rand(buf.other.shape[:-1], device=DEV, generator=g) * 5)
    buf.other[..., 1].fill_(0.99)
    buf.other[..., 2].copy_(torch.rand(buf.other.shape[:-1], device=DEV, generator=g) * 2 - 1)
    buf.next_slot, buf.if_full = 0, True
    for _ in range(2):
        ag.update_net(buf, STEPS * N, B, 1)
    torch.cuda.synchronize()
    assert (ag._fused_td3 not in (None, False)) == fused, "the path asked for is not the one that ran"
    times = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ag.update_net(buf, STEPS * N, B, 1)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e3 / STEPS)
    us = sorted(times)[len(times) // 2]
    gf = td3_gflop(md, D, B)
    return {"path": "fused" if fused else "module", "md": md, "D": D, "B": B, "us_per_step": round(us, 1),
            "us_per_step_all": [round(t, 1) for t in times], "gflop_per_step": round(gf, 3),
            "tflops": round(gf / us * 1e3, 2), "frac_f32_mfma_peak": round(gf / us * 1e3 / F32_MFMA_PEAK_TFLOPS, 4)}


def _timed_ms(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return sorted(times)[len(times) // 2], times


def measure_rollout(fused, md=256, stack=10, lock_steps=200):
    """ms per explore_env call of `lock_steps` lock-steps x N lanes, and per evaluation episode, on the Stacking water tank."""
    env = gym_control.make_vec(gym_control.WT_STACKING.format(stack), N, device=DEV, state_mode="mixed", seed=3, reward_type="distance",
                               max_step=lock_steps)
    eval_env = env.clone()   # as run.py gives an off-policy run its own evaluation env
    torch.manual_seed(0)
    ag = AgentResidualTD3(device=DEV)
    ag.use_fused_rollout = fused
    ag.init(md, env.state_dim, 1)
    ag.init_residual({"init_K": env.K.reshape(-1, 1)})
    with torch.no_grad():
        ag.act.net[-1].weight.normal_(0, 0.05)
    buf = VecReplayBuffer((lock_steps + 56) * N, N, env.state_dim, 1, DEV)
    assert (ag._fused_explore(env) is not None) == fused, "the path asked for is not the one that runs"
    explore_ms, explore_all = _timed_ms(lambda: ag.explore_env(env, buf, lock_steps * N, 1.0, 0.99))
    policy, fused_eval = Evaluator._policy(ag), ag.fused_eval_policy(eval_env)
    assert (fused_eval is not None) == fused, "the path asked for is not the one that runs"
    returns = []
    eval_ms, eval_all = _timed_ms(lambda: returns.append(get_episode_return_vec(eval_env, policy, fused=ag.fused_eval_policy(eval_env))))
    shape = {"path": "fused" if fused else "lock_step", "md": md, "D": env.state_dim, "lanes": N, "lock_steps": lock_steps}
    rows = [dict(shape, what="explore_env", ms_per_call=round(explore_ms, 3), ms_per_call_all=[round(t, 3) for t in explore_all]),
            dict(shape, what="evaluation_episode", ms_per_call=round(eval_ms, 3), ms_per_call_all=[round(t, 3) for t in eval_all],
                 mean_return=round(float(returns[-1].mean()), 3))]
    env.close()
    eval_env.close()
    return rows


def main():
    what = sys.argv[2] if len(sys.argv) > 2 else "all"
    rows = []
    if what in ("all", "step"):
        rows = [measure(256, 30, 4096, True), measure(256, 30, 4096, False), measure(128, 30, 4096, True), measure(128, 4, 4096, True)]
        rows.append({"speedup_fused_vs_module_256_30_4096": round(rows[1]["us_per_step"] / rows[0]["us_per_step"], 2)})
    if what in ("all", "rollout"):
        r = measure_rollout(True) + measure_rollout(False)
        rows += r
        rows.append({"speedup_fused_vs_lock_step_explore_256_30_4096": round(r[2]["ms_per_call"] / r[0]["ms_per_call"], 2),
                     "speedup_fused_vs_lock_step_evaluation_256_30_4096": round(r[3]["ms_per_call"] / r[1]["ms_per_call"], 2)})
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
