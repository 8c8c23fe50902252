#!/usr/bin/env python3
"""usage: tools/policy_sweep_bench.py [--policies 64] [--plants 1024] [--state mixed] [--md 128] [--out profiles/policy_sweep_bench.jsonl]

What the fused policy sweep costs against the routes the tree has without it, on one GPU.  Workload: `policies` modular residual
actors at width `md` (one agent, every layer's weights moved by a seed per policy, each with its own prior gain) x `plants` water-tank
plants (a1 x a2 x Kp grid over the ensemble ranges), the tank's step-response protocol (set-points 3, 6, 9, 4, 2 x 500 steps = 2 500
steps), process noise on: 64 x 1 024 x 2 500 = 1.6e8 pair-steps.

  sweep   ONE pime_policy_sweep call (two launches), pairs / actions / outputs NULL: HIP events around it
  (a)     one pime_rollout_eval_metrics launch per policy, each on a fresh handle (the launch advances its handle; making the handle is
          not counted): HIP events around each launch, summed over ALL the policies.  rollout_eval.hip is unchanged by the sweep, so
          this is the parent's kernel and the only way to ask the question there.
  (b)     ONE pime_margin_sweep call with `policies` nominal rows (1, 0, 0) of ONE policy: the same loop, the same tiling, the image
          staged once per workgroup -- what re-staging costs.
sweep and (b) alternate in one loop, 1 warm-up round and 5 timed rounds, medians reported with every sample.  Row p of the sweep must
equal launch p of (a) in its worst-plant ITAE exactly.  One JSON line is appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETPOINTS, STEPS = (3., 6., 9., 4., 2.), 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=64)
    ap.add_argument("--plants", type=int, default=1024)
    ap.add_argument("--state", default="mixed", choices=["mixed", "f64"])
    ap.add_argument("--md", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_sweep_bench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pime_amd import gym_control, native, protocols
    from pime_amd.ops import PackedMLP, PackedPolicies
    from pime_amd.utils import MODELS
    dev = "cuda:0"
    p = args.plants.bit_length() - 1
    assert args.plants == 1 << p, "plants must be a power of two"
    shape = (1 << (p - 2 * (p // 3)), 1 << (p // 3), 1 << (p // 3))     # 1 024 -> 16 x 8 x 8
    a1, a2, kp = np.meshgrid(np.linspace(0.0015, 0.0024, shape[0]), np.linspace(0.0015, 0.0024, shape[1]),
                             np.linspace(0.07, 0.17, shape[2]), indexing="ij")
    plants = np.stack([a1.reshape(-1), a2.reshape(-1), kp.reshape(-1)], axis=1)
    n = len(SETPOINTS) * STEPS

    def fresh():
        env = gym_control.make_vec(gym_control.WT_INTEGRATOR, args.plants, device=dev, state_mode=args.state, seed=0, reward_type="distance")
        protocols._protocol_start(env, False, STEPS, plants)
        return env

    def timed(f):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    env = fresh()
    torch.manual_seed(0)
    agent = MODELS["residualintegratormodularppo"](device=dev)
    agent.init(args.md, env.state_dim, 1, 1)
    agent.init_residual({"init_K": env.K.reshape(-1, 1)})
    with torch.no_grad():
        agent.act.net[-1].weight.normal_(0, 0.1)
        agent.act.net[-1].bias.normal_(0, 0.05)
    agent.weights_changed()
    pk0, K0 = agent.fused_eval_policy(env)
    K0 = np.asarray(K0, dtype=np.float64).reshape(-1)
    singles, stack = [], None
    for j in range(args.policies):          # policy j: the layers' weights moved by seed j, the prior gain scaled by 1 +- 10 %
        torch.manual_seed(100 + j)
        with torch.no_grad():
            for name, par in agent.act.named_parameters():
                if "net" in name and name.endswith("weight"):
                    par.add_(0.01 * torch.randn_like(par))
        agent.weights_changed()
        pk, _ = agent.fused_eval_policy(env)
        K = K0 * (0.9 + 0.2 * j / max(args.policies - 1, 1))
        if stack is None:
            stack = PackedPolicies(pk.kind, pk.D, pk.Di, pk.md, dev, capacity=args.policies)
        stack.append(pk, K)
        own = PackedMLP(pk.kind, pk.D, pk.Di, pk.md, dev)       # the image as it is now, for launch j of (a)
        own.packed.copy_(pk.packed)
        singles.append((own, K))
    assert env.policy_supported(stack) and env.margin_supported(pk0)
    nominal = np.tile([[1.0, 0.0, 0.0]], (args.policies, 1))
    sweep_ms, b_ms = [], []
    for i in range(args.rounds + 1):
        t_s, summary = timed(lambda: env.policy_sweep(stack, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10))
        t_b, _ = timed(lambda: env.margin_sweep(singles[0][0], singles[0][1], nominal, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10))
        if i >= 1:
            sweep_ms.append(t_s)
            b_ms.append(t_b)
    summary = summary.cpu().numpy()
    env.close()

    st = {name: j for j, name in enumerate(native.SWEEP_STATS)}
    itae = native.METRIC_NAMES.index("itae")
    a_ms, agree = [], True
    for j, (own, K) in enumerate(singles):
        c = fresh()
        t, (_, m, _) = timed(lambda: c.rollout_eval_metrics(own, K, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10))
        a_ms.append(t)
        agree = agree and bool(np.array_equal(m[:, itae].max(dim=1).values.cpu().numpy(), summary[j, :, itae, st["max"]]))
        c.close()

    sweep, b, a = statistics.median(sweep_ms), statistics.median(b_ms), sum(a_ms)
    rec = dict(tool="policy_sweep_bench", policies=args.policies, plants=args.plants, steps=n, state=args.state, kind="modular_actor", md=args.md,
               pair_steps=args.policies * args.plants * n, sweep_ms=round(sweep, 3), sweep_ms_all=[round(v, 3) for v in sweep_ms],
               a_launches_timed=len(a_ms), a_ms_per_launch=round(a / len(a_ms), 3), a_ms_total=round(a, 1), speedup_vs_a=round(a / sweep, 2),
               b_margin_nominal_ms=round(b, 3), b_ms_all=[round(v, 3) for v in b_ms], sweep_over_b=round(sweep / b, 4),
               pair_steps_per_s=round(args.policies * args.plants * n / (sweep * 1e-3), 1), every_row_equals_its_launch=agree)
    print(json.dumps(rec))
    assert agree, "a row's worst-plant ITAE differs from its launch's"
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
