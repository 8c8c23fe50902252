#!/usr/bin/env python3
"""usage: tools/margin_sweep_bench.py [--plants 1024] [--subset 8] [--state mixed] [--md 128] [--out profiles/margin_sweep_bench.jsonl]

What the fused loop-perturbation sweep costs against the routes the tree had before it, on one GPU.  Workload: 288 perturbation rows
(9 delays 0 .. 8 x 8 gains x 4 sigmas) x `plants` water-tank plants (a1 x a2 x Kp grid over the ensemble ranges), the tank's
step-response protocol (set-points 3, 6, 9, 4, 2 x 500 steps = 2 500 steps), process noise on, the modular residual actor at width
`md`: 288 x 1 024 x 2 500 = 7.4e8 pair-steps.

  sweep   ONE pime_margin_sweep call (two launches), pairs / actions / outputs NULL: HIP events around it, median of 3 after 1 warm-up
  (a)     P sequential pime_rollout_eval_metrics launches on the same lane state -- which cannot delay, scale or disturb the loop:
          strictly less work per launch.  The first `subset` launches are timed (HIP events around each, summed; a fresh env per
          launch, not counted) and scaled linearly to 288.  rollout_eval.hip is unchanged by the sweep, so this is the parent's kernel.
  (b)     the step-per-launch loop with a host-side delay line, the only way the question could be asked before: per step the
          actor's torch module on the noisy observation, a deque of device tensors, VecControlEnv.step.  2 rows x 250 steps timed
          (HIP events around the whole loop) and scaled linearly to 288 rows x 2 500 steps.
The nominal row of the sweep must equal launch (a)'s worst-plant ITAE exactly.  One JSON line is appended to --out."""
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETPOINTS, STEPS = (3., 6., 9., 4., 2.), 500
DELAYS = tuple(range(9))
GAINS = (0.25, 0.35, 0.5, 0.7, 1.0, 1.4, 2.0, 2.8)
SIGMAS = (0.0, 0.01, 0.02, 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=1024)
    ap.add_argument("--subset", type=int, default=8)
    ap.add_argument("--state", default="mixed", choices=["mixed", "f64"])
    ap.add_argument("--md", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "margin_sweep_bench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pime_amd import gym_control, native, protocols
    from pime_amd.utils import MODELS
    dev = "cuda:0"
    p = args.plants.bit_length() - 1
    assert args.plants == 1 << p, "plants must be a power of two"
    shape = (1 << (p - 2 * (p // 3)), 1 << (p // 3), 1 << (p // 3))     # 1 024 -> 16 x 8 x 8
    a1, a2, kp = np.meshgrid(np.linspace(0.0015, 0.0024, shape[0]), np.linspace(0.0015, 0.0024, shape[1]),
                             np.linspace(0.07, 0.17, shape[2]), indexing="ij")
    plants = np.stack([a1.reshape(-1), a2.reshape(-1), kp.reshape(-1)], axis=1)
    n = len(SETPOINTS) * STEPS
    grid = protocols.perturbation_grid(gains=GAINS, delays=DELAYS, sigmas=SIGMAS)
    nominal = int(np.flatnonzero((grid[:, 0] == 1.0) & (grid[:, 1] == 0.0) & (grid[:, 2] == 0.0))[0])

    def fresh():
        env = gym_control.make_vec(gym_control.WT_INTEGRATOR, args.plants, device=dev, state_mode=args.state, seed=0, reward_type="distance")
        protocols._protocol_start(env, False, STEPS, plants)
        return env

    env = fresh()
    torch.manual_seed(0)
    agent = MODELS["residualintegratormodularppo"](device=dev)
    agent.init(args.md, env.state_dim, 1, 1)
    agent.init_residual({"init_K": env.K.reshape(-1, 1)})
    with torch.no_grad():
        agent.act.net[-1].weight.normal_(0, 0.1)
        agent.act.net[-1].bias.normal_(0, 0.05)
    agent.weights_changed()
    pk, K = agent.fused_eval_policy(env)
    assert env.margin_supported(pk)
    sweep_ms = []
    for i in range(4):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        summary = env.margin_sweep(pk, K, grid, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10)
        e1.record()
        torch.cuda.synchronize()
        if i >= 1:
            sweep_ms.append(e0.elapsed_time(e1))
    summary = summary.cpu().numpy()
    env.close()

    st = {name: j for j, name in enumerate(native.SWEEP_STATS)}
    itae = native.METRIC_NAMES.index("itae")
    base_ms, agree = [], True
    for g in range(args.subset):
        c = fresh()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, m, _ = c.rollout_eval_metrics(pk, K, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10)
        e1.record()
        torch.cuda.synchronize()
        base_ms.append(e0.elapsed_time(e1))
        if g == 0:
            agree = bool(np.array_equal(m[:, itae].max(dim=1).values.cpu().numpy(), summary[nominal, :, itae, st["max"]]))
        c.close()
    a_ms = sum(base_ms) / args.subset * len(grid)

    # (b) step per launch, host delay line
    rows_b, steps_b = grid[[nominal + 1, len(grid) - 1]], 250
    act = agent.act
    c = fresh()
    obs = c.obs.clone()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for gain, delay, sigma in rows_b:
        line = collections.deque([torch.zeros(args.plants, dtype=torch.float64, device=dev)] * int(delay), maxlen=int(delay) + 1)
        for t in range(steps_b):
            om = obs.clone()
            if sigma > 0:
                om[:, :2] += float(sigma) * torch.randn((args.plants, 2), device=dev)
            with torch.no_grad():
                line.append(act(om)[:, 0].double())
            obs, _, _ = c.step(float(gain) * line[0], auto_reset=False)[:3]
    e1.record()
    torch.cuda.synchronize()
    b_ms = e0.elapsed_time(e1) / (len(rows_b) * steps_b) * (len(grid) * n)
    c.close()

    sweep = statistics.median(sweep_ms)
    rec = dict(tool="margin_sweep_bench", rows=len(grid), plants=args.plants, steps=n, state=args.state, kind="modular_actor", md=args.md,
               pair_steps=len(grid) * args.plants * n, sweep_ms=round(sweep, 3), sweep_ms_all=[round(v, 3) for v in sweep_ms],
               a_launches_timed=args.subset, a_ms_per_launch=round(sum(base_ms) / args.subset, 3), a_ms_scaled=round(a_ms, 1),
               b_rows_timed=len(rows_b), b_steps_timed=steps_b, b_ms_scaled=round(b_ms, 1), speedup_vs_a=round(a_ms / sweep, 2),
               speedup_vs_b=round(b_ms / sweep, 1), pair_steps_per_s=round(len(grid) * args.plants * n / (sweep * 1e-3), 1),
               nominal_row_equals_launch=agree, estimate_ms_at_half_f32_matrix_peak=640.0,
               note="estimate: 7.4e8 pair-steps x 68 kFLOP at 0.50 of the f32 matrix peak, derived from the code, not measured")
    print(json.dumps(rec))
    assert agree, "the nominal row's worst-plant ITAE differs from the launch's"
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
