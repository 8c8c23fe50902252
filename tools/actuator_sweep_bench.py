#!/usr/bin/env python3
"""usage: tools/actuator_sweep_bench.py [--plants 1024] [--rows 288] [--state mixed] [--md 128] [--out profiles/actuator_sweep_bench.jsonl]

What the fused actuator-limits sweep costs against the routes the tree had before it, on one GPU in one run, at the shape of
tools/disturb_sweep_bench.py.  Workload: `rows` actuator rows x `plants` water-tank plants (a1 x a2 x Kp grid over the ensemble
ranges), the tank's step-response protocol (set-points 3, 6, 9, 4, 2 x 500 steps = 2 500 steps), process noise on, the modular
residual actor at width `md`: 288 x 1 024 x 2 500 = 7.4e8 pair-steps.  The grid is a realistic one: the all-off row first, then the
product of clamps, slew rates, dead-bands, actuator quanta and sensor quanta around the reference rig's values (every stage on in most
rows), cut to `rows`.

  (a)     ONE pime_actuator_sweep call (two launches), pairs / actions / commands / outputs NULL: HIP events around it, median of 3
          after 1 warm-up
  (b)     ONE pime_disturb_sweep call with `rows` NOMINAL rows (no load, unit multipliers) on the same lane state: the same loop
          without the sensor, the actuator chain and the eight actuator rows -- the parent commit's kernels.  The yardstick: the
          ratio (a) / (b) is what the actuator costs.  Timed the same way.
  (a0)    pime_actuator_sweep with `rows` ALL-OFF rows: the loop with every stage branch not taken (what the metrics alone cost).
  (c)     the step-per-launch loop with the chain in torch on the host side, the only way the question could be asked before: per
          step the actor's torch module on the quantised observation, the four stages as torch operations, VecControlEnv.step.
          2 rows x 250 steps timed (HIP events around the whole loop) and scaled linearly to rows x 2 500 steps.
The all-off row's first eight rows must equal the disturbance sweep's nominal row exactly.  One JSON line is appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETPOINTS, STEPS = (3., 6., 9., 4., 2.), 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=288)
    ap.add_argument("--state", default="mixed", choices=["mixed", "f64"])
    ap.add_argument("--md", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actuator_sweep_bench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pime_amd import gym_control, protocols
    from pime_amd.utils import MODELS
    dev = "cuda:0"
    p = args.plants.bit_length() - 1
    assert args.plants == 1 << p, "plants must be a power of two"
    shape = (1 << (p - 2 * (p // 3)), 1 << (p // 3), 1 << (p // 3))     # 1 024 -> 16 x 8 x 8
    a1, a2, kp = np.meshgrid(np.linspace(0.0015, 0.0024, shape[0]), np.linspace(0.0015, 0.0024, shape[1]),
                             np.linspace(0.07, 0.17, shape[2]), indexing="ij")
    plants = np.stack([a1.reshape(-1), a2.reshape(-1), kp.reshape(-1)], axis=1)
    n = len(SETPOINTS) * STEPS
    rig = protocols.rig_row()
    # 3 x 3 x 2 x 4 x 4 = 288 rows around the rig's values
    grid = protocols.actuator_grid(limits=[(-1.0, 1.0), (-0.5, 0.5)], rates=(0.5, 0.1), deadbands=(rig[4],), qu=(rig[4], 4 * rig[4], 16 * rig[4]),
                                   qy=(rig[5], 4 * rig[5], 16 * rig[5]))
    grid = np.ascontiguousarray(np.resize(grid, (args.rows, 6)) if len(grid) < args.rows else grid[:args.rows])
    all_off = np.tile(np.asarray(protocols.ACT_OFF, dtype=np.float64), (len(grid), 1))
    nominal = np.tile(protocols.disturbance_grid(STEPS // 2)[:1], (len(grid), 1))

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
    assert env.actuator_supported(pk) and env.disturbance_supported(pk)

    def timed(call):
        ms = []
        for i in range(4):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            if i >= 1:
                ms.append(e0.elapsed_time(e1))
        return ms, out.cpu().numpy()

    kw = dict(setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10)
    a_ms, summary = timed(lambda: env.actuator_sweep(pk, K, grid, n, **kw))
    b_ms, disturb = timed(lambda: env.disturbance_sweep(pk, K, nominal, n, **kw))
    a0_ms, off = timed(lambda: env.actuator_sweep(pk, K, all_off, n, **kw))
    a_ms2, _ = timed(lambda: env.actuator_sweep(pk, K, grid, n, **kw))          # (a) again after (b): the order does not decide
    agree = bool(np.array_equal(summary[0, :, :8].view(np.uint64), disturb[0, :, :8].view(np.uint64)) and
                 np.array_equal(off[:, :, :8].view(np.uint64), disturb[:, :, :8].view(np.uint64)))
    st = {name: j for j, name in enumerate(protocols.SWEEP_STATS)}
    acted = [float(summary[:, :, 8 + j, st["sum"]].sum()) for j in range(3)]      # SAT, RATE, HOLD steps over the whole grid
    env.close()

    # (c) step per launch, the chain in torch between the launches
    rows_c, steps_c = grid[[len(grid) // 2, len(grid) - 1]], 250
    act = agent.act
    c = fresh()
    obs = c.obs.clone()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for lo, hi, rate, db, qu, qy in (tuple(float(v) for v in r) for r in rows_c):
        c.reset_changable_parameters(plants[:, 0], plants[:, 1], plants[:, 2])
        u_prev = torch.zeros(args.plants, dtype=torch.float64, device=dev)
        for t in range(steps_c):
            with torch.no_grad():
                om = obs.clone()
                if qy > 0:
                    om[:, :2] = (qy * torch.round(obs[:, :2].double() / qy)).float()
                v = act(om)[:, 0].double()               # the residual actor's forward: tanh(mean) + om @ priorK
                if db > 0:
                    v = torch.where((v - u_prev).abs() <= db, u_prev, v)
                if 0 < rate < float("inf"):
                    v = u_prev + (v - u_prev).clamp(-rate, rate)
                if qu > 0:
                    v = qu * torch.round(v / qu)
                v = v.clamp(lo, hi)
            obs = c.step(v, auto_reset=False)[0]
            u_prev = v
    e1.record()
    torch.cuda.synchronize()
    c_ms = e0.elapsed_time(e1) / (len(rows_c) * steps_c) * (len(grid) * n)
    c.close()

    a, b, a0, a2 = (statistics.median(v) for v in (a_ms, b_ms, a0_ms, a_ms2))
    rec = dict(tool="actuator_sweep_bench", rows=len(grid), plants=args.plants, steps=n, state=args.state, kind="modular_actor", md=args.md,
               pair_steps=len(grid) * args.plants * n, a_actuator_ms=round(a, 3), a_actuator_ms_all=[round(v, 3) for v in a_ms],
               a_actuator_again_ms=round(a2, 3), a_actuator_again_ms_all=[round(v, 3) for v in a_ms2],
               b_disturb_nominal_ms=round(b, 3), b_disturb_nominal_ms_all=[round(v, 3) for v in b_ms], ratio_a_to_b=round(a / b, 4),
               ratio_a_again_to_b=round(a2 / b, 4), a0_all_off_ms=round(a0, 3), a0_all_off_ms_all=[round(v, 3) for v in a0_ms],
               ratio_a0_to_b=round(a0 / b, 4), c_rows_timed=len(rows_c), c_steps_timed=steps_c, c_ms_scaled=round(c_ms, 1),
               speedup_vs_c=round(c_ms / a, 1), pair_steps_per_s=round(len(grid) * args.plants * n / (a * 1e-3), 1),
               sat_rate_hold_steps=acted, all_off_row_equals_disturb_sweep=agree)
    print(json.dumps(rec))
    assert agree, "the all-off rows' first eight rows differ from the disturbance sweep's nominal row"
    assert all(v > 0 for v in acted), "a stage of the grid never acted"
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
