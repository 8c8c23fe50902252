#!/usr/bin/env python3
"""usage: tools/disturb_sweep_bench.py [--plants 1024] [--rows 288] [--state mixed] [--md 128] [--out profiles/disturb_sweep_bench.jsonl]

What the fused disturbance-rejection sweep costs against the routes the tree had before it, on one GPU, at the shape of
tools/margin_sweep_bench.py.  Workload: `rows` disturbance rows (the nominal one first, then loads and multipliers of a1, a2 and Kp in
equal shares, onset at half a segment) x `plants` water-tank plants (a1 x a2 x Kp grid over the ensemble ranges), the tank's
step-response protocol (set-points 3, 6, 9, 4, 2 x 500 steps = 2 500 steps), process noise on, the modular residual actor at width
`md`: 288 x 1 024 x 2 500 = 7.4e8 pair-steps.

  sweep   ONE pime_disturb_sweep call (two launches), pairs / actions / outputs NULL: HIP events around it, median of 3 after 1 warm-up
  (a)     ONE pime_margin_sweep call with `rows` NOMINAL rows (1, 0, 0) on the same lane state: the same loop without the plant select,
          the load and the seven rejection rows.  The yardstick: the ratio sweep / (a) is what the disturbance costs.  Timed the same way.
  (b)     the step-per-launch loop with set_field at the onset, the only way the question could be asked before: per step the actor's
          torch module on the observation and VecControlEnv.step; the plant words are rewritten from the host at the onset and at every
          segment boundary.  2 rows x 250 steps timed (HIP events around the whole loop) and scaled linearly to rows x 2 500 steps.
The nominal row's first eight rows must equal the margin sweep's nominal row exactly.  One JSON line is appended to --out."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disturb_sweep_bench.jsonl"))
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
    per = (args.rows - 1 + 3) // 4
    grid = protocols.disturbance_grid(STEPS // 2, loads=np.linspace(-0.3, 0.3, per), m0=np.linspace(0.6, 1.6, per), m1=np.linspace(0.6, 1.6, per),
                                      m2=np.linspace(0.6, 1.6, per))[:args.rows]
    nominal_rows = np.tile(np.array([[1.0, 0.0, 0.0]]), (len(grid), 1))

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
    assert env.disturbance_supported(pk) and env.margin_supported(pk)

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

    sweep_ms, summary = timed(lambda: env.disturbance_sweep(pk, K, grid, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10))
    a_ms, margin = timed(lambda: env.margin_sweep(pk, K, nominal_rows, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10))
    agree = bool(np.array_equal(summary[0, :, :8].view(np.uint64), margin[0].view(np.uint64)))
    env.close()

    # (b) step per launch, set_field at the onset and at the segment boundaries
    rows_b, steps_b, onset_b = grid[[1, len(grid) - 1]], 250, 125
    act = agent.act
    c = fresh()
    obs = c.obs.clone()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _, _, load, m0, m1, m2 in rows_b:
        c.reset_changable_parameters(plants[:, 0], plants[:, 1], plants[:, 2])
        for t in range(steps_b):
            if t == onset_b:
                c.reset_changable_parameters(plants[:, 0] * m0, plants[:, 1] * m1, plants[:, 2] * m2)
            with torch.no_grad():
                a = act(obs)[:, 0].double()
            obs, _, _ = c.step(a + float(load) if t >= onset_b else a, auto_reset=False)[:3]
    e1.record()
    torch.cuda.synchronize()
    b_ms = e0.elapsed_time(e1) / (len(rows_b) * steps_b) * (len(grid) * n)
    c.close()

    sweep, a = statistics.median(sweep_ms), statistics.median(a_ms)
    rec = dict(tool="disturb_sweep_bench", rows=len(grid), plants=args.plants, steps=n, state=args.state, kind="modular_actor", md=args.md,
               pair_steps=len(grid) * args.plants * n, sweep_ms=round(sweep, 3), sweep_ms_all=[round(v, 3) for v in sweep_ms],
               a_margin_nominal_ms=round(a, 3), a_margin_nominal_ms_all=[round(v, 3) for v in a_ms], ratio_to_a=round(sweep / a, 4),
               b_rows_timed=len(rows_b), b_steps_timed=steps_b, b_ms_scaled=round(b_ms, 1), speedup_vs_b=round(b_ms / sweep, 1),
               pair_steps_per_s=round(len(grid) * args.plants * n / (sweep * 1e-3), 1), nominal_row_equals_margin_sweep=agree)
    print(json.dumps(rec))
    assert agree, "the nominal row's first eight rows differ from the margin sweep's nominal row"
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
