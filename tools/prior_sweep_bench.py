#!/usr/bin/env python3
"""usage: tools/prior_sweep_bench.py [--gains 4096] [--plants 1024] [--subset 64] [--state mixed] [--out profiles/prior_sweep_bench.jsonl]

What the fused prior-gain sweep costs against the route the tree had before it, on one GPU.  Workload: `gains` prior gains (a
square box of factors in [0.25, 4] on the tank's two non-zero gain components) x `plants` water-tank plants (a1 x a2 x Kp grid over
the ensemble ranges), the tank's step-response protocol (set-points 3, 6, 9, 4, 2 x 500 steps), process noise on.

  (a) sweep      ONE pime_prior_sweep call (two launches), pairs = NULL: HIP events around it, median of 3 after 1 warm-up
  (b) per gain   the parent's route: one pime_rollout_eval_metrics(kind = -1) launch per gain and torch reductions of its
                 [segments, 8, N] table on the device (finite mask, sum, min, max, argmax, count).  Timed on the FIRST `subset` gains
                 -- HIP events around launch + reductions of each, summed; putting the lanes back to the starting state between gains
                 (a fresh env per gain here) is NOT counted -- and scaled linearly to `gains`.
The MAX / ARGMAX / FINITE rows of the two routes must agree exactly on the subset.  One JSON line is appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETPOINTS, STEPS = (3., 6., 9., 4., 2.), 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gains", type=int, default=4096)
    ap.add_argument("--plants", type=int, default=1024)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--state", default="mixed", choices=["mixed", "f64"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_sweep_bench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pime_amd import gym_control, native, protocols
    dev = "cuda:0"
    side = int(round(args.gains ** 0.5))
    assert side * side == args.gains, "gains must be a square (a box over two gain components)"
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

    env = fresh()
    gains = protocols.gain_box(-env.K, list(np.geomspace(0.25, 4.0, side)))
    g_dev = torch.as_tensor(gains, device=dev)
    ws_bytes = int(native.lib().pime_prior_sweep_workspace_bytes(env._h, args.gains, n, STEPS))
    sweep_ms = []
    for i in range(4):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        summary = env.prior_sweep(g_dev, n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10)
        e1.record()
        torch.cuda.synchronize()
        if i >= 1:
            sweep_ms.append(e0.elapsed_time(e1))
    summary = summary.cpu().numpy()
    env.close()

    st = {name: j for j, name in enumerate(native.SWEEP_STATS)}
    sub = min(args.subset, args.gains)
    base_ms, agree = [], True
    for g in range(sub):
        c = fresh()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, m, _ = c.rollout_eval_metrics(None, gains[g], n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10)
        ok = torch.isfinite(m)
        total = torch.where(ok, m, torch.zeros_like(m)).sum(dim=2)
        lo = torch.where(ok, m, torch.full_like(m, float("inf"))).min(dim=2).values
        hi, arg = torch.where(ok, m, torch.full_like(m, float("-inf"))).max(dim=2)
        cnt = ok.sum(dim=2)
        e1.record()
        torch.cuda.synchronize()
        base_ms.append(e0.elapsed_time(e1))
        m_host = m.cpu().numpy()
        hi_np = np.where(np.isfinite(m_host), m_host, -np.inf)
        agree = agree and bool((hi.cpu().numpy() == summary[g, :, :, st["max"]]).all()) and \
            bool((hi_np.argmax(axis=2) == summary[g, :, :, st["argmax"]]).all()) and \
            bool((cnt.cpu().numpy() == summary[g, :, :, st["finite"]]).all()) and bool((lo.cpu().numpy() == summary[g, :, :, st["min"]]).all())
        del total, arg
        c.close()
    subset_ms = sum(base_ms[1:]) * sub / max(sub - 1, 1) if sub > 1 else sum(base_ms)    # the first gain's launch warms up: left out, rescaled
    row = {"workload": f"tank protocol {len(SETPOINTS)} x {STEPS} steps, prior controller alone, process noise on, state {args.state}",
           "gains": args.gains, "plants": args.plants, "plant_grid": list(shape), "pairs": args.gains * args.plants,
           "pair_steps": args.gains * args.plants * n,
           "sweep_ms": statistics.median(sweep_ms), "sweep_all_ms": sweep_ms, "sweep_launches": 2,
           "sweep_workspace_bytes": ws_bytes, "sweep_table_bytes": int(summary.nbytes),
           "sweep_pair_steps_per_s": args.gains * args.plants * n / (statistics.median(sweep_ms) * 1e-3),
           "per_gain_subset": sub, "per_gain_subset_ms": subset_ms, "per_gain_ms_each": subset_ms / sub,
           "per_gain_scaled_ms": subset_ms / sub * args.gains, "per_gain_scaling": f"timed on the first {sub} gains, scaled linearly to {args.gains}; "
           "state restoration between gains not counted",
           "per_gain_launches": args.gains, "per_gain_workspace_bytes": 0,
           "per_gain_table_bytes": args.gains * len(SETPOINTS) * native.METRIC_ROWS * args.plants * 8,
           "max_argmax_min_finite_agree_on_subset": agree,
           "sweep_over_per_gain": statistics.median(sweep_ms) / (subset_ms / sub * args.gains)}
    line = json.dumps(row)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    if not agree:
        sys.exit("the two routes disagree on the subset")


if __name__ == "__main__":
    main()
