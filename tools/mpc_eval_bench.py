#!/usr/bin/env python3
"""usage: tools/mpc_eval_bench.py [--env wt|ph] [--state mixed|f64] [--plants 1024] [--horizon 20] [--passes 2] [--subset 32]
                                 [--threads 16] [--out profiles/mpc_eval_bench.jsonl]

What the fused receding-horizon benchmark controller costs on one GPU.  Workload: `plants` plants (tank: an a1 x a2 x Kp grid over the
ensemble ranges, as tools/prior_sweep_bench.py; pH: a qww_V x qc_V grid), the env's step-response protocol (tank: set-points 3, 6, 9,
4, 2 x 500 steps; pH: 10, 6, 3, 8, 5 x 50 steps), process noise on, horizon 20, 2 passes, rho 0, metrics only (no trace).

  (a) fused   ONE pime_mpc_eval launch: HIP events around it, 1 warm-up, median of 3
  (b) host    libpime_mpc_host.so -- the same closed loop compiled for the host, the only other implementation there is: the
              controller is sequential in time and cannot be composed from the GPU entry points the tree had, so there is no
              parent-commit GPU time to compare with.  Timed (wall clock) on the FIRST `subset` plants split over `threads` host
              threads and SCALED linearly to `plants`; labelled as such in the line.
The metrics of the two must agree on the subset in float64 state with the noise off; here the noise is on, so only the largest
relative ITAE difference is reported.  Also prints, for information, the ITAE regret of the env's built-in prior gain K against the
baseline on these plants.  One JSON line is appended to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="wt", choices=["wt", "ph"])
    ap.add_argument("--state", default="mixed", choices=["mixed", "f64"])
    ap.add_argument("--plants", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--subset", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_eval_bench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import mpc_eval as M                      # the ctypes binding of the host build (test infrastructure)
    from pime_amd import gym_control, native, protocols
    dev, is_ph = "cuda:0", args.env == "ph"
    p = args.plants.bit_length() - 1
    assert args.plants == 1 << p, "plants must be a power of two"
    if is_ph:
        shape = (1 << (p - p // 2), 1 << (p // 2))
        g = np.meshgrid(np.linspace(0.005, 0.015, shape[0]), np.linspace(0.0015, 0.0025, shape[1]), indexing="ij")
        setpoints, steps, name, kw = protocols.PH_SETPOINTS, 50, gym_control.PH_V35, {}
    else:
        shape = (1 << (p - 2 * (p // 3)), 1 << (p // 3), 1 << (p // 3))     # 1 024 -> 16 x 8 x 8
        g = np.meshgrid(np.linspace(0.0015, 0.0024, shape[0]), np.linspace(0.0015, 0.0024, shape[1]), np.linspace(0.07, 0.17, shape[2]),
                        indexing="ij")
        setpoints, steps, name, kw = protocols.WT_SETPOINTS, 500, gym_control.WT_INTEGRATOR, dict(reward_type="distance")
    plants = np.stack([a.reshape(-1) for a in g], axis=1)
    n = len(setpoints) * steps

    env = gym_control.make_vec(name, args.plants, device=dev, state_mode=args.state, seed=0, **kw)
    protocols._protocol_start(env, is_ph, steps, plants)
    fields = ("x", "A", "B", "C", "r", "I", "t", "episode") if is_ph else ("h1", "h2", "a1", "a2", "Kp", "r", "I", "t", "episode")
    lanes = {k: np.ascontiguousarray(env.get_field(k)) for k in fields}
    lanes["t"], lanes["episode"] = lanes["t"].astype(np.int32), lanes["episode"].astype(np.int32)
    fused_ms = []
    for i in range(4):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        metrics = env.mpc_eval(args.horizon, passes=args.passes, n_steps=n, seg_len=steps, setpoints=setpoints, band=0.05, tail=10)
        e1.record()
        torch.cuda.synchronize()
        if i >= 1:
            fused_ms.append(e0.elapsed_time(e1))
    metrics = metrics.cpu().numpy()
    _, prior, _ = env.rollout_eval_metrics(None, -env.K, n, setpoints=setpoints, seg_len=steps, band=0.05, tail=10)
    prior = prior.cpu().numpy()
    cfg0 = native.EnvCfg.from_buffer_copy(env.cfg)
    env.close()

    # (b) the host build on the first `subset` plants, `threads` threads, each a contiguous slice at its own lane offset
    sub = min(args.subset, args.plants)
    table = native.ph_table_build() if is_ph else None
    bounds = np.linspace(0, sub, min(args.threads, sub) + 1).astype(int)

    def part(j):
        lo, hi = int(bounds[j]), int(bounds[j + 1])
        cfg = native.EnvCfg.from_buffer_copy(cfg0)
        cfg.n_envs, cfg.env_offset = hi - lo, cfg0.env_offset + lo
        keep = None
        if is_ph:
            keep = np.ascontiguousarray(table, dtype=np.float64)
            cfg.ph_table, cfg.ph_table_len = keep.ctypes.data_as(C.POINTER(C.c_double)), len(keep)
        out = M.host_mpc(args.env, cfg, {k: np.ascontiguousarray(v[lo:hi]) for k, v in lanes.items()}, horizon=args.horizon, passes=args.passes,
                         n_steps=n, seg_len=steps, setpoints=setpoints, band=0.05, tail=10, trace=False)["metrics"]
        del keep
        return out

    M.host_lib()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(len(bounds) - 1) as pool:
        host = np.concatenate(list(pool.map(part, range(len(bounds) - 1))), axis=2)
    host_s = time.perf_counter() - t0
    j = protocols.METRIC_NAMES.index("itae")
    itae_diff = float(np.max(np.abs(host[:, j] - metrics[:, j, :sub]) / np.maximum(np.abs(host[:, j]), 1e-300)))

    med = statistics.median(fused_ms)
    cand_steps = args.plants * n * args.passes * 64 * args.horizon
    diff, ratio = protocols.regret({"itae": prior[:, j]}, {"itae": metrics[:, j]})
    print(f"ITAE of the built-in prior K against the MPC baseline, {args.plants} plants, per set-point segment (for information):")
    print("segment  set-point  MPC median  prior median  ratio median  ratio max  ratio min")
    for s, sp in enumerate(setpoints):
        print(f"{s:7d}  {sp:9.1f}  {np.median(metrics[s, j]):10.2f}  {np.median(prior[s, j]):12.2f}  {np.nanmedian(ratio[s]):12.2f}  "
              f"{np.nanmax(ratio[s]):9.2f}  {np.nanmin(ratio[s]):9.2f}")
    row = {"workload": f"{'pH' if is_ph else 'tank'} protocol {len(setpoints)} x {steps} steps, receding-horizon controller, process noise on, "
                       f"state {args.state}", "plants": args.plants, "plant_grid": list(shape), "horizon": args.horizon, "passes": args.passes,
           "rho": 0.0, "control_steps": args.plants * n, "candidate_lane_steps": cand_steps,
           "fused_ms": med, "fused_all_ms": fused_ms, "fused_launches": 1, "fused_candidate_lane_steps_per_s": cand_steps / (med * 1e-3),
           "host_subset": sub, "host_threads": len(bounds) - 1, "host_subset_s": host_s, "host_scaled_s": host_s * args.plants / sub,
           "host_scaling": f"libpime_mpc_host.so timed on the first {sub} plants over {len(bounds) - 1} threads (wall clock), scaled linearly "
                           f"to {args.plants}; no parent-commit GPU route exists",
           "fused_over_host_scaled": med * 1e-3 / (host_s * args.plants / sub), "itae_max_rel_diff_on_subset": itae_diff,
           "prior_over_mpc_itae_median": float(np.nanmedian(ratio)), "prior_over_mpc_itae_max": float(np.nanmax(ratio))}
    line = json.dumps(row)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
