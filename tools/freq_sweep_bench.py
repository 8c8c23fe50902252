#!/usr/bin/env python3
"""usage: tools/freq_sweep_bench.py [--plants 1024] [--rows 288] [--state mixed] [--md 128] [--out profiles/freq_sweep_bench.jsonl]

What the fused frequency-response sweep costs against the routes the tree had before it, on one GPU, at the shape of
tools/disturb_sweep_bench.py.  Workload: `rows` excitation rows (rows / 3 frequencies -- whole numbers of cycles in the second half of
a segment -- at the set-point, in front of the actuator and on the measurement, amplitude 0.05) x `plants` water-tank plants (a1 x a2 x
Kp grid over the ensemble ranges), the tank's step-response protocol (set-points 3, 6, 9, 4, 2 x 500 steps = 2 500 steps), process noise
on, the modular residual actor at width `md`: 288 x 1 024 x 2 500 = 7.4e8 pair-steps.

  sweep   ONE pime_freq_sweep call (two launches), pairs / actions / outputs NULL: HIP events around it, median of 3 after 1 warm-up
  (a)     ONE pime_disturb_sweep call with `rows` NOMINAL rows on the same lane state: the same loop without the excitation, the table
          loads and the lock-in sums (it stores fifteen rows per segment, this sweep sixteen).  The yardstick: the ratio sweep / (a) is
          what the excitation costs.  Timed the same way.
  (b)     the step-per-launch loop with a host-modulated set-point, the only way the question could be asked before: per step
          set_field("r", sp + e_k) from the host, the actor's torch module on the observation, VecControlEnv.step, and the eight lock-in
          sums as torch reductions.  2 rows x 250 steps timed (HIP events around the whole loop) and scaled linearly to rows x 2 500.
With every amplitude set to 0 the first eight rows must equal the disturbance sweep's nominal rows exactly.  One JSON line is appended to
--out."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freq_sweep_bench.jsonl"))
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
    onset = STEPS // 2
    per = -(-args.rows // 3)
    cycles = np.rint(np.linspace(1, (STEPS - onset - 1) // 2, per))
    rows, wave = protocols.excitation_grid(np.tile(cycles, 3)[:args.rows], 0.05, np.repeat([0, 1, 2], per)[:args.rows], STEPS, onset)
    quiet = rows.copy()
    quiet[:, 1] = 0.0
    nominal_rows = np.tile(np.array([[float(onset), 0.0, 0.0, 1.0, 1.0, 1.0]]), (len(rows), 1))

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
    assert env.frequency_supported(pk) and env.disturbance_supported(pk)
    rows_d = torch.as_tensor(rows, dtype=torch.float64, device=dev).contiguous()      # uploaded once: the call alone is timed
    wave_d = torch.as_tensor(wave, dtype=torch.float64, device=dev).contiguous()
    quiet_d = torch.as_tensor(quiet, dtype=torch.float64, device=dev).contiguous()
    nominal_d = torch.as_tensor(nominal_rows, dtype=torch.float64, device=dev).contiguous()

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
    sweep_ms, summary = timed(lambda: env.frequency_sweep(pk, K, rows_d, wave_d, n, **kw))
    a_ms, disturb = timed(lambda: env.disturbance_sweep(pk, K, nominal_d, n, **kw))
    still = env.frequency_sweep(pk, K, quiet_d, wave_d, n, **kw).cpu().numpy()
    agree = bool(np.array_equal(still[:, :, :8].view(np.uint64), disturb[:, :, :8].view(np.uint64)))
    env.close()

    # (b) step per launch, the set-point written from the host before every step, the lock-in sums as torch reductions
    pick, steps_b = [0, len(rows) - 1], 250
    act = agent.act
    c = fresh()
    obs = c.obs.clone()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for q in pick:
        amp, k0 = float(rows[q, 1]), min(int(rows[q, 2]), steps_b // 2)
        acc = [torch.zeros(args.plants, dtype=torch.float64, device=dev) for _ in range(8)]
        for t in range(steps_b):
            cs, sn = float(wave[q, t, 0]), float(wave[q, t, 1])
            c.set_field("r", np.full(args.plants, SETPOINTS[0] + amp * sn))
            with torch.no_grad():
                a = act(obs)[:, 0].double()
            obs = c.step(a, auto_reset=False)[0]
            if t >= k0:
                y = obs[:, 1].double()
                for j, term in enumerate((y * cs, y * sn, a * cs, a * sn, y, a, y * y, a * a)):
                    acc[j] += term
    e1.record()
    torch.cuda.synchronize()
    b_ms = e0.elapsed_time(e1) / (len(pick) * steps_b) * (len(rows) * n)
    c.close()

    sweep, a = statistics.median(sweep_ms), statistics.median(a_ms)
    rec = dict(tool="freq_sweep_bench", rows=len(rows), plants=args.plants, steps=n, state=args.state, kind="modular_actor", md=args.md,
               pair_steps=len(rows) * args.plants * n, sweep_ms=round(sweep, 3), sweep_ms_all=[round(v, 3) for v in sweep_ms],
               a_disturb_nominal_ms=round(a, 3), a_disturb_nominal_ms_all=[round(v, 3) for v in a_ms], ratio_to_a=round(sweep / a, 4),
               b_rows_timed=len(pick), b_steps_timed=steps_b, b_ms_scaled=round(b_ms, 1), speedup_vs_b=round(b_ms / sweep, 1),
               pair_steps_per_s=round(len(rows) * args.plants * n / (sweep * 1e-3), 1), zero_amplitude_equals_disturb_nominal=agree)
    print(json.dumps(rec))
    assert agree, "with zero amplitude the first eight rows differ from the disturbance sweep's nominal rows"
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
