#!/usr/bin/env python3
"""usage: tools/eval_metrics_bench.py [--lanes 65536] [--parent-tree DIR] [--rounds 3] [--out profiles/eval_metrics_bench.jsonl]

What the fused step-response metrics cost and save, on one GPU.  Workload: the water tank's robustness protocol (set-points
3, 6, 9, 4, 2 x 500 steps) under a width-128 ResidualIntegratorModularPPO actor on a grid of `lanes` plants (a1 x a2 x Kp).

  1. in this process, HIP events around the launch, median of 5 after 2 warm-ups:
       (a) metrics only   pime_rollout_eval_metrics without ret / trace: 64 bytes per plant and segment leave the device
       (b) traced         pime_rollout_eval with the float64 trace (48 bytes per plant and step), then the trace copied to the
                          host and reduced there by protocols.metrics_from_records (wall clock, the same 5 + 2 runs)
  2. the returns-only pime_rollout_eval launch of this tree against the same launch of another build's tree (--parent-tree: a
     checkout of the parent commit with its library built), child processes interleaved on the same box, `--rounds` rounds.

One JSON line per measurement is appended to --out.  A child that fails ends the script: nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETPOINTS, STEPS, MD = (3., 6., 9., 4., 2.), 500, 128


def setup(tree, lanes):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from pime_amd import gym_control
    from pime_amd.utils import MODELS
    dev = "cuda:0"
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, lanes, device=dev, state_mode="mixed", seed=0, reward_type="distance")
    p = lanes.bit_length() - 1
    assert lanes == 1 << p, "lanes must be a power of two"
    shape = (1 << (p - 2 * (p // 3)), 1 << (p // 3), 1 << (p // 3))     # 65 536 -> 64 x 32 x 32
    a1, a2, kp = np.meshgrid(np.linspace(0.0015, 0.0025, shape[0]), np.linspace(0.0015, 0.0025, shape[1]),
                             np.linspace(0.07, 0.17, shape[2]), indexing="ij")
    env.set_reset_all(False)
    env.set_max_step(STEPS)
    env.reset_changable_parameters(a1.reshape(-1), a2.reshape(-1), kp.reshape(-1))
    torch.manual_seed(0)
    ag = MODELS["residualintegratormodularppo"](device=dev)
    ag.init(MD, env.state_dim, 1, 1)
    ag.init_residual({"init_K": env.K.reshape(-1, 1)})
    with torch.no_grad():
        ag.act.net[-1].weight.normal_(0, 0.1)
    ag.weights_changed()
    fused = ag.fused_eval_policy(env)
    assert fused is not None and env.eval_supported(fused[0], trace=True, schedule=True)
    return env, fused, shape


def start(env):
    import numpy as np
    env.reset()
    env.set_field("h1", np.zeros(env.num_envs)); env.set_field("h2", np.zeros(env.num_envs))


def timed(env, launch, after=None, reps=5, warm=2):
    """median over `reps` runs after `warm`: (HIP-event ms of `launch`, wall-clock ms of `after(result)`)."""
    import torch
    dev_ms, host_ms = [], []
    for i in range(warm + reps):
        start(env)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = launch()
        e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if after is not None:
            after(res)
        t1 = time.perf_counter()
        del res
        if i >= warm:
            dev_ms.append(e0.elapsed_time(e1)); host_ms.append((t1 - t0) * 1e3)
    return statistics.median(dev_ms), statistics.median(host_ms)


def returns_only(tree, lanes):
    env, fused, _ = setup(tree, lanes)
    n = len(SETPOINTS) * STEPS
    ms, _ = timed(env, lambda: env.rollout_eval(fused[0], fused[1], n, setpoints=SETPOINTS, seg_len=STEPS))
    print("RETURNS_ONLY_MS " + json.dumps(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_bench.jsonl"))
    ap.add_argument("--returns-only", default=None, metavar="TREE", help="(child mode) time the returns-only launch of TREE")
    args = ap.parse_args()
    if args.returns_only:
        return returns_only(args.returns_only, args.lanes)

    env, fused, shape = setup(ROOT, args.lanes)
    from pime_amd import protocols
    n = len(SETPOINTS) * STEPS
    base = {"workload": f"tank protocol {len(SETPOINTS)} x {STEPS} steps, modular actor width {MD}", "lanes": args.lanes,
            "grid": list(shape), "reps": 5, "warmups": 2}
    rows = []
    a_ms, _ = timed(env, lambda: env.rollout_eval_metrics(fused[0], fused[1], n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10))
    rows.append(dict(base, what="metrics_only_launch", device_ms=a_ms, bytes_out=len(SETPOINTS) * 8 * 8 * args.lanes))

    def reduce_on_host(res):
        tr = res[1].cpu().numpy()
        y_after = tr[:, 1]
        import numpy as np
        y_start = np.concatenate([np.zeros((1, args.lanes)), y_after[STEPS - 1:-1:STEPS]])
        protocols.metrics_from_records(y_after, tr[:, 2], tr[:, 5], tr[:, 4], y_start, seg_len=STEPS, band=0.05, tail=10)
    b_ms, b_host = timed(env, lambda: env.rollout_eval(fused[0], fused[1], n, setpoints=SETPOINTS, seg_len=STEPS, want_trace=True),
                         after=reduce_on_host)
    rows.append(dict(base, what="traced_launch_plus_host_reduction", device_ms=b_ms, host_copy_and_reduce_ms=b_host,
                     total_ms=b_ms + b_host, bytes_out=n * 6 * 8 * args.lanes))
    env.close()
    del env

    if args.parent_tree:
        res = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for tag, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--returns-only", tree, "--lanes", str(args.lanes)],
                                   capture_output=True, text=True, timeout=300)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RETURNS_ONLY_MS ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit(f"the returns-only child on the {tag} tree failed ({r.returncode}): stopping")
                res[tag].append(json.loads(line[-1].split(" ", 1)[1]))
        this, parent = statistics.median(res["this"]), statistics.median(res["parent"])
        rows.append(dict(base, what="returns_only_launch_ab", rounds=args.rounds, this_ms=res["this"], parent_ms=res["parent"],
                         this_median_ms=this, parent_median_ms=parent, this_over_parent=this / parent))
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
