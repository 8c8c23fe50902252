#!/usr/bin/env python3
"""usage: tools/eval_band_bench.py [--lanes 65536] [--parent-tree DIR] [--rounds 3] [--out profiles/eval_band_bench.jsonl]

What the fused response band costs and saves, on one GPU.  Workload: tools/eval_metrics_bench.py's -- the water tank's
robustness protocol (set-points 3, 6, 9, 4, 2 x 500 steps) under a width-128 ResidualIntegratorModularPPO actor on a grid of
`lanes` plants, all lanes one group.

  1. in this process, HIP events around the launch (and what follows it on the device), median of 5 after 2 warm-ups, with the
     peak device memory above what the env and the actor hold:
       (a) band, stats only           pime_rollout_eval_band without ret / trace / hist
       (b) band, stats + histogram    ... with a 128-bin histogram of the output
       (c) metrics only               pime_rollout_eval_metrics, the launch the band adds to
       (d) traced + torch             the best route without the band: pime_rollout_eval with the float64 trace (48 bytes per lane
                                      and step), then the same sixteen rows by torch reductions of the trace on the device
                                      (no histogram: torch has none per step at this size)
  2. the returns-only and the metrics-only launch of this tree against the same launches of another build's tree
     (--parent-tree: a checkout of the parent commit with its library built), child processes interleaved on the same box.

One JSON line per measurement is appended to --out.  A child that fails ends the script: nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from eval_metrics_bench import MD, SETPOINTS, STEPS, setup, start  # noqa: E402  (the same workload, by construction)

BINS, LO, HI = 128, 0.0, 10.0


def timed(env, launch, reps=5, warm=2):
    """median HIP-event ms of `launch()` over `reps` runs after `warm`, and the peak device memory it added (bytes)."""
    import torch
    ms, peak = [], 0
    for i in range(warm + reps):
        start(env)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = launch()
        e1.record()
        torch.cuda.synchronize()
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del res
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), peak


def child(tree, lanes):
    env, fused, _ = setup(tree, lanes)
    n = len(SETPOINTS) * STEPS
    r_ms, _ = timed(env, lambda: env.rollout_eval(fused[0], fused[1], n, setpoints=SETPOINTS, seg_len=STEPS))
    m_ms, _ = timed(env, lambda: env.rollout_eval_metrics(fused[0], fused[1], n, setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10))
    print("CHILD_MS " + json.dumps({"returns_only": r_ms, "metrics_only": m_ms}))


def torch_rows(tr):
    """The band's sixteen rows [T, 16] from the tank's trace [T, 6, N] (h1, h2, r, I after the step | reward, action)."""
    import torch
    y, r = tr[:, 1], tr[:, 2]
    rows = []
    for x in (y, r - y, tr[:, 5], tr[:, 4]):
        rows += [x.sum(dim=1), (x * x).sum(dim=1), x.amin(dim=1), x.amax(dim=1)]
    return torch.stack(rows, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_band_bench.jsonl"))
    ap.add_argument("--child", default=None, metavar="TREE", help="(child mode) time the returns-only and metrics-only launches of TREE")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.lanes)

    env, fused, shape = setup(ROOT, args.lanes)
    from pime_amd import native
    n = len(SETPOINTS) * STEPS
    base = {"workload": f"tank protocol {len(SETPOINTS)} x {STEPS} steps, modular actor width {MD}, one group", "lanes": args.lanes,
            "grid": list(shape), "reps": 5, "warmups": 2}
    kw = dict(setpoints=SETPOINTS, seg_len=STEPS, band=0.05, tail=10)
    ws = int(native.lib().pime_rollout_eval_band_workspace_bytes(env._h, native.MLP_MODULAR_ACTOR, MD, n, args.lanes))
    rows = []

    def band(hist):
        return env.rollout_eval_band(fused[0], fused[1], n, hist=hist, **kw)
    a_ms, a_peak = timed(env, lambda: band(None))
    rows.append(dict(base, what="band_stats_only", device_ms=a_ms, workspace_bytes=ws, peak_device_bytes=a_peak, bytes_out=n * 16 * 8))
    b_ms, b_peak = timed(env, lambda: band((BINS, LO, HI)))
    rows.append(dict(base, what="band_stats_and_histogram", bins=BINS, device_ms=b_ms, workspace_bytes=ws, peak_device_bytes=b_peak,
                     bytes_out=n * (16 * 8 + BINS * 4), counter_adds_per_s=args.lanes * n / (b_ms * 1e-3)))
    c_ms, c_peak = timed(env, lambda: env.rollout_eval_metrics(fused[0], fused[1], n, **kw))
    rows.append(dict(base, what="metrics_only_launch", device_ms=c_ms, peak_device_bytes=c_peak))

    def traced():
        _, tr = env.rollout_eval(fused[0], fused[1], n, setpoints=SETPOINTS, seg_len=STEPS, want_trace=True)
        return torch_rows(tr)
    d_ms, d_peak = timed(env, traced)
    rows.append(dict(base, what="traced_launch_plus_torch_reductions", device_ms=d_ms, peak_device_bytes=d_peak, trace_bytes=n * 6 * 8 * args.lanes,
                     band_stats_only_over_this=a_ms / d_ms, band_peak_bytes_over_this=a_peak / d_peak))
    env.close()
    del env

    if args.parent_tree:
        res = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for tag, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--lanes", str(args.lanes)],
                                   capture_output=True, text=True, timeout=300)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_MS ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit(f"the child on the {tag} tree failed ({r.returncode}): stopping")
                res[tag].append(json.loads(line[-1].split(" ", 1)[1]))
        for what in ("returns_only", "metrics_only"):
            this, parent = ([x[what] for x in res[t]] for t in ("this", "parent"))
            rows.append(dict(base, what=f"{what}_launch_ab", rounds=args.rounds, this_ms=this, parent_ms=parent,
                             this_median_ms=statistics.median(this), parent_median_ms=statistics.median(parent),
                             this_over_parent=statistics.median(this) / statistics.median(parent)))
    with open(args.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
