#!/usr/bin/env python3
"""TD3 optimizer steps at width 256 on the Stacking10 observation, in ONE process: the fused step (csrc/td3_fused.hip) and the module
path (AgentTD3._one_update, PIME_TD3_FUSED=0's route) at (256, 30, 4096), and the fused step at (128, 30, 4096) and (128, 4, 4096).
Each is AgentTD3.update_net on a synthetic vector replay ring (no env): two warm-up calls (eager, then the capture of the update's
graphs), then REPS calls of STEPS optimizer steps timed with HIP events.  One JSON line per shape: us per step, GFLOP per step from the
layer shapes, and the fraction of the f32 matrix peak.

    python tools/td3_wide_bench.py [out.jsonl]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pime_amd.elegantrl.agent import AgentTD3  # noqa: E402
from pime_amd.elegantrl.replay import VecReplayBuffer  # noqa: E402

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


def main():
    rows = [measure(256, 30, 4096, True), measure(256, 30, 4096, False), measure(128, 30, 4096, True), measure(128, 4, 4096, True)]
    rows.append({"speedup_fused_vs_module_256_30_4096": round(rows[1]["us_per_step"] / rows[0]["us_per_step"], 2)})
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
