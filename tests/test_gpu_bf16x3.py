"""PIME_GRAD_BF16X3=1 (opt-in): the streamed layers of the 16-tile gradient kernels on bf16 matrix instructions, every f32 operand
split into three bf16 pieces (csrc/mlp16.hip: layer16r_b3, six v_mfma_f32_16x16x32_bf16 per 16 x 16 x 32 block).  A different rounding
of the same f32 products, so the contract is the f32 path's own: pime_ppo_minibatch_grad against PyTorch fp32 autograd of the
reference loss (agent.py:637-655) within 3e-4 of each tensor's largest entry, bitwise repeatable (tests/test_gpu_mlp16.py:
check_grads); the optimizer step fused into the slab reduction leaves the bf16 planes equal to a fresh split of the new parameters;
whole update_net calls against the weights the unmodified reference produced (tests/golden/ppo_update*.npz: width 256 plain and
modular, width 128 modular) at the f32 path's tolerances.
Child processes: both switches are read once per process.  The layer alone against float64: tools/layer16_b3_bench.hip
(profiles/r04_n_layer16_b3_bench.txt: 3.5e-7 of max |y|, the f32 chain 4.0e-7)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import torch
import test_gpu_mlp16 as t
import test_gpu_ppo_fused as f
from pime_amd import native
lib = native.lib()
for kind, k in (("critic", native.MLP_CRITIC), ("actor", native.MLP_PLAIN_ACTOR), ("modular", native.MLP_MODULAR_ACTOR)):
    plain = lib.pime_ppo_bwd_image_floats(k, 4, 1, 128)
    assert plain > (3 if kind == "modular" else 2) * 128 * 128, (kind, plain)   # the planes sit behind the f32 transposed image
for kind, md, D, B in CASES:
    t.check_grads(kind, md, D, B)
for kind, md, D in (("modular", 128, 3), ("resid", 128, 3), ("resid", 256, 3)):
    f.test_fused_step_keeps_the_packed_images_current(kind, md, D)
    f.test_adam_fused_into_the_slab_reduction_equals_the_separate_step(kind, md, D)
import test_gpu_update_golden as u   # the UNMODIFIED reference's weights after a whole update_net, same tolerances as the f32 path
for tag, mode in (("wts10_256", "one_graph"), ("wtmod256", "two_graph"), ("ph128", "one_graph")):
    u.test_hip_update_net_matches_reference_weights(tag, mode)
for case in ("mw", "big"):   # the reference's own first-step .grad tensors, multi-workgroup / slab-accumulating batches (width 128)
    u.test_multi_workgroup_update_against_reference_gradients(case)
print("BF16X3_OK")
'''

# One minibatch gradient against FLOAT64 autograd of the same loss on the same minibatch: max and rms error of every net's flat
# gradient, relative to that gradient's largest entry.  Run once per path (child processes), reported side by side.
_ERR_CHILD = r'''
import copy, json, os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import torch
from pime_amd import ops
from test_gpu_ppo_fused import _data, _make, _torch_grads, DEV
out = {}
for kind, md, D, B in (("resid", 128, 3, 16384), ("modular", 128, 4, 16384), ("resid", 256, 30, 16384), ("modular", 256, 4, 16384)):
    act, cri = _make(kind, md, D, seed=B + md)
    L = 3 * B
    state, action, logprob, adv, r_sum = _data(L, D, act, seed=1)
    idx = torch.randint(L, (B,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    act64, cri64 = copy.deepcopy(act).double(), copy.deepcopy(cri).double()
    want = _torch_grads(act64, cri64, state.double(), action.double(), logprob.double(), adv.double(), r_sum.double(), idx, 0.2, 0.02)[0]
    fused = ops.FusedPPOGrad(act, cri, B)
    fused.zero_grad()
    fused(state, action.reshape(-1).contiguous(), logprob, adv, r_sum, idx, 0.2, 0.02, torch.zeros(1, device=DEV))
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in list(act.named_parameters()) + [("cri." + k, v) for k, v in cri.named_parameters()] if p.requires_grad}
    for net in ("act", "cri"):
        names = [n for n in want if n.startswith("cri.") == (net == "cri")]
        w = torch.cat([want[n].reshape(-1) for n in names])
        g = torch.cat([got[n].double().reshape(-1) for n in names])
        d = (g - w).abs() / w.abs().max()
        out[f"{kind}{md}.{net}"] = {"max": float(d.max()), "rms": float(d.pow(2).mean().sqrt()), "p99": float(torch.quantile(d, 0.99)),
                                    "far": float((d > 2e-6).double().mean())}
print("GRAD_ERR " + json.dumps(out))
'''


def _run(cases, extra_env):
    env = dict(os.environ, PIME_ROOT=ROOT, PIME_MLP16="1", **extra_env)
    r = subprocess.run([sys.executable, "-c", _CHILD.replace("CASES", repr(cases))], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "BF16X3_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bf16x3_gradients_match_autograd_and_repeat_bitwise():
    _run([("resid", 128, 3, 4096), ("resid", 128, 3, 70000), ("resid", 128, 30, 1000), ("ppo", 128, 4, 777),
          ("modular", 128, 3, 4096), ("modular", 128, 4, 1000), ("modular", 128, 4, 40000),
          ("resid", 256, 30, 4096), ("resid", 256, 3, 777), ("modular", 256, 4, 4096), ("modular", 256, 3, 1000)],
         {"PIME_GRAD_BF16X3": "1"})


def test_gradient_error_against_float64_autograd_is_reported_for_both_paths():
    """max / rms error of one minibatch gradient against float64 autograd, f32 MFMA path and bf16x3 path side by side (both through the
    16-tile family: PIME_MLP16=1).  The variant's contract is "f32-level error": the 99th percentile of its error may not exceed twice
    the f32 path's (in practice it is at or below it -- six exact bf16 products summed in f32 round less often than a chain of f32
    FMAs)."""
    import json
    res = {}
    for name, extra in (("f32", {}), ("bf16x3", {"PIME_GRAD_BF16X3": "1"})):
        env = dict(os.environ, PIME_ROOT=ROOT, PIME_MLP16="1", **extra)
        env.pop("PIME_GRAD_BF16X3", None) if not extra else None
        r = subprocess.run([sys.executable, "-c", _ERR_CHILD], env=env, capture_output=True, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("GRAD_ERR ")]
        assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-4000:]
        res[name] = json.loads(line[-1][len("GRAD_ERR "):])
    rows = []
    for key in res["f32"]:
        a, b = res["f32"][key], res["bf16x3"][key]
        rows.append(f"{key:16s} f32 p99 {a['p99']:.2e} rms {a['rms']:.2e} max {a['max']:.2e} | bf16x3 p99 {b['p99']:.2e} rms {b['rms']:.2e} "
                    f"max {b['max']:.2e} (entries beyond 2e-6: {b['far']:.4f})")
        # p99, not max: the critic is a ReLU net, and a unit whose pre-activation is within rounding of zero for ONE sample flips its
        # mask between any two float evaluations -- that sample's whole contribution to the unit's weight row (1 / B of the gradient,
        # ~1e-5 of its largest entry at B = 16 384) then differs.  Either path shows such rows against float64 for some seeds; they
        # say nothing about the products' precision.  At most one row per hundred may be such a row.
        assert b["p99"] <= max(2.0 * a["p99"], 5e-7), rows[-1]
        assert b["far"] <= 0.01, rows[-1]
    report = "\n".join(rows)
    print("\ngradient error / max |gradient| against float64 autograd (B = 16 384):\n" + report)
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "bf16x3_gradient_error.txt"), "w") as f:
        f.write("gradient error / max |gradient| against float64 autograd of the same minibatch (B = 16 384), tests/test_gpu_bf16x3.py\n" + report + "\n")


_PLANES_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import numpy as np, torch
from pime_amd import ops
from test_gpu_ppo_fused import _make, DEV
for md in (128, 256):
    act, cri = _make("resid", md, 3, seed=5)
    f = ops.FusedPPOGrad(act, cri, 4096)
    torch.cuda.synchronize()
    T = md // 16
    per_layer = (T // 2) * T * 768 * 2          # bf16 elements of one layer's three planes
    for net, mod in zip(f.nets, (act, cri)):
        planes = net["img_bwd"][net["n_bwd_f32"]:].cpu().numpy().view(np.uint16)
        assert planes.size == 4 * per_layer
        sd = dict(mod.named_parameters())
        W1, W2 = sd["net.2.weight"].detach().cpu().numpy(), sd["net.4.weight"].detach().cpu().numpy()
        for name, base, W in (("w1", 0, W1), ("w2", per_layer, W2), ("w2t", 2 * per_layer, W2.T), ("w1t", 3 * per_layer, W1.T)):
            # image [k-step ks][output tile to][plane][lane (i, g)][e]: W[16 to + i][16 (2 ks + (e >> 2)) + 4 g + (e & 3)]
            img = (planes[base:base + per_layer].astype(np.uint32) << 16).view(np.float32).reshape(T // 2, T, 3, 4, 16, 2, 4)
            #                                                                 ks      to plane g   i  e>>2 e&3
            rec = img.astype(np.float64).sum(axis=2)                       # hi + mid + lo: [ks][to][g][i][eh][el]
            rec = rec.transpose(1, 3, 0, 4, 2, 5).reshape(md, md)          # [to][i] x [ks][eh][g][el]  (k = 32 ks + 16 eh + 4 g + el)
            assert np.array_equal(rec.astype(np.float32), W), (md, name, float(np.abs(rec - W).max()))
            hi = img[:, :, 0].astype(np.float64).transpose(1, 3, 0, 4, 2, 5).reshape(md, md)
            assert np.abs(hi - W).max() <= 2.0 ** -8 * np.abs(W).max()     # the leading piece alone is W at bf16 precision
print("PLANES_OK")
'''


def test_bf16_planes_hold_the_weights_exactly_in_the_documented_layout():
    """The three bf16 planes behind the transposed f32 image, unpacked on the host with the layout DESIGN.md section 4b states, sum to
    the layer's weights EXACTLY (hi + mid + lo is an exact decomposition of an f32 value), for the forward layers and their
    transposes, widths 128 and 256; the hi plane alone is the weight at bf16 precision."""
    env = dict(os.environ, PIME_ROOT=ROOT, PIME_MLP16="1", PIME_GRAD_BF16X3="1")
    r = subprocess.run([sys.executable, "-c", _PLANES_CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PLANES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


_MODULAR_PLANES_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import numpy as np, torch
import ppo_cases as PC
import test_gpu_ppo_sweep as SW

def unpack(planes, base, n_out, n_k):
    # One layer's image, pack16_b3_layer of csrc/mlp16.hip: [k-step ks][output tile to][plane][lane (g, i)][e], bf16, holding
    # V[16 to + i][32 ks + 16 (e >> 2) + 4 g + (e & 3)] of the [n_out x n_k] matrix V the layer multiplies by.  base: in floats.
    TO, KS = n_out // 16, n_k // 32
    n = KS * TO * 3 * 512
    img = (planes[2 * base:2 * base + n].astype(np.uint32) << 16).view(np.float32).reshape(KS, TO, 3, 4, 16, 2, 4).astype(np.float64)
    order = lambda a: a.transpose(1, 3, 0, 4, 2, 5).reshape(n_out, n_k)   # [ks][to][g][i][eh][el] -> [to][i] x [ks][eh][g][el]
    return order(img.sum(axis=2)), order(img[:, :, 0]), base + n // 2

def check(name, planes, base, V):
    rec, hi, end = unpack(planes, base, *V.shape)
    assert np.array_equal(rec.astype(np.float32), V), (name, float(np.abs(rec - V).max()))   # hi + mid + lo: exact
    assert np.abs(hi - V).max() <= 2.0 ** -8 * np.abs(V).max(), name                          # the leading piece: bf16 precision
    assert np.abs(V).max() > 0
    return end

forced16 = PC.forced16_process()
assert PC.b3_process()
for kind, D, Di, md in ((("modular", 7, 3, 256), ("modular", 20, 1, 128)) if forced16 else (("modular", 4, 1, 256), ("modular", 20, 1, 128))):
    s = PC.b3_spec(kind, D, Di, md, 37, forced16=forced16, vet=False)
    act, cri, f = SW._fused(PC.build(s))
    torch.cuda.synchronize()
    hd = md // 2
    for net, mod, role, on in zip(f.nets, (act, cri), ("modular", "critic"), PC.b3_nets(s, forced16)):
        planes = net["img_bwd"][net["n_bwd_f32"]:].cpu().numpy().view(np.uint16)
        assert (planes.size > 0) == on, (md, role)
        if not on:
            continue   # width 128 without PIME_MLP16: the split-pipeline actor carries no planes, the critic next to it does
        sd = {k: v.detach().cpu().numpy() for k, v in mod.named_parameters()}
        if role == "modular":
            # layout_b3_16m: w1o, w1i (the towers' second layers, [md / 2 x md]: parameters 2 and 6 of the pack order), wn, wnt
            # (net.0, [md x md]: parameter 8, and its transpose), w1ot, w1it (the towers' transposes, [md x md / 2])
            Wo, Wi, Wn = sd["other_net.2.weight"], sd["integrator_net.2.weight"], sd["net.0.weight"]
            assert Wo.shape == Wi.shape == (hd, md) and Wn.shape == (md, md)
            layers = (("w1o", Wo), ("w1i", Wi), ("wn", Wn), ("wnt", Wn.T), ("w1ot", Wo.T), ("w1it", Wi.T))
        else:   # layout_b3_16: w1, w2, w2t, w1t
            W1, W2 = sd["net.2.weight"], sd["net.4.weight"]
            layers = (("w1", W1), ("w2", W2), ("w2t", W2.T), ("w1t", W1.T))
        base = 0
        for name, V in layers:
            base = check((md, role, name), planes, base, np.ascontiguousarray(V))
        assert 2 * base == planes.size, (md, role, base, planes.size)
print("PLANES_OK")
"""


@pytest.mark.parametrize("forced16", (True, False), ids=("mlp16", "alone"))
def test_bf16_planes_of_the_modular_actor_and_of_a_lone_critic(forced16):
    """layout_b3_16m unpacked on the host -- six images, the towers' second layers and their transposes half as wide or half as
    deep as net.0's -- at width 256 (Di 3 and Di 1) and, under PIME_MLP16=1, at width 128; hi + mid + lo is the f32 weight or its
    transpose exactly, hi alone within 2^-8 of the largest weight.  The critic (plain layout, its own module) at width 256 next
    to them, and at width 128 on 20 floats WITHOUT PIME_MLP16: the one configuration in which the critic alone carries planes
    (its actor runs the split pipeline)."""
    env = {k: v for k, v in os.environ.items() if k not in ("PIME_MLP16", "PIME_GRAD_BF16X3")}
    env.update(PIME_ROOT=ROOT, PIME_GRAD_BF16X3="1")
    if forced16:
        env["PIME_MLP16"] = "1"
    r = subprocess.run([sys.executable, "-c", _MODULAR_PLANES_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLANES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
