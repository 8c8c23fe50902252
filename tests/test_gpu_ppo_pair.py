"""ppo_fused_pair_kernel (csrc/ppo_fused.hip): one workgroup runs a 256-sample group's actor AND critic -- one gather for both,
the critic's targets parked in LDS, its small segments and forward images loaded behind the actor's body, the per-workgroup sums
written out and re-zeroed between the two bodies.  The four (actor kind, width) instantiations, at the smallest batches at which
the merged workgroup can go wrong, against torch fp32 autograd at the bar of test_gpu_ppo_fused.py (3e-4 of each tensor's largest
entry; loss sums 1e-3-level), plus bit-level properties: reproducibility, independence of what the workspace held, and the Adam
step fused into the slab reduction.  These are the reference's own initialisation and random data at D = 3 and 4; the pair kernel's
other shapes (width 64 up to D = 32, width 128 at D = 1, 2 and 8 -- the only one whose actor body does not free the weight
buffer early), batches below a group, NaN in the trajectory rows the indices do not name and frozen parameters are swept against a
float64 oracle on vetted inputs by tests/test_gpu_ppo_sweep.py."""
import numpy as np
import pytest
import torch

from test_gpu_ppo_fused import _data, _make, _torch_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the pair kernel's instantiations: modular actor D = 3 (integrator_dim 1) and D = 4, plain actor, width 128; modular actor, width 64
NETS = [("modular", 128, 3), ("modular", 128, 4), ("resid", 128, 3), ("modular", 64, 3)]


def _grid_cap():
    """Workgroups the library launches for a batch too large for one group per workgroup (read from the library)."""
    from pime_amd import native
    L = native.lib()
    cap = L.pime_ppo_fused_grid(1 << 30)
    assert cap >= 1 and L.pime_ppo_fused_grid(cap * 256) == cap and L.pime_ppo_fused_grid(256) == 1 and L.pime_ppo_fused_grid(257) == 2
    return cap


def _batch(name):
    # one full group | a second workgroup with one valid tile and seven clamped ones | ragged last tile | some workgroups take
    # a second group (shared gather, LDS targets, re-zeroed sums and prefetched critic images across the group loop; `accum` slabs)
    return {"one_group": 256, "one_tile_more": 288, "ragged": 1000, "second_group": _grid_cap() * 256 + 300}[name]


def _setup(kind, md, D, B, seed):
    from pime_amd import native, ops
    act, cri = _make(kind, md, D, seed=seed)
    k = {"modular": native.MLP_MODULAR_ACTOR, "resid": native.MLP_PLAIN_ACTOR}[kind]
    assert native.lib().pime_ppo_pair_fits(k, D, getattr(act, "integrator_dim", 0), md) == 1, "the pair kernel does not serve this case"
    L = max(3 * B, 5000)
    data = _data(L, D, act, seed=1)
    idx = torch.randint(L, (B,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    return act, cri, data, idx, ops.FusedPPOGrad(act, cri, B)


def _call(fused, data, idx, scale, **kw):
    state, action, logprob, adv, r_sum = data
    fused(state, action.reshape(-1).contiguous(), logprob, adv, r_sum, idx, 0.2, 0.02, scale, **kw)


@pytest.mark.parametrize("bname", ["one_group", "one_tile_more", "ragged", "second_group"])
@pytest.mark.parametrize("kind,md,D", NETS)
def test_pair_gradients_match_autograd(kind, md, D, bname):
    B = _batch(bname)
    act, cri, data, idx, fused = _setup(kind, md, D, B, seed=B + md)
    want, s_sur, s_ent, s_cri, scale = _torch_grads(act, cri, *data, idx, 0.2, 0.02)
    fused.zero_grad()
    fused.loss_sums.zero_()
    got_scale = torch.zeros(1, device=DEV)
    _call(fused, data, idx, got_scale)
    torch.cuda.synchronize()
    np.testing.assert_allclose(got_scale.item(), scale.item(), rtol=3e-6)
    got = {n: p.grad for n, p in list(act.named_parameters()) + [("cri." + k, v) for k, v in cri.named_parameters()]
           if p.requires_grad}
    assert set(got) == set(want)
    for name in want:
        w, g = want[name], got[name]
        tol = 3e-4 * float(w.abs().max()) + 1e-7   # f32 sums over B samples in a different order
        err = float((w - g).abs().max())
        print(f"{kind}-{md}-{D} B={B} {name}: max |diff| {err:.3e} (bar {tol:.3e})")
        assert err <= tol, f"{name}: max |diff| {err:.3e} > {tol:.3e} (|grad|max {float(w.abs().max()):.3e})"
    sums = fused.loss_sums.tolist()
    np.testing.assert_allclose(sums[0], s_sur, rtol=2e-4, atol=1e-3 * B ** 0.5)
    np.testing.assert_allclose(sums[1], s_ent, rtol=2e-4, atol=1e-3 * B ** 0.5)
    np.testing.assert_allclose(sums[2], s_cri, rtol=2e-4)


@pytest.mark.parametrize("kind,md,D", NETS)
def test_pair_is_reproducible_and_ignores_what_the_workspace_held(kind, md, D):
    """Two calls on the same inputs give the same flat-gradient bits; so does a call whose workspaces (activation stash + slabs of
    both nets) were filled with NaN, and one with zeros: nothing is read before the same call has written it."""
    B = _batch("second_group")
    act, cri, data, idx, fused = _setup(kind, md, D, B, seed=5)
    scale = torch.zeros(1, device=DEV)

    def run(fill=None):
        if fill is not None:
            for net in fused.nets:
                net["ws"].fill_(fill)
        _call(fused, data, idx, scale, overwrite=True)
        torch.cuda.synchronize()
        return fused.flat_grad.clone()

    g1, g2 = run(), run()
    assert torch.isfinite(g1).all()
    assert torch.equal(g1, g2), "gradients differ between two identical calls"
    assert torch.equal(run(float("nan")), g1), "a NaN-filled workspace changed the gradients"
    assert torch.equal(run(0.0), g1), "a zero-filled workspace changed the gradients"


@pytest.mark.parametrize("kind,md,D", NETS)
def test_pair_with_adam_in_the_slab_reduction_equals_the_separate_step(kind, md, D):
    """pime_ppo_minibatch_step through the pair kernel against pime_ppo_minibatch_grad + a separate Adam step: bit-equal."""
    B = _batch("second_group")
    outs = []
    for fuse in (False, True):
        act, cri, data, _, fused = _setup(kind, md, D, B, seed=7)
        adam = fused.make_optimizer(1e-3)
        scale = torch.zeros(1, device=DEV)
        for step in range(2):
            idx = torch.randint(data[0].shape[0], (B,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(10 + step))
            _call(fused, data, idx, scale, overwrite=True, adam=adam if fuse else None)
            if not fuse:
                adam.step()
            fused.repack()
        torch.cuda.synchronize()
        outs.append((fused.flat_param.clone(), adam.exp_avg.clone(), adam.exp_avg_sq.clone(), adam.step_count.clone(),
                     fused.flat_grad.clone()))
    for a, b, name in zip(outs[0], outs[1], ("param", "exp_avg", "exp_avg_sq", "step", "grad")):
        assert torch.equal(a, b), f"{name} differs between the fused and the separate optimizer step"
    assert float(outs[1][3][0]) == 2.0 and float(outs[1][3][1]) == 0.0
