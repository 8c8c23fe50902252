"""ppo_fused_pair_kernel (csrc/ppo_fused.hip) runs a group's two bodies in either order: half of the workgroups (pair_flip, a
function of the workgroup index) run the critic's body first, so that the chip is not in the same phase everywhere at once.  The
order may not show in any result.  A flipped workgroup differs from an unflipped one in what waits in LDS during the first body
(the actor's action / old log-prob / advantage instead of the critic's target; at D = 4, width 128, there is no room and they are
read again through the index), in which net's forward images are started behind the first body's tail, and in which net's totals
are written first.  The four pair instantiations at the smallest batches at which a flipped workgroup exists and can go wrong:

  257              workgroup 0 full, workgroup 1 with one valid sample and 255 clamped ones
  512              two full groups: one unflipped and one flipped workgroup if odd workgroups flip
  16 * 256 + 33    workgroups 8..15 flip if every second set of eight does; ragged last tile
  16 * 256         sixteen full groups, one per workgroup: group 0 and group 8 swap bit for bit (see that test)
  cap * 256 + 4096 the first sixteen workgroups take a second group: under either rule an unflipped and a flipped workgroup run
                   the `accum` path (cap: the grid of a large batch, read from the library)

against torch f32 autograd at the bars of test_gpu_ppo_pair.py, plus bit-level properties: reproducibility, independence of what
the workspace held, independence of which workgroup (flipped or not) gets a group, and the Adam step fused into the reduction."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_ppo_fused import _torch_grads
from test_gpu_ppo_pair import NETS, _call, _grid_cap, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(name):
    return {"one_sample_more": 257, "two_groups": 512, "two_sets_of_eight": 16 * 256 + 33, "sixteen_groups": 16 * 256,
            "second_group": _grid_cap() * 256 + 16 * 256}[name]


@functools.lru_cache(maxsize=None)
def _case(kind, md, D, bname):
    """Nets, data, indices, the fused gradient object and the autograd reference of a case: computed once, shared, left unchanged
    (every call below overwrites the gradients)."""
    B = _batch(bname)
    act, cri, data, idx, fused = _setup(kind, md, D, B, seed=B + md)
    ref = _torch_grads(act, cri, *data, idx, 0.2, 0.02)
    return B, act, cri, data, idx, fused, ref


def _grads(fused, act, cri):
    """The kernels' gradients by parameter name, read from the flat gradient buffer they write (optimizer order: trainable
    actor parameters, then the critic's) -- not from p.grad, which autograd re-binds to tensors of its own in _torch_grads."""
    names = {id(p): n for n, p in list(act.named_parameters()) + [("cri." + k, v) for k, v in cri.named_parameters()]}
    out, off = {}, 0
    for p in fused.params:
        out[names[id(p)]] = fused.flat_grad[off:off + p.numel()].view_as(p)
        off += p.numel()
    assert off == fused.flat_grad.numel()
    return out


def _assert_at_autograd_bar(tag, got, want):
    assert set(got) == set(want)
    for name in want:
        w, g = want[name], got[name]
        tol = 3e-4 * float(w.abs().max()) + 1e-7   # f32 sums over B samples in a different order (test_gpu_ppo_pair.py)
        err = float((w - g).abs().max())
        print(f"{tag} {name}: max |diff| {err:.3e} (bar {tol:.3e})")
        assert err <= tol, f"{name}: max |diff| {err:.3e} > {tol:.3e} (|grad|max {float(w.abs().max()):.3e})"


@pytest.mark.parametrize("bname", ["one_sample_more", "two_groups", "two_sets_of_eight", "second_group"])
@pytest.mark.parametrize("kind,md,D", NETS)
def test_either_order_matches_autograd(kind, md, D, bname):
    B, act, cri, data, idx, fused, (want, s_sur, s_ent, s_cri, scale) = _case(kind, md, D, bname)
    fused.loss_sums.zero_()
    got_scale = torch.zeros(1, device=DEV)
    _call(fused, data, idx, got_scale, overwrite=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(got_scale.item(), scale.item(), rtol=3e-6)
    _assert_at_autograd_bar(f"{kind}-{md}-{D} B={B}", _grads(fused, act, cri), want)
    sums = fused.loss_sums.tolist()
    np.testing.assert_allclose(sums[0], s_sur, rtol=2e-4, atol=1e-3 * B ** 0.5)
    np.testing.assert_allclose(sums[1], s_ent, rtol=2e-4, atol=1e-3 * B ** 0.5)
    np.testing.assert_allclose(sums[2], s_cri, rtol=2e-4)


@pytest.mark.parametrize("bname", ["two_sets_of_eight", "second_group"])
@pytest.mark.parametrize("kind,md,D", NETS)
def test_either_order_is_reproducible_and_ignores_what_the_workspace_held(kind, md, D, bname):
    """Two calls on the same inputs give the same flat-gradient bits; so does a call whose workspaces (activation stash + slabs of
    both nets) were filled with NaN, and one with zeros: neither order reads anything before the same call has written it."""
    _, _, _, data, idx, fused, _ = _case(kind, md, D, bname)
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
def test_two_groups_swapped_between_the_workgroups_give_the_same_bits(kind, md, D):
    """Indices [g0 | g1] against [g1 | g0]: each 256-sample group is processed once by workgroup 0 and once by workgroup 1 (one of
    them flipped if odd workgroups flip).  A group's slab does not depend on the workgroup that computes it, and the reduction adds
    the same two slabs in the other order, which is exact for two addends: the flat gradients are bit-identical."""
    _, _, _, data, idx, fused, _ = _case(kind, md, D, "two_groups")
    scale = torch.zeros(1, device=DEV)
    _call(fused, data, idx, scale, overwrite=True)
    torch.cuda.synchronize()
    g_ab, s_ab = fused.flat_grad.clone(), scale.clone()
    _call(fused, data, torch.cat([idx[256:], idx[:256]]).contiguous(), scale, overwrite=True)
    torch.cuda.synchronize()
    assert torch.isfinite(g_ab).all()
    assert torch.equal(fused.flat_grad, g_ab), "swapping the two groups between the workgroups changed gradient bits"
    assert torch.equal(scale, s_ab), "swapping the two groups between the workgroups changed the critic scale"


@pytest.mark.parametrize("kind,md,D", NETS)
def test_sets_of_eight_groups_swapped_match_autograd(kind, md, D):
    """Indices [b0 | b1 | rest] against [b1 | b0 | rest] with 2 048-index blocks: the groups of workgroups 0..7 go to workgroups
    8..15 and back (flipped if every second set of eight flips).  The reduction then adds sixteen slabs in another order, so the
    comparison is with the same autograd reference at the same bar, not bit for bit."""
    B, act, cri, data, idx, fused, (want, _, _, _, scale) = _case(kind, md, D, "two_sets_of_eight")
    swapped = torch.cat([idx[2048:4096], idx[:2048], idx[4096:]]).contiguous()
    got_scale = torch.zeros(1, device=DEV)
    _call(fused, data, swapped, got_scale, overwrite=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(got_scale.item(), scale.item(), rtol=3e-6)
    _assert_at_autograd_bar(f"{kind}-{md}-{D} B={B} swapped", _grads(fused, act, cri), want)


@pytest.mark.parametrize("kind,md,D", NETS)
def test_group_swapped_between_workgroups_0_and_8_gives_the_same_bits(kind, md, D):
    """Sixteen full groups, one per workgroup; the indices of group 0 and group 8 change places and the other fourteen stay.
    Workgroup 8 runs the critic first where every second set of eight workgroups flips, workgroup 0 never does.  Slabs 0 and 8
    are the only two addends of the reduction's wave 0 (it sums slabs w, w + 8, ... and there are sixteen), and in the float64
    target moments they meet first in the butterfly's step of 8 with nothing else added yet: both sums are exact under the
    swap, so the flat gradient and the critic scale are bit-identical."""
    _, _, _, data, idx, fused, _ = _case(kind, md, D, "sixteen_groups")
    scale = torch.zeros(1, device=DEV)
    _call(fused, data, idx, scale, overwrite=True)
    torch.cuda.synchronize()
    g_ab, s_ab = fused.flat_grad.clone(), scale.clone()
    swapped = torch.cat([idx[2048:2304], idx[256:2048], idx[:256], idx[2304:]]).contiguous()
    _call(fused, data, swapped, scale, overwrite=True)
    torch.cuda.synchronize()
    assert torch.isfinite(g_ab).all()
    assert torch.equal(fused.flat_grad, g_ab), "swapping group 0 and group 8 between their workgroups changed gradient bits"
    assert torch.equal(scale, s_ab), "swapping group 0 and group 8 between their workgroups changed the critic scale"


@pytest.mark.parametrize("kind,md,D", NETS)
def test_either_order_with_adam_in_the_slab_reduction_equals_the_separate_step(kind, md, D):
    """pime_ppo_minibatch_step through the pair kernel against pime_ppo_minibatch_grad + a separate Adam step, two steps, where an
    unflipped and a flipped workgroup both accumulate a second group: bit-equal parameters, moments, step count and gradients."""
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
