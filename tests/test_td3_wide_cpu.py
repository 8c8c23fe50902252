"""CPU side of the fused TD3 step at width 256 and on the Stacking observations (state_dim up to 31): the shapes the library
accepts, its flat parameter layout for them, and the float64 oracle (oracle/td3.py) against the reference's own first step at
net_dim 256 / state_dim 30 / batch 4 096 (tests/golden/td3_update_256*.npz, made by make_golden_td3_wide.py)."""
import numpy as np
import pytest

from conftest import load_golden


def _lib():
    import pime_amd.native as nt
    return nt.lib()


@pytest.mark.parametrize("D,A,md,want", [(30, 1, 256, 1), (12, 1, 64, 1), (31, 1, 128, 1), (3, 1, 256, 1), (4, 1, 128, 1),
                                         (32, 1, 256, 0), (30, 2, 256, 0), (30, 1, 96, 0), (0, 1, 256, 0), (30, 1, 512, 0)])
def test_td3_supported_shapes(D, A, md, want):
    assert _lib().pime_td3_supported(D, A, md) == want


@pytest.mark.parametrize("D,md", [(30, 256), (31, 256), (12, 64), (30, 128), (3, 256), (17, 128)])
def test_td3_param_offsets_follow_module_order(D, md):
    """Every tensor of Actor / CriticTwin at its nn.Module position, starting on a multiple of 4 floats, right behind the previous
    one (padded to 4); the flat size covers the last."""
    import ctypes as C
    import torch
    from pime_amd.elegantrl.net import Actor, CriticTwin
    L = _lib()
    for which, net in ((0, Actor(md, D, 1)), (1, CriticTwin(md, D, 1))):
        offs = (C.c_int32 * 8)()
        assert L.pime_td3_param_offsets(which, D, md, offs) == 0
        total = L.pime_td3_param_floats(which, D, md)
        params = [p for _, p in net.named_parameters()]
        assert len(params) == 8
        pos = 0
        for off, p in zip(offs, params):
            assert off % 4 == 0 and off == (pos + 3) // 4 * 4
            pos = off + p.numel()
        assert total == (pos + 3) // 4 * 4
        assert isinstance(params[0], torch.nn.Parameter)
    assert L.pime_td3_workspace_floats(D, md, 4096) > 0


def test_td3_unsupported_shape_reports_the_supported_set():
    import ctypes as C
    import pime_amd.native as nt
    offs = (C.c_int32 * 8)()
    assert _lib().pime_td3_param_offsets(0, 32, 256, offs) != 0
    assert _lib().pime_td3_param_floats(0, 30, 96) == -1
    assert "width" in nt.last_error()


def _wide():
    g = load_golden("td3_update_256.npz")
    nets = load_golden("td3_update_256_nets0.npz")
    grads = load_golden("td3_update_256_grad1.npz")
    steps = load_golden("td3_update_256_step1.npz")
    return g, nets, grads, steps


def _np_sd(g, prefix):
    return {k[len(prefix) + 1:]: g[k] for k in g.files if k.startswith(prefix + ".")}


def test_oracle_reproduces_the_width_256_reference_step():
    """The reference's first TD3 step at net_dim 256, state_dim 30, batch 4 096: the oracle's gradients within 1e-5 of each
    tensor's largest entry, its objectives within 1e-5 and the online nets after Adam within 2e-6."""
    from oracle import td3
    g, nets, grads, steps = _wide()
    md, D, B = (int(v) for v in g["td3w:hyper"][:3])
    assert (md, D, B) == (256, 30, 4096)
    act, cri = _np_sd(nets, "td3w:act0"), _np_sd(nets, "td3w:cri0")
    assert act["net.0.weight"].shape == (256, 30) and cri["net_sa.0.weight"].shape == (256, 31)
    o = td3.Td3(act, act, cri, cri, lr=float(g["td3w:hyper"][3]), tau=float(g["td3w:hyper"][4]),
                policy_noise=float(g["td3w:hyper"][5]), update_freq=int(g["td3w:hyper"][6]))
    idx = g["td3w:indices"][0].astype(np.int64)
    obj_a, obj_c, gc, ga = o.step(0, g["td3w:state"], g["td3w:other"], idx, idx + 1, g["td3w:noise"][0])
    for tag, gr in (("cri", gc), ("act", ga)):
        for name, v in gr.items():
            want = grads[f"td3w:grad1:{tag}.{name}"]
            np.testing.assert_allclose(v.reshape(want.shape), want, rtol=0, atol=1e-5 * max(np.abs(want).max(), 1e-6),
                                       err_msg=f"{tag}.{name}")
    np.testing.assert_allclose([obj_a, obj_c / 2], g["td3w:obj"], rtol=1e-5, atol=1e-6)   # update_net returns obj_critic / 2
    for tag, ref in (("act_step1", o.act), ("cri_step1", o.cri)):
        for k, v in ref.items():
            np.testing.assert_allclose(v, steps[f"td3w:{tag}.{k}"], rtol=0, atol=2e-6, err_msg=f"{tag}.{k}")
