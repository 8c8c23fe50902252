"""Every shape and instantiation of the fused SAC step (csrc/sac_fused.hip) against the float64 oracle on the vetted cases of
tests/sac_cases.py (kink margins, mutants and float32 stability checked on the CPU by tests/test_sac_cases_cpu.py):

  a. every supported (width, state_dim) at a ragged batch of 37;
  b. every instantiation (width 64 / 128 x state width 3 / 4 compiled in / run-time) at B = 1, 17 and 8 193 (8 193 = 513 tiles > 512
     workgroups: workgroup 0 takes a second tile and accumulates into its slab);
  c. every hyper-parameter off its default (lr, betas, eps, tau, a target_entropy != 0, alpha_log != 0), table row 3 of 4;
  d. the Adam step base across three update_net calls through the captured graph.
Every step runs on a NaN-poisoned workspace.  Gradients: 3e-4 of each tensor's largest entry.  Weights, moments, the target critic
and the temperature: a float64 replay of Adam / the soft update from the kernel's OWN gradient within the bounds that the float32
operation count gives (tests/td3_cases.py: replay_bounds) -- Adam's first step moves every element by lr * sign(g), so an element
whose gradient is rounding noise cannot be compared with the oracle's weights at 2e-6, and 2e-6 is not widened."""
import numpy as np
import pytest
import torch

import sac_cases as SC
import sac_oracle as S
from oracle.td3 import CRITIC_KEYS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fused(case):
    """A fresh agent holding the case's nets and temperature, and an ops.FusedSAC with the case's hyper-parameters."""
    from pime_amd import ops
    from pime_amd.elegantrl.agent_sac import AgentSAC
    s, h = case.spec, case.spec.hyper
    ag = AgentSAC(device=DEV)
    ag.init(s.width, s.D, 1)
    for net, sd in zip((ag.act, ag.cri, ag.cri_target), case.nets):
        net.load_state_dict({k: torch.from_numpy(v.copy()).to(DEV) for k, v in sd.items()}, strict=True)
    with torch.no_grad():
        ag.alpha_log.fill_(h.alpha_log0)
    f = ops.FusedSAC(ag.act, ag.cri, ag.cri_target, ag.alpha_log, s.B, h.lr, lr_alpha=h.lr_alpha, betas=h.betas, eps=h.eps)
    return ag, f


def _step(case, f):
    s, h = case.spec, case.spec.hyper
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)   # noqa: E731  (a writable copy: the case's arrays are read-only)
    f.workspace.fill_(float("nan"))
    f.step(t(case.state), t(case.other), t(case.idx), t(case.nxt), t(case.noise_next), t(case.noise_pg), h.tau, h.target_entropy, row=s.row)
    torch.cuda.synchronize()


def _flat(net, keys):
    sd = net.state_dict()
    return np.concatenate([sd[k].detach().cpu().numpy().astype(np.float64).reshape(-1) for k in keys])


def _check(case, ag, f):
    s, h, mid = case.spec, case.spec.hyper, case.mid
    worst = 0.0
    for tag, net, grads in (("cri", ag.cri, mid["gc"]), ("act", ag.act, mid["ga"])):
        for name, p in net.named_parameters():
            want = grads[name].reshape(p.shape)
            got = p.grad.cpu().numpy()
            assert np.isfinite(got).all(), f"{tag}.{name}: non-finite gradient"
            err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
            worst = max(worst, err)
            assert err <= SC.BAR, f"{SC.spec_id(s)}: gradient of {tag}.{name}: {err:.2e} of the largest entry"
    print(f"sac sweep {SC.spec_id(s)}: worst gradient error {worst:.1e} of a tensor's largest entry")
    # Adam (+ soft update) replayed in float64 from the kernel's own gradients
    for keys, net, tgt, grad, before, before_t, m, v in (
            (CRITIC_KEYS, ag.cri, ag.cri_target, f.cri_grad, case.nets[1], case.nets[2], "cri_m", "cri_v"),
            (S.ACTOR_KEYS, ag.act, None, f.act_grad, case.nets[0], None, "act_m", "act_v")):
        p0 = SC.flatten(before, keys)
        g = np.concatenate([dict(net.named_parameters())[k].grad.detach().cpu().numpy().astype(np.float64).reshape(-1) for k in keys])
        t0 = SC.flatten(before_t, keys) if tgt is not None else None
        got_p = _flat(net, keys)
        rep = SC.adam_replay(p0, np.zeros_like(p0), np.zeros_like(p0), g, s.row + 1, h.lr, h.betas, h.eps, target=t0, tau=h.tau, blend_param=got_p)
        bounds = SC.replay_bounds(rep, np.zeros_like(p0), g, h.lr, target_before=t0)
        assert (np.abs(got_p - rep["param"]) <= bounds["param"]).all(), f"{SC.spec_id(s)}: parameters of {keys[0]}"
        if tgt is not None:
            assert (np.abs(_flat(tgt, keys) - rep["target"]) <= bounds["target"]).all(), f"{SC.spec_id(s)}: target critic"
    # the temperature: gradient mean(lp) - target_entropy from the oracle, its Adam step replayed in float64
    al = ag.alpha_log.item()
    assert abs(al - mid["alpha_log1"]) <= 2.0 ** -23 * abs(mid["alpha_log1"]) + 1e-5 * h.lr_alpha, (al, mid["alpha_log1"])   # replay_bounds' parameter bound
    loss = f.loss.cpu().numpy()
    np.testing.assert_allclose(loss[4:8], [mid["obj_a"], mid["obj_c"], mid["obj_alpha"], np.exp(mid["alpha_log1"])], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("s", SC.shape_cases(), ids=SC.spec_id)
def test_every_supported_shape(s):
    import pime_amd.native as nt
    assert nt.lib().pime_sac_supported(s.D, 1, s.width) == 1
    case = SC.build(s)
    ag, f = _fused(case)
    _step(case, f)
    _check(case, ag, f)


@pytest.mark.parametrize("s", SC.regime_cases(), ids=SC.spec_id)
def test_every_instantiation_at_three_batch_regimes(s):
    case = SC.build(s)
    ag, f = _fused(case)
    _step(case, f)
    _check(case, ag, f)


@pytest.mark.parametrize("s", SC.hyper_cases(), ids=SC.spec_id)
def test_non_default_hyper_parameters(s):
    case = SC.build(s)
    ag, f = _fused(case)
    _step(case, f)
    _check(case, ag, f)


def test_the_lists_are_what_the_library_serves():
    import pime_amd.native as nt
    L = nt.lib()
    assert {(md, D) for md in (32, 64, 128, 256) for D in range(0, 33) if L.pime_sac_supported(D, 1, md)} == set(SC.served())


def test_step_base_across_update_net_calls_through_the_graph():
    """Three update_net calls of two optimizer steps each (the second and third replay the captured graph): Adam step numbers 1..6.
    The float64 oracle stepped six times on the same draws must end at the same weights (1e-5) and temperature."""
    from pime_amd.elegantrl.replay import ReplayBuffer
    s = SC.spec(64, 4, 100, rows=6, vet=False)
    case = SC.build(s)
    ag, _ = _fused(case)
    ag._fused_sac = None
    with torch.no_grad():
        ag.alpha_log.fill_(-0.75)
    buf = ReplayBuffer(SC.N_BUF + 8, s.D, 1, if_on_policy=False, device=DEV)
    buf.extend_buffer(np.array(case.state), np.array(case.other))
    calls = []

    def hook(n, b):
        k = 2 * len(calls)
        calls.append(k)
        return case.idx[k:k + n], case.nxt[k:k + n], case.noise_next[k:k + n], case.noise_pg[k:k + n]
    ag.draw_hook = hook
    o = S.Sac(*case.nets, alpha_log=-0.75, lr=ag.learning_rate, tau=ag.soft_update_tau)
    for call in range(3):
        obj = ag.update_net(buf, 2, s.B, 1)
        for k in (2 * call, 2 * call + 1):
            r = o.step(case.state, case.other, case.idx[k], case.nxt[k], case.noise_next[k], case.noise_pg[k])
        np.testing.assert_allclose(obj, [r["obj_a"], r["obj_c"]], rtol=1e-3, atol=1e-6)
    f = ag._fused_sac
    assert f.tables["graph"] is not None and float(f.steps_done) == 4.0 and f.row == 2
    for net, ref in ((ag.act, o.act), (ag.cri, o.cri), (ag.cri_target, o.cri_t)):
        for k, v in net.state_dict().items():
            assert np.abs(v.cpu().numpy() - ref[k]).max() <= 1e-5, k
    assert abs(ag.alpha_log.item() - o.alpha_log) <= 6 * 2.0 ** -25 + 1e-8   # six float32 steps on a value in [0.5, 1): half an ulp (2^-25) each
