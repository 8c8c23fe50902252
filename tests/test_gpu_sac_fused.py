"""The fused SAC optimizer step (csrc/sac_fused.hip, `pime_sac_step`) against the reference and the oracle.

  * the reference's OWN four-iteration update at batch 4 096 / width 128 / state_dim 4 (tests/golden/sac_update*.npz, made by
    make_golden_sac.py from the unmodified elegantrl/agent.py:397-478): first-step gradients, alpha_log, weights after one and four
    steps, objectives -- through `pime_sac_step` directly and through AgentSAC.update_net (fused and module path);
  * run-to-run bit reproducibility, padding words that stay exactly zero;
  * the kernels' own Philox draws (streams 4 and 5) reproduced on the host by tests/sac_oracle.py;
  * update_net from one HIP graph against eager launches."""
import numpy as np
import pytest
import torch

import sac_oracle as S
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx():
    g, nets, steps = load_golden("sac_update.npz"), load_golden("sac_update_nets0.npz"), load_golden("sac_update_steps.npz")
    return {"g": g, "nets": nets, "steps": steps, "md": int(g["sac:hyper"][0]), "D": int(g["sac:hyper"][1]), "B": int(g["sac:hyper"][2]),
            "iters": int(g["sac:hyper"][3]), "lr": float(g["sac:hyper"][4]), "tau": float(g["sac:hyper"][5]), "te": float(g["sac:hyper"][6])}


def _np_sd(g, prefix):
    return {k[len(prefix) + 1:]: g[k] for k in g.files if k.startswith(prefix + ".")}


def _agent(md, D, act=None, cri=None, cri_t=None, seed=0):
    from pime_amd.elegantrl.agent_sac import AgentSAC
    torch.manual_seed(seed)
    ag = AgentSAC(device=DEV)
    ag.init(md, D, 1)
    to = lambda sd: {k: torch.from_numpy(np.asarray(v).copy()).to(DEV) for k, v in sd.items()}   # noqa: E731
    if act is not None:
        ag.act.load_state_dict(to(act), strict=True)
        ag.cri.load_state_dict(to(cri), strict=True)
        ag.cri_target.load_state_dict(to(cri_t), strict=True)
    else:
        with torch.no_grad():   # a target that differs from the online critic, heads away from their tiny initial scale
            for p in ag.cri_target.parameters():
                p.add_(torch.randn_like(p) * 0.02)
            ag.act.net_a_avg.weight.normal_(0, 0.1)
    return ag


def _fixture_agent(fx):
    return _agent(fx["md"], fx["D"], _np_sd(fx["nets"], "sac:act0"), _np_sd(fx["nets"], "sac:cri0"), _np_sd(fx["nets"], "sac:cri0"))


def _sd_np(net):
    return {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}


def _check_nets(fx, ag, tag, bar):
    for name, net in (("act", ag.act), ("cri", ag.cri), ("cri_target", ag.cri_target)):
        for k, v in net.state_dict().items():
            want = fx["steps"][f"sac:{name}_{tag}.{k}"]
            err = np.abs(v.cpu().numpy() - want).max()
            assert err <= bar, f"{name}_{tag}.{k}: {err:.2e}"


def _random_buffer(n, D, seed):
    rng = np.random.RandomState(seed)
    scale = np.array([10., 10., 10., 50., 5., 5., 5.])[:D]
    shift = np.array([0., 0., 0., 25., 0., 0., 0.])[:D]
    state = (rng.rand(n, D) * scale - shift).astype(np.float32)
    other = np.stack([-rng.rand(n) * 5, np.where(rng.rand(n) < 0.02, 0.0, 0.99), np.tanh(rng.randn(n))], axis=1).astype(np.float32)
    return state, other


def test_fused_step_against_the_references_update_at_batch_4096(fx):
    """Step 1: every critic / actor gradient element within 3e-4 of its tensor's largest entry of the REFERENCE's .grad, alpha_log
    within 1e-9, all three nets within 2e-6; after the fourth step: weights within 1e-5,
    alpha_log within 1e-9, objectives within 1e-3."""
    from pime_amd import ops
    g = fx["g"]
    ag = _fixture_agent(fx)
    f = ag._fused_step(fx["B"])
    assert isinstance(f, ops.FusedSAC), "batch 4 096 / width 128 / state_dim 4 must be served by the fused step"
    state, other = torch.from_numpy(g["sac:state"]).to(DEV), torch.from_numpy(g["sac:other"]).to(DEV)
    idx = torch.from_numpy(g["sac:indices"].astype(np.int64)).to(DEV)
    n1, n2 = torch.from_numpy(g["sac:noise_next"]).to(DEV), torch.from_numpy(g["sac:noise_pg"]).to(DEV)
    f.workspace.fill_(float("nan"))
    # in stages: critic gradients / critic apply + temperature / actor gradients / actor apply
    f.step(state, other, idx, idx + 1, n1, n2, fx["tau"], fx["te"], phases=1, row=0)
    torch.cuda.synchronize()
    for name, p in ag.cri.named_parameters():
        assert float(p.grad.abs().max()) == 0.0, "phase 1 leaves the slabs only"
    f.step(state, other, idx, idx + 1, n1, n2, fx["tau"], fx["te"], phases=2, row=0)
    torch.cuda.synchronize()
    loss = f.loss.cpu().numpy()
    assert loss[6] == 0.0   # obj_alpha = alpha_log * gradient, alpha_log = 0 before the first step
    assert abs(ag.alpha_log.item() - g["sac:alpha_log"][1]) <= 1e-9
    assert abs(loss[7] - np.exp(g["sac:alpha_log"][1])) <= 1e-6
    f.step(state, other, idx, idx + 1, n1, n2, fx["tau"], fx["te"], phases=4, row=0)
    f.step(state, other, idx, idx + 1, n1, n2, fx["tau"], fx["te"], phases=8, row=0)
    torch.cuda.synchronize()
    for tag, net in (("cri", ag.cri), ("act", ag.act)):
        for name, p in net.named_parameters():
            want = fx["nets"][f"sac:grad1:{tag}.{name}"]
            err = np.abs(p.grad.cpu().numpy() - want).max() / np.abs(want).max()
            print(f"sac fused grad1 {tag}.{name}: {err:.2e} of the largest entry")
            assert err <= 3e-4, f"first-step gradient of {tag}.{name}: {err:.2e}"
    _check_nets(fx, ag, "step1", 2e-6)
    f.row = 1
    for _ in range(fx["iters"] - 1):
        f.step(state, other, idx, idx + 1, n1, n2, fx["tau"], fx["te"])
    torch.cuda.synchronize()
    assert f.row == fx["iters"]
    _check_nets(fx, ag, "step4", 1e-5)
    assert abs(ag.alpha_log.item() - g["sac:alpha_log"][2]) <= 1e-9
    loss = f.loss.cpu().numpy()
    np.testing.assert_allclose([loss[4], loss[5]], g["sac:obj"], rtol=1e-3)
    # padding words of the flat tensors (between tensors whose size is no multiple of 4) stay exactly zero
    for flat, offs, net in ((f.act_flat, f.act_off, ag.act), (f.cri_flat, f.cri_off, ag.cri), (f.cri_t_flat, f.cri_off, ag.cri_target)):
        used = torch.zeros_like(flat, dtype=torch.bool)
        for off, p in zip(offs, net.parameters()):
            used[off:off + p.numel()] = True
        assert int((~used).sum()) > 0 and float(flat[~used].abs().max()) == 0.0


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "modules"])
def test_update_net_with_injected_draws_matches_the_reference(fx, fused):
    """AgentSAC.update_net on the GPU with the reference's draws injected (draw_hook), on the fused kernels and on the PyTorch
    modules: the nets after four iterations within 1e-5, alpha_log within 1e-9 (fused) / 2e-9 (modules: torch's own float32 Adam),
    the returned objectives within 1e-3."""
    from pime_amd.elegantrl.replay import ReplayBuffer
    g = fx["g"]
    ag = _fixture_agent(fx)
    ag.use_fused_update = fused
    buf = ReplayBuffer(len(g["sac:state"]) + 8, fx["D"], 1, if_on_policy=False, device=DEV)
    buf.extend_buffer(g["sac:state"], g["sac:other"])
    idx = g["sac:indices"].astype(np.int64)
    ag.draw_hook = lambda n, b: (idx[:n], idx[:n] + 1, g["sac:noise_next"][:n], g["sac:noise_pg"][:n])
    obj_a, obj_c = ag.update_net(buf, fx["iters"], fx["B"], 1)
    assert (ag._fused_sac is not None and ag._fused_sac is not False) == fused
    _check_nets(fx, ag, "step4", 1e-5)
    assert abs(ag.alpha_log.item() - g["sac:alpha_log"][2]) <= (1e-9 if fused else 2e-9)
    np.testing.assert_allclose([obj_a, obj_c], g["sac:obj"], rtol=1e-3)


def test_fused_step_is_bit_reproducible():
    """Two agents, same start, same rows, same draws: identical bits in every parameter, gradient and the temperature after three
    steps (every workgroup's partial gradient goes to its own slab; the slabs are summed in slab order; no atomics)."""
    outs = []
    state, other = _random_buffer(5000, 4, 1)
    ts, to = torch.from_numpy(state).to(DEV), torch.from_numpy(other).to(DEV)
    idx = torch.from_numpy(np.random.RandomState(3).randint(0, 4999, size=(3, 4096)).astype(np.int64)).to(DEV)
    n1 = torch.from_numpy(np.random.RandomState(4).randn(3, 4096).astype(np.float32)).to(DEV)
    n2 = torch.from_numpy(np.random.RandomState(5).randn(3, 4096).astype(np.float32)).to(DEV)
    for _ in range(2):
        ag = _agent(128, 4, seed=9)
        f = ag._fused_step(4096)
        for _ in range(3):
            f.step(ts, to, idx, idx + 1, n1, n2, ag.soft_update_tau, ag.target_entropy)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (f.act_flat, f.cri_flat, f.cri_t_flat, f.act_grad, f.cri_grad, ag.alpha_log.detach(), f.loss)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("md,D", [(128, 4), (64, 3)])
def test_fused_step_draws_the_oracles_noise(md, D):
    """Both noise tables NULL: the kernels draw themselves (Philox streams 4 and 5, counter (batch position, epoch, table row)); the
    host restatement of those draws through the float64 step must give the same gradients -- the actor launch has to form the SAME
    policy-gradient draw as the critic launch used for the temperature."""
    B = 256
    ag = _agent(md, D, seed=4)
    with torch.no_grad():
        ag.alpha_log.fill_(-0.5)
    o = S.Sac(_sd_np(ag.act), _sd_np(ag.cri), _sd_np(ag.cri_target), alpha_log=-0.5, lr=ag.learning_rate, tau=ag.soft_update_tau)
    f = ag._fused_step(B)
    state, other = _random_buffer(1000, D, 6)
    idx = np.random.RandomState(2).randint(0, 999, size=(3, B)).astype(np.int64)
    ti, ts, to = torch.from_numpy(idx).to(DEV), torch.from_numpy(state).to(DEV), torch.from_numpy(other).to(DEV)
    f.epoch[0] = 5                     # epoch offset 5 (what begin_update advances), table row 2
    seed, epoch = 0x1234567890AB, 7
    f.step(ts, to, ti, ti + 1, None, None, ag.soft_update_tau, 0.0, noise_seed=seed, noise_epoch=epoch, row=2)
    e1, e2 = S.philox_noise(seed, epoch + 5, 2, B, S.STREAM_NEXT), S.philox_noise(seed, epoch + 5, 2, B, S.STREAM_PG)
    assert abs(float(e1.std()) - 1.0) < 0.15 and abs(float(e2.std()) - 1.0) < 0.15 and abs(float(np.corrcoef(e1, e2)[0, 1])) < 0.2
    o.opt_a.t = o.opt_c.t = o.opt_t.t = 2   # table row 2 on a fresh agent is Adam step number 3
    r = o.step(state, other, idx[2], idx[2] + 1, e1, e2)
    torch.cuda.synchronize()
    for tag, net, grads in (("cri", ag.cri, r["gc"]), ("act", ag.act, r["ga"])):
        for name, p in net.named_parameters():
            want = grads[name].reshape(p.shape)
            err = np.abs(p.grad.cpu().numpy() - want).max() / np.abs(want).max()
            assert err <= 3e-4, f"{tag}.{name}: {err:.2e}"
    loss = f.loss.cpu().numpy()
    np.testing.assert_allclose(loss[4:8], [r["obj_a"], r["obj_c"], r["obj_alpha"], r["alpha"]], rtol=1e-3, atol=1e-6)


def test_update_net_runs_the_fused_step_from_one_graph_and_matches_eager():
    """AgentSAC.update_net on a VecReplayBuffer: the first call launches eagerly, later calls replay ONE HIP graph of the whole
    update; with the same injected tables both give the same bits, and the graph survives from call to call."""
    from pime_amd.elegantrl.replay import VecReplayBuffer
    N, D, B, n_steps = 256, 4, 512, 6
    state, other = _random_buffer(40 * N, D, 2)

    def run(graphs):
        ag = _agent(64, D, seed=12)
        ag.use_hip_graphs = graphs
        buf = VecReplayBuffer(40 * N, N, D, 1, DEV)
        buf.state.copy_(torch.from_numpy(state).to(DEV).view(40, N, D))
        buf.other.copy_(torch.from_numpy(other).to(DEV).view(40, N, 3))
        buf.next_slot, buf.if_full = 0, True
        rng = np.random.RandomState(21)

        def hook(steps, batch):
            idx = rng.randint(0, 39 * N, size=(steps, batch)).astype(np.int64)
            return idx, idx + N, rng.randn(steps, batch).astype(np.float32), rng.randn(steps, batch).astype(np.float32)
        ag.draw_hook = hook
        res = [ag.update_net(buf, n_steps * N, B, 1) for _ in range(3)]
        torch.cuda.synchronize()
        f = ag._fused_sac
        assert (f.tables["graph"] is not None) == graphs and float(f.steps_done) == 2 * n_steps
        return res, [t.clone() for t in (f.act_flat, f.cri_flat, f.cri_t_flat, ag.alpha_log.detach())]

    res_g, w_g = run(True)
    res_e, w_e = run(False)
    assert res_g == res_e and all(np.isfinite(v) for r in res_g for v in r)
    for a, b in zip(w_g, w_e):
        assert torch.equal(a, b)


def test_wide_agent_takes_the_module_path_with_one_warning():
    """Width 256 is outside the fused step: update_net runs on the PyTorch modules, with exactly one RuntimeWarning per shape."""
    import warnings
    from pime_amd.elegantrl.replay import ReplayBuffer
    ag = _agent(256, 5, seed=2)
    state, other = _random_buffer(600, 5, 3)
    buf = ReplayBuffer(608, 5, 1, if_on_policy=False, device=DEV)
    buf.extend_buffer(state, other)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for _ in range(2):
            oa, oc = ag.update_net(buf, 2, 64, 1)
    assert ag._fused_sac is False and np.isfinite(oa) and np.isfinite(oc)
    assert len([x for x in w if issubclass(x.category, RuntimeWarning) and "SAC" in str(x.message)]) == 1
