"""Every route of the fused PPO minibatch gradient (pime_ppo_minibatch_grad / _step) against the float64 oracle of
tests/ppo_oracle.py, on the cases of tests/ppo_cases.py that are vetted on the CPU (tests/test_ppo_cases_cpu.py: no sample within
1e-5 of a kink of the objective, float32 numpy within 1e-4 of float64, every mutant of the oracle at least 10 x the bar away, every
branch of the loss populated) -- so "within 3e-4 of the tensor's largest entry" is neither flaky nor blind to a branch.

  a. every shape: widths 64 / 128 / 256 x plain D 1..32 and modular D 2..32, Di 1..3, ActorPPO, at a ragged batch of 37;
  b. every kernel class (route, widths, actor kind, first-layer variant) at fewer than a tile, a tile - 1 / + 1, a group - 1 / + 1
     and, per (route, width), grid cap x group + 1 samples (a workgroup takes a second group);
  c. actor and critic of different widths: ppo_fused_kernel<T, KIND> as a launch of its own;
  d. per (route, widths): NaN in the workspaces and in every trajectory row the indices do not name; stale slabs of a larger
     launch; frozen parameters (gradients routed to the dump, skipped by the fused Adam, images kept equal to a re-pack);
  e. widths 64 / 128 through the 16-tile family under PIME_MLP16=1, in a child process;
  f. the bf16x3 variant (PIME_GRAD_BF16X3=1: ppo16_kernel<8 | 16, ., true>, ppo16m_kernel<8 | 16, true>, pack16_b3_kernel) in child
     processes, one test per list of ppo_cases.B3_LISTS: the same run_case and the same properties of d., the same bars; per B3
     kernel class the error of every gradient element pooled and held to the f32 path's pool of the same list (99th percentile
     at most twice the f32 path's, or 5e-7: the contract of tests/test_gpu_bf16x3.py), since the 3e-4 bar cannot see a lost
     low-order piece (2^-16 per term); and the one shape the variant does not serve.  The report's key "b3" holds the variant's
     shares, routes, cap grids and both paths' pools (a record: profiles/ppo_sweep_b3_gpu.txt).
Every case asserts the route its spec names against pime_ppo_route.  Per case: every gradient tensor, every element, at 3e-4 of
the oracle tensor's largest entry; critic_scale at rtol 3e-6; the float64 target moments at rtol 1e-12; loss_sums[0, 1, 2, 4] at
the bars of tests/test_gpu_ppo_fused.py and tests/test_gpu_mlp16.py.  PIME_PPO_SWEEP_REPORT=<path> writes the largest used share
of every bar and the routes hit as JSON (a record -- profiles/ppo_sweep_gpu.txt --, not a threshold).

The split pipeline (a modular actor of width 128 on 14 floats or more) sums with float atomics: its gradients are not
reproducible bit for bit (tests/test_gpu_mlp16.py), so where the properties of d. say "bit-equal" that net is held to the oracle
at the bar instead, and pime_ppo_minibatch_step refuses it (tests/test_gpu_ppo_fused.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppo_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_USED = {}     # bar -> largest used share seen
_ROUTES = {}   # "actor family/critic family/launch widths" -> cases
_POOL = {}     # (B3 kernel class, net) -> [every gradient element's error / the tensor's largest entry]: part f
_POOL_CLASS = [None]   # (class label, (pool the actor, pool the critic)) of the case that run_case is on, set by part f's children
# part f's record: the variant's own used shares and routes, per list and class both paths' pools, the grids read for the cap batches
_B3 = {"used_share_of_bar": {}, "routes_hit": {}, "pools": {}, "grids": {}}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("PIME_PPO_SWEEP_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump({"used_share_of_bar": _USED, "routes_hit": _ROUTES, "b3": _B3}, fh, indent=1, sort_keys=True)


def _note(kind, value):
    _USED[kind] = max(_USED.get(kind, 0.0), float(value))


def _modules(case, freeze=()):
    """(actor, critic) torch modules holding the case's nets; freeze: "integrator" / "transfer" (actor), "critic"."""
    from pime_amd.elegantrl.net import ActorPPO, CriticAdv
    from pime_amd.elegantrl.net_residual import ActorResidualIntegratorModularPPO, ActorResidualPPO
    s = case.spec
    act = (ActorResidualIntegratorModularPPO(s.aw, s.D, 1, s.Di) if s.kind == "modular" else
           ActorPPO(s.aw, s.D, 1) if s.kind == "ppo" else ActorResidualPPO(s.aw, s.D, 1))
    cri = CriticAdv(s.D, s.cw)
    for net, sd in zip((act, cri), case.nets):
        missing, unexpected = net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=False)
        assert not unexpected and set(missing) <= {"priorK"}, (missing, unexpected)
    if "integrator" in freeze:
        act.frozen_integrator()
    if "transfer" in freeze:
        act.frozen_transfer()
    if "critic" in freeze:
        cri.frozen_transfer()
    return act.to(DEV), cri.to(DEV)


def _tables(case):
    return [torch.from_numpy(np.array(t)).to(DEV) for t in case.table], torch.from_numpy(np.array(case.idx)).to(DEV)


def _fused(case, max_batch=None, freeze=()):
    from pime_amd import ops
    act, cri = _modules(case, freeze)
    return act, cri, ops.FusedPPOGrad(act, cri, max_batch or case.spec.B)


def _call(fused, tables, idx, scale, **kw):
    state, action, logprob, adv, r_sum = tables
    fused(state, action, logprob, adv, r_sum, idx, PC.RATIO_CLIP, PC.LAMBDA_ENTROPY, scale, **kw)
    torch.cuda.synchronize()


def _assert_route(s, forced16=None):
    """The library's route is the spec's and the model's of THIS process (its PIME_MLP16, its PIME_GRAD_BF16X3); per net, the
    transposed image carries bf16 planes exactly where the model says the net runs a B3 kernel -- launch_ppo16 picks the kernel by
    the same b3_grad that sizes the image, so no case passes by silently running the f32 kernel."""
    import pime_amd.native as nt
    forced16 = PC.forced16_process() if forced16 is None else forced16
    b3 = PC.b3_process()
    got = PC.library_route(s.kind, s.D, s.Di, s.aw, s.cw)
    assert got == s.route == PC.expected_route(s.kind, s.D, s.Di, s.aw, s.cw, forced16, b3), f"{PC.spec_id(s)}: the library routes {got}"
    L = nt.lib()
    ka = nt.MLP_MODULAR_ACTOR if s.kind == "modular" else nt.MLP_PLAIN_ACTOR
    for k, kind, w, di in ((ka, PC.okind(s.kind), s.aw, s.Di), (nt.MLP_CRITIC, "critic", s.cw, 0)):
        n_bwd, n_f32 = L.pime_ppo_bwd_image_floats(k, s.D, di, w), L.pime_ppo_bwd_image_f32_floats(k, s.D, di, w)
        assert n_f32 > 0 and (n_bwd > n_f32) == (b3 and PC.b3_net(kind, w, s.D, di, forced16)) and n_bwd >= n_f32, \
            f"{PC.spec_id(s)}: {kind} of width {w}: image of {n_bwd} floats, {n_f32} of them f32"
    key = "/".join(got) + f" {s.aw}+{s.cw}" + (" (PIME_MLP16)" if forced16 else "") + (" (PIME_GRAD_BF16X3)" if b3 else "")
    _ROUTES[key] = _ROUTES.get(key, 0) + 1


def _named_grads(act, cri):
    return [("act." + n, p) for n, p in act.named_parameters() if p.requires_grad] + \
           [("cri." + n, p) for n, p in cri.named_parameters() if p.requires_grad]


def _check_gradients(case, act, cri, what, only=None):
    mid = case.mid
    for name, p in _named_grads(act, cri):
        if only is not None and not name.startswith(only):
            continue
        net, key = name.split(".", 1)
        want = mid["ga" if net == "act" else "gc"][key].reshape(p.shape)
        got = p.grad.cpu().numpy()
        assert np.isfinite(got).all(), f"{what}: non-finite gradient of {name}"
        big = np.abs(want).max()
        assert big > 0
        err = np.abs(got - want).max() / big
        if _POOL_CLASS[0] is not None and _POOL_CLASS[0][1][net == "cri"]:
            _POOL.setdefault((_POOL_CLASS[0][0], net), []).append((np.abs(got - want) / big).astype(np.float32).ravel())
        print(f"ppo sweep {what} {name}: {err:.2e} of the largest entry")
        _note(f"grad {name} (bar 3e-4 of the largest entry)", err / PC.BAR)
        assert err <= PC.BAR, f"{what}: gradient of {name}: {err:.2e} of the largest entry (bar {PC.BAR:.0e})"


def run_case(case, forced16=False):
    """One vetted case on a fresh object with NaN-filled workspaces: route, gradients, scale, moments, loss sums."""
    s, mid = case.spec, case.mid
    assert s.vet and mid is not None
    _assert_route(s, forced16)
    act, cri, fused = _fused(case)
    from pime_amd import ops
    assert ops.FusedPPOGrad.supported(act, cri) is True, f"{PC.spec_id(s)}: served by the library, refused by supported()"
    planes = PC.b3_nets(s, forced16) if PC.b3_process() else (False, False)
    assert tuple(n["img_bwd"].numel() > n["n_bwd_f32"] for n in fused.nets) == planes, f"{PC.spec_id(s)}: bf16 planes"
    tables, idx = _tables(case)
    for net in fused.nets:
        net["ws"].fill_(float("nan"))
    fused.zero_grad()
    fused.loss_sums.zero_()
    scale = torch.zeros(1, device=DEV)
    _call(fused, tables, idx, scale)
    what = PC.spec_id(s)
    names = {n for n, _ in _named_grads(act, cri)}
    assert names == {"act." + k for k in mid["ga"]} | {"cri." + k for k in mid["gc"]}
    _check_gradients(case, act, cri, what)
    got_scale = scale.item()
    _note("critic_scale (rtol 3e-6)", abs(got_scale / mid["scale"] - 1) / 3e-6)
    print(f"ppo sweep {what} critic_scale: {abs(got_scale / mid['scale'] - 1):.2e} relative")
    np.testing.assert_allclose(got_scale, mid["scale"], rtol=3e-6, err_msg=what)
    mom = fused.moments.cpu().numpy()
    _note("target moments (rtol 1e-12)", np.abs(mom / np.array(mid["moments"]) - 1).max() / 1e-12)
    np.testing.assert_allclose(mom, mid["moments"], rtol=1e-12, err_msg=what)
    sums = fused.loss_sums.tolist()
    s_sur, s_ent, s_cri = mid["sums"]
    atol = 1e-3 * s.B ** 0.5
    for i, want, rtol, at in ((0, s_sur, 2e-4, atol), (1, s_ent, 2e-4, atol), (2, s_cri, 2e-4, 0.0), (4, s_cri * mid["scale"], 3e-4, 0.0)):
        _note(f"loss_sums[{i}] (rtol {rtol:.0e}" + (", atol 1e-3 sqrt(B))" if at else ")"), abs(sums[i] - want) / (at + rtol * abs(want)))
        np.testing.assert_allclose(sums[i], want, rtol=rtol, atol=at, err_msg=f"{what}: loss_sums[{i}]")
    np.testing.assert_allclose(sums[3], got_scale, rtol=1e-6, err_msg=f"{what}: loss_sums[3]")


# ---------------------------------------------------------------------------------------------------------------- a, b, c
@pytest.mark.parametrize("s", PC.shape_cases(), ids=PC.spec_id)
def test_every_shape(s):
    run_case(PC.build(s))


@pytest.mark.parametrize("s", PC.regime_cases(), ids=PC.spec_id)
def test_every_class_in_every_batch_regime(s):
    """Positions 0 and B - 1 of the index list name the table's first and last row; a row is named twice from 4 samples on."""
    import pime_amd.native as nt
    L = nt.lib()
    case = PC.build(s)
    assert case.idx[0] == 0 and case.idx[-1] == PC.N_ROWS - 1
    assert L.pime_ppo_fused_grid(1 << 30) == PC.FUSED_CAP   # the cap batches are cap x group + 1
    if s.B > 10000:
        k = nt.MLP_MODULAR_ACTOR if s.kind == "modular" else nt.MLP_PLAIN_ACTOR
        for fam, grid, cap in ((s.route[0], L.pime_ppo_grid16(k, s.B, s.aw, s.D, s.Di), PC.GRID16_CAP),
                               (s.route[1], L.pime_ppo_grid16(nt.MLP_CRITIC, s.B, s.cw, s.D, 0), PC.GRID16_CAP)):
            if fam == "16tile":
                assert grid == cap and (s.B + 63) // 64 > cap, "no workgroup of the 16-tile kernel takes a second group"
        if "lds" in s.route:
            assert L.pime_ppo_fused_grid(s.B) == PC.FUSED_CAP and (s.B + 255) // 256 > PC.FUSED_CAP
    run_case(case)


@pytest.mark.parametrize("s", PC.mixed_cases(), ids=PC.spec_id)
def test_nets_of_different_widths_take_launches_of_their_own(s):
    assert s.route[2] == "single" and s.aw != s.cw
    run_case(PC.build(s))


def test_the_lists_cover_what_the_library_routes():
    """On the GPU machine's library: the route of every swept shape is the model's (the CPU test's assertion, repeated where the
    kernels run), and the lists hold every route the library answers."""
    routes = set()
    for w in PC.WIDTHS:
        for D in range(1, PC.MAX_D + 1):
            routes.add(PC.library_route("plain", D, 0, w, w))
            assert PC.library_route("plain", D, 0, w, w) == PC.expected_route("plain", D, 0, w, w)
            for Di in range(1, min(D, 4)):
                routes.add(PC.library_route("modular", D, Di, w, w))
                assert PC.library_route("modular", D, Di, w, w) == PC.expected_route("modular", D, Di, w, w)
    assert routes == {s.route for s in PC.shape_cases()} == {s.route for s in PC.regime_cases()}


# ------------------------------------------------------------------------------------------------------------------------ d
_PER_ROUTE = PC.per_route_shapes()   # one shape per (route, widths); their batches of 293 and 100 are PC.property_cases()


def _split(s):
    return "act." if s.route[0] == "split" else None


def _equal_or_close(case, flat_a, flat_b, fused, act, cri, what):
    """Bit-equal flat gradients; a split-pipeline actor's part (float atomics) is held to the oracle at the bar instead."""
    if _split(case.spec) is None:
        assert torch.equal(flat_a, flat_b), what
        return
    n_act = fused.critic_offset
    assert torch.equal(flat_a[n_act:], flat_b[n_act:]), what + " (critic)"
    _check_gradients(case, act, cri, what, only="act.")


@pytest.mark.parametrize("s", _PER_ROUTE, ids=PC.spec_id)
def test_nothing_unwritten_or_unnamed_is_read(s):
    """B = 293 (a second workgroup with a ragged tile and six clamped ones; a ragged 16-tile): the same call as is, and with NaN in
    the workspaces (stash, slabs), in the gradient buffer (PIME_PPO_OVERWRITE_GRADS) and in every trajectory row that the indices
    do not name -- a clamped lane that leaked into a sum would carry one in.  Bit-equal and finite."""
    case = PC.build(s._replace(B=293))
    _assert_route(case.spec)
    runs = []
    for poison in (False, True):
        act, cri, fused = _fused(case)
        tables, idx = _tables(case)
        if poison:
            for net in fused.nets:
                net["ws"].fill_(float("nan"))
            fused.flat_grad.fill_(float("nan"))
            unnamed = torch.ones(PC.N_ROWS, dtype=torch.bool, device=DEV)
            unnamed[idx] = False
            assert int(unnamed.sum()) > PC.N_ROWS // 2
            for t in tables:
                t[unnamed] = float("nan")
        scale = torch.zeros(1, device=DEV)
        _call(fused, tables, idx, scale, overwrite=True)
        runs.append((fused.flat_grad.clone(), scale.clone(), fused.moments.clone(), fused.loss_sums.clone(), act, cri, fused))
        for t in runs[-1][:4]:
            assert torch.isfinite(t).all(), "a poisoned word reached the call's results"
    a, b = runs
    _equal_or_close(case, a[0], b[0], b[6], b[4], b[5], "NaN in the workspaces / unnamed rows changed the gradients")
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    if s.route[:2] == ("lds", "lds"):
        assert torch.equal(a[3], b[3])
    else:   # the 16-tile kernels and the split pipeline add their workgroups' LOGGED loss sums with float atomics, in any order
        torch.testing.assert_close(a[3], b[3], rtol=1e-5, atol=0)
    _check_gradients(case, b[4], b[5], PC.spec_id(case.spec) + " poisoned")


@pytest.mark.parametrize("s", _PER_ROUTE, ids=PC.spec_id)
def test_stale_slabs_of_a_larger_launch_do_not_reach_a_smaller_one(s):
    """B = 4 096 (16 workgroups of the LDS-resident kernels, 64 of the 16-tile ones), then B = 100 on the same object: bit-equal to
    a fresh object's call at B = 100 (the reduction must stop at the slabs this call wrote)."""
    small, large = PC.build(s._replace(B=100)), PC.build(s._replace(B=4096, vet=False))
    act, cri, fused = _fused(small, max_batch=4096)
    scale = torch.zeros(1, device=DEV)
    _call(fused, *_tables(large), scale, overwrite=True)
    assert torch.isfinite(fused.flat_grad).all()
    _call(fused, *_tables(small), scale, overwrite=True)
    act2, cri2, fresh = _fused(small)
    scale2 = torch.zeros(1, device=DEV)
    _call(fresh, *_tables(small), scale2, overwrite=True)
    _equal_or_close(small, fused.flat_grad, fresh.flat_grad, fused, act, cri, "call at B = 100 after one at B = 4 096")
    assert torch.equal(scale, scale2) and torch.equal(fused.moments, fresh.moments)
    _check_gradients(small, act, cri, PC.spec_id(small.spec) + " after B=4096")


def _freezes(s):
    out = [("transfer", "critic")]
    if s.kind == "modular":
        out.append(("integrator",))
    return out


@pytest.mark.parametrize("s", _PER_ROUTE, ids=PC.spec_id)
def test_frozen_parameters(s):
    """frozen_transfer() on actor and critic, and frozen_integrator() on a modular actor: the trainable tensors' gradients are
    bit-equal to the unfrozen run's (the frozen ones go to the dump), and after pime_ppo_minibatch_step the frozen parameters are
    bit-unchanged, the trainable ones moved, and the packed images equal a re-pack."""
    case = PC.build(s._replace(B=293))
    tables, idx = _tables(case)
    act0, cri0, plain = _fused(case)
    scale = torch.zeros(1, device=DEV)
    _call(plain, tables, idx, scale, overwrite=True)
    full = dict(_named_grads(act0, cri0))
    for freeze in _freezes(s):
        act, cri, fused = _fused(case, freeze=freeze)
        frozen = {("act." if m is act else "cri.") + n: p for m in (act, cri) for n, p in m.named_parameters()
                  if not p.requires_grad and n != "priorK"}
        assert frozen and fused.flat_param.numel() < plain.flat_param.numel()
        assert "act.a_std_log" not in frozen
        before = {n: p.detach().clone() for n, p in frozen.items()}
        scale2 = torch.zeros(1, device=DEV)
        fused._dump.fill_(float("nan"))   # (a sink: nothing may read it back)
        _call(fused, tables, idx, scale2, overwrite=True)
        assert torch.equal(scale, scale2)
        for name, p in _named_grads(act, cri):
            if name.startswith("act.") and _split(s):
                continue   # float atomics: held to the oracle below
            assert torch.equal(p.grad, full[name].grad), f"{freeze}: gradient of the trainable {name} differs from the unfrozen run's"
        _check_gradients(case, act, cri, PC.spec_id(case.spec) + f" frozen {'+'.join(freeze)}")
        if _split(s):
            continue   # pime_ppo_minibatch_step refuses the split pipeline (tests/test_gpu_ppo_fused.py)
        adam = fused.make_optimizer(1e-3)
        assert fused.images_follow_step, f"the library could not derive the image map: {fused.image_map_error}"
        start = fused.flat_param.clone()
        for _ in range(2):
            _call(fused, tables, idx, scale2, overwrite=True, adam=adam)
        for name, p in frozen.items():
            assert torch.equal(p.detach(), before[name]), f"{freeze}: the frozen {name} changed in the fused optimizer step"
        assert float(adam.step_count[0]) == 2.0 and bool((fused.flat_param != start).float().mean() > 0.5)
        got = [(n["img_fwd"].clone(), n["img_bwd"].clone()) for n in fused.nets]
        fused.repack()
        torch.cuda.synchronize()
        planes = PC.b3_nets(s, PC.forced16_process()) if PC.b3_process() else (False, False)
        for (gf, gb), n, b3 in zip(got, fused.nets, planes):
            assert torch.equal(gf, n["img_fwd"]) and torch.equal(gb, n["img_bwd"]), f"{freeze}: packed images drifted from the parameters"
            assert (gb.numel() > n["n_bwd_f32"]) == b3, f"{freeze}: the compared transposed image does not hold the bf16 planes"


# ------------------------------------------------------------------------------------------------------------------------ e
_CHILD = r'''
import json, os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import ppo_cases as PC
import test_gpu_ppo_sweep as t
for s in PC.forced16_cases():
    t.run_case(PC.build(s), forced16=True)
print("PPO_SWEEP_FORCED16 " + json.dumps({"used_share_of_bar": t._USED, "routes_hit": t._ROUTES}))
'''


def test_widths_64_and_128_through_the_16_tile_family():
    """PIME_MLP16=1 is read once per process: a child runs forced16_cases (plain D 3 and 20, modular D 4, and at width 128 modular D 20: the two-tile
    first layer of ppo16m_kernel<8>; widths 64 / 128, B 37 and 65) through run_case, asserting the forced routes."""
    env = dict(os.environ, PIME_ROOT=ROOT, PIME_MLP16="1")
    env.pop("PIME_PPO_SWEEP_REPORT", None)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PPO_SWEEP_FORCED16 ")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(line[0].split(" ", 1)[1])
    for k, v in rec["used_share_of_bar"].items():
        _note(k, v)
    for k, v in rec["routes_hit"].items():
        _ROUTES[k] = _ROUTES.get(k, 0) + v
    assert set(rec["routes_hit"]) == {"16tile/16tile/single 64+64 (PIME_MLP16)", "16tile/16tile/single 128+128 (PIME_MLP16)",
                                      "lds/16tile/single 64+64 (PIME_MLP16)"}


# ------------------------------------------------------------------------------------------------------------------------ f
_B3_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import test_gpu_ppo_sweep as t
t.b3_child(sys.argv[1])
"""


def _class_label(s, forced16):
    route, aw, cw, kind, fa, fc, on = PC.b3_kernel_class(s, forced16)
    return "/".join(route) + f" {aw}+{cw} {kind} first layer {fa}/{fc} B3 " + "+".join(n for n, b in zip(("actor", "critic"), on) if b)


def _pool_stats():
    out = {}
    for (label, net), parts in _POOL.items():
        d = np.concatenate(parts).astype(np.float64)
        out[f"{label} | {net}"] = {"n": int(d.size), "p99": float(np.quantile(d, 0.99)), "rms": float(np.sqrt((d * d).mean())),
                                   "max": float(d.max()), "far": float((d > 2e-6).mean())}
    return out


def b3_child(name):
    """What a child of part f runs (both switches are read once per process, and the parent set them): a list of
    ppo_cases.B3_LISTS through run_case -- under the variant, or with the variable unset for the f32 path's pools --, the three
    properties of d. over the variant's per-route shapes, or the shape the variant does not serve."""
    forced16, grids = PC.forced16_process(), {}
    if name == "boundary":
        _b3_boundary()
    elif name == "properties":
        assert PC.b3_process() and not forced16
        for s in PC.b3_per_route_shapes():
            for prop in (test_nothing_unwritten_or_unnamed_is_read, test_stale_slabs_of_a_larger_launch_do_not_reach_a_smaller_one,
                         test_frozen_parameters):
                prop(s)
    else:
        want16, cases = PC.B3_LISTS[name]
        assert want16 == forced16
        for s in cases():
            if s.B == PC.CAP_B:   # grid x 64 + 1, from the grid of THIS process's kernels
                label = PC.spec_id(s)
                s, g = PC.resolve_cap(s, forced16)
                grids[label] = dict(g, B=s.B)
            _POOL_CLASS[0] = (_class_label(s, forced16), PC.b3_nets(s, forced16))
            run_case(PC.build(s), forced16)
        _POOL_CLASS[0] = None
        if forced16 and PC.b3_process():   # the properties on ppo16_kernel<8, ., true> below 14 floats and ppo16m_kernel<8, true>
            for s in PC.b3_per_route_shapes(True):
                for prop in (test_nothing_unwritten_or_unnamed_is_read, test_stale_slabs_of_a_larger_launch_do_not_reach_a_smaller_one,
                             test_frozen_parameters):
                    prop(s)
    print("PPO_SWEEP_B3 " + json.dumps({"used_share_of_bar": _USED, "routes_hit": _ROUTES, "pools": _pool_stats(), "grids": grids}))


def _b3_run(name, variant=True, forced16=False, timeout=300):
    """One child, given only the switches it needs.  A child that dies on a signal or runs into its time limit fails the test there
    (TimeoutExpired, or the assertion below): the test's remaining children are not started."""
    env = {k: v for k, v in os.environ.items() if k not in ("PIME_MLP16", "PIME_GRAD_BF16X3", "PIME_PPO_SWEEP_REPORT")}
    env["PIME_ROOT"] = ROOT
    if variant:
        env["PIME_GRAD_BF16X3"] = "1"
    if forced16:
        env["PIME_MLP16"] = "1"
    r = subprocess.run([sys.executable, "-c", _B3_CHILD, name], env=env, capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PPO_SWEEP_B3 ")]
    assert r.returncode == 0 and line, f"child {name} (variant: {variant}) exited with {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-4000:]
    return json.loads(line[0].split(" ", 1)[1])


def _merge(rec):
    for k, v in rec["used_share_of_bar"].items():
        _note(k, v)
        _B3["used_share_of_bar"][k] = max(_B3["used_share_of_bar"].get(k, 0.0), float(v))
    for k, v in rec["routes_hit"].items():
        _ROUTES[k] = _ROUTES.get(k, 0) + v
        _B3["routes_hit"][k] = _B3["routes_hit"].get(k, 0) + v
    _B3["grids"].update(rec["grids"])


def _b3_list(name, routes, forced16=False):
    """The list under the variant (every bar of run_case), then with the variable unset: the f32 path's pools, class by class."""
    rec = _b3_run(name, True, forced16)
    _merge(rec)
    tag = (" (PIME_MLP16)" if forced16 else "") + " (PIME_GRAD_BF16X3)"
    assert set(rec["routes_hit"]) == {r + tag for r in routes}
    assert rec["pools"], "no B3 net in the list"
    ref = _b3_run(name, False, forced16)
    assert set(ref["pools"]) == set(rec["pools"])
    failed = []
    for key, b in sorted(rec["pools"].items()):
        a = ref["pools"][key]
        _B3["pools"][f"{name}: {key}"] = {"f32": a, "bf16x3": b}
        row = (f"{name}: {key}: f32 p99 {a['p99']:.2e} rms {a['rms']:.2e} max {a['max']:.2e} beyond 2e-6 {a['far']:.5f} | bf16x3 p99 "
               f"{b['p99']:.2e} rms {b['rms']:.2e} max {b['max']:.2e} beyond 2e-6 {b['far']:.5f} ({b['n']} elements)")
        print("ppo sweep b3 pool " + row)
        if not b["p99"] <= max(2.0 * a["p99"], 5e-7):
            failed.append(row)
    assert not failed, "the variant's 99th percentile exceeds max(2 x the f32 path's, 5e-7):\n" + "\n".join(failed)
    return rec


def test_b3_shapes_at_width_256():
    """ppo16_kernel<16, actor | critic, true> on D 1..32 (one and two first-layer column blocks), ppo16m_kernel<16, true> on every
    plant tower up to 28 floats and Di 1..3."""
    _b3_list("shapes256", {"16tile/16tile/single 256+256"})


def test_b3_shapes_at_width_128():
    """ppo16_kernel<8, actor | critic, true> on D 14..32; the split-pipeline actor (f32, atomics) next to ppo16_kernel<8, critic, true>."""
    _b3_list("shapes128", {"16tile/16tile/single 128+128", "split/16tile/single 128+128"})


def test_b3_classes_in_every_batch_regime():
    rec = _b3_list("regimes", {"16tile/16tile/single 256+256", "16tile/16tile/single 128+128", "split/16tile/single 128+128"})
    assert len(rec["grids"]) == 3 and all(g["B"] > 64 * max(v for k, v in g.items() if k != "B") for g in rec["grids"].values())


def test_b3_nets_of_different_widths():
    """ppo16_kernel<16, actor, true> next to the LDS-resident f32 critic, next to ppo16_kernel<8, critic, true>; the LDS-resident
    modular actor next to ppo16_kernel<16, critic, true>; ppo16_kernel<8, actor, true> next to the LDS-resident critic of width 64."""
    _b3_list("mixed", {"16tile/lds/single 256+128", "16tile/16tile/single 256+128", "lds/16tile/single 128+256", "16tile/lds/single 128+64"})


def test_b3_under_forced_16_tile_family():
    """Both switches: ppo16_kernel<8, ., true> below 14 floats and ppo16m_kernel<8, true> (Di 1 and 3, one and two first-layer
    tiles), B 2 .. 65 and the cap batch, and the three properties on both."""
    rec = _b3_list("forced16", {"16tile/16tile/single 128+128", "16tile/16tile/single 128+64"}, forced16=True)
    assert len(rec["grids"]) == 1


def test_b3_properties():
    """NaN in the workspaces and the unnamed rows, stale slabs of a larger launch, frozen parameters (the re-packed images compared
    include the planes) over ppo_cases.b3_per_route_shapes()."""
    rec = _b3_run("properties", True, timeout=300)
    _merge(rec)
    assert set(rec["routes_hit"]) == {r + " (PIME_GRAD_BF16X3)" for r in (
        "16tile/16tile/single 256+256", "16tile/16tile/single 128+128", "split/16tile/single 128+128", "16tile/lds/single 256+128",
        "16tile/16tile/single 256+128", "lds/16tile/single 128+256", "16tile/lds/single 128+64")}


def _b3_boundary():
    """(in the child, under the variable)"""
    import ctypes
    import warnings
    import pime_amd.native as nt
    from pime_amd import backend, ops
    assert PC.b3_process() and not PC.forced16_process()
    for D, Di in ((30, 1), (32, 3)):
        s = PC.b3_spec("modular", D, Di, 256, 37, vet=False)
        assert s.route == ("none", "16tile", "single") == PC.library_route(s.kind, s.D, s.Di, s.aw, s.cw)
        r = (ctypes.c_int32 * 3)()
        assert nt.lib().pime_ppo_route(nt.MLP_MODULAR_ACTOR, D, Di, 256, 256, r) != 0
        assert "LDS map does not fit" in nt.last_error() and "actor" in nt.last_error()
        case = PC.build(s)
        act, cri = _modules(case)
        assert ops.FusedPPOGrad.supported(act, cri) is False
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            assert backend.HipBackend().fused_ppo(act, cri, 37) is False
        text = " ".join(str(w.message) for w in seen)
        assert "no fused PPO gradient kernel" in text and "runs through torch autograd" in text and "LDS map does not fit" in text, text
        # the object built all the same: the call refuses, and writes no gradient
        act, cri, fused = _fused(case)
        tables, idx = _tables(case)
        fused.flat_grad_dp.fill_(-7.25)
        fused._dump.fill_(-7.25)
        with pytest.raises(nt.PimeError, match="LDS"):
            _call(fused, tables, idx, torch.zeros(1, device=DEV), overwrite=True)
        torch.cuda.synchronize()
        assert bool((fused.flat_grad_dp == -7.25).all()) and bool((fused._dump == -7.25).all()), "a refused call wrote gradients"
        with pytest.raises(nt.PimeError, match="LDS"):
            _call(fused, tables, idx, torch.zeros(1, device=DEV))
        torch.cuda.synchronize()
        assert bool((fused.flat_grad_dp == -7.25).all())
    s = PC.b3_spec("modular", 31, 3, 256, 37)
    act, cri = _modules(PC.build(s))
    assert ops.FusedPPOGrad.supported(act, cri) is True
    run_case(PC.build(s))


def test_b3_does_not_serve_a_wide_plant_tower_at_width_256():
    """Modular actor, width 256, (D, Di) = (30, 1) and (32, 3) -- plant towers of 29 floats: pime_ppo_route refuses and names the
    LDS map; FusedPPOGrad.supported and HipBackend.fused_ppo answer what the library answers (False, with the "no fused PPO gradient
    kernel ... runs through torch autograd" warning up front); an object constructed all the same raises PimeError on the call and
    writes no element of the gradient buffer.  (31, 3), a tower of 28 floats, is served in the same process and passes run_case."""
    rec = _b3_run("boundary", True, timeout=240)
    _merge(rec)
    assert set(rec["routes_hit"]) == {"16tile/16tile/single 256+256 (PIME_GRAD_BF16X3)"}
