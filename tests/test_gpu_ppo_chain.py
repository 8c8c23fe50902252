"""The fused PPO update as a chain: every optimizer step of a K-step chain recorded and held to tests/ppo_chain.py's checker
(whose own conditions tests/test_ppo_chain_cpu.py asserts on numpy alone), and the production host path -- AgentPPO.update_net
in every launch form -- held bit for bit to a step-by-step loop whose every step has been checked.

  a. Per spec of ppo_chain.chain_specs() (every route, B = 293, K = 4 rows walked with the device-side cursor, lr 1e-3, NaN in the
     workspaces before step 0 only): the fused step (pime_ppo_minibatch_step) through check_chain -- gradient against the oracle
     at step 0, against a FRESH object's gradient at the chain's own pre-step weights at every step (bit-equal on the
     deterministic routes), Adam against the float64 replay of the step's own gradient, counters, scale, loss sums, images -- and
     the two other step forms of the host path (gradient then pime_adam_step_images; gradient, pime_adam_step, re-pack) bit-equal
     to it at every step.  The split pipeline, which pime_ppo_minibatch_step refuses, runs the last form only.
  b. The data-parallel step form at world 1 without a communicator (defer_critic_scale, then pime_adam_step_dp): the actor's part
     of the state bit-equal to a., the critic's within ppo_chain.dp_replay_bounds of the replay of (unscaled gradient x the scale
     recomputed in float64 from dp_moments).
  c. update_net on a 10 x 48 trajectory buffer, batch 96 (5 steps per update), three consecutive updates (Adam steps 1..15), for
     one agent per kernel family: a twin agent runs the pre-pass through the same methods (each held to float64) and the manual
     loop of a. with recorder and check_chain; the agent under test must end every update with parameters, moments, counter and
     packed images equal to the twin's (loss sums: see below), in each launch form (index table: eager / probe / capture / per-step graph,
     then the whole-update graph; index hook: two graphs; launch timer: separate Adam; no graphs; no whole-update graph), and
     when the third update reads a second buffer with the same contents (other data pointers: new graphs, the same end state).
  e. Parts a. and b. under the bf16x3 variant (PIME_GRAD_BF16X3=1, alone and with PIME_MLP16=1; child processes) over
     ppo_chain.b3_chain_specs(): every step form re-splits the bf16 planes behind the transposed image (refresh_b3 of csrc/abi.hip:
     the fused step, pime_adam_step_images, pime_adam_step_dp) or re-packs them; a form that left them stale would take the
     streamed layers at the previous weights and the first layer at the new ones, which the gradient of a fresh object at the
     chain's own pre-step weights -- bit-equal on every B3 net -- shows at the step after.
  d. PIME_PPO_CHAIN_REPORT=<path> writes the largest used share of every bound as JSON (a record -- profiles/ppo_chain_gpu.txt --,
     not a threshold).

Bit-equality is asked only where the library documents determinism: gradients of the split pipeline are float atomics, and
every gradient kernel adds its workgroups' LOGGED loss sums with float atomics (csrc/ppo_fused.hip, csrc/mlp16.hip,
csrc/ppo_train.hip; "reproducible to rounding, not bitwise", tests/test_gpu_update_golden.py) -- from the second step on the
accumulator is not 0 and the order of two workgroups shows in the last bit -- so loss sums are compared at rtol 1e-5, the sweep's
bar between two runs, and the objectives update_net returns (differences of two such sums) at 1e-5 of the sums they are formed
from.  Against float64 the loss sums are held per step by check_chain."""
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import ppo_cases as PC
import ppo_chain as CH
import ppo_oracle as P
import test_gpu_ppo_sweep as SW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_USED = {}
_BIT_EQUAL = {}
SPECS = CH.chain_specs()
DET_SPECS = [s for s in SPECS if CH.deterministic(s)]
SPLIT_SPECS = [s for s in SPECS if not CH.deterministic(s)]
FORMS = ("fused", "step_images", "step_repack")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("PIME_PPO_CHAIN_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump({"used_share_of_bound": _USED, "bit_equal": _BIT_EQUAL}, fh, indent=1, sort_keys=True)


def _note(used, where):
    for k, v in used.items():
        print(f"ppo chain {where} {k}: {v:.3f}")
        _USED[k] = max(_USED.get(k, 0.0), float(v))


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- recorder
def _state(fused, opt, row):
    return dict(param=_np(fused.flat_param), exp_avg=_np(opt.exp_avg), exp_avg_sq=_np(opt.exp_avg_sq),
                step_count=float(opt.step_count[0]), arrival=int(opt.step_count.view(torch.int32)[1]),
                loss_sums=_np(fused.loss_sums), cursor=int(row))


def _images(fused):
    return [(_np(n["img_fwd"]), _np(n["img_bwd"])) for n in fused.nets]


def _assert_planes(s, *objects):
    """Under the bf16x3 variant the transposed images that the recorder compares hold the bf16 planes of the B3 nets."""
    want = PC.b3_nets(s, PC.forced16_process()) if PC.b3_process() else (False, False)
    for fused in objects:
        assert tuple(n["img_bwd"].numel() > n["n_bwd_f32"] for n in fused.nets) == want, f"{PC.spec_id(s)}: bf16 planes"


def _load_flat(act, cri, flat):
    """Writes a flat parameter vector into the trainable parameters of (act, cri), in the flat order."""
    o = 0
    with torch.no_grad():
        for p in list(act.parameters()) + list(cri.parameters()):
            if p.requires_grad:
                p.copy_(flat[o:o + p.numel()].view_as(p))
                o += p.numel()
    assert o == flat.numel()


def _layout_of(case, act, cri):
    lay = CH.shaped_layout(case.spec, case.nets)
    names = [("act", n, tuple(p.shape)) for n, p in act.named_parameters() if p.requires_grad] + \
            [("cri", n, tuple(p.shape)) for n, p in cri.named_parameters() if p.requires_grad]
    assert names == lay, "the flat parameter order is not the helper's layout"
    return lay


class Chain:
    """One (fused object, optimizer) with a twin for re-packs and a third pair of modules for the fresh objects' gradients."""

    def __init__(self, case, fused, opt, hyper, batch):
        from pime_amd import ops
        self.case, self.fused, self.opt, self.hyper, self.batch = case, fused, opt, hyper, batch
        self.lay = _layout_of(case, fused.act, fused.cri)
        assert fused.critic_offset == CH.n_actor(self.lay)
        self.twin = ops.FusedPPOGrad(*SW._modules(case), batch)
        if case.table is not None:
            _assert_planes(case.spec, fused, self.twin)
        self.fresh_modules = SW._modules(case)
        imap = fused.image_map()
        self.image_map = None if imap is None else _np(imap).reshape(-1, 2).astype(np.int64)
        self.scale = torch.zeros(1, device=DEV)
        self.row = torch.zeros(1, dtype=torch.int64, device=DEV)

    def run(self, tables, tab, form, first_k=0, fresh=True, fresh_from=None):
        """Walks the rows of `tab` ([rows, B] on the device) from the cursor's 0; returns the recorded steps."""
        from pime_amd import ops
        fused, opt, h = self.fused, self.opt, self.hyper
        state, action, logprob, adv, r_sum = tables
        self.row.zero_()
        steps = []
        for j in range(tab.shape[0]):
            before = _state(fused, opt, self.row)
            kw = dict(overwrite=True, index_row=self.row)
            if form == "fused":
                fused(state, action, logprob, adv, r_sum, tab, h["clip"], h["lam"], self.scale, adam=opt, **kw)
            else:
                fused(state, action, logprob, adv, r_sum, tab, h["clip"], h["lam"], self.scale, **kw)
                if form == "step_images":
                    assert fused.images_follow_step, fused.image_map_error
                    opt.step(images=fused)
                else:
                    opt.step()
                    fused.repack()
            torch.cuda.synchronize()
            st = dict(k=first_k + j, row=j, before=before, after=_state(fused, opt, self.row), grad=_np(fused.flat_grad),
                      scale=float(self.scale), images=_images(fused))
            self.twin.flat_param.copy_(fused.flat_param.detach())
            self.twin.repack()
            st["repack"] = _images(self.twin)
            if fresh_from is not None:
                st["fresh_grad"] = fresh_from[j]["fresh_grad"]
            elif fresh:   # a fresh object at the chain's own pre-step weights, re-packed from scratch, the row as a plain index tensor
                _load_flat(*self.fresh_modules, torch.from_numpy(before["param"]).to(DEV))
                f2 = ops.FusedPPOGrad(*self.fresh_modules, self.batch)
                f2(state, action, logprob, adv, r_sum, tab[j].contiguous(), h["clip"], h["lam"], torch.zeros(1, device=DEV),
                   overwrite=True)
                torch.cuda.synchronize()
                st["fresh_grad"] = _np(f2.flat_grad)
            steps.append(st)
        return steps

    def recording(self, steps):
        return {"layout": self.lay, "n_act": self.fused.critic_offset, "deterministic": CH.deterministic(self.case.spec),
                "image_map": self.image_map, "steps": steps}


@functools.lru_cache(maxsize=None)
def _fused_chain(s):
    """The chain of fused steps of a deterministic-route spec: parts a. and b. compare with it."""
    return _spec_chain(s, FORMS[0])


def _spec_chain(s, form):
    """The K-step chain of part a. in one step form, on a new object: (recording, case, table)."""
    from pime_amd import ops
    case = PC.build(s)
    table = CH.index_table(case)
    SW._assert_route(s)
    act, cri = SW._modules(case)
    fused = ops.FusedPPOGrad(act, cri, s.B)
    opt = fused.make_optimizer(CH.HYPER["lr"])
    assert (opt.betas, opt.eps) == (CH.HYPER["betas"], CH.HYPER["eps"])
    ch = Chain(case, fused, opt, CH.HYPER, s.B)
    for net in fused.nets:
        net["ws"].fill_(float("nan"))   # before step 0 only: later steps cope with their own leftovers
    tables, _ = SW._tables(case)
    base = None if form == FORMS[0] or not CH.deterministic(s) else _fused_chain(s)[0]["steps"]
    steps = ch.run(tables, torch.from_numpy(table).to(DEV), form, fresh_from=base)
    return ch.recording(steps), case, table


def _steps_equal(a, b, what):
    for sa, sb in zip(a, b):
        for side in ("before", "after"):
            key = CH.states_equal(sa[side], sb[side])
            assert key is None, f"{what}: step {sa['k']}: {key} {side} the step differs"
        assert np.array_equal(sa["grad"], sb["grad"]) and sa["scale"] == sb["scale"], f"{what}: step {sa['k']}: gradient / scale"
        for (af, ab), (bf, bb) in zip(sa["images"], sb["images"]):
            assert np.array_equal(af, bf) and np.array_equal(ab, bb), f"{what}: step {sa['k']}: packed images"
        np.testing.assert_allclose(sa["after"]["loss_sums"], sb["after"]["loss_sums"], rtol=1e-5, atol=0, err_msg=what)


# ----------------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("s", DET_SPECS, ids=PC.spec_id)
def test_chain_of_fused_steps(s):
    rec, case, table = _fused_chain(s)
    assert rec["image_map"] is not None and (rec["image_map"] < 0).all(axis=1).sum() >= 1   # a_std_log sits in no image
    _note(CH.check_chain(rec, case, table), PC.spec_id(s) + " fused")
    _BIT_EQUAL[PC.spec_id(s) + " gradient: chain == fresh object, 4 steps"] = True


@pytest.mark.parametrize("form", FORMS[1:])
@pytest.mark.parametrize("s", DET_SPECS, ids=PC.spec_id)
def test_chain_in_the_other_step_forms(s, form):
    """Gradient then pime_adam_step_images; gradient, pime_adam_step, re-pack: through check_chain, and bit-equal to the fused
    step at every step (tests/test_gpu_ppo_fused.py asks that of four shapes after the last step)."""
    base = _fused_chain(s)[0]
    rec, case, table = _spec_chain(s, form)
    _note(CH.check_chain(rec, case, table), PC.spec_id(s) + " " + form)
    _steps_equal(base["steps"], rec["steps"], f"{PC.spec_id(s)} {form} against the fused step")
    _BIT_EQUAL[PC.spec_id(s) + f" {form} == fused step, every step"] = True


@pytest.mark.parametrize("s", SPLIT_SPECS, ids=PC.spec_id)
def test_chain_on_the_split_pipeline(s):
    from pime_amd import native, ops
    case = PC.build(s)
    act, cri = SW._modules(case)
    fused = ops.FusedPPOGrad(act, cri, s.B)
    tables, idx = SW._tables(case)
    with pytest.raises(native.PimeError, match="split pipeline"):
        fused(*tables, idx, PC.RATIO_CLIP, PC.LAMBDA_ENTROPY, torch.zeros(1, device=DEV), overwrite=True,
              adam=fused.make_optimizer(1e-3))
    rec, case, table = _spec_chain(s, "step_repack")
    _note(CH.check_chain(rec, case, table), PC.spec_id(s) + " step_repack")


# ----------------------------------------------------------------------------------------------------------------------- b
def _dp_scale(mom):
    """1 / (unbiased std + 1e-5) in float64 from the float32 words (sum r, sum r^2, B) at world 1."""
    m1, m2, n = (float(x) for x in mom[:3])
    var = max((m2 - m1 * m1 / n) / (n - 1.0), 0.0)
    return 1.0 / (np.sqrt(var) + 1e-5)


@pytest.mark.parametrize("s", DET_SPECS, ids=PC.spec_id)
def test_data_parallel_step_form_at_world_1(s):
    from pime_amd import ops
    base, case, table = _fused_chain(s)
    act, cri = SW._modules(case)
    fused = ops.FusedPPOGrad(act, cri, s.B)
    opt = fused.make_optimizer(CH.HYPER["lr"])
    twin = ops.FusedPPOGrad(*SW._modules(case), s.B)
    _assert_planes(s, fused, twin)
    n_act, h = fused.critic_offset, CH.HYPER
    tables, _ = SW._tables(case)
    tab = torch.from_numpy(table).to(DEV)
    row, scale = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, device=DEV)
    assert fused.images_follow_step
    for k, want in enumerate(base["steps"]):
        before = _state(fused, opt, row)
        fused(*tables, tab, h["clip"], h["lam"], scale, overwrite=True, index_row=row, defer_critic_scale=True)
        torch.cuda.synchronize()
        unscaled, mom = _np(fused.flat_grad), _np(fused.dp_moments)
        opt.step(images=fused, dp=(fused, 1))
        torch.cuda.synchronize()
        after = _state(fused, opt, row)
        what = f"{PC.spec_id(s)} step {k}"
        # the actor: bit-equal to the fused step's chain
        assert np.array_equal(unscaled[:n_act], want["grad"][:n_act]), f"{what}: actor gradient"
        for key in ("param", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(after[key][:n_act], want["after"][key][:n_act]), f"{what}: actor's {key}"
        assert (after["step_count"], after["arrival"], after["cursor"]) == (k + 1, 0, k + 1), what
        # the target moments and the critic
        r = case.table[4][table[k]].astype(np.float64)
        np.testing.assert_allclose(mom[:3], [r.sum(), (r * r).sum(), s.B], rtol=2.0 ** -23, err_msg=what)
        sc = _dp_scale(mom)
        g = np.concatenate([unscaled[:n_act].astype(np.float64), unscaled[n_act:].astype(np.float64) * sc])
        err = np.abs(_np(fused.flat_grad)[n_act:] - g[n_act:])
        assert (err <= 2.0 ** -22 * np.abs(g[n_act:])).all(), f"{what}: the gradient written back is not unscaled x scale"
        used = CH.adam_shares(before, after, g, k + 1, h, bounds=CH.dp_replay_bounds, sel=slice(n_act, None))
        _note({f"dp adam {key} (dp_replay_bounds)": v for key, v in used.items()}, what)
        assert max(used.values()) <= 1.0, f"{what}: critic off the replay of unscaled gradient x float64 scale: {used}"
        twin.flat_param.copy_(fused.flat_param.detach())
        twin.repack()
        for (gf, gb), (wf, wb) in zip(_images(fused), _images(twin)):
            assert np.array_equal(gf, wf) and np.array_equal(gb, wb), f"{what}: packed images"
    _BIT_EQUAL[PC.spec_id(s) + " dp form, actor == fused step, every step"] = True


@pytest.mark.parametrize("s", SPLIT_SPECS, ids=PC.spec_id)
def test_defer_critic_scale_next_to_a_split_actor(s):
    """The critic of a split-pipeline actor takes the 16-tile family: defer_critic_scale is served (the critic's gradient unscaled,
    the moments written), or refused with the message AgentPPO's probe expects -- nothing in between."""
    from pime_amd import native, ops
    case = PC.build(s)
    fused = ops.FusedPPOGrad(*SW._modules(case), s.B)
    plain = ops.FusedPPOGrad(*SW._modules(case), s.B)
    tables, idx = SW._tables(case)
    scale = torch.zeros(1, device=DEV)
    SW._call(plain, tables, idx, scale, overwrite=True)
    try:
        SW._call(fused, tables, idx, torch.zeros(1, device=DEV), overwrite=True, defer_critic_scale=True)
    except native.PimeError as exc:
        assert "dp_moments needs the critic on a slab kernel" in str(exc)
        return
    n_act = fused.critic_offset
    r = case.table[4][case.idx].astype(np.float64)
    np.testing.assert_allclose(_np(fused.dp_moments)[:3], [r.sum(), (r * r).sum(), s.B], rtol=2.0 ** -23)
    want = _np(fused.flat_grad)[n_act:].astype(np.float64) * float(scale)
    np.testing.assert_allclose(_np(plain.flat_grad)[n_act:], want, rtol=2.0 ** -22, atol=0)


# ----------------------------------------------------------------------------------------------------------------------- e
_B3_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import test_gpu_ppo_chain as t
t.b3_child()
"""


def b3_child():
    """What a child of part e runs: parts a. and b. as they are, over the variant's specs of THIS process."""
    assert PC.b3_process()
    ran = []
    for s in CH.b3_chain_specs(PC.forced16_process()):
        if CH.deterministic(s):
            test_chain_of_fused_steps(s)
            for form in FORMS[1:]:
                test_chain_in_the_other_step_forms(s, form)
            test_data_parallel_step_form_at_world_1(s)
        else:   # the split-pipeline actor (f32, atomics) next to a B3 critic, whose part stays bit-equal (check_chain)
            test_chain_on_the_split_pipeline(s)
            test_defer_critic_scale_next_to_a_split_actor(s)
        ran.append(PC.spec_id(s))
    print("PPO_CHAIN_B3 " + json.dumps({"used": _USED, "bit_equal": _BIT_EQUAL, "ran": ran, "routes": SW._ROUTES}))


def test_chain_under_the_bf16x3_variant():
    """Two children, one after the other: PIME_GRAD_BF16X3=1 alone (ppo16_kernel<16 | 8, ., true> and ppo16m_kernel<16, true> alone,
    next to each other at different widths, next to the LDS-resident kernels and next to the split pipeline), then with
    PIME_MLP16=1 (ppo16_kernel<8, ., true> on 3 floats, ppo16m_kernel<8, true> next to a B3 critic and next to an f32 one).  A child that dies on a signal or runs into its
    time limit fails the test there; the second is not started."""
    for forced16 in (False, True):
        env = {k: v for k, v in os.environ.items() if k not in ("PIME_MLP16", "PIME_GRAD_BF16X3", "PIME_PPO_CHAIN_REPORT",
                                                                 "PIME_PPO_SWEEP_REPORT")}
        env.update(PIME_ROOT=SW.ROOT, PIME_GRAD_BF16X3="1")
        if forced16:
            env["PIME_MLP16"] = "1"
        r = subprocess.run([sys.executable, "-c", _B3_CHILD], env=env, capture_output=True, text=True, timeout=300)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("PPO_CHAIN_B3 ")]
        assert r.returncode == 0 and line, f"child (PIME_MLP16: {forced16}) exited with {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-4000:]
        rec = json.loads(line[0].split(" ", 1)[1])
        tag = " (PIME_MLP16)" * forced16 + " (PIME_GRAD_BF16X3)"
        for k, v in rec["used"].items():
            _USED[k] = max(_USED.get(k, 0.0), float(v))
        for k in rec["bit_equal"]:
            _BIT_EQUAL[k + tag] = True
        assert rec["ran"] == [PC.spec_id(s) for s in CH.b3_chain_specs(forced16)]
        want = {"/".join(s.route) + f" {s.aw}+{s.cw}" + tag for s in CH.b3_chain_specs(forced16)}
        assert set(rec["routes"]) == want and len(want) == (7 if not forced16 else 2)


# ----------------------------------------------------------------------------------------------------------------------- c
T_, N_, BATCH, N_STEPS, N_UPDATES = 10, 48, 96, 5, 3
AGENTS = {   # one per family the agents can reach: (class, width, D, Di)
    "ppo-64-D4": ("AgentPPO", 64, 4, 0),
    "residual-128-D5": ("AgentResidualPPO", 128, 5, 0),
    "residual-256-D30": ("AgentResidualPPO", 256, 30, 0),
    "residual-128-D14": ("AgentResidualPPO", 128, 14, 0),
    "modular-128-D3": ("AgentResidualIntegratorModularPPO", 128, 3, 1),
    "modular-64-D4": ("AgentResidualIntegratorModularPPO", 64, 4, 1),
    "modular-256-D4": ("AgentResidualIntegratorModularPPO", 256, 4, 1),
}
SPLIT_AGENT = ("AgentResidualIntegratorModularPPO", 128, 14, 1)
HOST_FORMS = ("index_table", "index_hook", "launch_timer", "no_graphs", "no_update_graph")


def _agent_spec(cfg):
    name, w, D, Di = cfg
    kind = "modular" if Di else "ppo" if name == "AgentPPO" else "plain"
    return PC.spec(kind, D, Di, w, BATCH, vet=False)


def _make_agent(cfg):
    from pime_amd.elegantrl import agent, agent_residual
    name, w, D, Di = cfg
    s = _agent_spec(cfg)
    ag = (agent.AgentPPO if name == "AgentPPO" else getattr(agent_residual, name))(device=DEV)
    if Di:
        ag.init(w, D, 1, Di)
    else:
        ag.init(w, D, 1)
    if name != "AgentPPO":
        ag.init_residual({"init_K": np.full((D, 1), 0.01)})
        ag.fix_K()
    nets = PC.make_nets(PC.okind(s.kind), D, Di, w, w, 20261)
    for net, sd in zip((ag.act, ag.cri), nets):
        missing, unexpected = net.load_state_dict({k: torch.from_numpy(v.copy()).to(DEV) for k, v in sd.items()}, strict=False)
        assert not unexpected and set(missing) <= {"priorK"}
    ag.weights_changed()
    return ag, s, nets


def _buffer(ag, D):
    """states uniform in [-1.5, 1.5], masks 0.99 with zeros on the last row and on five other cells, rewards N(-2, 3), noise
    N(0, 1), action = mean + sigma x noise with the agent's own modules."""
    from pime_amd.elegantrl.replay import TrajectoryBuffer
    rng = np.random.RandomState([D, 8, 15])
    buf = TrajectoryBuffer(T_, N_, D, 1, DEV)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(DEV)   # noqa: E731
    buf.state[:] = f(rng.uniform(-1.5, 1.5, (T_ + 1, N_, D)))
    mask = np.full((T_, N_), 0.99)
    mask[-1] = 0
    for t, n in ((1, 3), (2, 40), (4, 17), (6, 0), (8, 47)):
        mask[t, n] = 0
    buf.mask[:] = f(mask)
    buf.reward[:] = f(rng.normal(-2, 3, (T_, N_)))
    buf.noise[:] = f(rng.standard_normal((T_, N_, 1)))
    with torch.no_grad():
        mean = ag.act.mean(buf.state[:T_].reshape(-1, D))
        buf.action[:] = (mean + buf.noise.reshape(-1, 1) * ag.act.a_std_log.exp()).reshape(T_, N_, 1)
    buf.length = T_
    return buf


def _index_table(D):
    return torch.from_numpy(np.random.RandomState([D, 96]).randint(0, T_ * N_, (N_UPDATES * N_STEPS, BATCH)).astype(np.int64))


def _objectives(tot, lst, lam):
    """(obj_a, obj_c) of AgentPPO._update_fused from the loss sums at the end of the update and in front of its last step, and
    what 1e-5 of each of those sums comes to in them."""
    tot, lst, B = [float(x) for x in tot], [float(x) for x in lst], float(BATCH)
    obj = (tot[0] - lst[0]) / B + lam * (tot[1] - lst[1]) / B, (tot[2] - lst[2]) / B
    atol = (1e-5 * (abs(tot[0]) + abs(lst[0]) + lam * (abs(tot[1]) + abs(lst[1]))) / B, 1e-5 * (abs(tot[2]) + abs(lst[2])) / B)
    return obj, atol


def _end_state(ag):
    fused, opt = ag._packed["fused"], ag.optimizer
    return dict(flat_param=fused.flat_param.detach().clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(),
                step_count=opt.step_count.clone(), loss_sums=fused.loss_sums.clone(),
                images=[(n["img_fwd"].clone(), n["img_bwd"].clone()) for n in fused.nets])


def _prepass(ag, buf):
    """The pre-pass of update_net through the agent's own methods, and everything the checks need of it."""
    T, N, rew, mask, action, noise, state = ag._trajectory_views(buf)
    with torch.no_grad():
        value = ag.state_value(state)
        logprob = ag.act.old_logprob(noise)
        r_sum, adv = ag.compute_reward(T * N, rew, mask, value, shape=(T, N))
        raw = ag.backend.gae(rew.reshape(T, N), mask.reshape(T, N), value.reshape(T, N), ag.lambda_gae_adv, True)
    torch.cuda.synchronize()
    return types.SimpleNamespace(T=T, N=N, rew=rew, mask=mask, action=action.reshape(-1).contiguous(), noise=noise, state=state,
                                 value=value, logprob=logprob, r_sum=r_sum, adv=adv, raw_r_sum=raw[0], raw_adv=raw[1],
                                 cri={k: _np(v).astype(np.float64) for k, v in ag.cri.state_dict().items()},
                                 a_std_log=float(ag.act.a_std_log.detach().double().reshape(-1)[0]))


def _check_prepass(pp, what):
    import oracle
    v, want = _np(pp.value), P.critic_forward(pp.cri, _np(pp.state))[0]
    bar = 3e-5 * max(1.0, float(np.abs(want).max()))
    _note({"value pass (3e-5 of max(1, largest |value|))": np.abs(v - want).max() / bar}, what)
    assert np.abs(v - want).max() <= bar, f"{what}: value pass"
    z = _np(pp.noise).astype(np.float64)[:, 0]
    np.testing.assert_allclose(_np(pp.logprob), -(z * z * 0.5 + pp.a_std_log + P.LOG_SQRT_2PI), rtol=0, atol=1e-6, err_msg=what)
    w_r, w_a = oracle.gae(_np(pp.rew).reshape(pp.T, pp.N), _np(pp.mask).reshape(pp.T, pp.N), v.reshape(pp.T, pp.N), 0.97, True)
    assert np.array_equal(_np(pp.raw_r_sum), w_r) and np.array_equal(_np(pp.raw_adv), w_a), f"{what}: GAE scan on the kernel's values"
    assert np.array_equal(_np(pp.r_sum), w_r.reshape(-1)), f"{what}: r_sum"
    a = w_a.reshape(-1).astype(np.float64)
    np.testing.assert_allclose(_np(pp.adv), (a - a.mean()) / (a.std(ddof=1) + 1e-5), rtol=2e-5, atol=2e-5, err_msg=what)


@functools.lru_cache(maxsize=None)
def _twin(cfg, form="fused"):
    """Three consecutive updates of a twin agent as the manual loop of part a.: per update (pre-pass, recording, case, end state,
    objectives).  Nothing is asserted here but the plumbing; test_twin_chain_of_the_host_path checks the recordings."""
    ag, s, nets = _make_agent(cfg)
    assert ag.lambda_gae_adv == 0.97
    buf = _buffer(ag, cfg[2])
    table = _index_table(cfg[2])
    fused = ag._fused_grad(BATCH)
    assert fused and ag.optimizer.param is fused.flat_param
    hyper = dict(lr=ag.learning_rate, betas=ag.optimizer.betas, eps=ag.optimizer.eps, clip=ag.ratio_clip, lam=ag.lambda_entropy)
    chain = Chain(PC.Case(s, nets, None, None, 0, 0, None, 0), fused, ag.optimizer, hyper, BATCH)
    for net in fused.nets:
        net["ws"].fill_(float("nan"))
    out = []
    for u in range(N_UPDATES):
        pp = _prepass(ag, buf)
        tables = (pp.state, pp.action, pp.logprob, pp.adv, pp.r_sum)
        fused.loss_sums.zero_()
        rows = table[u * N_STEPS:(u + 1) * N_STEPS]
        steps = chain.run(tables, rows.to(DEV), form, first_k=u * N_STEPS, fresh=CH.deterministic(s))
        ag.weights_changed()   # what update_net leaves behind: the value pass packs the new critic
        case = PC.Case(s, nets, tuple(_np(t) for t in tables), None, 0, 0, None, 0)
        obj = _objectives(steps[-1]["after"]["loss_sums"], steps[-1]["before"]["loss_sums"], ag.lambda_entropy)
        out.append(types.SimpleNamespace(prepass=pp, rec=chain.recording(steps), case=case, rows=rows.numpy(), hyper=hyper,
                                         end=_end_state(ag), obj=obj))
    return buf, table, out


@pytest.mark.parametrize("tag", list(AGENTS))
def test_twin_chain_of_the_host_path(tag):
    """The twin's pre-pass against float64 at every update, and its 15 recorded steps through check_chain (without the step-0
    oracle gradient: these tables are not vetted; every step's gradient is bit-equal to a fresh object's, which the sweep pins)."""
    _, _, updates = _twin(AGENTS[tag])
    for u, up in enumerate(updates):
        _check_prepass(up.prepass, f"{tag} update {u}")
        assert [st["k"] for st in up.rec["steps"]] == list(range(u * N_STEPS, (u + 1) * N_STEPS))
        _note(CH.check_chain(up.rec, up.case, up.rows, up.hyper, oracle_step0=False), f"{tag} update {u}")
    _BIT_EQUAL[f"{tag} twin gradient: chain == fresh object, 15 steps"] = True


def _configure(ag, form, table, counter):
    by_table = lambda n, L, B: table[counter[0] * N_STEPS:counter[0] * N_STEPS + n]   # noqa: E731
    if form == "index_hook":
        ag.index_hook = lambda step, L, B: table[counter[0] * N_STEPS + step]
        return
    ag.index_table_hook = by_table
    if form == "launch_timer":
        ag.launch_timer = lambda name, fn: fn()
    elif form == "no_graphs":
        ag.use_hip_graphs = False
    elif form == "no_update_graph":
        ag.use_update_graph = False


@pytest.mark.parametrize("form", HOST_FORMS)
@pytest.mark.parametrize("tag", list(AGENTS))
def test_update_net_equals_the_chain(tag, form):
    cfg = AGENTS[tag]
    buf, table, updates = _twin(cfg)
    ag, s, _ = _make_agent(cfg)
    counter = [0]
    _configure(ag, form, table, counter)
    for u, want in enumerate(updates):
        counter[0] = u
        obj = ag.update_net(buf, T_ * N_, BATCH, 1)
        torch.cuda.synchronize()
        got, what = _end_state(ag), f"{tag} {form} update {u}"
        st = ag._packed["fused"].static
        if form == "index_table":
            assert st.graph_full is not None and (u == 0 or st.graph_update is not None), f"{what}: graphs"
        elif form == "index_hook":
            assert st.graph_a is not None and st.graph_full is None
        elif form == "no_graphs":
            assert st.graph_a is None and st.graph_full is None and st.graph_update is None
        elif form == "no_update_graph":
            assert st.graph_full is not None and st.graph_update is None
        else:
            assert st.graph_full is None and st.graph_update is None
        for key in ("flat_param", "exp_avg", "exp_avg_sq", "step_count"):
            assert torch.equal(got[key], want.end[key]), f"{what}: {key} differs from the step-by-step chain's"
        for (gf, gb), (wf, wb) in zip(got["images"], want.end["images"]):
            assert torch.equal(gf, wf) and torch.equal(gb, wb), f"{what}: packed images"
        # float atomics over the workgroups' logged sums; an objective is the difference of two of them
        torch.testing.assert_close(got["loss_sums"], want.end["loss_sums"], rtol=1e-5, atol=0)
        (want_a, want_c), (atol_a, atol_c) = want.obj
        assert abs(obj[0] - want_a) <= atol_a and abs(obj[1] - want_c) <= atol_c, f"{what}: (obj_a, obj_c) {obj} against {want.obj}"
    _BIT_EQUAL[f"{tag} update_net[{form}] == chain, 3 updates"] = True


def _copy_of(buf):
    """A second TrajectoryBuffer with `buf`'s contents: the same update at other data pointers."""
    from pime_amd.elegantrl.replay import TrajectoryBuffer
    out = TrajectoryBuffer(buf.horizon, buf.num_envs, buf.state_dim, buf.action_dim, DEV)
    for name in ("state", "reward", "mask", "action", "noise", "done"):
        getattr(out, name).copy_(getattr(buf, name))
    out.length = buf.length
    return out


@pytest.mark.parametrize("tag", ["ppo-64-D4", "modular-256-D4"])
def test_graphs_are_dropped_when_their_key_changes(tag):
    """Updates 0 and 1 leave the per-step graph and the whole-update graph; update 2 reads a second buffer with the same contents.
    The captured graphs hold the first buffer's data pointers, so neither may be replayed: a new per-step graph, no (or a new)
    whole-update graph, and -- with the first buffer's states and actions set to NaN meanwhile -- the end state of the twin's chain
    all the same."""
    cfg = AGENTS[tag]
    buf, table, updates = _twin(cfg)
    ag, s, _ = _make_agent(cfg)
    counter = [0]
    _configure(ag, "index_table", table, counter)
    for u in range(2):
        counter[0] = u
        ag.update_net(buf, T_ * N_, BATCH, 1)
    torch.cuda.synchronize()
    st = ag._packed["fused"].static
    old_full, old_update = st.graph_full, st.graph_update
    assert old_full is not None and old_update is not None, f"{tag}: graphs after two updates"
    other = _copy_of(buf)
    assert other.state.data_ptr() != buf.state.data_ptr() and other.action.data_ptr() != buf.action.data_ptr()
    counter[0] = 2
    # NaN where the old graphs read their states and actions: a replay of either would show in the end state (`buf` is the twin's
    # cached buffer, shared with the other tests: restored below)
    kept = buf.state.clone(), buf.action.clone()
    try:
        buf.state.fill_(float("nan")); buf.action.fill_(float("nan"))
        obj = ag.update_net(other, T_ * N_, BATCH, 1)
        torch.cuda.synchronize()
    finally:
        buf.state.copy_(kept[0]); buf.action.copy_(kept[1])
    st = ag._packed["fused"].static
    assert st.graph_full is not None and st.graph_full is not old_full, f"{tag}: the per-step graph of the first buffer survived"
    assert st.graph_update is None or st.graph_update is not old_update, f"{tag}: the whole-update graph of the first buffer survived"
    got, want, what = _end_state(ag), updates[2], f"{tag} update 2 on a second buffer"
    for key in ("flat_param", "exp_avg", "exp_avg_sq", "step_count"):
        assert torch.equal(got[key], want.end[key]), f"{what}: {key} differs from the step-by-step chain's"
    for (gf, gb), (wf, wb) in zip(got["images"], want.end["images"]):
        assert torch.equal(gf, wf) and torch.equal(gb, wb), f"{what}: packed images"
    torch.testing.assert_close(got["loss_sums"], want.end["loss_sums"], rtol=1e-5, atol=0)
    (want_a, want_c), (atol_a, atol_c) = want.obj
    assert abs(obj[0] - want_a) <= atol_a and abs(obj[1] - want_c) <= atol_c, f"{what}: (obj_a, obj_c) {obj} against {want.obj}"


def test_update_net_on_the_split_pipeline():
    """A modular actor of width 128 on 14 floats: its gradient is a sum of float atomics, so no two runs agree bit for bit and Adam
    turns an element whose gradient is rounding noise into a full step of either sign -- between two runs such an element can
    differ by one sign-flipped step each way, 2 lr + 2 lr, and nothing tighter than 4 lr can be derived for the weights.  What
    can be asserted: update_net took the separate Adam + re-pack form (pime_ppo_minibatch_step refuses), it left the packed images
    equal to a re-pack, and after the first update its weights are within 4 lr of the twin's manual loop."""
    buf, table, updates = _twin(SPLIT_AGENT, "step_repack")
    ag, s, _ = _make_agent(SPLIT_AGENT)
    assert s.route[0] == "split"
    counter = [0]
    _configure(ag, "index_table", table, counter)
    ag.update_net(buf, T_ * N_, BATCH, 1)
    torch.cuda.synchronize()
    fused = ag._packed["fused"]
    assert fused.adam_fusable is False and float(ag.optimizer.step_count[0]) == N_STEPS
    got = [(n["img_fwd"].clone(), n["img_bwd"].clone()) for n in fused.nets]
    fused.repack()
    torch.cuda.synchronize()
    for (gf, gb), n in zip(got, fused.nets):
        assert torch.equal(gf, n["img_fwd"]) and torch.equal(gb, n["img_bwd"]), "packed images differ from a re-pack"
    diff = float((fused.flat_param - updates[0].end["flat_param"]).abs().max())
    print(f"ppo chain split update_net: largest weight difference to the twin {diff:.2e} (4 lr = {4 * ag.learning_rate:.0e})")
    assert diff <= 4 * ag.learning_rate
