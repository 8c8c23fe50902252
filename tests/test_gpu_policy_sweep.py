"""The policy sweep on the GPU (pime_policy_sweep, csrc/policy_sweep.hip) against tests/policy_sweep.py.  Shapes: 81 plants on a handle
at lane offset 1000 (six 16-lane tiles per row: two quads, the second with two idle waves that must still meet the re-staging
barriers), five policy rows (rows 0 and 4 the same actor and gain, rows 1 - 3 actors of other seeds, row 2 with K halved), 23 steps in
segments of 9 (the last one ragged), tail 4.
  1. the served set is exactly the 32 classes (2 envs x 4 policy kinds x widths 64, 128 x float64 / mixed state); in each, every row
     bit-equal to pime_rollout_eval_metrics with that row's actor and gain on a twin env in the same state, rows 0 and 4 bit-equal,
     every row through the checker, summary bit-equal to summary_from_pairs(pairs);
  2. the handle's fields are bit-unchanged, two calls give equal bits, a NaN-filled workspace gives the same bits, NULL pairs /
     actions / outputs leave summary unchanged, an image_stride with NaN-filled padding gives the same bits, a tile's pairs give the
     same bits alone (P = 1, N = 16) as inside the grid, one captured replay gives equal bits;
  3. re-staging: at widths 64 and 128 more quads than resident workgroups (every workgroup walks on and changes its image), row p
     carrying image p mod 3: every row equals the pime_rollout_eval_metrics result its index says;
  4. every refusal and its message;
  5. protocols.policy_sweep / select_policy on the three WT_ROBUST_PLANTS with a shortened protocol;
  6. train.py --checkpoints 3 --select_policy writes policy_sweep.npz and actor_robust.pth on a toy run, leaves actor.pth as the run
     without the flags writes it, and is skipped on a Stacking id."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import policy_sweep as S
import prior_sweep as P
from rollout_replay import DEV, make_agent
from test_gpu_margin_sweep import FIELDS, KINDS, _cfg, _lanes, _make_env

pytestmark = pytest.mark.gpu
POLICIES = [(k, md) for k in ("td3", "plain", "modular", "sac") for md in (64, 128)]
CLASSES = [(env, k, md, sm) for env in ("ph", "wt") for k, md in POLICIES for sm in ("f64", "mixed")]


def _actor(kind, env, md, seed=0):
    """(packed actor, priorK, the float64 tanh term) of an agent with a non-trivial output layer; seed > 0: every parameter of the
    actor moved by that seed's draws.  The float64 term is the agent's own torch module in double precision on the CPU."""
    if kind in ("modular", "plain"):
        ag = make_agent("ResidualIntegratorModularPPO" if kind == "modular" else "ResidualPPO", env, md)
    else:
        torch.manual_seed(0x5EED00000007 + md)
        if kind == "sac":
            from pime_amd.elegantrl.agent_sac import AgentSAC
            ag = AgentSAC(device=DEV)
            ag.init(md, env.state_dim, 1)
            with torch.no_grad():
                ag.act.net_a_avg.weight.normal_(0, 0.08)
        else:
            from pime_amd.elegantrl.agent_residual import AgentResidualTD3
            ag = AgentResidualTD3(device=DEV)
            ag.init(md, env.state_dim, 1)
            ag.init_residual({"init_K": env.K.reshape(-1, 1)})
            with torch.no_grad():
                ag.act.net[-1].weight.normal_(0, 0.05)
                ag.act.net[-1].bias.normal_(0, 0.05)
    if seed:
        torch.manual_seed(1000 + seed)
        with torch.no_grad():
            for name, par in ag.act.named_parameters():
                if "net" in name and name.endswith("weight"):   # (the layers' weights; the prior gain stays)
                    par.add_(0.03 * torch.randn_like(par))
        ag.weights_changed()
    fused = ag.fused_eval_policy(env)
    assert fused is not None and fused[0].md == md, "the fused evaluation must serve this configuration"
    act = copy.deepcopy(ag.act).double().cpu()

    def term(obs):
        with torch.no_grad():
            x = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float64))
            if kind in ("modular", "plain"):
                return act.mean(x).tanh()[:, 0].numpy()
            if kind == "td3":
                return act.net(x).tanh()[:, 0].numpy()
            return act(x)[:, 0].numpy()
    return fused[0], np.asarray(fused[1], dtype=np.float64).reshape(-1).copy(), term


def _rows(kind, env, md):
    """The five rows: (packed actors, gains [5, D], terms) and the ops.PackedPolicies stack of them."""
    from pime_amd.ops import PackedPolicies
    made = [_actor(kind, env, md, seed) for seed in range(4)]
    made.append(made[0])
    pks, Ks, terms = [m[0] for m in made], np.stack([m[1] for m in made]), [m[2] for m in made]
    Ks[2] *= 0.5
    stack = PackedPolicies.from_packed(list(zip(pks, Ks)))
    assert len(stack) == 5 and stack.packed.shape == (5, stack.stride) and stack.K.shape == (5, env.obs_dim) and stack.stride % 4 == 0
    return pks, Ks, terms, stack


def _run(env, kind, stack, pairs=True, trace=True, **kw):
    args = dict(n_steps=S.N_STEPS, seg_len=S.SEG, setpoints=S.SETPOINTS[kind], band=S.BAND, tail=S.TAIL)
    args.update(kw)
    n_steps = args.pop("n_steps")
    out = env.policy_sweep(stack, n_steps, want_pairs=pairs, want_trace=trace, **args)
    torch.cuda.synchronize()
    if not (pairs or trace):
        return dict(summary=out.cpu().numpy())
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _metrics(kind, state_mode, pk, K, n=S.N, offset=S.OFFSET):
    """pime_rollout_eval_metrics with one actor and gain on a fresh twin env in the state the sweep's env holds: [S, 8, n]."""
    twin = _make_env(kind, state_mode, n=n, offset=offset)
    _, m, _ = twin.rollout_eval_metrics(pk, K, S.N_STEPS, setpoints=S.SETPOINTS[kind], seg_len=S.SEG, band=S.BAND, tail=S.TAIL)
    m = m.cpu().numpy()
    twin.close()
    return m


# ---- 1. every served class -------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_served_classes():
    from pime_amd import gym_control, native
    served = set()
    for kind, name in (("ph", gym_control.PH_V35), ("wt", gym_control.WT_INTEGRATOR), ("stacking", gym_control.WT_STACKING.format(4))):
        for sm in ("f64", "mixed", "mixed16"):
            env = gym_control.make_vec(name, 4, device=DEV, state_mode=sm, seed=S.SEED)
            assert native.lib().pime_policy_sweep_supported(env._h, -1, 0) == 0, "the prior alone is pime_prior_sweep"
            for pol, code in KINDS.items():
                for md in ((0,) if pol == "prior" else (64, 128, 256)):
                    if native.lib().pime_policy_sweep_supported(env._h, code, md):
                        served.add((kind, pol, md, sm))
            env.close()
    assert served == set(CLASSES) and len(CLASSES) == 32


@pytest.mark.parametrize("kind,pol,md,state_mode", CLASSES, ids=lambda v: str(v))
def test_every_served_class(kind, pol, md, state_mode, ph_table_oracle):
    env = _make_env(kind, state_mode)
    pks, Ks, terms, stack = _rows(pol, env, md)
    assert env.policy_supported(stack)
    cfg, keep = _cfg(env, kind, ph_table_oracle)
    lanes = _lanes(env, kind)
    rec = _run(env, kind, stack)
    assert rec["pairs"].shape == (3, 8, 5, S.N) and rec["actions"].shape == rec["outputs"].shape == (S.N_STEPS, 5, S.N)
    for p in range(4):
        want = _metrics(kind, state_mode, pks[p], Ks[p])
        assert S.bits_equal(rec["pairs"][:, :, p], want), f"row {p} is not bit-equal to pime_rollout_eval_metrics with its actor and gain"
    for k in ("pairs", "actions", "outputs"):
        assert S.bits_equal(rec[k][..., 0, :], rec[k][..., 4, :]), f"{k}: rows 0 and 4 are the same policy"
        assert not S.bits_equal(rec[k][..., 0, :], rec[k][..., 1, :]), f"{k}: rows 0 and 1 are different policies"
    tag = f"{kind}-{pol}{md}-{state_mode}"
    use = S.check_recording(kind, cfg, lanes, ph_table_oracle, rec, Ks, terms, tag=tag)
    P.check_summary(rec["summary"], rec["pairs"], tag=tag)
    print(f"\nPOLICY id={tag} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action {use['action']:.3g} "
          f"(gap {use['gap']:.4g})")
    env.close()


# ---- 2. structure ----------------------------------------------------------------------------------------------------------------
def _raw(env, code, md, images, stride, K, Pn, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, outputs, workspace):
    import pime_amd.native as nt
    rc = nt.lib().pime_policy_sweep(env._h, code, md, images if isinstance(images, C.c_void_p) else nt.ptr(images), C.c_int64(stride),
                                    nt.ptr(K), Pn, n_steps, seg_len, nt.ptr(sp), n_sp, band, tail, nt.ptr(pairs), nt.ptr(summary),
                                    nt.ptr(actions), nt.ptr(outputs), nt.ptr(workspace), env._stream())
    torch.cuda.synchronize()
    return rc, nt.last_error()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "sac", 64, "f64")], ids=lambda v: str(v))
def test_the_handle_is_untouched_and_the_outputs_are_independent(kind, pol, md, state_mode):
    import pime_amd.native as nt
    env, twin = _make_env(kind, state_mode), _make_env(kind, state_mode)
    _, _, _, stack = _rows(pol, env, md)
    before = _lanes(env, kind)
    counters = (env._t_all, env._was_reset, env.reset_count)
    obs0 = env.obs.clone()
    first, second = _run(env, kind, stack), _run(env, kind, stack)
    assert all(S.bits_equal(first[k], second[k]) for k in first), "two calls must be bit-identical"
    quiet = _run(env, kind, stack, pairs=False, trace=False)
    assert S.bits_equal(quiet["summary"], first["summary"]), "NULL pairs / actions / outputs must not change a bit of summary"
    ws_bytes = nt.lib().pime_policy_sweep_workspace_bytes(env._h, 5, S.N_STEPS, S.SEG)
    assert ws_bytes == 3 * 8 * 5 * S.N * 8
    sp = np.ascontiguousarray(S.SETPOINTS[kind], dtype=np.float64)
    wide = torch.full((5, stack.stride + 8), float("nan"), dtype=torch.float32, device=DEV)     # NaN-filled padding between the images
    wide[:, :stack.floats] = stack.packed[:, :stack.floats]
    for images, stride, with_pairs in ((stack.packed, stack.stride, False), (stack.packed, stack.stride, True), (wide, stack.stride + 8, True)):
        ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
        summary = torch.full((5, 3, 8, 5), float("nan"), dtype=torch.float64, device=DEV)
        pairs = torch.full((3, 8, 5, S.N), float("nan"), dtype=torch.float64, device=DEV) if with_pairs else None
        rc, msg = _raw(env, KINDS[pol], md, images, stride, stack.K, 5, S.N_STEPS, S.SEG, sp, 3, S.BAND, S.TAIL, pairs, summary, None, None, ws)
        assert rc == 0, msg
        assert S.bits_equal(summary.cpu().numpy(), first["summary"]), "a NaN-filled workspace / padding must not change a bit"
        if with_pairs:
            assert S.bits_equal(pairs.cpu().numpy(), first["pairs"])
    after = _lanes(env, kind)
    for k in before:
        assert S.bits_equal(before[k].astype(np.float64), after[k].astype(np.float64)), k
    assert (env._t_all, env._was_reset, env.reset_count) == counters and env._t_lanes is None
    assert torch.equal(env.obs, obs0)
    a = torch.full((S.N,), 0.25, dtype=torch.float64, device=DEV)
    got, want = env.step(a, auto_reset=False), twin.step(a, auto_reset=False)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "the next step equals that of an env that never ran the sweep"
    env.close(); twin.close()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "plain", 64, "f64")], ids=lambda v: str(v))
def test_a_tile_alone_gives_the_bits_it_gives_inside_the_grid(kind, pol, md, state_mode):
    from pime_amd.ops import PackedPolicies
    big, small = _make_env(kind, state_mode), _make_env(kind, state_mode, n=16, offset=S.OFFSET + 32)
    for k in FIELDS[kind]:
        if k not in ("t", "episode"):
            assert S.bits_equal(big.get_field(k)[32:48], small.get_field(k)), "the same global lanes draw the same state"
    pks, Ks, _, stack = _rows(pol, big, md)
    a = _run(big, kind, stack)
    b = _run(small, kind, PackedPolicies.from_packed([(pks[2], Ks[2])]))
    for k in ("pairs", "actions", "outputs"):
        assert S.bits_equal(a[k][..., 2:3, 32:48], b[k]), k
    big.close(); small.close()


@pytest.mark.parametrize("kind,pol,md", [("wt", "modular", 128), ("ph", "td3", 64)], ids=lambda v: str(v))
def test_captured_in_a_graph_and_replayed(kind, pol, md):
    import pime_amd.native as nt
    env = _make_env(kind, "mixed")
    _, _, _, stack = _rows(pol, env, md)
    want = _run(env, kind, stack)
    graph = torch.cuda.CUDAGraph()
    with nt.capture_guard(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = env.policy_sweep(stack, S.N_STEPS, setpoints=S.SETPOINTS[kind], seg_len=S.SEG, band=S.BAND, tail=S.TAIL, want_pairs=True,
                               want_trace=True)
    for x in out.values():
        x.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(S.bits_equal(got[k], want[k]) for k in want)
    env.close()


# ---- 3. re-staging ---------------------------------------------------------------------------------------------------------------
# N = 16: one tile per row, so a quad is one row with three idle waves.  The launcher keeps at most 4 workgroups resident per compute
# unit (one at width 128): with 4 x CUs + 5 rows every workgroup walks more than one quad and stages a new image for each
@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "plain", 64, "f64")], ids=lambda v: str(v))
def test_a_workgroup_stages_the_image_of_every_row_it_walks(kind, pol, md, state_mode):
    from pime_amd.ops import PackedPolicies
    env = _make_env(kind, state_mode, n=16)
    three = [_actor(pol, env, md, seed)[:2] for seed in (0, 1, 2)]
    three[1] = (three[1][0], 0.5 * three[1][1])
    want = [_metrics(kind, state_mode, pk, K, n=16) for pk, K in three]
    assert not S.bits_equal(want[0], want[1]) and not S.bits_equal(want[1], want[2]) and not S.bits_equal(want[0], want[2])
    Pn = 4 * torch.cuda.get_device_properties(DEV).multi_processor_count + 5
    stack = PackedPolicies.from_packed([three[p % 3] for p in range(Pn)])
    rec = _run(env, kind, stack, trace=False)
    assert rec["pairs"].shape == (3, 8, Pn, 16)
    bad = [p for p in range(Pn) if not S.bits_equal(rec["pairs"][:, :, p], want[p % 3])]
    assert not bad, f"rows that are not the pime_rollout_eval_metrics result of image p mod 3: {bad[:8]} ({len(bad)} of {Pn})"
    P.check_summary(rec["summary"], rec["pairs"], tag="re-staging")
    env.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_unserved_handles_kinds_and_widths_are_refused():
    from pime_amd import gym_control, native
    from pime_amd.ops import PackedPolicies
    ws = torch.zeros(8 * 5 * 8, dtype=torch.float64, device=DEV)
    img = torch.zeros(5 * 64, dtype=torch.float32, device=DEV)
    for name, sm, word in ((gym_control.PH_V35, "mixed16", "state_mode"), (gym_control.WT_INTEGRATOR, "mixed16", "state_mode"),
                           (gym_control.WT_STACKING.format(1), "mixed", "Stacking"), (gym_control.WT_STACKING.format(10), "f64", "Stacking")):
        env = gym_control.make_vec(name, 8, device=DEV, state_mode=sm, seed=S.SEED)
        env.reset()
        assert native.lib().pime_policy_sweep_supported(env._h, 2, 64) == 0
        assert native.lib().pime_policy_sweep_workspace_bytes(env._h, 5, S.N_STEPS, 0) == -1
        summary = torch.full((5, 1, 8, 5), -777.0, dtype=torch.float64, device=DEV)
        K = torch.zeros((5, env.obs_dim), dtype=torch.float64, device=DEV)
        rc, msg = _raw(env, 2, 64, img, 64, K, 5, S.N_STEPS, 0, None, 0, S.BAND, S.TAIL, None, summary, None, None, ws)
        assert rc == -1 and word in msg and "not served" in msg and (summary == -777.0).all(), (name, sm, rc, msg)
        env.close()
    env = _make_env("wt", "mixed", n=8)
    summary = torch.full((5, 1, 8, 5), -777.0, dtype=torch.float64, device=DEV)
    K = torch.zeros((5, 4), dtype=torch.float64, device=DEV)
    rc, msg = _raw(env, -1, 0, img, 64, K, 5, S.N_STEPS, 0, None, 0, S.BAND, S.TAIL, None, summary, None, None, ws)
    assert rc == -1 and "kind -1" in msg and "pime_prior_sweep" in msg and (summary == -777.0).all(), msg
    for code in (0, 1, 2):
        assert native.lib().pime_policy_sweep_supported(env._h, code, 256) == 0
        rc, msg = _raw(env, code, 256, img, 64, K, 5, S.N_STEPS, 0, None, 0, S.BAND, S.TAIL, None, summary, None, None, ws)
        assert rc == -1 and "md 256" in msg and (summary == -777.0).all(), (code, rc, msg)
    rc, msg = _raw(env, 7, 64, img, 64, K, 5, S.N_STEPS, 0, None, 0, S.BAND, S.TAIL, None, summary, None, None, ws)
    assert rc == -1 and "kind 7" in msg
    env.close()
    # injected draws: the wrapper refuses (the kernels draw the tank's process noise themselves)
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, 8, device=DEV, state_mode="mixed", seed=S.SEED, draws="mt19937")
    env.reset()
    ok = _make_env("wt", "mixed", n=8)
    pk, Kp, _ = _actor("modular", ok, 64)
    stack = PackedPolicies.from_packed([(pk, Kp)])
    assert ok.policy_supported(stack) and not env.policy_supported(stack) and not ok.policy_supported(None)
    with pytest.raises(native.PimeError, match="injected draws"):
        env.policy_sweep(stack, 4)
    env.close(); ok.close()


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_argument_errors(kind):
    import pime_amd.native as nt
    env = _make_env(kind, "mixed", n=8, reset=False)
    pk, Kp, _ = _actor("modular", env, 64)
    floats = int(nt.lib().pime_mlp_packed_floats(nt.MLP_MODULAR_ACTOR, env.obs_dim, 1, 64))
    stride = (floats + 3) // 4 * 4
    images = torch.zeros(5 * stride + 8, dtype=torch.float32, device=DEV)
    for p in range(5):
        images[p * stride:p * stride + floats] = pk.packed
    sp = np.ascontiguousarray(S.SETPOINTS[kind], dtype=np.float64)
    K = torch.as_tensor(np.tile(Kp, (5, 1)), dtype=torch.float64, device=DEV).contiguous()
    summary = torch.full((5, 3, 8, 5), -777.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(3 * 8 * 5 * 8, dtype=torch.float64, device=DEV)
    base = dict(img=images, stride=stride, K=K, P=5, n_steps=S.N_STEPS, seg_len=S.SEG, sp=sp, n_sp=3, band=S.BAND, tail=S.TAIL, summary=summary,
                ws=ws)
    call = lambda kw: _raw(env, nt.MLP_MODULAR_ACTOR, 64, kw["img"], kw["stride"], kw["K"], kw["P"], kw["n_steps"], kw["seg_len"], kw["sp"],
                           kw["n_sp"], kw["band"], kw["tail"], None, kw["summary"], None, None, kw["ws"])
    rc, msg = call(base)
    assert rc == -4 and "before pime_env_reset" in msg and (summary == -777.0).all()
    env.reset()
    off_by_4 = C.c_void_p(images.data_ptr() + 4)                        # a base that is 4-byte but not 16-byte aligned
    cases = [("P = 0", dict(P=0)), ("P = -3", dict(P=-3)), ("exceed 2^31 - 1", dict(P=2 ** 28)), ("packed_actors is NULL", dict(img=None)),
             ("summary is NULL", dict(summary=None)), ("workspace is NULL", dict(ws=None)), ("priorK is NULL", dict(K=None)),
             ("smaller than a packed image", dict(stride=floats - 4)), ("smaller than a packed image", dict(stride=0)),
             ("not a multiple of 4", dict(stride=stride + 2)), ("not 16-byte aligned", dict(img=off_by_4)),
             ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))), ("band", dict(band=float("inf"))), ("tail 0", dict(tail=0)),
             ("n_steps 0", dict(n_steps=0)), ("n_setpoints 17", dict(n_sp=17)), ("set-point schedule", dict(n_sp=2)),
             ("set-point schedule", dict(sp=None)), ("set-point schedule", dict(seg_len=-1))]
    bad = []
    for word, over in cases:
        rc, msg = call(dict(base, **over))
        if rc != -1 or word not in msg or "pime_policy_sweep" not in msg or not (summary == -777.0).all():
            bad.append((word, rc, msg))
    assert not bad, bad
    rc, msg = call(base)          # and the good call goes through
    assert rc == 0 and not (summary == -777.0).any(), msg
    env.close()


# ---- 5. protocols ----------------------------------------------------------------------------------------------------------------
def test_policy_sweep_and_select_policy_on_the_robust_plants():
    from pime_amd import protocols
    from pime_amd.ops import PackedPolicies
    plants = np.asarray(protocols.WT_ROBUST_PLANTS)
    steps = 60
    env = _make_env("wt", "mixed", n=3, reset=False, offset=0)
    agents = [make_agent("ResidualIntegratorModularPPO", env, 64)]
    pk, K = agents[0].fused_eval_policy(env)
    K = np.asarray(K, dtype=np.float64).reshape(-1)
    stack = PackedPolicies.from_packed([(pk, K), (pk, 0.5 * K), (pk, K)])
    res = protocols.policy_sweep(env, stack, plants=plants, steps=steps, want_pairs=True)
    env.close()
    assert res["summary"].shape == (3, 5, 8, 5) and res["pairs"].shape == (5, 8, 3, 3) and res["n"] == 3 and res["settled"].shape == (3,)
    P.check_summary(res["summary"], res["pairs"], tag="policy_sweep")
    assert S.bits_equal(res["pairs"][:, :, 0], res["pairs"][:, :, 2]) and not S.bits_equal(res["pairs"][:, :, 0], res["pairs"][:, :, 1])
    env = _make_env("wt", "mixed", n=3, reset=False, offset=0)
    one = protocols.step_response_metrics(env, agent=agents[0], plants=plants, steps=steps)
    env.close()
    for j, name in enumerate(protocols.METRIC_NAMES):
        assert S.bits_equal(res["pairs"][:, j, 0], one[name]), f"row 0 is the step-response protocol's {name} under that agent"
    settle = res["pairs"][:, protocols.METRIC_NAMES.index("settling_step")]                      # [S, P, N]
    want = (np.isfinite(res["pairs"]).all(axis=1) & (settle < steps)).all(axis=0).sum(axis=1)
    assert res["settled"].tolist() == want.tolist()
    sel = protocols.select_policy(res)
    best, nominal, order = S.numpy_select(res["summary"], res["settled"], res["n"])
    assert (sel["best_index"], sel["nominal_index"], sel["order"].tolist()) == (best, nominal, order)
    assert sel["best_index"] in (0, 1), "rows 0 and 2 tie: the lower one ranks first"
    assert sel["worst_cost"][0] == sel["worst_cost"][2] and sel["order"].tolist().index(0) < sel["order"].tolist().index(2)
    print(f"\nPOLICY robust plants: worst-plant ITAE {sel['worst_cost'].tolist()}, mean ITAE {sel['mean_cost'].tolist()}, settled "
          f"{sel['settled'].tolist()}, chosen {sel['best_index']} (nominal ranking: {sel['nominal_index']})")
    with pytest.raises(ValueError):
        protocols.policy_sweep(_make_env("wt", "mixed16", n=3, reset=False, offset=0), stack, plants=plants, steps=steps)


# ---- 6. training -----------------------------------------------------------------------------------------------------------------
def test_train_select_policy_writes_the_files(tmp_path, capsys, monkeypatch):
    import argparse
    from pime_amd import gym_control, protocols, train
    common = ["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
              "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
              "--break_step", str(4 * 64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1"]
    seen, real = {}, train.select_policy

    def spy(args, evaluator, cwd):     # the selection itself must not touch actor.pth
        before = open(os.path.join(cwd, "actor.pth"), "rb").read()
        seen.update(evaluator=evaluator, cwd=cwd)
        path = real(args, evaluator, cwd)
        assert open(os.path.join(cwd, "actor.pth"), "rb").read() == before, "actor.pth stays the nominal best"
        return path
    monkeypatch.setattr(train, "select_policy", spy)
    train.main(common + ["--checkpoints", "3", "--select_policy", "--log_root", str(tmp_path / "sel")])
    out = capsys.readouterr().out
    ev, cwd = seen["evaluator"], seen["cwd"]
    assert os.path.exists(os.path.join(cwd, "policy_sweep.npz")) and os.path.exists(os.path.join(cwd, "actor_robust.pth"))
    snaps = ev.snapshot_list()
    assert [s["step"] for s in ev.snapshots] == [2 * 64 * 200, 3 * 64 * 200, 4 * 64 * 200], "the last three of five evaluations"
    z = np.load(os.path.join(cwd, "policy_sweep.npz"), allow_pickle=False)
    Pn = len(snaps)
    assert 3 <= Pn <= 4 and z["snapshot_steps"].tolist() == [s["step"] for s in snaps]
    assert z["summary"].shape == (Pn, 5, 8, 5) and z["worst_cost"].shape == z["mean_cost"].shape == z["settled"].shape == (Pn,)
    np.testing.assert_array_equal(z["plants"], protocols.WT_ROBUST_PLANTS)
    assert np.isfinite(z["summary"][..., P.FINITE]).all()
    best, nominal, order = S.numpy_select(z["summary"], z["settled"], len(z["plants"]))
    assert (int(z["best_index"]), int(z["nominal_index"]), z["order"].tolist()) == (best, nominal, order)
    assert "robust" in out and "nominal" in out and "policy sweep:" in out
    # actor.pth is the evaluator's nominal best, as without the flags; actor_robust.pth is the chosen snapshot
    same = lambda path, sd: (lambda got: got.keys() == sd.keys() and all(torch.equal(got[k], sd[k].cpu()) for k in sd))(
        torch.load(path, map_location="cpu", weights_only=True))
    assert same(os.path.join(cwd, "actor.pth"), ev.best_snapshot["state_dict"])
    assert same(os.path.join(cwd, "actor_robust.pth"), snaps[best]["state_dict"])
    monkeypatch.undo()
    assert train.select_policy(argparse.Namespace(env=gym_control.WT_STACKING.format(4)), None, str(tmp_path / "b")) is None
    assert "policy selection skipped" in capsys.readouterr().out
