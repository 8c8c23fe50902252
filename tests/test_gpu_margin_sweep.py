"""The loop-perturbation sweep on the GPU (pime_margin_sweep, csrc/margin_sweep.hip) against tests/margin_sweep.py.  Shapes: 81 plants
on a handle at lane offset 1000 (six 16-lane tiles per row, the last one with a single plant; two 64-lane tiles under the prior
alone), five perturbation rows with the nominal one first and last (delays 0, 1, 3, 8; gains 0.5, 2; sigma 0, 0.05), 23 steps in
segments of 9 (the last one ragged), tail 4.
  1. all 36 served classes (2 envs x {prior, 4 policy kinds x widths 64, 128} x float64 / mixed state): the nominal rows bit-equal to
     pime_rollout_eval_metrics from the same lane state, every row through the checker, summary bit-equal to
     summary_from_pairs(pairs); also N = 130 (three summary blocks) with the prior alone;
  2. the handle's fields are bit-unchanged, two calls give equal bits, a NaN-filled workspace gives the same bits, NULL pairs /
     actions / outputs leave summary unchanged, a tile's pairs give the same bits alone (P = 1, N = 16) as inside the grid, a grid
     with more quads than resident workgroups (a workgroup walks on to its second quad) repeats its rows bit for bit, one captured
     replay gives equal bits;
  3. float64, the prior alone: device bit-equal to the host build (the tank with process noise off);
  4. every refusal and its message;
  5. protocols.loop_sweep / loop_margins on the three WT_ROBUST_PLANTS with a shortened protocol;
  6. train.py --margins writes margins.npz on a toy run and is skipped on a Stacking id."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import margin_sweep as G
import prior_sweep as P
from rollout_replay import DEV, make_agent

pytestmark = pytest.mark.gpu
KINDS = {"prior": -1, "td3": 0, "plain": 1, "modular": 2, "sac": 3}
POLICIES = [("prior", 0)] + [(k, md) for k in ("td3", "plain", "modular", "sac") for md in (64, 128)]
CLASSES = [(env, k, md, sm) for env in ("ph", "wt") for k, md in POLICIES for sm in ("f64", "mixed")]
FIELDS = {"ph": ("x", "A", "B", "C", "r", "I", "t", "episode"), "wt": ("h1", "h2", "a1", "a2", "Kp", "r", "I", "t", "episode")}


def _make_env(kind, state_mode, n=G.N, reset=True, offset=G.OFFSET, **extra):
    from pime_amd import gym_control
    name = gym_control.PH_V35 if kind == "ph" else gym_control.WT_INTEGRATOR
    kw = dict(reward_type="distance") if kind == "wt" else {}
    kw.update(extra)
    env = gym_control.make_vec(name, n, device=DEV, state_mode=state_mode, seed=G.SEED, env_offset=offset, **kw)
    if reset:
        env.reset()
    return env


def _lanes(env, kind):
    out = {k: np.ascontiguousarray(env.get_field(k)) for k in FIELDS[kind]}
    out["t"], out["episode"] = out["t"].astype(np.int32), out["episode"].astype(np.int32)
    return out


def _cfg(env, kind, table):
    import pime_amd.native as nt
    cfg = nt.EnvCfg.from_buffer_copy(env.cfg)
    keep = None
    if kind == "ph":
        keep = np.ascontiguousarray(table, dtype=np.float64)
        cfg.ph_table = keep.ctypes.data_as(C.POINTER(C.c_double))
        cfg.ph_table_len = len(keep)
    return cfg, keep


def _policy(kind, env, md):
    """(packed actor or None, priorK, the float64 tanh term as a callable or None) of a freshly initialised agent with a non-trivial
    output layer.  The float64 term is the agent's own torch module in double precision on the CPU."""
    if kind == "prior":
        return None, -env.K, None
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
    return fused[0], np.asarray(fused[1], dtype=np.float64).reshape(-1), term


def _run(env, kind, pk, K, perturb=G.PERTURB, pairs=True, trace=True, **kw):
    args = dict(n_steps=G.N_STEPS, seg_len=G.SEG, setpoints=G.SETPOINTS[kind], band=G.BAND, tail=G.TAIL, noise_seed=G.NOISE_SEED,
                noise_epoch=G.NOISE_EPOCH)
    args.update(kw)
    n_steps = args.pop("n_steps")
    out = env.margin_sweep(pk, K, perturb, n_steps, want_pairs=pairs, want_trace=trace, **args)
    torch.cuda.synchronize()
    if not (pairs or trace):
        return dict(summary=out.cpu().numpy())
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


# ---- 1. every served class -------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_served_classes():
    from pime_amd import gym_control, native
    served = set()
    for kind, name in (("ph", gym_control.PH_V35), ("wt", gym_control.WT_INTEGRATOR), ("stacking", gym_control.WT_STACKING.format(4))):
        for sm in ("f64", "mixed", "mixed16"):
            env = gym_control.make_vec(name, 4, device=DEV, state_mode=sm, seed=G.SEED)
            assert env.margin_supported() == bool(native.lib().pime_margin_sweep_supported(env._h, -1, 0))
            for pol, code in KINDS.items():
                for md in ((0,) if pol == "prior" else (64, 128, 256)):
                    if native.lib().pime_margin_sweep_supported(env._h, code, md):
                        served.add((kind, pol, md, sm))
            env.close()
    assert served == set(CLASSES) and len(CLASSES) == 36


@pytest.mark.parametrize("kind,pol,md,state_mode", CLASSES, ids=lambda v: str(v))
def test_every_served_class(kind, pol, md, state_mode, ph_table_oracle):
    env, twin = _make_env(kind, state_mode), _make_env(kind, state_mode)
    pk, K, term = _policy(pol, env, md)
    assert env.margin_supported(pk)
    cfg, keep = _cfg(env, kind, ph_table_oracle)
    lanes = _lanes(env, kind)
    rec = _run(env, kind, pk, K)
    assert rec["pairs"].shape == (3, 8, 5, G.N) and rec["actions"].shape == rec["outputs"].shape == (G.N_STEPS, 5, G.N)
    _, want, _ = twin.rollout_eval_metrics(pk, K, G.N_STEPS, setpoints=G.SETPOINTS[kind], seg_len=G.SEG, band=G.BAND, tail=G.TAIL)
    want = want.cpu().numpy()
    for p in (0, 4):
        assert G.bits_equal(rec["pairs"][:, :, p], want), f"the nominal row {p} is not bit-equal to pime_rollout_eval_metrics"
    use = G.check_recording(kind, cfg, lanes, ph_table_oracle, rec, K=K, policy=term, tag=f"{kind}-{pol}{md}-{state_mode}")
    P.check_summary(rec["summary"], rec["pairs"], tag=f"{kind}-{pol}{md}-{state_mode}")
    print(f"\nMARGIN id={kind}-{pol}{md}-{state_mode} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action "
          f"{use['action']:.3g} (gap {use['gap']:.4g})")
    env.close(); twin.close()


def test_three_summary_blocks():
    env = _make_env("wt", "mixed", n=130)
    rec = _run(env, "wt", None, -env.K, trace=False)
    P.check_summary(rec["summary"], rec["pairs"], tag="N = 130")
    assert (rec["summary"][..., P.FINITE] == 130).all() and rec["summary"].shape == (5, 3, 8, 5)
    env.close()


# ---- 2. structure ----------------------------------------------------------------------------------------------------------------
def _raw(env, kind_code, md, img, K, perturb, Pn, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, outputs, workspace):
    import pime_amd.native as nt
    rc = nt.lib().pime_margin_sweep(env._h, kind_code, md, nt.ptr(img), nt.ptr(K), nt.ptr(perturb), Pn, C.c_uint64(G.NOISE_SEED),
                                    C.c_uint32(G.NOISE_EPOCH), n_steps, seg_len, nt.ptr(sp), n_sp, band, tail, nt.ptr(pairs), nt.ptr(summary),
                                    nt.ptr(actions), nt.ptr(outputs), nt.ptr(workspace), env._stream())
    torch.cuda.synchronize()
    return rc, nt.last_error()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "prior", 0, "f64"), ("ph", "sac", 64, "mixed"),
                                                   ("wt", "prior", 0, "mixed")], ids=lambda v: str(v))
def test_the_handle_is_untouched_and_the_outputs_are_independent(kind, pol, md, state_mode):
    import pime_amd.native as nt
    env, twin = _make_env(kind, state_mode), _make_env(kind, state_mode)
    pk, K, _ = _policy(pol, env, md)
    before = _lanes(env, kind)
    counters = (env._t_all, env._was_reset, env.reset_count)
    obs0 = env.obs.clone()
    first, second = _run(env, kind, pk, K), _run(env, kind, pk, K)
    assert all(G.bits_equal(first[k], second[k]) for k in first), "two calls must be bit-identical"
    quiet = _run(env, kind, pk, K, pairs=False, trace=False)
    assert G.bits_equal(quiet["summary"], first["summary"]), "NULL pairs / actions / outputs must not change a bit of summary"
    # the raw call with a NaN-filled workspace: pairs NULL (the finishing launch reads the workspace copy) and pairs given
    ws_bytes = nt.lib().pime_margin_sweep_workspace_bytes(env._h, 5, G.N_STEPS, G.SEG)
    assert ws_bytes == 3 * 8 * 5 * G.N * 8
    Kd = np.ascontiguousarray(K, dtype=np.float64)
    pt = torch.as_tensor(G.PERTURB, dtype=torch.float64, device=DEV).contiguous()
    sp = np.ascontiguousarray(G.SETPOINTS[kind], dtype=np.float64)
    code, img = (-1, None) if pk is None else (KINDS[pol], pk.packed)
    for with_pairs in (False, True):
        ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
        summary = torch.full((5, 3, 8, 5), float("nan"), dtype=torch.float64, device=DEV)
        pairs = torch.full((3, 8, 5, G.N), float("nan"), dtype=torch.float64, device=DEV) if with_pairs else None
        rc, msg = _raw(env, code, md, img, Kd, pt, 5, G.N_STEPS, G.SEG, sp, 3, G.BAND, G.TAIL, pairs, summary, None, None, ws)
        assert rc == 0, msg
        assert G.bits_equal(summary.cpu().numpy(), first["summary"]), "a NaN-filled workspace must not change a bit"
        if with_pairs:
            assert G.bits_equal(pairs.cpu().numpy(), first["pairs"])
    after = _lanes(env, kind)
    for k in before:
        assert G.bits_equal(before[k].astype(np.float64), after[k].astype(np.float64)), k
    assert (env._t_all, env._was_reset, env.reset_count) == counters and env._t_lanes is None
    assert torch.equal(env.obs, obs0)
    a = torch.full((G.N,), 0.25, dtype=torch.float64, device=DEV)
    got, want = env.step(a, auto_reset=False), twin.step(a, auto_reset=False)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "the next step equals that of an env that never ran the sweep"
    env.close(); twin.close()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "plain", 64, "f64"), ("wt", "prior", 0, "f64")],
                         ids=lambda v: str(v))
def test_a_tile_alone_gives_the_bits_it_gives_inside_the_grid(kind, pol, md, state_mode):
    big, small = _make_env(kind, state_mode), _make_env(kind, state_mode, n=16, offset=G.OFFSET + 32)
    for k in FIELDS[kind]:
        if k not in ("t", "episode"):
            assert G.bits_equal(big.get_field(k)[32:48], small.get_field(k)), "the same global lanes draw the same state"
    pk, K, _ = _policy(pol, big, md)
    a = _run(big, kind, pk, K)
    b = _run(small, kind, pk, K, perturb=G.PERTURB[2:3])
    for k in ("pairs", "actions", "outputs"):
        assert G.bits_equal(a[k][..., 2:3, 32:48], b[k]), k
    big.close(); small.close()


# one tile per row (N = 16 with a policy, N = 64 under the prior alone), so a quad is four rows; the launcher keeps at most 4 policy
# workgroups (8 without an image) resident per compute unit: beyond 16 (32) x CUs rows some workgroup takes its second quad
WALKS = [("wt", "modular", 128, "mixed", 16, 16, True), ("ph", "prior", 0, "f64", 64, 32, False)]
SEVEN = (0, 1, 2, 3, 4, 1, 2)      # the file's five rows as a period of seven


def walk_rows(per_cu):
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return 7 * -(-(per_cu * cus + 4) // 7)


def check_walk(big, small, Pn):
    """Rows repeated with period 7: every row p of `big` is bit-equal to row p % 7, and rows 0 .. 6 to the P = 7 call `small`."""
    axis = dict(summary=0, pairs=2, actions=1, outputs=1)
    assert set(big) == set(small)
    for k in big:
        assert big[k].shape[axis[k]] == Pn and small[k].shape[axis[k]] == 7
        assert P.bits_equal(big[k], np.take(small[k], np.arange(Pn) % 7, axis=axis[k])), f"{k}: a row is not the row of its period"


@pytest.mark.parametrize("kind,pol,md,state_mode,n,per_cu,trace", WALKS, ids=lambda v: str(v))
def test_a_workgroup_walks_more_than_one_quad(kind, pol, md, state_mode, n, per_cu, trace):
    env = _make_env(kind, state_mode, n=n)
    pk, K, _ = _policy(pol, env, md)
    Pn = walk_rows(per_cu)
    seven = G.PERTURB[list(SEVEN)]
    big = _run(env, kind, pk, K, perturb=np.tile(seven, (Pn // 7, 1)), trace=trace)
    small = _run(env, kind, pk, K, perturb=seven, trace=trace)
    check_walk(big, small, Pn)
    env.close()


@pytest.mark.parametrize("kind,pol,md", [("wt", "modular", 128), ("ph", "prior", 0)], ids=lambda v: str(v))
def test_captured_in_a_graph_and_replayed(kind, pol, md):
    import pime_amd.native as nt
    env = _make_env(kind, "mixed")
    pk, K, _ = _policy(pol, env, md)
    want = _run(env, kind, pk, K)
    pt = torch.as_tensor(G.PERTURB, dtype=torch.float64, device=DEV).contiguous()   # uploaded (and validated) before the capture
    graph = torch.cuda.CUDAGraph()
    with nt.capture_guard(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = env.margin_sweep(pk, K, pt, G.N_STEPS, setpoints=G.SETPOINTS[kind], seg_len=G.SEG, band=G.BAND, tail=G.TAIL,
                               noise_seed=G.NOISE_SEED, noise_epoch=G.NOISE_EPOCH, want_pairs=True, want_trace=True)
    for x in out.values():
        x.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(G.bits_equal(got[k], want[k]) for k in want)
    env.close()


# ---- 3. the host build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_prior_is_bit_equal_to_the_host_build(kind, ph_table_oracle):
    env = _make_env(kind, "f64", **({"noise_scale": 0.} if kind == "wt" else {}))
    cfg, keep = _cfg(env, kind, ph_table_oracle)
    lanes = _lanes(env, kind)
    K = np.asarray(-env.K, dtype=np.float64).reshape(-1)
    rec = _run(env, kind, None, K)
    host = G.host_margin(kind, cfg, lanes, K=K)
    for k in rec:
        assert G.bits_equal(rec[k], host[k]), f"{k} is not bit-equal to the host build's"
    env.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_unserved_handles_and_widths_are_refused():
    from pime_amd import gym_control, native
    pt = torch.as_tensor(G.PERTURB, dtype=torch.float64, device=DEV).contiguous()
    ws = torch.zeros(8 * 5 * 8, dtype=torch.float64, device=DEV)
    for name, sm, word in ((gym_control.PH_V35, "mixed16", "state_mode"), (gym_control.WT_INTEGRATOR, "mixed16", "state_mode"),
                           (gym_control.WT_STACKING.format(1), "mixed", "Stacking"), (gym_control.WT_STACKING.format(10), "f64", "Stacking")):
        env = gym_control.make_vec(name, 8, device=DEV, state_mode=sm, seed=G.SEED)
        env.reset()
        assert not env.margin_supported() and native.lib().pime_margin_sweep_supported(env._h, -1, 0) == 0
        assert native.lib().pime_margin_sweep_workspace_bytes(env._h, 5, G.N_STEPS, 0) == -1
        summary = torch.full((5, 1, 8, 5), -777.0, dtype=torch.float64, device=DEV)
        K = np.zeros(env.obs_dim)
        rc, msg = _raw(env, -1, 0, None, K, pt, 5, G.N_STEPS, 0, None, 0, G.BAND, G.TAIL, None, summary, None, None, ws)
        assert rc == -1 and word in msg and "not served" in msg and (summary == -777.0).all(), (name, sm, rc, msg)
        with pytest.raises(native.PimeError):
            env.margin_sweep(None, K, G.PERTURB, G.N_STEPS)
        env.close()
    env = _make_env("wt", "mixed", n=8)
    img = torch.zeros(16, dtype=torch.float32, device=DEV)
    summary = torch.full((5, 1, 8, 5), -777.0, dtype=torch.float64, device=DEV)
    for code in (0, 1, 2):
        assert native.lib().pime_margin_sweep_supported(env._h, code, 256) == 0
        rc, msg = _raw(env, code, 256, img, np.zeros(4), pt, 5, G.N_STEPS, 0, None, 0, G.BAND, G.TAIL, None, summary, None, None, ws)
        assert rc == -1 and "md 256" in msg and (summary == -777.0).all(), (code, rc, msg)
    rc, msg = _raw(env, 7, 64, img, np.zeros(4), pt, 5, G.N_STEPS, 0, None, 0, G.BAND, G.TAIL, None, summary, None, None, ws)
    assert rc == -1 and "kind 7" in msg
    env.close()


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_argument_errors(kind):
    env = _make_env(kind, "mixed", n=8, reset=False)
    sp = np.ascontiguousarray(G.SETPOINTS[kind], dtype=np.float64)
    K = np.ascontiguousarray(G.PRIOR_K[kind])
    pt = torch.as_tensor(G.PERTURB, dtype=torch.float64, device=DEV).contiguous()
    summary = torch.full((5, 3, 8, 5), -777.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(3 * 8 * 5 * 8, dtype=torch.float64, device=DEV)
    base = dict(K=K, pt=pt, P=5, n_steps=G.N_STEPS, seg_len=G.SEG, sp=sp, n_sp=3, band=G.BAND, tail=G.TAIL, summary=summary, ws=ws, code=-1,
                md=0, img=None)
    call = lambda kw: _raw(env, kw["code"], kw["md"], kw["img"], kw["K"], kw["pt"], kw["P"], kw["n_steps"], kw["seg_len"], kw["sp"], kw["n_sp"],
                           kw["band"], kw["tail"], None, kw["summary"], None, None, kw["ws"])
    rc, msg = call(base)
    assert rc == -4 and "before pime_env_reset" in msg and (summary == -777.0).all()
    env.reset()
    cases = [("P = 0", dict(P=0)), ("P = -3", dict(P=-3)), ("exceed 2^31 - 1", dict(P=2 ** 28)), ("perturb is NULL", dict(pt=None)),
             ("summary is NULL", dict(summary=None)), ("workspace is NULL", dict(ws=None)), ("priorK is NULL", dict(K=None)),
             ("packed_actor is NULL", dict(code=2, md=64)), ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))),
             ("band", dict(band=float("inf"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)), ("n_setpoints 17", dict(n_sp=17)),
             ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)), ("set-point schedule", dict(seg_len=-1))]
    bad = []
    for word, over in cases:
        rc, msg = call(dict(base, **over))
        if rc != -1 or word not in msg or "pime_margin_sweep" not in msg or not (summary == -777.0).all():
            bad.append((word, rc, msg))
    assert not bad, bad
    rc, msg = call(base)          # and the good call goes through
    assert rc == 0 and not (summary == -777.0).any(), msg
    for rows in ([[float("nan"), 0, 0]], [[1, 0.5, 0]], [[1, 9, 0]], [[1, 0, -1.0]]):
        with pytest.raises(ValueError):
            env.margin_sweep(None, K, rows, 4)
    env.close()


# ---- 5. protocols ----------------------------------------------------------------------------------------------------------------
def test_loop_sweep_and_margins_on_the_robust_plants():
    from pime_amd import protocols
    plants = np.asarray(protocols.WT_ROBUST_PLANTS)
    steps = 60
    grid = np.concatenate([protocols.perturbation_grid(delays=(0, 1, 2, 4, 8)), protocols.perturbation_grid(gains=(0.5, 2.0)),
                           protocols.perturbation_grid(sigmas=(0.02, 0.05))])
    env = _make_env("wt", "mixed", n=3, reset=False, offset=0)
    res = protocols.loop_sweep(env, grid, plants=plants, steps=steps, want_pairs=True)
    env.close()
    assert res["summary"].shape == (9, 5, 8, 5) and res["pairs"].shape == (5, 8, 9, 3) and res["n"] == 3
    P.check_summary(res["summary"], res["pairs"], tag="loop_sweep")
    env = _make_env("wt", "mixed", n=3, reset=False, offset=0)
    prior = protocols.step_response_metrics(env, plants=plants, steps=steps)
    env.close()
    for j, name in enumerate(protocols.METRIC_NAMES):
        assert G.bits_equal(res["pairs"][:, j, 0], prior[name]), f"the nominal row is the step-response protocol's {name}"
    m = protocols.loop_margins(res)
    assert m["nominal"] == 0 and m["acceptable"].shape == (9,) and m["plant_delay_margin"].shape == (3,)
    assert m["sigma_slope"] > 0.0, "sensor noise makes the action move"
    print(f"\nMARGIN robust plants, prior alone: delay margin {m['delay_margin']} steps, gain margin {m['gain_margin']} / "
          f"{m['gain_margin_low']}, sigma margin {m['sigma_margin']}, action-variation slope {m['sigma_slope']:.4g}, per plant delay "
          f"{m['plant_delay_margin'].tolist()}")


def test_train_margins_writes_the_file(tmp_path, capsys):
    import os
    from pime_amd import protocols, train
    common = ["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
              "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
              "--break_step", str(64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1"]
    train.main(common + ["--margins", "--log_root", str(tmp_path / "a")])
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "margins.npz"]
    assert len(found) == 1
    z = np.load(found[0], allow_pickle=False)
    P_ = len(train.MARGIN_DELAYS) + len(train.MARGIN_GAINS) + len(train.MARGIN_SIGMAS)
    assert z["perturb"].shape == (P_, 3) and (z["perturb"][0] == [1.0, 0.0, 0.0]).all()
    np.testing.assert_array_equal(z["plants"], protocols.WT_ROBUST_PLANTS)
    for who in ("agent", "prior"):
        assert z[f"{who}_summary"].shape == (P_, 5, 8, 5) and z[f"{who}_acceptable"].shape == (P_,)
        assert z[f"{who}_plant_delay_margin"].shape == (3,) and z[f"{who}_delay_margin"].shape == ()
        assert np.isfinite(z[f"{who}_summary"][..., P.FINITE]).all()
    assert not G.bits_equal(z["agent_summary"], z["prior_summary"]), "the trained residual is not the prior alone"
    out = capsys.readouterr().out
    assert "delay margin" in out and "agent " in out and "prior " in out
    import argparse
    from pime_amd import gym_control
    assert train.margins(argparse.Namespace(env=gym_control.WT_STACKING.format(4)), None, str(tmp_path / "b")) is None
    assert "margins skipped" in capsys.readouterr().out
