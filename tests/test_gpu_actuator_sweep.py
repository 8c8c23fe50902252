"""The actuator-limits sweep on the GPU (pime_actuator_sweep, csrc/actuator_sweep.hip) against tests/actuator_sweep.py.  Shapes: 81
plants on a handle at lane offset 1000 (six 16-lane tiles per row, the last one with a single plant; two 64-lane tiles under the prior
alone), the ten rows of tests/actuator_sweep.py, 23 steps in segments of 9 (the last one ragged), tail 4.
  1. all 36 served classes (2 envs x {prior, 4 policy kinds x widths 64, 128} x float64 / mixed state): the eight metric rows of both
     all-off rows bit-equal to pime_rollout_eval_metrics from a twin handle, every row through the checker, summary bit-equal to
     summary_from_pairs(pairs); also N = 130 (three summary blocks) with the prior alone;
  2. the handle's fields are bit-unchanged, two calls give equal bits, a NaN-filled workspace gives the same bits, NULL pairs /
     actions / commands / outputs leave summary unchanged, a tile's pairs give the same bits alone (P = 1, N = 16) as inside the grid,
     a grid with more quads than resident workgroups (a workgroup walks on to its second quad) repeats its rows bit for bit, one
     captured replay gives equal bits;
  3. float64, the prior alone: device bit-equal to the host build (the tank with process noise off);
  4. every refusal and its message;
  5. protocols.actuator_sweep / actuator_summary on the three WT_ROBUST_PLANTS with a shortened protocol;
  6. train.py --actuator writes actuator_sweep.npz on a toy run and is skipped on a Stacking id."""
import numpy as np
import pytest
import torch

import actuator_sweep as A
import prior_sweep as P
from rollout_replay import DEV
from test_gpu_margin_sweep import CLASSES, FIELDS, KINDS, WALKS, _cfg, _make_env, _policy, walk_rows      # the handles, policies and
                                                                                                          # classes of that sweep
pytestmark = pytest.mark.gpu
PN = len(A.ACT["wt"])          # 10 rows
INF = float("inf")


def _lanes(env, kind):
    out = {k: np.ascontiguousarray(env.get_field(k)) for k in FIELDS[kind]}
    out["t"], out["episode"] = out["t"].astype(np.int32), out["episode"].astype(np.int32)
    return out


def _run(env, kind, pk, K, rows=None, pairs=True, trace=True, **kw):
    args = dict(n_steps=A.N_STEPS, seg_len=A.SEG, setpoints=A.SETPOINTS[kind], band=A.BAND, tail=A.TAIL)
    args.update(kw)
    n_steps = args.pop("n_steps")
    out = env.actuator_sweep(pk, K, A.ACT[kind] if rows is None else rows, n_steps, want_pairs=pairs, want_trace=trace, **args)
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
            env = gym_control.make_vec(name, 4, device=DEV, state_mode=sm, seed=A.SEED)
            assert env.actuator_supported() == bool(native.lib().pime_actuator_sweep_supported(env._h, -1, 0))
            for pol, code in KINDS.items():
                for md in ((0,) if pol == "prior" else (64, 128, 256)):
                    if native.lib().pime_actuator_sweep_supported(env._h, code, md):
                        served.add((kind, pol, md, sm))
            env.close()
    assert served == set(CLASSES) and len(CLASSES) == 36


@pytest.mark.parametrize("kind,pol,md,state_mode", CLASSES, ids=lambda v: str(v))
def test_every_served_class(kind, pol, md, state_mode, ph_table_oracle):
    env, twin = _make_env(kind, state_mode), _make_env(kind, state_mode)
    pk, K, term = _policy(pol, env, md)
    assert env.actuator_supported(pk)
    cfg, keep = _cfg(env, kind, ph_table_oracle)
    lanes = _lanes(env, kind)
    rec = _run(env, kind, pk, K)
    assert rec["pairs"].shape == (3, 16, PN, A.N) and rec["actions"].shape == rec["commands"].shape == rec["outputs"].shape == (A.N_STEPS, PN, A.N)
    _, want, _ = twin.rollout_eval_metrics(pk, K, A.N_STEPS, setpoints=A.SETPOINTS[kind], seg_len=A.SEG, band=A.BAND, tail=A.TAIL)
    want = want.cpu().numpy()
    for p in A.ALL_OFF:
        assert A.bits_equal(rec["pairs"][:, :8, p], want), f"the all-off row {p} is not bit-equal to pime_rollout_eval_metrics"
        assert A.bits_equal(rec["actions"][:, p], rec["commands"][:, p]), "with every stage off the applied action is the command's word"
    use = A.check_recording(kind, cfg, lanes, ph_table_oracle, rec, K=K, policy=term, tag=f"{kind}-{pol}{md}-{state_mode}")
    P.check_summary(rec["summary"], rec["pairs"], tag=f"{kind}-{pol}{md}-{state_mode}")
    assert (rec["summary"][..., P.FINITE] == A.N).all()
    # (that every stage acts is a property of the grid under the prior's commands: tests/test_actuator_sweep_cpu.py holds it there)
    print(f"\nACTUATOR id={kind}-{pol}{md}-{state_mode} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action "
          f"{use['action']:.3g} (gap {use['gap']:.4g})")
    env.close(); twin.close()


def test_three_summary_blocks():
    env = _make_env("wt", "mixed", n=130)
    rec = _run(env, "wt", None, -env.K, trace=False)
    P.check_summary(rec["summary"], rec["pairs"], tag="N = 130")
    assert (rec["summary"][..., P.FINITE] == 130).all() and rec["summary"].shape == (PN, 3, 16, 5)
    env.close()


# ---- 2. structure ----------------------------------------------------------------------------------------------------------------
def _raw(env, kind_code, md, img, K, rows, Pn, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, commands, outputs, workspace):
    import pime_amd.native as nt
    rc = nt.lib().pime_actuator_sweep(env._h, kind_code, md, nt.ptr(img), nt.ptr(K), nt.ptr(rows), Pn, n_steps, seg_len, nt.ptr(sp), n_sp, band,
                                      tail, nt.ptr(pairs), nt.ptr(summary), nt.ptr(actions), nt.ptr(commands), nt.ptr(outputs),
                                      nt.ptr(workspace), env._stream())
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
    assert all(A.bits_equal(first[k], second[k]) for k in first), "two calls must be bit-identical"
    quiet = _run(env, kind, pk, K, pairs=False, trace=False)
    assert A.bits_equal(quiet["summary"], first["summary"]), "NULL pairs / actions / commands / outputs must not change a bit of summary"
    # the raw call with a NaN-filled workspace: pairs NULL (the finishing launch reads the workspace copy) and pairs given; one trace
    # alone at a time
    ws_bytes = nt.lib().pime_actuator_sweep_workspace_bytes(env._h, PN, A.N_STEPS, A.SEG)
    assert ws_bytes == 3 * 16 * PN * A.N * 8
    Kd = np.ascontiguousarray(K, dtype=np.float64)
    at = torch.as_tensor(A.ACT[kind], dtype=torch.float64, device=DEV).contiguous()
    sp = np.ascontiguousarray(A.SETPOINTS[kind], dtype=np.float64)
    code, img = (-1, None) if pk is None else (KINDS[pol], pk.packed)
    for with_pairs, only in ((False, None), (True, "actions"), (False, "commands"), (True, "outputs")):
        ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
        summary = torch.full((PN, 3, 16, 5), float("nan"), dtype=torch.float64, device=DEV)
        pairs = torch.full((3, 16, PN, A.N), float("nan"), dtype=torch.float64, device=DEV) if with_pairs else None
        tr = {k: (torch.full((A.N_STEPS, PN, A.N), float("nan"), dtype=torch.float64, device=DEV) if k == only else None)
              for k in ("actions", "commands", "outputs")}
        rc, msg = _raw(env, code, md, img, Kd, at, PN, A.N_STEPS, A.SEG, sp, 3, A.BAND, A.TAIL, pairs, summary, tr["actions"], tr["commands"],
                       tr["outputs"], ws)
        assert rc == 0, msg
        assert A.bits_equal(summary.cpu().numpy(), first["summary"]), "a NaN-filled workspace must not change a bit"
        if with_pairs:
            assert A.bits_equal(pairs.cpu().numpy(), first["pairs"])
        if only is not None:
            assert A.bits_equal(tr[only].cpu().numpy(), first[only]), only
    after = _lanes(env, kind)
    for k in before:
        assert A.bits_equal(before[k].astype(np.float64), after[k].astype(np.float64)), k
    assert (env._t_all, env._was_reset, env.reset_count) == counters and env._t_lanes is None
    assert torch.equal(env.obs, obs0)
    a = torch.full((A.N,), 0.25, dtype=torch.float64, device=DEV)
    got, want = env.step(a, auto_reset=False), twin.step(a, auto_reset=False)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "the next step equals that of an env that never ran the sweep"
    env.close(); twin.close()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "plain", 64, "f64"), ("wt", "prior", 0, "f64")],
                         ids=lambda v: str(v))
def test_a_tile_alone_gives_the_bits_it_gives_inside_the_grid(kind, pol, md, state_mode):
    big, small = _make_env(kind, state_mode), _make_env(kind, state_mode, n=16, offset=A.OFFSET + 32)
    for k in FIELDS[kind]:
        if k not in ("t", "episode"):
            assert A.bits_equal(big.get_field(k)[32:48], small.get_field(k)), "the same global lanes draw the same state"
    pk, K, _ = _policy(pol, big, md)
    a = _run(big, kind, pk, K)
    b = _run(small, kind, pk, K, rows=A.ACT[kind][8:9])
    for k in ("pairs", "actions", "commands", "outputs"):
        assert A.bits_equal(a[k][..., 8:9, 32:48], b[k]), k
    big.close(); small.close()


@pytest.mark.parametrize("kind,pol,md,state_mode,n,per_cu,trace", WALKS, ids=lambda v: str(v))
def test_a_workgroup_walks_more_than_one_quad(kind, pol, md, state_mode, n, per_cu, trace):
    env = _make_env(kind, state_mode, n=n)
    pk, K, _ = _policy(pol, env, md)
    Pn = walk_rows(per_cu)
    seven = A.ACT[kind][[0, 1, 2, 3, 6, 7, 8]]
    big = _run(env, kind, pk, K, rows=np.tile(seven, (Pn // 7, 1)), trace=trace)
    small = _run(env, kind, pk, K, rows=seven, trace=trace)
    axis = dict(summary=0, pairs=2, actions=1, commands=1, outputs=1)
    assert set(big) == set(small) and (not trace or "commands" in big)
    for k in big:
        assert big[k].shape[axis[k]] == Pn and small[k].shape[axis[k]] == 7
        assert A.bits_equal(big[k], np.take(small[k], np.arange(Pn) % 7, axis=axis[k])), f"{k}: a row is not the row of its period"
    env.close()


@pytest.mark.parametrize("kind,pol,md", [("wt", "modular", 128), ("ph", "prior", 0)], ids=lambda v: str(v))
def test_captured_in_a_graph_and_replayed(kind, pol, md):
    import pime_amd.native as nt
    env = _make_env(kind, "mixed")
    pk, K, _ = _policy(pol, env, md)
    want = _run(env, kind, pk, K)
    at = torch.as_tensor(A.ACT[kind], dtype=torch.float64, device=DEV).contiguous()   # uploaded before the capture
    graph = torch.cuda.CUDAGraph()
    with nt.capture_guard(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = env.actuator_sweep(pk, K, at, A.N_STEPS, setpoints=A.SETPOINTS[kind], seg_len=A.SEG, band=A.BAND, tail=A.TAIL,
                                 want_pairs=True, want_trace=True)
    for x in out.values():
        x.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert set(got) == set(want) and all(A.bits_equal(got[k], want[k]) for k in want)
    env.close()


# ---- 3. the host build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_prior_is_bit_equal_to_the_host_build(kind, ph_table_oracle):
    env = _make_env(kind, "f64", **({"noise_scale": 0.} if kind == "wt" else {}))
    cfg, keep = _cfg(env, kind, ph_table_oracle)
    lanes = _lanes(env, kind)
    K = np.asarray(-env.K, dtype=np.float64).reshape(-1)
    rec = _run(env, kind, None, K)
    host = A.host_actuator(kind, cfg, lanes, K=K)
    for k in ("pairs", "actions", "commands", "outputs", "summary"):
        assert A.bits_equal(rec[k], host[k]), f"{k} is not bit-equal to the host build's"
    env.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_unserved_handles_and_widths_are_refused():
    from pime_amd import gym_control, native
    at = torch.as_tensor(A.ACT["wt"], dtype=torch.float64, device=DEV).contiguous()
    ws = torch.zeros(16 * PN * 8, dtype=torch.float64, device=DEV)
    for name, sm, word in ((gym_control.PH_V35, "mixed16", "state_mode"), (gym_control.WT_INTEGRATOR, "mixed16", "state_mode"),
                           (gym_control.WT_STACKING.format(1), "mixed", "Stacking"), (gym_control.WT_STACKING.format(10), "f64", "Stacking")):
        env = gym_control.make_vec(name, 8, device=DEV, state_mode=sm, seed=A.SEED)
        env.reset()
        assert not env.actuator_supported() and native.lib().pime_actuator_sweep_supported(env._h, -1, 0) == 0
        assert native.lib().pime_actuator_sweep_workspace_bytes(env._h, PN, A.N_STEPS, 0) == -1
        summary = torch.full((PN, 1, 16, 5), -777.0, dtype=torch.float64, device=DEV)
        K = np.zeros(env.obs_dim)
        rc, msg = _raw(env, -1, 0, None, K, at, PN, A.N_STEPS, 0, None, 0, A.BAND, A.TAIL, None, summary, None, None, None, ws)
        assert rc == -1 and word in msg and "not served" in msg and "pime_actuator_sweep" in msg and (summary == -777.0).all(), (name, sm, rc, msg)
        with pytest.raises(native.PimeError):
            env.actuator_sweep(None, K, [[-1, 1, INF, 0, 0, 0]], A.N_STEPS)
        env.close()
    env = _make_env("wt", "mixed", n=8)
    img = torch.zeros(16, dtype=torch.float32, device=DEV)
    summary = torch.full((PN, 1, 16, 5), -777.0, dtype=torch.float64, device=DEV)
    for code in (0, 1, 2):
        assert native.lib().pime_actuator_sweep_supported(env._h, code, 256) == 0
        rc, msg = _raw(env, code, 256, img, np.zeros(4), at, PN, A.N_STEPS, 0, None, 0, A.BAND, A.TAIL, None, summary, None, None, None, ws)
        assert rc == -1 and "md 256" in msg and (summary == -777.0).all(), (code, rc, msg)
    rc, msg = _raw(env, 7, 64, img, np.zeros(4), at, PN, A.N_STEPS, 0, None, 0, A.BAND, A.TAIL, None, summary, None, None, None, ws)
    assert rc == -1 and "kind 7" in msg
    env.close()


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_argument_errors(kind):
    env = _make_env(kind, "mixed", n=8, reset=False)
    sp = np.ascontiguousarray(A.SETPOINTS[kind], dtype=np.float64)
    K = np.ascontiguousarray(A.PRIOR_K[kind])
    at = torch.as_tensor(A.ACT[kind], dtype=torch.float64, device=DEV).contiguous()
    summary = torch.full((PN, 3, 16, 5), -777.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(3 * 16 * PN * 8, dtype=torch.float64, device=DEV)
    base = dict(K=K, at=at, P=PN, n_steps=A.N_STEPS, seg_len=A.SEG, sp=sp, n_sp=3, band=A.BAND, tail=A.TAIL, summary=summary, ws=ws, code=-1,
                md=0, img=None)
    call = lambda kw: _raw(env, kw["code"], kw["md"], kw["img"], kw["K"], kw["at"], kw["P"], kw["n_steps"], kw["seg_len"], kw["sp"], kw["n_sp"],
                           kw["band"], kw["tail"], None, kw["summary"], None, None, None, kw["ws"])
    rc, msg = call(base)
    assert rc == -4 and "before pime_env_reset" in msg and (summary == -777.0).all()
    env.reset()
    cases = [("P = 0", dict(P=0)), ("P = -3", dict(P=-3)), ("exceed 2^31 - 1", dict(P=2 ** 28)), ("actuator is NULL", dict(at=None)),
             ("summary is NULL", dict(summary=None)), ("workspace is NULL", dict(ws=None)), ("priorK is NULL", dict(K=None)),
             ("packed_actor is NULL", dict(code=2, md=64)), ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))),
             ("band", dict(band=float("inf"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)), ("n_setpoints 17", dict(n_sp=17)),
             ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)), ("set-point schedule", dict(seg_len=-1))]
    bad = []
    for word, over in cases:
        rc, msg = call(dict(base, **over))
        if rc != -1 or word not in msg or "pime_actuator_sweep" not in msg or not (summary == -777.0).all():
            bad.append((word, rc, msg))
    assert not bad, bad
    rc, msg = call(base)          # and the good call goes through
    assert rc == 0 and not (summary == -777.0).any(), msg
    for rows in ([[float("nan"), 1, INF, 0, 0, 0]], [[1, -1, INF, 0, 0, 0]], [[-1, 1, -0.5, 0, 0, 0]], [[-1, 1, INF, 0, INF, 0]],
                 [[-1, 1, INF, 0, 0]]):
        with pytest.raises(ValueError):
            env.actuator_sweep(None, K, rows, 4)
    env.close()


# ---- 5. protocols ----------------------------------------------------------------------------------------------------------------
def test_actuator_sweep_on_the_robust_plants():
    from pime_amd import protocols
    plants = np.asarray(protocols.WT_ROBUST_PLANTS)
    steps = 60
    grid = np.concatenate([protocols.actuator_grid(limits=[(-0.5, 0.5)], qu=(1 / 16,)), protocols.rig_row()[None]])
    env = _make_env("wt", "mixed", n=3, reset=False, offset=0)
    res = protocols.actuator_sweep(env, grid, plants=plants, steps=steps, want_pairs=True)
    env.close()
    assert res["summary"].shape == (5, 5, 16, 5) and res["pairs"].shape == (5, 16, 5, 3) and res["n"] == 3
    assert res["actions"].shape == res["commands"].shape == res["outputs"].shape == (5 * steps, 5, 3)
    P.check_summary(res["summary"], res["pairs"], tag="actuator_sweep")
    env = _make_env("wt", "mixed", n=3, reset=False, offset=0)
    prior = protocols.step_response_metrics(env, plants=plants, steps=steps)
    env.close()
    for j, name in enumerate(protocols.METRIC_NAMES):
        assert A.bits_equal(res["pairs"][:, j, 0], prior[name]), f"the all-off row is the step-response protocol's {name}"
    u, c = res["actions"], res["commands"]
    assert A.bits_equal(u[:, 0], c[:, 0]) and (u[:, 2] >= -0.5).all() and (u[:, 2] <= 0.5).all() and (c[:, 2] > 0.5).any()
    assert (u[:, 1] == np.rint(u[:, 1] * 16) / 16).all() and (u[:, 4] >= -1).all() and (u[:, 4] <= 1).all()
    assert (res["pairs"][:, A.SAT_STEPS, 2] > 0).any() and (res["pairs"][:, 8:11, 0] == 0).all()
    r = protocols.actuator_summary(res)
    assert all(np.shape(r[k]) == (5,) and np.isfinite(r[k]).all() for k in ("itae_ratio", "limit_cycle", "reversals"))
    assert r["itae_ratio"][0] == 1.0 and r["limit_cycle"].min() >= 0 and r["limit_cycle"].max() <= 1
    quiet_env = _make_env("wt", "mixed", n=3, reset=False, offset=0)
    quiet = protocols.actuator_sweep(quiet_env, grid, plants=plants, steps=steps)
    quiet_env.close()
    assert quiet["pairs"] is None and quiet["commands"] is None and A.bits_equal(quiet["summary"], res["summary"])
    print(f"\nACTUATOR robust plants, prior alone, {steps} steps: ITAE x {r['itae_ratio'].round(3).tolist()}, limit cycle "
          f"{r['limit_cycle'].round(3).tolist()}, reversals {r['reversals'].tolist()}, tolerated qu {r['qu_tolerated']}, span {r['limits_tolerated']}")


def test_train_actuator_writes_the_file(tmp_path, capsys):
    import os
    from pime_amd import protocols, train
    common = ["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
              "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
              "--break_step", str(64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1"]
    train.main(common + ["--actuator", "--actuator_points", "2", "--log_root", str(tmp_path / "a")])
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "actuator_sweep.npz"]
    assert len(found) == 1
    z = np.load(found[0], allow_pickle=False)
    P_ = 2 + 5 * 2
    assert z["rows"].shape == (P_, 6) and (z["rows"][0] == list(protocols.ACT_OFF)).all() and (z["rows"][-1] == protocols.rig_row()).all()
    np.testing.assert_array_equal(z["rows"], train.actuator_rows(2))
    np.testing.assert_array_equal(z["plants"], protocols.WT_ROBUST_PLANTS)
    assert list(z["metric_names"]) == list(protocols.METRIC_NAMES + protocols.ACT_ROW_NAMES)
    for who in ("agent", "prior"):
        assert z[f"{who}_summary"].shape == (P_, 5, 16, 5)
        for k in ("itae_ratio", "limit_cycle", "reversals"):
            assert z[f"{who}_{k}"].shape == (P_,) and np.isfinite(z[f"{who}_{k}"]).all(), (who, k)
        assert z[f"{who}_itae_ratio"][0] == 1.0
        for k in ("limits", "rate", "deadband", "qu", "qy"):
            assert z[f"{who}_{k}_tolerated"].shape == ()
    assert not A.bits_equal(z["agent_summary"], z["prior_summary"]), "the trained residual is not the prior alone"
    out = capsys.readouterr().out
    assert "limit cycle" in out and "agent clamp" in out and "prior clamp" in out and "tolerated" in out
    import argparse
    from pime_amd import gym_control
    assert train.actuator(argparse.Namespace(env=gym_control.WT_STACKING.format(4)), None, str(tmp_path / "b")) is None
    assert "actuator sweep skipped" in capsys.readouterr().out
