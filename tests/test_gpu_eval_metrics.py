"""Fused step-response metrics (`pime_rollout_eval_metrics`; csrc/eval_metrics.hpp in rollout_eval_kernel and in the METRICS variant
of rollout16_kernel's evaluation mode) against the numpy reference of tests/stepresponse_metrics.py:
  1. on the reference's golden protocol records (float64 state, prior controller): continuous rows 1e-9 relative -- the
     trajectories agree to 1e-11, 500 terms of size <= 10 give <= 1e-10 -- the settling step exactly;
  2. every served class against the trace of the SAME launch: a sum of n terms within n * 2^-52 * sum|term| (the bound for n
     sequential double additions; the kernel adds the same terms in the same order, so bit equality is expected), overshoot and
     settling step exactly;
  3. the launch leaves ret / trace bit-equal to pime_rollout_eval's, and metrics do not depend on ret / trace being asked for;
  4. a ragged launch of 4 100 lanes on the default tiling;
  5. protocols.step_response_metrics / robust_grid are one launch, and agree with the step-per-launch fallback;
  6. train.main --robust_test writes robust_metrics.npz.
Every comparison prints the largest used share of its bar."""
import os

import numpy as np
import pytest
import torch

import stepresponse_metrics as SM
from conftest import load_golden
from rollout_replay import DEV, make_agent

pytestmark = pytest.mark.gpu
N, OFFSET, SEED = 81, 8192, 6
T, SEG = 24, 7                      # three whole segments and one of three steps
BAND = {"ph": 1.0, "wt": 2.0}
TAIL = 5                            # longer than the cut segment: its window is min(tail, L) = 3
SETPOINTS = {"ph": (10., 6., 3., 8.), "wt": (3., 6., 9., 4.)}
TILES = {"quad": "2", "narrow": "1"}


def _no_stepwise(env):
    def boom(*a, **k):
        raise AssertionError("the metrics fell back to step-per-launch kernels")
    env.step = env.step_residual = boom


def _make_env(env_name, state_mode, n=N, **extra):
    from pime_amd import gym_control
    if env_name.startswith("WT_STACKING"):
        env_id = gym_control.WT_STACKING.format(int(env_name[len("WT_STACKING"):]))
    else:
        env_id = getattr(gym_control, env_name)
    kw = dict(max_episode_steps=64) if env_name == "PH_V35" else dict(reward_type="distance", max_step=64)
    kw.update(extra)
    return gym_control.make_vec(env_id, n, device=DEV, state_mode=state_mode, seed=SEED, env_offset=OFFSET, **kw)


def _policy(kind, env, md):
    """(packed actor or None, priorK) of a freshly initialised agent with a non-trivial output layer."""
    if kind == "prior":
        return None, -env.K
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
    assert fused is not None, "the fused evaluation kernel must serve this configuration"
    assert fused[0].md == md
    return fused


def _ph_y_of_x(env, x, state_mode):
    """The traced x through the titration table, in the state's precision (the mixed-mode table is the float32 rounding)."""
    import pime_amd.native as nt
    table = nt.ph_table_build()
    if state_mode == "mixed":
        table = table.astype(np.float32).astype(np.float64)
    return SM.ph_table_lookup(table, env.get_field("C"), x)


def _check_against_own_trace(env, env_name, state_mode, metrics, tr, y_first, seg_len, tag):
    is_ph = env_name == "PH_V35"
    which = "ph" if is_ph else "wt"
    rec = SM.records_from_trace(tr, is_ph, seg_len, y_last=_ph_y_of_x(env, tr[-1, 5], state_mode) if is_ph else None, y_first=y_first)
    want, bars = SM.reference_metrics(rec, BAND[which], TAIL)
    assert metrics.shape == want.shape, (metrics.shape, want.shape)
    assert np.isfinite(metrics).all()
    share, bit_equal = 0.0, True
    for j, name in enumerate(SM.ROWS):
        got, ref = metrics[:, j], want[:, j]
        if j in SM.EXACT_ROWS:
            continue
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = max(share, float(np.where(err > 0, err / bars[:, j], 0.0).max()))
        bit_equal &= bool((got == ref).all())
    print(f"\nSHARE metrics id={tag} sums={share:.4f} bit_equal={bit_equal}")
    for j, name in enumerate(SM.ROWS):
        got, ref = metrics[:, j], want[:, j]
        if j in SM.EXACT_ROWS:
            np.testing.assert_array_equal(got, ref, err_msg=f"{name} ({tag})")
        else:
            assert (np.abs(got - ref) <= bars[:, j]).all(), f"{name} ({tag}): {np.abs(got - ref).max():.3e} over the bar"
    return want


def _launch(env, fused, env_name, seg_len, want_trace=True, ret=None):
    which = "ph" if env_name == "PH_V35" else "wt"
    env.reset()
    y_first = None if which == "ph" else env.get_field("h2")
    ret, m, tr = env.rollout_eval_metrics(fused[0], fused[1], T, setpoints=SETPOINTS[which] if seg_len else None, seg_len=seg_len,
                                          band=BAND[which], tail=TAIL, want_trace=want_trace, ret=ret)
    torch.cuda.synchronize()
    return ret.cpu().numpy(), m.cpu().numpy(), None if tr is None else tr.cpu().numpy(), y_first


# ---- 1. golden --------------------------------------------------------------------------------------------------------------
def _compare_golden(metrics, want, tag):
    rel = 0.0
    for j, name in enumerate(SM.ROWS):
        got, ref = metrics[:, j], want[:, j]
        if j == SM.SETTLING:
            np.testing.assert_array_equal(got, ref, err_msg=name)
            continue
        scale = np.maximum(np.abs(ref), 1e-300)
        rel = max(rel, float((np.abs(got - ref) / scale)[ref != 0].max(initial=0.0)))
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=0, err_msg=name)
    print(f"\nSHARE golden id={tag} largest relative difference {rel:.3e} (bar 1e-9)")


def test_metrics_of_the_golden_protocols(ph_table_oracle):
    """Float64 state, the prior controller alone, the protocols of test_gpu_eval_fused.py; the reference reduces the REFERENCE's
    records (bands 0.05 / 2.0: no recorded |e| within 6e-5 of them, tests/test_stepresponse_metrics_cpu.py)."""
    import oracle
    from pime_amd import gym_control, protocols
    g = load_golden("ph_stepresponse.npz")
    env = gym_control.make_vec(gym_control.PH_V35, 2, device=DEV, state_mode="f64", seed=0)
    _no_stepwise(env)
    m = protocols.step_response_metrics(env, plants=[g["nominal_params"], g["corner_params"]], band=0.05, tail=10)
    want = SM.reference_metrics(SM.golden_ph_records(g, ph_table_oracle, oracle.ph_zoh), 0.05, 10)[0]
    _compare_golden(np.stack([m[k] for k in SM.ROWS], axis=1), want, "ph")
    env.close()
    gw = load_golden("wt_stepresponse.npz")
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, 2, device=DEV, state_mode="f64", seed=0, reward_type="distance", noise_scale=0.0)
    _no_stepwise(env)
    m = protocols.step_response_metrics(env, steps=500, plants=[gw["robust1_params"][:3], gw["robust3_params"][:3]], band=2.0, tail=10)
    want = SM.reference_metrics(SM.golden_wt_records(gw), 2.0, 10)[0]
    _compare_golden(np.stack([m[k] for k in SM.ROWS], axis=1), want, "wt")
    env.close()


# ---- 2. every served class against its own trace ------------------------------------------------------------------------------
CASES = []
for _env in ("PH_V35", "WT_INTEGRATOR"):
    CASES += [("prior", 0, _env, mode, "narrow") for mode in ("mixed", "f64")]
    for _t in ("quad", "narrow"):
        CASES += [(k, md, _env, "mixed", _t) for k in ("modular", "plain", "td3") for md in (64, 128, 256)]
        CASES += [("sac", md, _env, "mixed", _t) for md in (64, 128)]
        CASES += [(k, md, _env, "f64", _t) for k in ("modular", "plain", "sac", "td3") for md in (64, 128)]
CASES += [(k, 256, f"WT_STACKING{s}", "mixed", _t) for s in (1, 4, 10) for k in ("plain", "td3") for _t in ("quad", "narrow")]
KINDS = {"prior": -1, "td3": 0, "plain": 1, "modular": 2, "sac": 3}


def test_the_cases_are_the_served_shapes():
    from pime_amd import native
    lib = native.lib()
    served = set()
    for env_name in ("PH_V35", "WT_INTEGRATOR", "WT_STACKING1", "WT_STACKING4", "WT_STACKING10"):
        for mode in ("mixed", "f64"):
            env = _make_env(env_name, mode)
            for kind, code in KINDS.items():
                for md in ((0,) if kind == "prior" else (64, 128, 256)):
                    level = lib.pime_rollout_eval_supported(env._h, code, md)
                    if level:
                        assert level == (2 if env_name.startswith("WT_STACKING") else 1)
                        served.add((kind, md, env_name, mode))
            env.close()
    assert served == {c[:4] for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_metrics_against_the_trace_of_the_same_launch(case, monkeypatch):
    kind, md, env_name, mode, tiles = case
    monkeypatch.setenv("PIME_ROLLOUT_NARROW", TILES[tiles])
    seg_len = 0 if env_name.startswith("WT_STACKING") else SEG
    env = _make_env(env_name, mode)        # (the tank's process noise is on: noise_scale is the registered one)
    fused = _policy(kind, env, md)
    _no_stepwise(env)
    ret, m, tr, y_first = _launch(env, fused, env_name, seg_len)
    assert m.shape == ((4 if seg_len else 1), 8, N)
    want = _check_against_own_trace(env, env_name, mode, m, tr, y_first, seg_len, "-".join(str(x) for x in case))
    if seg_len == 0:
        np.testing.assert_array_equal(m[0, SM.RETURN], ret)                   # one segment: the same sum as ret
    np.testing.assert_allclose(m[:, SM.RETURN].sum(0), ret, rtol=1e-13)     # (per-segment sums re-added: a different order)
    if kind != "prior":
        assert float(m[:, SM.ACTION_VAR].min()) > 0
    env.close()


# ---- 3. no effect on what exists ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,md,env_name,mode", [("modular", 128, "WT_INTEGRATOR", "mixed"), ("plain", 256, "PH_V35", "mixed"),
                                                   ("td3", 256, "WT_STACKING4", "mixed"), ("prior", 0, "PH_V35", "f64"),
                                                   ("sac", 64, "WT_INTEGRATOR", "f64")])
def test_ret_and_trace_are_those_of_the_plain_evaluation_and_metrics_do_not_need_them(kind, md, env_name, mode):
    which = "ph" if env_name == "PH_V35" else "wt"
    seg_len = 0 if env_name.startswith("WT_STACKING") else SEG
    sp = SETPOINTS[which] if seg_len else None
    envs = [_make_env(env_name, mode) for _ in range(3)]
    fused = [_policy(kind, e, md) for e in envs]
    envs[0].reset()
    ret0, tr0 = envs[0].rollout_eval(fused[0][0], fused[0][1], T, setpoints=sp, seg_len=seg_len, want_trace=True)
    ret1, m1, tr1, _ = _launch(envs[1], fused[1], env_name, seg_len)
    np.testing.assert_array_equal(ret0.cpu().numpy(), ret1)
    np.testing.assert_array_equal(tr0.cpu().numpy(), tr1)
    # metrics only: no ret, no trace (the binding always passes a ret buffer: call the library)
    import pime_amd.native as nt
    envs[2].reset()
    m2 = torch.full((m1.shape[0], 8, N), float("nan"), dtype=torch.float64, device=DEV)
    k = np.ascontiguousarray(np.asarray(fused[2][1], dtype=np.float64).reshape(-1))
    spa = np.ascontiguousarray(np.asarray(sp if sp else [], dtype=np.float64))
    pk = fused[2][0]
    code, width, img = (-1, 0, None) if pk is None else (KINDS[kind], md, pk.packed)
    nt.check(nt.lib().pime_rollout_eval_metrics(envs[2]._h, code, width, nt.ptr(img), nt.ptr(k), T, seg_len, nt.ptr(spa) if spa.size else None,
                                                int(spa.size), BAND[which], TAIL, None, None, nt.ptr(m2), envs[2]._stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(m2.cpu().numpy(), m1)
    for f in (("x", "I") if which == "ph" else (("h1", "h2") if seg_len == 0 else ("h1", "h2", "I"))):   # (Stacking has no integrator)   # and the lanes end where the plain evaluation leaves them
        np.testing.assert_array_equal(envs[0].get_field(f), envs[1].get_field(f))
    for e in envs:
        e.close()


# ---- 4. lane count ------------------------------------------------------------------------------------------------------------
def test_a_ragged_launch_on_the_default_tiling(monkeypatch):
    """4 100 lanes: past the QUAD threshold (16-lane tiles, one per wave), the last workgroup holds 4 lanes and 60 idle ones."""
    monkeypatch.delenv("PIME_ROLLOUT_NARROW", raising=False)
    n = 4100
    env = _make_env("WT_INTEGRATOR", "mixed", n=n)
    fused = _policy("modular", env, 128)
    env.reset()
    y_first = env.get_field("h2")
    guard = torch.full((4 * 8 * n + 64,), -777.0, dtype=torch.float64, device=DEV)    # the metrics sit in front of a guard band
    ret, m, tr = env.rollout_eval_metrics(fused[0], fused[1], T, setpoints=SETPOINTS["wt"], seg_len=SEG, band=BAND["wt"], tail=TAIL, want_trace=True)
    k = np.ascontiguousarray(np.asarray(fused[1], dtype=np.float64).reshape(-1))
    env2 = _make_env("WT_INTEGRATOR", "mixed", n=n)
    fused2 = _policy("modular", env2, 128)
    env2.reset()
    import pime_amd.native as nt
    spa = np.asarray(SETPOINTS["wt"], dtype=np.float64)
    nt.check(nt.lib().pime_rollout_eval_metrics(env2._h, KINDS["modular"], 128, nt.ptr(fused2[0].packed), nt.ptr(k), T, SEG, nt.ptr(spa), 4,
                                                BAND["wt"], TAIL, None, None, nt.ptr(guard), env2._stream()))
    torch.cuda.synchronize()
    m, tr, guard = m.cpu().numpy(), tr.cpu().numpy(), guard.cpu().numpy()
    assert (guard[4 * 8 * n:] == -777.0).all(), "a store past the last lane"
    np.testing.assert_array_equal(guard[:4 * 8 * n].reshape(4, 8, n), m)
    _check_against_own_trace(env, "WT_INTEGRATOR", "mixed", m, tr, y_first, SEG, "modular-128-WT_INTEGRATOR-4100")
    env.close(); env2.close()


# ---- 5. protocols -------------------------------------------------------------------------------------------------------------
def test_robust_grid_is_one_launch_and_equals_the_same_plants_lane_for_lane_and_the_fallback():
    from collections import OrderedDict
    from pime_amd import gym_control, protocols
    axes = OrderedDict(a1=[0.0019, 0.0022, 0.0024], a2=[0.0015, 0.0019], Kp=[0.07, 0.12])
    kw = dict(device=DEV, state_mode="f64", seed=3, reward_type="distance")
    sp, steps = (3.0, 6.0, 4.0), 40
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, 12, **kw)
    _no_stepwise(env)
    calls = []
    orig = env.rollout_eval_metrics
    env.rollout_eval_metrics = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    grid, got_axes = protocols.robust_grid(env, axes, setpoints=sp, steps=steps)
    assert calls == [1] and list(got_axes) == ["a1", "a2", "Kp"]
    env.close()
    plants = np.array([(a1, a2, kp) for a1 in axes["a1"] for a2 in axes["a2"] for kp in axes["Kp"]])     # C order
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, 12, **kw)
    _no_stepwise(env)
    flat = protocols.step_response_metrics(env, setpoints=sp, steps=steps, plants=plants)
    env.close()
    assert tuple(grid) == SM.ROWS
    for name in SM.ROWS:
        assert grid[name].shape == (3, 3, 2, 2)
        np.testing.assert_array_equal(grid[name].reshape(3, 12), flat[name], err_msg=name)
    assert len(np.unique(flat["iae"][0])) == 12, "twelve different plants"
    with pytest.raises(ValueError):
        protocols.robust_grid(env, OrderedDict(a1=[0.002], a2=[0.002]), setpoints=sp, steps=steps)
    # an arbitrary policy callable equal to the prior controller: the step-per-launch loop + metrics_from_records.  The two
    # paths' trajectories agree to 1e-11 (test_gpu_facade.py::test_batched_step_response_protocols): 40 terms <= 10 -> 1e-9 relative
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, 12, **kw)
    slow = protocols.step_response_metrics(env, policy=protocols._prior(env), setpoints=sp, steps=steps, plants=plants)
    env.close()
    for j, name in enumerate(SM.ROWS):
        if j == SM.SETTLING:
            np.testing.assert_array_equal(slow[name], flat[name], err_msg=name)
        else:
            np.testing.assert_allclose(slow[name], flat[name], rtol=1e-9, atol=1e-9 if j == SM.OVERSHOOT else 0, err_msg=name)


def test_ph_grid_is_one_launch():
    from collections import OrderedDict
    from pime_amd import gym_control, protocols
    env = gym_control.make_vec(gym_control.PH_V35, 6, device=DEV, state_mode="mixed", seed=0)
    _no_stepwise(env)
    grid, _ = protocols.robust_grid(env, OrderedDict(qww_V=[0.005, 0.01, 0.015], qc_V=[0.0015, 0.0025]))
    assert grid["iae"].shape == (5, 3, 2) and all(np.isfinite(v).all() for v in grid.values())
    assert (grid["settling_step"] <= 50).all() and (grid["overshoot"] >= 0).all()
    env.close()


# ---- 6. train.main ------------------------------------------------------------------------------------------------------------
def test_train_robust_test_writes_the_metrics(tmp_path):
    from pime_amd import protocols, train
    train.main(["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
                "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
                "--break_step", str(64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1", "--robust_test",
                "--log_root", str(tmp_path)])
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "robust_metrics.npz"]
    assert len(found) == 1
    z = np.load(found[0], allow_pickle=False)
    assert z["metrics"].shape == (3, 5, 8) and np.isfinite(z["metrics"]).all()
    np.testing.assert_array_equal(z["plants"], np.asarray(protocols.WT_ROBUST_PLANTS))
    np.testing.assert_array_equal(z["setpoints"], np.asarray(protocols.WT_SETPOINTS))
    assert float(z["band"]) == 0.05 and int(z["tail"]) == 10 and int(z["steps"]) == 500
    assert (z["metrics"][:, :, SM.SETTLING] <= 500).all() and (z["metrics"][:, :, SM.IAE] > 0).all()
