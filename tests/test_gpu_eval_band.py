"""Fused response band (`pime_rollout_eval_band`: the band variants of rollout_eval_kernel and of rollout16_kernel's evaluation
mode, then eval_band_reduce_kernel) against the numpy reference of tests/response_band.py:
  1. on the reference's golden protocol records (float64 state, prior controller): mean, min and max of Y and A at 1e-9 relative
     -- the trajectories agree to 1e-11, the argument of tests/test_gpu_eval_metrics.py;
  2. every served class against the trace of the SAME launch, groups of 32, 32 and 17 lanes and a 32-bin histogram with lanes
     outside on both sides: sums within n * 2^-52 * sum|term| (the bound for n additions in any order), MIN / MAX / counts exact;
  3. ret / trace / metrics bit-equal to pime_rollout_eval_metrics', the same end state, two launches bit-equal, and stats that do
     not depend on ret / trace / hist being asked for;
  4. group shapes 16 .. 2 N on one class per kernel and tiling, and every argument error by name;
  5. a ragged launch of 4 100 lanes on the default tiling with a NaN-poisoned, exactly sized workspace and guard bands;
  6. protocols.step_response_band is one launch and agrees with the step-per-launch fallback;
  7. train.main --robust_test writes response_band.npz beside robust_metrics.npz.
Every comparison against a trace prints the largest used share of its bars.  Shapes, envs and policies are those of
tests/test_gpu_eval_metrics.py (N = 81 at lane offset 8 192, T = 24, SEG = 7, both tilings through PIME_ROLLOUT_NARROW)."""
import os

import numpy as np
import pytest
import torch

import response_band as RB
import stepresponse_metrics as SM
import test_gpu_eval_metrics as EM
from conftest import load_golden
from rollout_replay import DEV

pytestmark = pytest.mark.gpu
N, T, SEG, TAIL = EM.N, EM.T, EM.SEG, EM.TAIL
GROUP = 32                                           # 81 lanes: groups of 32, 32 and 17, the last ending on a one-lane tile
# 24 steps from a reset: the pH lanes are still near their starts (x in [0, 50]: y about 0.8 .. 2), the tank levels start in [0, 10]
HIST = {"ph": (32, 1.0, 1.5), "wt": (32, 2.0, 6.0)}
KINDS = EM.KINDS


def _which(env_name):
    return "ph" if env_name == "PH_V35" else "wt"


def _counts(c):
    return None if c is None else c.cpu().numpy().view(np.uint32)


def _launch(env, fused, env_name, seg_len, group_lanes=GROUP, hist="default", want_trace=True):
    which = _which(env_name)
    env.reset()
    y_first = None if which == "ph" else env.get_field("h2")
    ret, m, stats, counts, tr = env.rollout_eval_band(
        fused[0], fused[1], T, setpoints=EM.SETPOINTS[which] if seg_len else None, seg_len=seg_len, band=EM.BAND[which], tail=TAIL,
        group_lanes=group_lanes, hist=HIST[which] if hist == "default" else hist, want_trace=want_trace)
    torch.cuda.synchronize()
    return dict(ret=ret.cpu().numpy(), metrics=m.cpu().numpy(), stats=stats.cpu().numpy(), hist=_counts(counts),
                trace=None if tr is None else tr.cpu().numpy(), y_first=y_first)


def _records(env, env_name, mode, tr, y_first, seg_len):
    is_ph = env_name == "PH_V35"
    return SM.records_from_trace(tr, is_ph, seg_len, y_last=EM._ph_y_of_x(env, tr[-1, 5], mode) if is_ph else None, y_first=y_first)


def _check_against_own_trace(env, env_name, mode, out, seg_len, group_lanes, hist, tag):
    rec = _records(env, env_name, mode, out["trace"], out["y_first"], seg_len)
    want = RB.reference_band(rec, group_lanes, hist)
    share = RB.check_band(out["stats"], out["hist"], want, tag=tag)
    bit_equal = bool((out["stats"] == want["stats"]).all())
    print(f"\nSHARE band id={tag} groups={[int(c) for c in want['count']]} sums={share:.4f} bit_equal={bit_equal}")
    return rec, want


# ---- 1. golden --------------------------------------------------------------------------------------------------------------
def _compare_golden(b, rec, tag):
    rel = 0.0
    for name, x in (("y", rec["y_after"]), ("action", rec["action"])):
        for stat, ref in (("mean", x.mean(axis=1)), ("min", x.min(axis=1)), ("max", x.max(axis=1))):
            got = b[stat][name][:, 0]
            rel = max(rel, float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))[ref != 0].max(initial=0.0)))
    print(f"\nSHARE golden band id={tag} largest relative difference {rel:.3e} (bar 1e-9)")
    for name, x in (("y", rec["y_after"]), ("action", rec["action"])):
        for stat, ref in (("mean", x.mean(axis=1)), ("min", x.min(axis=1)), ("max", x.max(axis=1))):
            np.testing.assert_allclose(b[stat][name][:, 0], ref, rtol=1e-9, atol=0, err_msg=f"{stat} of {name} ({tag})")


def test_band_of_the_golden_protocols(ph_table_oracle):
    """Float64 state, the prior controller alone, the two golden plants of each env as one group; numpy reduces the REFERENCE's records."""
    import oracle
    from pime_amd import gym_control, protocols
    g = load_golden("ph_stepresponse.npz")
    env = gym_control.make_vec(gym_control.PH_V35, 2, device=DEV, state_mode="f64", seed=0)
    EM._no_stepwise(env)
    b = protocols.step_response_band(env, plants=[g["nominal_params"], g["corner_params"]], band=0.05, tail=10)
    assert list(b["count"]) == [2] and b["hist"] is None and b["mean"]["y"].shape == (250, 1)
    _compare_golden(b, SM.golden_ph_records(g, ph_table_oracle, oracle.ph_zoh), "ph")
    env.close()
    gw = load_golden("wt_stepresponse.npz")
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, 2, device=DEV, state_mode="f64", seed=0, reward_type="distance", noise_scale=0.0)
    EM._no_stepwise(env)
    b = protocols.step_response_band(env, steps=500, plants=[gw["robust1_params"][:3], gw["robust3_params"][:3]], band=2.0, tail=10)
    assert list(b["count"]) == [2] and b["mean"]["y"].shape == (2500, 1)
    _compare_golden(b, SM.golden_wt_records(gw), "wt")
    env.close()


# ---- 2. every served class against its own trace ------------------------------------------------------------------------------
def test_the_classes_are_the_served_shapes():
    from pime_amd import native
    lib = native.lib()
    served = set()
    for env_name in ("PH_V35", "WT_INTEGRATOR", "WT_STACKING1", "WT_STACKING4", "WT_STACKING10"):
        for mode in ("mixed", "f64"):
            env = EM._make_env(env_name, mode)
            for kind, code in KINDS.items():
                for md in ((0,) if kind == "prior" else (64, 128, 256)):
                    level = lib.pime_rollout_eval_supported(env._h, code, md)
                    ws = lib.pime_rollout_eval_band_workspace_bytes(env._h, code, md, T, GROUP)
                    if level:
                        assert level == (2 if env_name.startswith("WT_STACKING") else 1)
                        assert ws == T * 6 * 128 <= T * (8 * N + 128)     # six tiles: 8 bytes per lane and step, one tile of slack
                        served.add((kind, md, env_name, mode))
                    else:
                        assert ws == -1
            env.close()
    assert served == {c[:4] for c in RB.CLASSES}


@pytest.mark.parametrize("case", RB.CLASSES, ids=lambda c: "-".join(str(x) for x in c))
def test_band_against_the_trace_of_the_same_launch(case, monkeypatch):
    kind, md, env_name, mode, tiles = case
    monkeypatch.setenv("PIME_ROLLOUT_NARROW", EM.TILES[tiles])
    seg_len = 0 if env_name.startswith("WT_STACKING") else SEG
    hist = HIST[_which(env_name)]
    env = EM._make_env(env_name, mode)
    fused = EM._policy(kind, env, md)
    EM._no_stepwise(env)
    out = _launch(env, fused, env_name, seg_len)
    assert out["stats"].shape == (T, 16, 3) and out["hist"].shape == (T, 3, 32)
    rec, want = _check_against_own_trace(env, env_name, mode, out, seg_len, GROUP, hist, "-".join(str(x) for x in case))
    assert list(want["count"]) == [32, 32, 17]
    assert (rec["y_after"] < hist[1]).any() and (rec["y_after"] >= hist[2]).any(), "lanes outside the histogram on both sides"
    env.close()


# ---- 3. the metrics call's outputs, and independence from the optional outputs -------------------------------------------------
def _raw_band(env, fused, kind, md, seg_len, which, group_lanes, stats, hist, hist_args, metrics, workspace, ret=None, trace=None):
    import pime_amd.native as nt
    sp = EM.SETPOINTS[which] if seg_len else None
    k = np.ascontiguousarray(np.asarray(fused[1], dtype=np.float64).reshape(-1))
    spa = np.ascontiguousarray(np.asarray(sp if sp else [], dtype=np.float64))
    pk = fused[0]
    code, width, img = (-1, 0, None) if pk is None else (KINDS[kind], md, pk.packed)
    bins, lo, hi = hist_args
    return nt.lib().pime_rollout_eval_band(env._h, code, width, nt.ptr(img), nt.ptr(k), T, seg_len, nt.ptr(spa) if spa.size else None,
                                           int(spa.size), EM.BAND[which], TAIL, nt.ptr(ret), nt.ptr(trace), nt.ptr(metrics), group_lanes,
                                           nt.ptr(stats), nt.ptr(hist), bins, lo, hi, nt.ptr(workspace), env._stream())


@pytest.mark.parametrize("kind,md,env_name,mode", [("modular", 128, "WT_INTEGRATOR", "mixed"), ("plain", 256, "PH_V35", "mixed"),
                                                   ("td3", 256, "WT_STACKING4", "mixed"), ("prior", 0, "PH_V35", "f64"),
                                                   ("sac", 64, "WT_INTEGRATOR", "f64")])
def test_the_metrics_call_outputs_are_unchanged_and_the_stats_do_not_need_the_optional_outputs(kind, md, env_name, mode):
    import pime_amd.native as nt
    which = _which(env_name)
    seg_len = 0 if env_name.startswith("WT_STACKING") else SEG
    envs = [EM._make_env(env_name, mode) for _ in range(4)]
    fused = [EM._policy(kind, e, md) for e in envs]
    ret0, m0, tr0, _ = EM._launch(envs[0], fused[0], env_name, seg_len)              # pime_rollout_eval_metrics on a twin
    out1 = _launch(envs[1], fused[1], env_name, seg_len)
    out2 = _launch(envs[2], fused[2], env_name, seg_len)
    for key, ref in (("ret", ret0), ("trace", tr0), ("metrics", m0)):
        np.testing.assert_array_equal(out1[key], ref, err_msg=key)
    for key in ("ret", "trace", "metrics", "stats", "hist"):                         # two launches from equal state: the same bits
        np.testing.assert_array_equal(out1[key].view(np.uint64 if out1[key].dtype == np.float64 else out1[key].dtype),
                                      out2[key].view(np.uint64 if out2[key].dtype == np.float64 else out2[key].dtype), err_msg=key)
    # no ret, no trace, no histogram: the library directly
    envs[3].reset()
    n_seg = m0.shape[0]
    m3 = torch.full((n_seg, 8, N), float("nan"), dtype=torch.float64, device=DEV)
    s3 = torch.full((T, 16, 3), float("nan"), dtype=torch.float64, device=DEV)
    code, width = (-1, 0) if fused[3][0] is None else (KINDS[kind], md)
    ws = torch.full((nt.lib().pime_rollout_eval_band_workspace_bytes(envs[3]._h, code, width, T, GROUP) // 8,), float("nan"),
                    dtype=torch.float64, device=DEV)
    nt.check(_raw_band(envs[3], fused[3], kind, md, seg_len, which, GROUP, s3, None, (0, 0.0, 0.0), m3, ws))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(m3.cpu().numpy(), m0)
    np.testing.assert_array_equal(s3.cpu().numpy().view(np.uint64), out1["stats"].view(np.uint64))
    for f in (("x", "I") if which == "ph" else (("h1", "h2") if seg_len == 0 else ("h1", "h2", "I"))):   # (Stacking has no integrator)
        for e in envs[1:]:
            np.testing.assert_array_equal(envs[0].get_field(f), e.get_field(f), err_msg=f)
    for e in envs:
        e.close()


# ---- 4. group shapes and argument errors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,md,env_name,mode,tiles", [("modular", 128, "WT_INTEGRATOR", "mixed", "quad"),
                                                         ("modular", 128, "WT_INTEGRATOR", "mixed", "narrow"),
                                                         ("plain", 256, "PH_V35", "mixed", "quad"), ("plain", 256, "PH_V35", "mixed", "narrow")])
def test_group_shapes(kind, md, env_name, mode, tiles, monkeypatch):
    monkeypatch.setenv("PIME_ROLLOUT_NARROW", EM.TILES[tiles])
    env = EM._make_env(env_name, mode)
    fused = EM._policy(kind, env, md)
    hist = HIST[_which(env_name)]
    for group_lanes, sizes in ((16, [16] * 5 + [1]), (48, [48, 33]), (64, [64, 17]), (96, [81]), (N, [81]), (2 * N, [81])):
        out = _launch(env, fused, env_name, SEG, group_lanes=group_lanes)
        _, want = _check_against_own_trace(env, env_name, mode, out, SEG, group_lanes, hist, f"{kind}-{md}-{env_name}-{tiles}-group{group_lanes}")
        assert list(want["count"]) == sizes and out["stats"].shape == (T, 16, len(sizes))
    env.close()


def test_each_argument_error_names_its_argument():
    import pime_amd.native as nt
    env = EM._make_env("WT_INTEGRATOR", "mixed")
    fused = EM._policy("modular", env, 128)
    env.reset()
    m = torch.zeros((4, 8, N), dtype=torch.float64, device=DEV)
    s = torch.zeros((T, 16, 6), dtype=torch.float64, device=DEV)
    h = torch.zeros((T, 6, 256), dtype=torch.int32, device=DEV)
    ws = torch.zeros((T * 6 * 16,), dtype=torch.float64, device=DEV)
    ok = dict(group_lanes=GROUP, stats=s, hist=h, hist_args=(32, 2.0, 6.0), metrics=m, workspace=ws)
    nan = float("nan")
    for change, word in ((dict(group_lanes=0), "group_lanes"), (dict(group_lanes=-16), "group_lanes"), (dict(group_lanes=8), "group_lanes"),
                         (dict(group_lanes=24), "group_lanes"), (dict(stats=None), "stats"), (dict(metrics=None), "metrics"),
                         (dict(workspace=None), "workspace"), (dict(hist_args=(0, 2.0, 6.0)), "bins"), (dict(hist_args=(257, 2.0, 6.0)), "bins"),
                         (dict(hist_args=(32, 6.0, 6.0)), "lo"), (dict(hist_args=(32, 7.0, 6.0)), "lo"), (dict(hist_args=(32, nan, 6.0)), "lo"),
                         (dict(hist_args=(32, 2.0, nan)), "hi")):
        rc = _raw_band(env, fused, "modular", 128, SEG, "wt", **dict(ok, **change))
        assert rc == -1, (change, rc)     # PIME_ERR_ARG
        assert word in nt.last_error() and "pime_rollout_eval_band" in nt.last_error(), (change, nt.last_error())
    for gl in (0, -16, 8, 24):
        assert nt.lib().pime_rollout_eval_band_workspace_bytes(env._h, KINDS["modular"], 128, T, gl) == -1
        assert "group_lanes" in nt.last_error()
        with pytest.raises(nt.PimeError, match="group_lanes"):
            env.rollout_eval_band(fused[0], fused[1], T, setpoints=EM.SETPOINTS["wt"], seg_len=SEG, group_lanes=gl)
    nt.check(_raw_band(env, fused, "modular", 128, SEG, "wt", **ok))     # and the unchanged arguments are served
    torch.cuda.synchronize()
    env.close()


# ---- 5. lane count ------------------------------------------------------------------------------------------------------------
def test_a_ragged_launch_on_the_default_tiling(monkeypatch):
    """4 100 lanes: past the QUAD threshold, the last workgroup holds 4 lanes and 60 idle ones; groups of 1 024 lanes, the last of 4.
    The workspace is exactly the size the query returns, poisoned with NaN; stats, hist and workspace sit in front of guard bands."""
    import pime_amd.native as nt
    monkeypatch.delenv("PIME_ROLLOUT_NARROW", raising=False)
    n, gl, G, (bins, lo, hi) = 4100, 1024, 5, HIST["wt"]
    env = EM._make_env("WT_INTEGRATOR", "mixed", n=n)
    fused = EM._policy("modular", env, 128)
    env.reset()
    y_first = env.get_field("h2")
    ws_bytes = nt.lib().pime_rollout_eval_band_workspace_bytes(env._h, KINDS["modular"], 128, T, gl)
    assert ws_bytes % 8 == 0 and 0 < ws_bytes <= T * (8 * n + 128 * G), "8 bytes per lane and step, one tile of slack per group"
    ws = torch.full((ws_bytes // 8 + 64,), float("nan"), dtype=torch.float64, device=DEV)
    ws[ws_bytes // 8:] = -777.0
    stats = torch.full((T * 16 * G + 64,), -777.0, dtype=torch.float64, device=DEV)
    hist = torch.full((T * G * bins + 64,), 0x7777, dtype=torch.int32, device=DEV)
    m = torch.empty((4, 8, n), dtype=torch.float64, device=DEV)
    tr = torch.empty((T, 6, n), dtype=torch.float64, device=DEV)
    nt.check(_raw_band(env, fused, "modular", 128, SEG, "wt", gl, stats, hist, (bins, lo, hi), m, ws, trace=tr))
    torch.cuda.synchronize()
    ws, stats, hist = ws.cpu().numpy(), stats.cpu().numpy(), hist.cpu().numpy()
    assert (ws[ws_bytes // 8:] == -777.0).all(), "a store past the workspace"
    assert (stats[T * 16 * G:] == -777.0).all() and (hist[T * G * bins:] == 0x7777).all(), "a store past stats / hist"
    out = dict(stats=stats[:T * 16 * G].reshape(T, 16, G), hist=hist[:T * G * bins].reshape(T, G, bins).view(np.uint32),
               trace=tr.cpu().numpy(), y_first=y_first)
    _, want = _check_against_own_trace(env, "WT_INTEGRATOR", "mixed", out, SEG, gl, (bins, lo, hi), "modular-128-WT_INTEGRATOR-4100")
    assert list(want["count"]) == [1024] * 4 + [4]
    env.close()


# ---- 6. protocols -------------------------------------------------------------------------------------------------------------
def test_step_response_band_is_one_launch_and_agrees_with_the_fallback():
    from pime_amd import gym_control, protocols
    kw = dict(device=DEV, state_mode="f64", seed=3, reward_type="distance")
    sp, steps, n = (3.0, 6.0, 4.0), 40, 40
    rng = np.random.default_rng(11)
    plants = np.stack([rng.uniform(0.0015, 0.0024, n), rng.uniform(0.0015, 0.0024, n), rng.uniform(0.07, 0.17, n)], axis=1)
    hist = (32, -1.0, 11.0)          # bin width 0.375: neither the empty tanks nor a set-point sit on an edge
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, n, **kw)
    EM._no_stepwise(env)
    calls = []
    orig = env.rollout_eval_band
    env.rollout_eval_band = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    fast = protocols.step_response_band(env, setpoints=sp, steps=steps, plants=plants, group_lanes=16, hist=hist)
    assert calls == [1]
    env.close()
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, n, **kw)
    slow = protocols.step_response_band(env, policy=protocols._prior(env), setpoints=sp, steps=steps, plants=plants, group_lanes=16, hist=hist)
    env.close()
    assert list(fast["count"]) == list(slow["count"]) == [16, 16, 8]
    np.testing.assert_array_equal(fast["edges"], np.linspace(-1.0, 11.0, 33))
    np.testing.assert_array_equal(fast["edges"], slow["edges"])
    # the two paths' trajectories agree to 1e-11 (test_gpu_facade.py::test_batched_step_response_protocols), values <= 10: 1e-9
    # relative for the output, and 1e-9 absolute beside it for the signals that pass through zero
    for name in protocols.BAND_SIGNALS:
        for stat in ("mean", "min", "max"):
            assert fast[stat][name].shape == (len(sp) * steps, 3)
            np.testing.assert_allclose(fast[stat][name], slow[stat][name], rtol=1e-9, atol=1e-9 if name != "y" else 0, err_msg=f"{stat} {name}")
        # std = sqrt(sumsq / n - mean^2): the difference of two numbers each good to 1e-9 relative -- compared as a variance,
        # with 4e-9 of what is subtracted (at the first step every lane takes the same action: the variance is rounding noise)
        second = fast["std"][name] ** 2 + fast["mean"][name] ** 2
        assert (np.abs(fast["std"][name] ** 2 - slow["std"][name] ** 2) <= 4e-9 * second + 1e-300).all(), f"std {name}"
    np.testing.assert_array_equal(fast["hist"], slow["hist"])
    assert (fast["hist"].sum(axis=2) == fast["count"][None, :]).all()
    for name in SM.ROWS:
        np.testing.assert_allclose(fast["metrics"][name], slow["metrics"][name], rtol=1e-9, atol=1e-9 if name == "overshoot" else 0, err_msg=name)
    q = protocols.band_quantiles(fast["hist"], fast["edges"], [0.25, 0.5, 0.75])
    assert q.shape == (len(sp) * steps, 3, 3) and (np.diff(q, axis=2) >= 0).all()
    assert (q[:, :, 0] >= fast["min"]["y"] - 0.375).all() and (q[:, :, 2] <= fast["max"]["y"] + 0.375).all()


# ---- 7. train.main ------------------------------------------------------------------------------------------------------------
def test_train_robust_test_writes_the_band(tmp_path):
    from pime_amd import protocols, train
    train.main(["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
                "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
                "--break_step", str(64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1", "--robust_test",
                "--log_root", str(tmp_path)])
    found = {name: [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == name]
             for name in ("robust_metrics.npz", "response_band.npz")}
    assert len(found["robust_metrics.npz"]) == 1 and len(found["response_band.npz"]) == 1
    assert os.path.dirname(found["robust_metrics.npz"][0]) == os.path.dirname(found["response_band.npz"][0])
    z = np.load(found["response_band.npz"][0], allow_pickle=False)
    assert sorted(z.files) == sorted(["signals", "count", "hist", "edges", "quantile_levels", "quantiles", "setpoints", "steps",
                                      "mean", "std", "min", "max"])
    steps = 5 * 500
    assert tuple(z["signals"]) == tuple(protocols.BAND_SIGNALS) and int(z["steps"]) == 500
    for k in ("mean", "std", "min", "max"):
        assert z[k].shape == (4, steps) and np.isfinite(z[k]).all(), k
    tol = 1e-12 * np.maximum(np.abs(z["max"]), 1.0)      # (a mean of equal values may round an ulp past them)
    assert (z["min"] - tol <= z["mean"]).all() and (z["mean"] <= z["max"] + tol).all() and (z["std"] >= 0).all()
    assert list(z["count"]) == [train.BAND_LANES] and z["hist"].shape == (steps, train.BAND_BINS)
    assert (z["hist"].sum(axis=1) == train.BAND_LANES).all()
    assert z["edges"].shape == (train.BAND_BINS + 1,) and z["quantiles"].shape == (steps, 5) and np.isfinite(z["quantiles"]).all()
    np.testing.assert_array_equal(z["setpoints"], np.asarray(protocols.WT_SETPOINTS))
    assert z["std"][0, 100] > 0 and z["max"][0, 100] > z["min"][0, 100], "an ensemble of different plants"
