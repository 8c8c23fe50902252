"""Fused replay of recorded runs over a plant grid (`pime_env_replay_error`, csrc/replay_error.hip) on the device, held to the
oracle-based checker of tests/replay_error.py (vetted in tests/test_replay_error_cpu.py) and to the host build of the same lane
function:
  1. every served class -- {pH, tank} x {f64, mixed} x the served modes x {state0 given, hidden} for pH -- on 81 lanes of a handle
     with a lane offset, E = 3, T = 24, skip 0 and 5, and one record past each time limit (pH T = 70, tank T = 230): sim against the
     oracle (1e-12 in f64; mixed tank levels 2e-5 against one oracle step from the launch's own state; pH the oracle's titration
     cell on every lane and step), err bit-equal to the numpy reduction of the launch's own sim, err without sim bit-equal to err
     with it, and in f64 everything bit-equal to the host library;
  2. the launch-by-launch route (pime_env_step with zero injected noise, levels read back after every step) bit-equal to sim;
  3. the handle is untouched: every field bit-equal before and after, and the next pime_env_step equals a clone's that never replayed;
  4. lane counts 1, 63, 65, 257 and 4 100 with 1 and 5 records: every lane bit-equal to the same plant in the 81-lane run, every
     word of NaN-poisoned err / sim written, nothing written past them;
  5. every argument error returns PIME_ERR_ARG and leaves err untouched; MIXED16 and Stacking handles are refused;
  6. captured in a torch.cuda.graph and replayed twice: bit-equal to the eager call;
  7. protocols.identify_plants / ensemble_ranges and train.py --identify find the plant the records came from.
Every comparison prints the largest used share of its bar."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import replay_error as R
from rollout_replay import DEV

pytestmark = pytest.mark.gpu
N, OFFSET, SEED = 81, 8192, 6
E, T = 3, 24
_CACHE = {}


def _grids(table):
    """The plants and the records of tests/test_replay_error_cpu.py (generated once by the oracle, never changed)."""
    if "grids" not in _CACHE:
        out = {}
        for kind, axes in (("wt", R.WT_AXES), ("ph", R.PH_AXES)):
            plants = R.grid_plants(axes)
            true = R.true_lane(kind)
            out[kind] = dict(plants=plants, true=true, axes=axes, rec=R.make_records(kind, plants[true], E, T, 7, table),
                             long=R.make_records(kind, plants[true], 1, 70 if kind == "ph" else 230, 11, table))
        _CACHE["grids"] = out
    return _CACHE["grids"]


def _records(g, kind, variant, which="rec"):
    rec = dict(g[kind][which])
    if variant == "hidden":
        rec.pop("state0")
    return rec


def _make_env(kind, state_mode, plants, n=None, **extra):
    """A handle whose lanes hold `plants` (cycled to n lanes); never reset, never stepped."""
    from pime_amd import gym_control
    n = len(plants) if n is None else n
    name = gym_control.PH_V35 if kind == "ph" else gym_control.WT_INTEGRATOR
    kw = dict(reward_type="distance") if kind == "wt" else {}
    kw.update(extra)
    env = gym_control.make_vec(name, n, device=DEV, state_mode=state_mode, seed=SEED, env_offset=OFFSET, **kw)
    p = np.asarray(plants, dtype=np.float64)[np.arange(n) % len(plants)]
    if kind == "ph":
        env.set_params(p[:, 0], p[:, 1])
    else:
        env.reset_changable_parameters(p[:, 0], p[:, 1], p[:, 2])
    return env


def _held_plants(env, kind):
    """The plants as the handle holds them (mixed tank: rounded to float32)."""
    return np.stack(env.get_changable_parameters(), axis=1)


def _replay(env, rec, mode, skip, want_sim=True):
    err, sim = env.replay_error(rec, mode=mode, skip=skip, want_sim=want_sim)
    torch.cuda.synchronize()
    return err.cpu().numpy(), None if sim is None else sim.cpu().numpy()


# ---- 1. every served class ----------------------------------------------------------------------------------------------------
CLASSES = [("wt", sm, mode, "given") for sm in ("f64", "mixed") for mode in ("simulate", "predict")] + \
          [("ph", sm, "simulate", variant) for sm in ("f64", "mixed") for variant in ("given", "hidden")]
CASES = [c + ("rec", skip) for c in CLASSES for skip in (0, 5)] + [c + ("long", 5) for c in CLASSES if c[2] == "simulate" and c[3] == "given"]


def test_the_cases_are_the_served_classes():
    from pime_amd import gym_control, native
    served = set()
    for kind, name, kw in (("ph", gym_control.PH_V35, {}), ("wt", gym_control.WT_INTEGRATOR, {}),
                           ("stacking", gym_control.WT_STACKING.format(4), {})):
        for sm in ("f64", "mixed", "mixed16"):
            env = gym_control.make_vec(name, 4, device=DEV, state_mode=sm, seed=SEED, **kw)
            for mode, code in native.REPLAY_MODES.items():
                ok = env.replay_supported(mode)
                assert ok == bool(native.lib().pime_env_replay_supported(env._h, code))
                if ok:
                    served.add((kind, sm, mode))
            assert not env.replay_supported("nonsense") and native.lib().pime_env_replay_supported(env._h, 2) == 0
            assert native.lib().pime_env_replay_channels(env._h) == (1 if kind == "ph" else 2)
            env.close()
    assert served == {c[:3] for c in CLASSES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_every_served_class_against_the_checker_and_the_host_library(case, ph_table_oracle):
    kind, state_mode, mode, variant, which, skip = case
    g = _grids(ph_table_oracle)
    rec = _records(g, kind, variant, which)
    env = _make_env(kind, state_mode, g[kind]["plants"])
    assert env.replay_supported(mode)
    err, sim = _replay(env, rec, mode, skip)
    err_nosim, none = _replay(env, rec, mode, skip, want_sim=False)
    assert none is None
    held = _held_plants(env, kind)
    tag = "-".join(str(x) for x in case)
    share = R.check_recording(kind, held, rec, mode, skip, err, sim, state_mode, ph_table_oracle, err_nosim=err_nosim, tag=tag)
    bit = None
    if state_mode == "f64":
        np.testing.assert_array_equal(held, g[kind]["plants"])
        h_err, h_sim = R.host_replay(kind, held, rec, mode, skip, table=ph_table_oracle)
        bit = R._bits_equal(sim, h_sim) and R._bits_equal(err, h_err)
        assert R._bits_equal(sim, h_sim), "sim is not bit-equal to the host library's"
        assert R._bits_equal(err, h_err), "err is not bit-equal to the host library's"
    bar = "cell-exact" if (kind == "ph" and state_mode == "mixed") else ("1e-12" if state_mode == "f64" else "2e-5")
    print(f"\nSHARE replay id={tag} sim={share['sim']:.4f} (bar {bar}) err=bit-equal host_bit_equal={bit}")
    env.close()


# ---- 2. the launch-by-launch route --------------------------------------------------------------------------------------------
def test_a_chain_of_env_steps_with_zero_noise_is_sim_bit_for_bit(ph_table_oracle):
    import pime_amd.native as nt
    g = _grids(ph_table_oracle)
    plants, rec = g["wt"]["plants"], g["wt"]["rec"]
    env = _make_env("wt", "f64", plants)
    _, sim = _replay(env, rec, "simulate", 0)
    env.set_reset_all(False)
    env.reset()
    env.set_max_step(10 * T)
    zero = torch.zeros((N, 2), dtype=torch.float64, device=DEV)
    for e in range(E):
        env.set_field("h1", np.full(N, rec["output"][e, 0, 0])); env.set_field("h2", np.full(N, rec["output"][e, 0, 1]))
        for t in range(T):
            a = torch.full((N,), float(rec["action"][e, t]), dtype=torch.float64, device=DEV)
            nt.check(nt.lib().pime_env_step(env._h, nt.ptr(a), nt.F64, nt.ptr(zero), 0, None, nt.ptr(env.obs), nt.ptr(env.reward),
                                            nt.ptr(env.done), env._stream()), "pime_env_step")
            assert R._bits_equal(env.get_field("h1"), sim[e, t, 0]) and R._bits_equal(env.get_field("h2"), sim[e, t, 1]), (e, t)
    np.testing.assert_array_equal(_held_plants(env, "wt"), plants)     # (no reset resampled them)
    env.close()


# ---- 3. the handle is untouched -----------------------------------------------------------------------------------------------
FIELDS = {"ph": ("x", "I", "r", "y", "A", "B", "C", "qww_V", "qc_V", "t", "episode"),
          "wt": ("h1", "h2", "r", "I", "a1", "a2", "Kp", "t", "episode")}


@pytest.mark.parametrize("kind,state_mode", [("ph", "mixed"), ("ph", "f64"), ("wt", "mixed"), ("wt", "f64")])
def test_the_handle_is_untouched(kind, state_mode, ph_table_oracle):
    g = _grids(ph_table_oracle)
    rec = g[kind]["rec"]
    envs = [_make_env(kind, state_mode, g[kind]["plants"]) for _ in range(2)]
    for env in envs:
        env.set_reset_all(False)
        env.reset()
        env.step(torch.full((N,), 0.3, dtype=torch.float32, device=DEV))      # somewhere inside an episode
    before = {f: envs[0].get_field(f) for f in FIELDS[kind]}
    obs_before = envs[0].obs.clone()
    for mode in (("simulate", "predict") if kind == "wt" else ("simulate",)):
        _replay(envs[0], rec, mode, 0)
    for f in FIELDS[kind]:
        assert R._bits_equal(envs[0].get_field(f), before[f]), f
    assert torch.equal(envs[0].obs, obs_before) and envs[0]._t_all == envs[1]._t_all == 1
    a = torch.linspace(-0.9, 0.9, N, dtype=torch.float32, device=DEV)
    got = [tuple(x.clone() for x in env.step(a)) for env in envs]           # in-kernel (Philox) noise: the same counters on both
    for x, y in zip(*got):
        assert torch.equal(x, y)
    for f in FIELDS[kind]:
        assert R._bits_equal(envs[0].get_field(f), envs[1].get_field(f)), f
    for env in envs:
        env.close()


# ---- 4. lane and record counts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,state_mode,mode,variant", [("wt", "mixed", "simulate", "given"), ("wt", "f64", "predict", "given"),
                                                          ("ph", "mixed", "simulate", "hidden"), ("ph", "f64", "simulate", "given")])
def test_lane_and_record_counts_where_the_grid_can_go_wrong(kind, state_mode, mode, variant, ph_table_oracle):
    import pime_amd.native as nt
    g = _grids(ph_table_oracle)
    base = _records(g, kind, variant)
    rec5 = {k: np.concatenate([v, v[:2][::-1]]) for k, v in base.items()}           # five records
    env = _make_env(kind, state_mode, g[kind]["plants"])
    want_err, want_sim = _replay(env, rec5, mode, 2)
    env.close()
    Cn = 1 if kind == "ph" else 2
    guard = 64
    for n in (1, 63, 65, 257, 4100):
        env = _make_env(kind, state_mode, g[kind]["plants"], n=n)
        lane = np.arange(n) % N
        for n_rec in (1, 5):
            dev = {k: torch.as_tensor(np.ascontiguousarray(v[:n_rec]), dtype=torch.float64).to(DEV) for k, v in rec5.items()}
            err = torch.full((n_rec * R.ROWS * n + guard,), float("nan"), dtype=torch.float64, device=DEV)
            sim = torch.full((n_rec * T * Cn * n + guard,), float("nan"), dtype=torch.float64, device=DEV)
            err[-guard:] = -777.0; sim[-guard:] = -777.0
            r = nt.ReplayRecords(dev["action"].data_ptr(), dev["output"].data_ptr(), dev["state0"].data_ptr() if "state0" in dev else None,
                                 n_rec, T)
            nt.check(nt.lib().pime_env_replay_error(env._h, C.byref(r), nt.REPLAY_MODES[mode], 2, nt.ptr(err), nt.ptr(sim), env._stream()))
            torch.cuda.synchronize()
            err, sim = err.cpu().numpy(), sim.cpu().numpy()
            assert (err[-guard:] == -777.0).all() and (sim[-guard:] == -777.0).all(), f"N={n} E={n_rec}: a store past the last lane"
            err, sim = err[:-guard].reshape(n_rec, R.ROWS, n), sim[:-guard].reshape(n_rec, T, Cn, n)
            assert not np.isnan(err).any() and not np.isnan(sim).any(), f"N={n} E={n_rec}: words left unwritten"
            assert R._bits_equal(err, want_err[:n_rec][:, :, lane]), f"N={n} E={n_rec}: err depends on the lane / record count"
            assert R._bits_equal(sim, want_sim[:n_rec][:, :, :, lane]), f"N={n} E={n_rec}: sim depends on the lane / record count"
        env.close()


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_err_untouched(ph_table_oracle):
    import pime_amd.native as nt
    from pime_amd import gym_control
    g = _grids(ph_table_oracle)
    lib = nt.lib()
    bad = []

    def call(env, kind, word, **over):
        rec = g[kind]["rec"]
        dev = {k: torch.as_tensor(v, dtype=torch.float64).to(DEV) for k, v in rec.items()}
        kw = dict(action=dev["action"].data_ptr(), output=dev["output"].data_ptr(), state0=dev["state0"].data_ptr() if kind == "ph" else None,
                  E=E, T=T, mode=0, skip=0)
        kw.update(over)
        err = torch.full((E, R.ROWS, env.num_envs), -777.0, dtype=torch.float64, device=DEV)
        r = nt.ReplayRecords(kw["action"], kw["output"], kw["state0"], kw["E"], kw["T"])
        rc = lib.pime_env_replay_error(env._h, C.byref(r), kw["mode"], kw["skip"], None if word == "err" else nt.ptr(err), None, env._stream())
        torch.cuda.synchronize()
        if rc != -1 or word not in nt.last_error() or not bool((err == -777.0).all()):
            bad.append((kind, word, rc, nt.last_error()))

    for kind in ("wt", "ph"):
        env = _make_env(kind, "mixed", g[kind]["plants"])
        for word, over in (("E", dict(E=0)), ("T", dict(T=0)), ("skip", dict(skip=-1)), ("skip", dict(skip=T)), ("action", dict(action=None)),
                           ("output", dict(output=None)), ("err", dict()), ("mode", dict(mode=2)), ("mode", dict(mode=-1))):
            call(env, kind, word, **over)
        if kind == "wt":
            call(env, kind, "state0", state0=torch.zeros(E, dtype=torch.float64, device=DEV).data_ptr())
        else:
            call(env, kind, "PREDICT", mode=1)
        env.close()
    # refused handles: the binary16 state mode and the Stacking observation
    for kind, name, sm in (("wt", gym_control.WT_INTEGRATOR, "mixed16"), ("ph", gym_control.PH_V35, "mixed16"),
                           ("wt", gym_control.WT_STACKING.format(4), "mixed")):
        env = gym_control.make_vec(name, N, device=DEV, state_mode=sm, seed=SEED)
        assert not env.replay_supported("simulate")
        call(env, kind, "not served")
        with pytest.raises(nt.PimeError):
            env.replay_error(g[kind]["rec"])
        env.close()
    assert not bad, bad


# ---- 6. capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", [("wt", "predict"), ("ph", "simulate")])
def test_captured_and_replayed_twice_equals_the_eager_call(kind, mode, ph_table_oracle):
    import pime_amd.native as nt
    g = _grids(ph_table_oracle)
    env = _make_env(kind, "mixed", g[kind]["plants"])
    dev = {k: torch.as_tensor(v, dtype=torch.float64).to(DEV) for k, v in g[kind]["rec"].items()}
    want_err, want_sim = _replay(env, dev, mode, 5)
    graph = torch.cuda.CUDAGraph()
    with nt.capture_guard(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        err, sim = env.replay_error(dev, mode=mode, skip=5, want_sim=True)
    for _ in range(2):
        err.fill_(float("nan")); sim.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert R._bits_equal(err.cpu().numpy(), want_err) and R._bits_equal(sim.cpu().numpy(), want_sim)
    del graph
    env.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode,variant", [("wt", "simulate", "given"), ("wt", "predict", "given"), ("ph", "simulate", "given"),
                                               ("ph", "simulate", "hidden")])
def test_identify_plants_finds_the_plant_the_records_came_from(kind, mode, variant, ph_table_oracle):
    from pime_amd import gym_control, protocols
    g = _grids(ph_table_oracle)
    rec, true, plants = _records(g, kind, variant), g[kind]["true"], g[kind]["plants"]
    name = gym_control.PH_V35 if kind == "ph" else gym_control.WT_INTEGRATOR
    env = gym_control.make_vec(name, N, device=DEV, state_mode="mixed", seed=SEED)
    env.step = env.step_residual = None         # the env is not stepped
    calls = []
    orig = env.replay_error
    env.replay_error = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    res = protocols.identify_plants(env, rec, g[kind]["axes"], mode=mode, skip=0)
    assert calls == [1], "one replay_error launch"
    env.close()
    oracle_cost = R.cost_of(R.synthesize(kind, plants, rec, mode, 0, ph_table_oracle)[0])
    runner_up = np.sort(oracle_cost)[1]
    cost = res["cost"].reshape(-1)
    print(f"\nSEPARATION device {kind}-{mode}-{variant}: cost at the true plant {cost[true]:.3e}, the oracle's runner-up {runner_up:.3e} "
          f"(share of the 1e-4 bar: {cost[true] / (1e-4 * runner_up):.4f})")
    assert res["best_index"] == true == int(np.argmin(cost))
    np.testing.assert_array_equal(list(res["best"].values()), plants[true])
    assert cost[true] <= 1e-4 * runner_up
    assert res["cost"].shape == tuple(len(v) for v in g[kind]["axes"].values()) and (res["count"] == E * T * (1 if kind == "ph" else 2)).all()
    box = protocols.ensemble_ranges(res, 2.0)
    for (k, (lo, hi)), v in zip(box.items(), plants[true]):
        assert lo <= v <= hi, (k, lo, hi, v)
    with pytest.raises(ValueError):
        protocols.identify_plants(env, rec, dict(list(g[kind]["axes"].items())[:1]))


def test_records_from_a_trace_identify_the_lane_they_came_from(ph_table_oracle):
    """Sim-to-sim: the trace of a fused evaluation (prior controller, zero process noise) turned into records by
    protocols.records_from_trace; every record's own plant scores best."""
    from pime_amd import gym_control, protocols
    plants = R.grid_plants(R.WT_AXES)
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, N, device=DEV, state_mode="f64", seed=SEED, reward_type="distance", noise_scale=0.0)
    env.set_reset_all(False)
    env.reset_changable_parameters(plants[:, 0], plants[:, 1], plants[:, 2])
    env.reset()
    first = np.stack([env.get_field("h1"), env.get_field("h2")])
    _, trace = env.rollout_eval(None, -env.K, 30, want_trace=True)
    lanes = [3, 40, 77]
    rec = protocols.records_from_trace(trace, env.kind, lanes=lanes, first=first)
    assert rec["action"].shape == (3, 30) and rec["output"].shape == (3, 31, 2)
    short = protocols.records_from_trace(trace, env.kind, lanes=lanes)
    assert short["action"].shape == (3, 29) and short["output"].shape == (3, 30, 2)
    for records in (rec, short):
        err = env.replay_error(records)[0].cpu().numpy()
        per_record = err[:, R.SSE0] + err[:, R.SSE1]
        own, second = per_record[np.arange(3), lanes], np.sort(per_record, axis=1)[:, 1]
        print(f"\nSEPARATION trace records: own plant {own.max():.3e}, runner-up {second.min():.3e}")
        assert list(per_record.argmin(axis=1)) == lanes and (own <= 1e-9 * second).all()
    env.close()
    # pH: the trace holds y BEFORE each step and x after it, so the records start after step 0 (state0 = x after step 0)
    plants = R.grid_plants(R.PH_AXES)
    env = gym_control.make_vec(gym_control.PH_V35, N, device=DEV, state_mode="f64", seed=SEED)
    env.set_reset_all(False)
    env.set_params(plants[:, 0], plants[:, 1])
    env.reset()
    _, trace = env.rollout_eval(None, -env.K, 30, want_trace=True)
    full = protocols.records_from_trace(trace, env.kind, lanes=lanes, y_last=env.get_field("y"))
    assert full["action"].shape == (3, 29) and full["output"].shape == (3, 30, 1) and full["state0"].shape == (3,)
    short = protocols.records_from_trace(trace, env.kind, lanes=lanes)
    assert short["action"].shape == (3, 28) and short["output"].shape == (3, 29, 1)
    hidden = {k: v for k, v in full.items() if k != "state0"}
    for records, skip in ((full, 0), (short, 0), (hidden, 8)):
        err = env.replay_error(records, skip=skip)[0].cpu().numpy()[:, R.SSE0]
        own, second = err[np.arange(3), lanes], np.sort(err, axis=1)[:, 1]
        print(f"\nSEPARATION pH trace records: own plant {own.max():.3e}, runner-up {second.min():.3e}")
        assert list(err.argmin(axis=1)) == lanes and (own <= 1e-4 * second).all()
        if "state0" in records:
            assert (own == 0.0).all()
    env.close()
    u = 5.0 * rec["action"] + 5.0
    phys = protocols.records_from_physical(u, rec["output"], "wt")
    np.testing.assert_allclose(phys["action"], rec["action"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(protocols.records_from_physical(0.75 * (rec["action"] + 1.0), np.zeros((3, 31)), "ph")["action"], rec["action"],
                               rtol=0, atol=1e-15)


def test_train_identify_writes_the_identified_plant(tmp_path, ph_table_oracle):
    from pime_amd import train
    g = _grids(ph_table_oracle)
    rec, plants, true = g["wt"]["rec"], g["wt"]["plants"], g["wt"]["true"]
    path = tmp_path / "records.npz"
    np.savez(path, action=rec["action"], output=rec["output"])
    train.main(["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
                "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
                "--break_step", str(64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1",
                "--identify", str(path), "--identify_points", "9", "--log_root", str(tmp_path)])
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "identified.npz"]
    assert len(found) == 1
    z = np.load(found[0], allow_pickle=False)
    assert z["cost"].shape == (9, 9, 9) and list(z["axis_names"]) == ["a1", "a2", "Kp"]
    np.testing.assert_allclose(z["best"], plants[true], rtol=1e-12, atol=0)      # the 9-point axes contain the 3-point ones
    assert (z["ensemble_low"] <= z["best"]).all() and (z["best"] <= z["ensemble_high"]).all()
    assert str(z["mode"]) == "simulate" and int(z["skip"]) == 0
