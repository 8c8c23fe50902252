"""The prior-gain sweep on the GPU (pime_prior_sweep, csrc/prior_sweep.hip) against tests/prior_sweep.py:
  1. every served class (pH / Integrator tank x float64 / mixed state) on 81 lanes at a lane offset, the G = 3 gain rows of the CPU
     tests, 23 steps in segments of 10: pairs bit-equal to G launches of pime_rollout_eval_metrics(kind = -1) on clones, summary
     bit-equal to the numpy restatement of the call's own pairs, summary without pairs bit-equal to summary with them, and in
     float64 everything bit-equal to the host library (the tank there with process noise off: its Box-Muller runs on the device's
     log / sincos and on the host's, two libraries that are not bit-identical; the noisy tank is held to the metrics launches);
  2. lane counts 1, 63, 64, 65, 130 with 1 and 5 gain rows;
  3. the handle is untouched: every field and step counter bit-equal before and after, the next step equals a clone's;
  4. two runs bit-identical;  5. a NaN gain row;
  6. MIXED16 and Stacking1 / 10 handles are refused, every argument error returns PIME_ERR_ARG and leaves summary untouched;
  7. captured in a torch.cuda.graph and replayed twice: bit-equal to the eager call;
  8. protocols.tune_prior on a 4 x 4 gain box x 27 tank plants, train.py --tune_prior / --prior_K."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import prior_sweep as P
from rollout_replay import DEV

pytestmark = pytest.mark.gpu
N, OFFSET, SEED = 81, 8192, 6
N_STEPS, SEG, TAIL, BAND = 23, 10, 4, 0.05
CLASSES = [(kind, sm) for kind in ("ph", "wt") for sm in ("f64", "mixed")]
FIELDS = {"ph": ("x", "A", "B", "C", "r", "I", "t", "episode"), "wt": ("h1", "h2", "a1", "a2", "Kp", "r", "I", "t", "episode")}


def _make_env(kind, state_mode, n=N, reset=True, **extra):
    from pime_amd import gym_control
    name = gym_control.PH_V35 if kind == "ph" else gym_control.WT_INTEGRATOR
    kw = dict(reward_type="distance") if kind == "wt" else {}
    kw.update(extra)
    env = gym_control.make_vec(name, n, device=DEV, state_mode=state_mode, seed=SEED, env_offset=OFFSET, **kw)
    if reset:
        env.reset()
    return env


def _lanes(env, kind):
    out = {k: np.ascontiguousarray(env.get_field(k)) for k in FIELDS[kind]}
    out["t"], out["episode"] = out["t"].astype(np.int32), out["episode"].astype(np.int32)
    return out


def _sweep(env, gains, seg_len=SEG, tail=TAIL, want_pairs=True, kind=None):
    kind = kind or ("ph" if env.obs_dim == 3 else "wt")
    out = env.prior_sweep(gains, N_STEPS, setpoints=P.SETPOINTS[kind] if seg_len > 0 else None, seg_len=seg_len, band=BAND, tail=tail,
                          want_pairs=want_pairs)
    torch.cuda.synchronize()
    if want_pairs:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy(), None


def _metrics_route(env, kind, gains, seg_len=SEG, tail=TAIL):
    """pairs [S, 8, G, N] by the parent's route: one pime_rollout_eval_metrics(kind = -1) launch per gain on a clone in env's state."""
    want = _lanes(env, kind)
    cols = []
    for g in range(len(gains)):
        c = env.clone()
        c.reset()
        got = _lanes(c, kind)
        assert all(P.bits_equal(got[k].astype(np.float64), want[k].astype(np.float64)) for k in want), "a reset clone holds env's state"
        _, m, _ = c.rollout_eval_metrics(None, gains[g], N_STEPS, setpoints=P.SETPOINTS[kind] if seg_len > 0 else None, seg_len=seg_len,
                                         band=BAND, tail=tail)
        cols.append(m.cpu().numpy())
        c.close()
    return np.ascontiguousarray(np.stack(cols, axis=2))


def _host(env, kind, lanes, gains, seg_len, tail, table):
    import pime_amd.native as nt
    cfg = nt.EnvCfg.from_buffer_copy(env.cfg)
    keep = None
    if kind == "ph":
        keep = np.ascontiguousarray(table, dtype=np.float64)
        cfg.ph_table = keep.ctypes.data_as(C.POINTER(C.c_double))
        cfg.ph_table_len = len(keep)
    gains = np.ascontiguousarray(gains, dtype=np.float64)
    n, G, S = env.num_envs, len(gains), P.n_segments(N_STEPS, seg_len)
    sp = np.ascontiguousarray(P.SETPOINTS[kind], dtype=np.float64)
    summary, pairs = np.full((G, S, P.ROWS, P.STATS), -777.0), np.full((S, P.ROWS, G, n), -777.0)
    rc, msg = P.host_sweep_raw(kind, cfg, lanes, n, gains, G, N_STEPS, seg_len, sp if seg_len > 0 else None, len(sp) if seg_len > 0 else 0,
                               BAND, tail, pairs, summary)
    del keep
    assert rc == 0, msg
    return summary, pairs


# ---- 1. every served class -------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_served_classes():
    from pime_amd import gym_control, native
    served = set()
    for kind, name in (("ph", gym_control.PH_V35), ("wt", gym_control.WT_INTEGRATOR), ("stacking", gym_control.WT_STACKING.format(4))):
        for sm in ("f64", "mixed", "mixed16"):
            env = gym_control.make_vec(name, 4, device=DEV, state_mode=sm, seed=SEED)
            assert env.prior_sweep_supported() == bool(native.lib().pime_prior_sweep_supported(env._h))
            if env.prior_sweep_supported():
                served.add((kind, sm))
            env.close()
    assert served == set(CLASSES)


@pytest.mark.parametrize("seg_len,tail", [(SEG, TAIL), (0, 50)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind,state_mode", CLASSES, ids=lambda v: str(v))
def test_every_served_class(kind, state_mode, seg_len, tail, ph_table_oracle):
    gains = P.gain_rows(kind)
    env = _make_env(kind, state_mode)
    assert env.prior_sweep_supported()
    summary, pairs = _sweep(env, gains, seg_len, tail)
    P.check_pairs(pairs, _metrics_route(env, kind, gains, seg_len, tail), f"{kind}-{state_mode}")
    P.check_summary(summary, pairs)
    nopairs, _ = _sweep(env, gains, seg_len, tail, want_pairs=False)
    assert P.bits_equal(nopairs, summary), "pairs = NULL must not change a bit of summary"
    assert (summary[..., P.FINITE] == N).all()
    noisy_bit = None
    if state_mode == "f64":
        if kind == "wt":
            h_summary, h_pairs = _host(env, kind, _lanes(env, kind), gains, seg_len, tail, ph_table_oracle)
            noisy_bit = P.bits_equal(pairs, h_pairs)
            # (the noisy tank: two libms; reported, not asserted -- settling steps and peaks are no continuous functions of the noise)
            env.close()
            env = _make_env(kind, state_mode, noise_scale=0.)
            summary, pairs = _sweep(env, gains, seg_len, tail)
        h_summary, h_pairs = _host(env, kind, _lanes(env, kind), gains, seg_len, tail, ph_table_oracle)
        assert P.bits_equal(pairs, h_pairs), "pairs are not bit-equal to the host library's"
        assert P.bits_equal(summary, h_summary), "summary is not bit-equal to the host library's"
    print(f"\nSWEEP id={kind}-{state_mode}-{seg_len}-{tail} pairs=bit-equal summary=bit-equal noisy_tank_host_bit_equal={noisy_bit}")
    env.close()


# ---- 2. lane counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind,state_mode", [("wt", "mixed"), ("ph", "f64")], ids=lambda v: str(v))
def test_ragged_lane_counts(kind, state_mode, n, G):
    rows = P.gain_rows(kind)
    gains = np.ascontiguousarray(np.stack([rows[j % 3] * (1.0 + 0.1 * (j // 3)) for j in range(G)]))
    env = _make_env(kind, state_mode, n=n)
    summary, pairs = _sweep(env, gains)
    assert pairs.shape == (3, P.ROWS, G, n) and summary.shape == (G, 3, P.ROWS, P.STATS)
    P.check_pairs(pairs, _metrics_route(env, kind, gains), f"{kind} n={n} G={G}")
    P.check_summary(summary, pairs)
    nopairs, _ = _sweep(env, gains, want_pairs=False)
    assert P.bits_equal(nopairs, summary)
    env.close()


# ---- 3. / 4. the handle is read, never written; two runs ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,state_mode", CLASSES, ids=lambda v: str(v))
def test_the_handle_is_untouched_and_two_runs_agree(kind, state_mode):
    gains = P.gain_rows(kind)
    env, twin = _make_env(kind, state_mode), _make_env(kind, state_mode)
    before = _lanes(env, kind)
    counters = (env._t_all, None if env._t_lanes is None else env._t_lanes.copy(), env._was_reset, env.reset_count)
    obs0 = env.obs.clone()
    first = _sweep(env, gains)
    second = _sweep(env, gains)
    assert P.bits_equal(first[0], second[0]) and P.bits_equal(first[1], second[1]), "two runs must be bit-identical"
    after = _lanes(env, kind)
    for k in before:
        assert P.bits_equal(before[k].astype(np.float64), after[k].astype(np.float64)), k
    assert (env._t_all, env._was_reset, env.reset_count) == (counters[0], counters[2], counters[3]) and env._t_lanes is None
    assert torch.equal(env.obs, obs0)
    a = torch.full((N,), 0.25, dtype=torch.float64, device=DEV)
    got, want = env.step(a, auto_reset=False), twin.step(a, auto_reset=False)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "the next step equals that of an env that never swept"
    env.close(); twin.close()


# ---- 5. a NaN gain row -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,state_mode", [("wt", "mixed"), ("ph", "mixed")], ids=lambda v: str(v))
def test_a_nan_gain_row(kind, state_mode):
    rows = P.gain_rows(kind)
    gains = np.ascontiguousarray(np.stack([rows[0], np.full(rows.shape[1], np.nan), rows[1]]))
    env = _make_env(kind, state_mode, n=130)
    summary, pairs = _sweep(env, gains)
    P.check_summary(summary, pairs)
    dead = np.isnan(pairs[:, :, 1]).all(axis=-1)
    assert dead[:, 7].all()
    got = summary[1][dead]
    assert (got[:, P.FINITE] == 0).all() and P.bits_equal(got[:, P.SUM], np.zeros(len(got))) and (got[:, P.MIN] == np.inf).all()
    assert (got[:, P.MAX] == -np.inf).all() and (got[:, P.ARGMAX] == -1).all()
    clean, _ = _sweep(env, np.ascontiguousarray(gains[[0, 2]]))
    assert P.bits_equal(summary[[0, 2]], clean), "the NaN row must not change a bit of the other gains"
    env.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def _raw(env, gains, G, n_steps, seg_len, sp, n_sp, band, tail, summary, workspace, pairs=None):
    import pime_amd.native as nt
    rc = nt.lib().pime_prior_sweep(env._h, nt.ptr(gains), G, n_steps, seg_len, nt.ptr(sp), n_sp, band, tail, nt.ptr(pairs), nt.ptr(summary),
                                   nt.ptr(workspace), env._stream())
    torch.cuda.synchronize()
    return rc, nt.last_error()


def test_unserved_handles_are_refused():
    from pime_amd import gym_control, native
    for name, sm in ((gym_control.PH_V35, "mixed16"), (gym_control.WT_INTEGRATOR, "mixed16"), (gym_control.WT_STACKING.format(1), "mixed"),
                     (gym_control.WT_STACKING.format(10), "mixed"), (gym_control.WT_STACKING.format(10), "f64")):
        env = gym_control.make_vec(name, 8, device=DEV, state_mode=sm, seed=SEED)
        env.reset()
        assert not env.prior_sweep_supported()
        assert native.lib().pime_prior_sweep_workspace_bytes(env._h, 3, N_STEPS, 0) == -1
        gains = torch.zeros((3, env.obs_dim), dtype=torch.float64, device=DEV)
        summary = torch.full((3, 1, P.ROWS, P.STATS), -777.0, dtype=torch.float64, device=DEV)
        ws = torch.zeros(4096, dtype=torch.float64, device=DEV)
        rc, msg = _raw(env, gains, 3, N_STEPS, 0, None, 0, BAND, TAIL, summary, ws)
        assert rc == -1 and "not served" in msg and (summary == -777.0).all(), (name, sm, rc, msg)
        with pytest.raises(native.PimeError):
            env.prior_sweep(gains, N_STEPS)
        env.close()


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_argument_errors(kind):
    from pime_amd import native
    env = _make_env(kind, "mixed", n=8, reset=False)
    gains = torch.as_tensor(P.gain_rows(kind), device=DEV)
    sp = np.ascontiguousarray(P.SETPOINTS[kind], dtype=np.float64)
    summary = torch.full((3, 3, P.ROWS, P.STATS), -777.0, dtype=torch.float64, device=DEV)
    ws_bytes = native.lib().pime_prior_sweep_workspace_bytes(env._h, 3, N_STEPS, SEG)
    assert ws_bytes == 3 * 1 * 3 * P.ROWS * P.STATS * 8
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=DEV)
    base = dict(gains=gains, G=3, n_steps=N_STEPS, seg_len=SEG, sp=sp, n_sp=3, band=BAND, tail=TAIL, summary=summary, ws=ws)
    rc, msg = _raw(env, gains, 3, N_STEPS, SEG, sp, 3, BAND, TAIL, summary, ws)
    assert rc == -4 and "before pime_env_reset" in msg and (summary == -777.0).all()
    env.reset()
    bad = []
    cases = [("G = 0", dict(G=0)), ("2^31 - 1", dict(G=2 ** 28)), ("gains is NULL", dict(gains=None)), ("summary is NULL", dict(summary=None)),
             ("workspace is NULL", dict(ws=None)), ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))), ("band", dict(band=float("inf"))),
             ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)), ("n_setpoints 17", dict(n_sp=17)), ("set-point schedule", dict(n_sp=2)),
             ("set-point schedule", dict(sp=None)), ("set-point schedule", dict(seg_len=-1))]
    for word, over in cases:
        kw = dict(base, **over)
        rc, msg = _raw(env, kw["gains"], kw["G"], kw["n_steps"], kw["seg_len"], kw["sp"], kw["n_sp"], kw["band"], kw["tail"], kw["summary"], kw["ws"])
        if rc != -1 or word not in msg or not (summary == -777.0).all():
            bad.append((word, rc, msg))
    assert not bad, bad
    for G, n_steps, seg_len in ((0, N_STEPS, SEG), (2 ** 28, N_STEPS, SEG), (3, 0, SEG), (3, N_STEPS, -1), (3, 1000, 10)):
        assert native.lib().pime_prior_sweep_workspace_bytes(env._h, G, n_steps, seg_len) == -1
    with pytest.raises(native.PimeError):
        env.prior_sweep(np.zeros((3, 7)), N_STEPS)
    rc, _ = _raw(env, gains, 3, N_STEPS, SEG, sp, 3, BAND, TAIL, summary, ws)      # and the good call goes through
    assert rc == 0 and not (summary == -777.0).any()
    env.close()


# ---- 7. stream capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_captured_in_a_graph_and_replayed(kind):
    import pime_amd.native as nt
    gains = torch.as_tensor(P.gain_rows(kind), device=DEV)
    env = _make_env(kind, "mixed")
    want_summary, want_pairs = _sweep(env, gains)
    graph = torch.cuda.CUDAGraph()
    with nt.capture_guard(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        summary, pairs = env.prior_sweep(gains, N_STEPS, setpoints=P.SETPOINTS[kind], seg_len=SEG, band=BAND, tail=TAIL, want_pairs=True)
    for _ in range(2):
        summary.fill_(float("nan")); pairs.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert P.bits_equal(summary.cpu().numpy(), want_summary) and P.bits_equal(pairs.cpu().numpy(), want_pairs)
    env.close()


# ---- 8. protocols and train.py ---------------------------------------------------------------------------------------------------
WT_AXES = dict(a1=np.linspace(0.0015, 0.0024, 3), a2=np.linspace(0.0015, 0.0024, 3), Kp=np.linspace(0.07, 0.17, 3))


@pytest.mark.parametrize("robust", ["worst", "mean"])
def test_tune_prior_on_a_gain_box(robust):
    from pime_amd import protocols
    env = _make_env("wt", "mixed", n=27, reset=False)
    factors = [0.5, 1.0, 2.0, 4.0]
    gains = protocols.gain_box(-env.K, factors)
    assert gains.shape == (16, 4)
    steps = 40
    res = protocols.tune_prior(env, gains, axes=WT_AXES, steps=steps, robust=robust)
    summary, pairs = env.prior_sweep(gains, 5 * steps, setpoints=protocols.WT_SETPOINTS, seg_len=steps, band=0.05, tail=10, want_pairs=True)
    summary, pairs = summary.cpu().numpy(), pairs.cpu().numpy()
    assert P.bits_equal(summary, res["summary"])
    P.check_summary(summary, pairs)
    itae = pairs[:, protocols.METRIC_NAMES.index("itae")]                       # [S, G, N]
    cost = (itae.max(axis=2) if robust == "worst" else itae.mean(axis=2)).sum(axis=0)
    assert res["best_index"] == int(np.argmin(cost))
    np.testing.assert_allclose(res["cost"], cost, rtol=1e-12)
    builtin = int(np.flatnonzero((gains == -env.K).all(axis=1))[0])             # factor 1 on both components
    assert res["cost"][res["best_index"]] <= res["cost"][builtin]
    np.testing.assert_array_equal(res["worst_plant"], itae.argmax(axis=2).T)
    settled = (pairs[:, protocols.METRIC_NAMES.index("settling_step")] < steps).all(axis=(0, 2))
    np.testing.assert_array_equal(res["settled_all"], settled)
    np.testing.assert_array_equal(res["best_gain"], gains[res["best_index"]])
    nan = protocols.tune_prior(env, np.concatenate([gains[:2], np.full((1, 4), np.nan)]), axes=WT_AXES, steps=steps, robust=robust)
    assert nan["cost"][2] == np.inf and np.isfinite(nan["cost"][:2]).all() and not nan["settled_all"][2]
    print(f"\nTUNE robust={robust} best gain {res['best_gain'].tolist()} cost {res['cost'][res['best_index']]:.6g} built-in {res['cost'][builtin]:.6g}")
    env.close()


def test_train_tune_prior_writes_the_file_and_prior_K_loads_it(tmp_path):
    from pime_amd import train
    common = ["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
              "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
              "--break_step", str(64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1"]
    train.main(common + ["--tune_prior", "3", "--tune_prior_points", "3", "--log_root", str(tmp_path / "a")])
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "tuned_prior.npz"]
    assert len(found) == 1
    z = np.load(found[0], allow_pickle=False)
    assert z["plants"].shape == (27, 3) and z["gains_priorK"].shape == (10, 4) and z["cost"].shape == (10,)
    np.testing.assert_array_equal(z["builtin_K"], [0.0, 0.4, -0.4, 0.0])
    np.testing.assert_array_equal(z["best_gain"], -z["gains_priorK"][int(z["best_index"])])
    assert z["cost"][int(z["best_index"])] <= float(z["builtin_cost"]) == z["cost"][-1]
    tuned = tmp_path / "tuned.npz"
    np.savez(tuned, best_gain=np.array([0.0, 0.7, -0.3, 0.0]))                  # not the built-in gain, whatever the sweep found
    agent = train.main(common + ["--prior_K", str(tuned), "--log_root", str(tmp_path / "b")])
    np.testing.assert_array_equal(np.asarray(agent.priorK).reshape(-1), [-0.0, -0.7, 0.3, -0.0])
    env = _make_env("wt", "mixed", n=4, reset=False)                            # the file --tune_prior wrote, on an env and its clone
    train.apply_prior_K(env, found[0])
    clone = env.clone()
    np.testing.assert_array_equal(env.K, z["best_gain"])
    np.testing.assert_array_equal(clone.K, z["best_gain"])
    env.close(); clone.close()
