"""The frequency-response sweep on the GPU (pime_freq_sweep, csrc/freq_sweep.hip) against tests/freq_sweep.py.  Shapes: 21 plants under
a policy (one full 16-lane tile and a partial one per row), 70 under the prior alone (one 64-lane tile and a partial one), on a handle
at lane offset 1000; 60 steps in segments of 24 with three set-points (the last segment has 12 steps), tail 4; eight rows: nominal,
set-point with 1 and with 4 cycles in the window of 16 from step 8, load with 2 cycles and at the Nyquist rate (8 cycles: s vanishes),
measurement with 2 cycles, an onset of 12 that lands exactly on the short segment's end (NaN rows there), an onset of 0.
  1. all 36 served classes (2 envs x {prior, 4 policy kinds x widths 64, 128} x float64 / mixed state): the eight metric rows of the
     A = 0 row bit-equal to pime_rollout_eval_metrics from the same lane state, every row through the checker (all sixteen rows bit for
     bit to the recorded traces), summary bit-equal to summary_from_pairs(pairs); also N = 130 (three summary blocks) with the prior;
  2. the handle's fields are bit-unchanged, two calls give equal bits, a NaN-filled workspace gives the same bits, NULL pairs /
     actions / outputs leave summary unchanged, a tile's pairs give the same bits alone (P = 1, N = 16) as inside the grid, a grid
     with more quads than resident workgroups repeats its rows bit for bit, one captured replay gives equal bits;
  3. float64, the prior alone: device bit-equal to the host build (the tank with process noise off);
  4. every refusal and its message;
  5. train.py --bode writes frequency_response.npz on a toy run and is skipped on a Stacking id."""
import numpy as np
import pytest
import torch

import freq_sweep as F
import prior_sweep as P
from rollout_replay import DEV
from test_gpu_margin_sweep import CLASSES, FIELDS, KINDS, WALKS, _cfg, _lanes, _make_env, _policy   # the handles, policies and classes of that sweep

pytestmark = pytest.mark.gpu

N_POLICY, N_PRIOR = 21, 70
N_STEPS, SEG, TAIL, BAND = 60, 24, F.TAIL, F.BAND
# (POINT, A, k0) and the cycles in the window of SEG - k0 steps
EXCITE = np.array([(0, 0.0, 8), (0, 0.5, 8), (0, 0.5, 8), (1, 0.1, 8), (1, 0.1, 8), (2, 0.2, 8), (1, 0.1, 12), (0, 0.5, 0)], dtype=np.float64)
CYCLES = (1, 1, 4, 2, 8, 2, 3, 3)
WAVE = F.sinusoids(CYCLES, EXCITE[:, 2], SEG)
PN = len(EXCITE)


def _n(pol):
    return N_PRIOR if pol == "prior" else N_POLICY


def _run(env, kind, pk, K, rows=None, wave=None, pairs=True, trace=True, **kw):
    args = dict(n_steps=N_STEPS, seg_len=SEG, setpoints=F.SETPOINTS[kind], band=BAND, tail=TAIL)
    args.update(kw)
    n_steps = args.pop("n_steps")
    out = env.frequency_sweep(pk, K, EXCITE if rows is None else rows, WAVE if wave is None else wave, n_steps, want_pairs=pairs,
                              want_trace=trace, **args)
    torch.cuda.synchronize()
    if not (pairs or trace):
        return dict(summary=out.cpu().numpy())
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _check(kind, cfg, lanes, table, rec, **kw):
    return F.check_recording(kind, cfg, lanes, table, rec, rows=EXCITE, wave=WAVE, n_steps=N_STEPS, seg_len=SEG, band=BAND, tail=TAIL, **kw)


def test_the_table_is_what_the_rows_say():
    assert np.abs(WAVE[4, :, 1]).max() < 1e-14 and (np.abs(WAVE[4, :, 0]) == 1.0).all(), "the Nyquist rate: s vanishes, c alternates"
    assert N_STEPS - 2 * SEG == 12 == EXCITE[6, 2], "an onset on the short segment's end"
    from pime_amd import protocols
    rows, wave = protocols.excitation_grid(CYCLES, EXCITE[:, 1], EXCITE[:, 0], SEG, EXCITE[:, 2])
    assert F.bits_equal(rows, EXCITE) and F.bits_equal(wave, WAVE)


# ---- 1. every served class -------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_served_classes():
    from pime_amd import gym_control, native
    served = set()
    for kind, name in (("ph", gym_control.PH_V35), ("wt", gym_control.WT_INTEGRATOR), ("stacking", gym_control.WT_STACKING.format(4))):
        for sm in ("f64", "mixed", "mixed16"):
            env = gym_control.make_vec(name, 4, device=DEV, state_mode=sm, seed=F.SEED)
            assert env.frequency_supported() == bool(native.lib().pime_freq_sweep_supported(env._h, -1, 0))
            for pol, code in KINDS.items():
                for md in ((0,) if pol == "prior" else (64, 128, 256)):
                    assert native.lib().pime_freq_sweep_supported(env._h, code, md) == native.lib().pime_margin_sweep_supported(env._h, code, md)
                    if native.lib().pime_freq_sweep_supported(env._h, code, md):
                        served.add((kind, pol, md, sm))
            env.close()
    assert served == set(CLASSES) and len(CLASSES) == 36


@pytest.mark.parametrize("kind,pol,md,state_mode", CLASSES, ids=lambda v: str(v))
def test_every_served_class(kind, pol, md, state_mode, ph_table_oracle):
    n = _n(pol)
    env, twin = _make_env(kind, state_mode, n=n), _make_env(kind, state_mode, n=n)
    pk, K, term = _policy(pol, env, md)
    assert env.frequency_supported(pk)
    cfg, keep = _cfg(env, kind, ph_table_oracle)
    lanes = _lanes(env, kind)
    rec = _run(env, kind, pk, K)
    assert rec["pairs"].shape == (3, 16, PN, n) and rec["actions"].shape == rec["outputs"].shape == (N_STEPS, PN, n)
    _, want, _ = twin.rollout_eval_metrics(pk, K, N_STEPS, setpoints=F.SETPOINTS[kind], seg_len=SEG, band=BAND, tail=TAIL)
    assert F.bits_equal(rec["pairs"][:, :8, 0], want.cpu().numpy()), "the A = 0 row is not bit-equal to pime_rollout_eval_metrics"
    tag = f"{kind}-{pol}{md}-{state_mode}"
    use = _check(kind, cfg, lanes, ph_table_oracle, rec, K=K, policy=term, tag=tag)
    P.check_summary(rec["summary"], rec["pairs"], tag=tag)
    assert np.isnan(rec["pairs"][2, 8:, 6]).all() and np.isfinite(rec["pairs"][:2, 8:, 6]).all(), "an onset on the short segment's end"
    assert (rec["summary"][6, 2, 8:, P.FINITE] == 0).all() and (rec["summary"][6, 2, :8, P.FINITE] == n).all()
    assert np.isfinite(np.delete(rec["pairs"], 6, axis=2)).all()
    print(f"\nFREQ id={tag} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action {use['action']:.3g} "
          f"(gap {use['gap']:.4g})")
    env.close(); twin.close()


def test_three_summary_blocks():
    env = _make_env("wt", "mixed", n=130)
    rec = _run(env, "wt", None, -env.K, trace=False)
    P.check_summary(rec["summary"], rec["pairs"], tag="N = 130")
    counted = rec["summary"][..., P.FINITE]
    assert ((counted == 130) | (counted == 0)).all() and (counted[:, :, :8] == 130).all() and rec["summary"].shape == (PN, 3, 16, 5)
    env.close()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "td3", 64, "f64"), ("wt", "prior", 0, "f64")],
                         ids=lambda v: str(v))
def test_zero_amplitude_rows_are_rollout_eval_metrics_lanes(kind, pol, md, state_mode):
    n = _n(pol)
    env, twin = _make_env(kind, state_mode, n=n), _make_env(kind, state_mode, n=n)
    pk, K, _ = _policy(pol, env, md)
    rows = np.array([(0, 0.0, 8), (1, 0.0, 0), (2, 0.0, 30), (2, -0.0, 5)], dtype=np.float64)
    rec = _run(env, kind, pk, K, rows=rows, wave=WAVE[[1, 3, 5, 2]])
    _, want, _ = twin.rollout_eval_metrics(pk, K, N_STEPS, setpoints=F.SETPOINTS[kind], seg_len=SEG, band=BAND, tail=TAIL)
    for p in range(len(rows)):
        assert F.bits_equal(rec["pairs"][:, :8, p], want.cpu().numpy()), p
        assert F.bits_equal(rec["actions"][:, p], rec["actions"][:, 0]) and F.bits_equal(rec["outputs"][:, p], rec["outputs"][:, 0]), p
    assert np.isnan(rec["pairs"][:, 8:, 2]).all() and np.isfinite(rec["pairs"][:, 8:, [0, 1, 3]]).all()
    env.close(); twin.close()


# ---- 2. structure ----------------------------------------------------------------------------------------------------------------
def _raw(env, kind_code, md, img, K, rows, wave, wave_len, Pn, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, outputs, workspace):
    import pime_amd.native as nt
    rc = nt.lib().pime_freq_sweep(env._h, kind_code, md, nt.ptr(img), nt.ptr(K), nt.ptr(rows), nt.ptr(wave), wave_len, Pn, n_steps, seg_len,
                                  nt.ptr(sp), n_sp, band, tail, nt.ptr(pairs), nt.ptr(summary), nt.ptr(actions), nt.ptr(outputs),
                                  nt.ptr(workspace), env._stream())
    torch.cuda.synchronize()
    return rc, nt.last_error()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV).contiguous()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "prior", 0, "f64"), ("ph", "sac", 64, "mixed"),
                                                   ("wt", "prior", 0, "mixed")], ids=lambda v: str(v))
def test_the_handle_is_untouched_and_the_outputs_are_independent(kind, pol, md, state_mode):
    import pime_amd.native as nt
    n = _n(pol)
    env, twin = _make_env(kind, state_mode, n=n), _make_env(kind, state_mode, n=n)
    pk, K, _ = _policy(pol, env, md)
    before = _lanes(env, kind)
    counters = (env._t_all, env._was_reset, env.reset_count)
    obs0 = env.obs.clone()
    first, second = _run(env, kind, pk, K), _run(env, kind, pk, K)
    assert all(F.bits_equal(first[k], second[k]) for k in first), "two calls must be bit-identical"
    quiet = _run(env, kind, pk, K, pairs=False, trace=False)
    assert F.bits_equal(quiet["summary"], first["summary"]), "NULL pairs / actions / outputs must not change a bit of summary"
    only_pairs = _run(env, kind, pk, K, pairs=True, trace=False)
    assert "actions" not in only_pairs and F.bits_equal(only_pairs["pairs"], first["pairs"])
    # the raw call with a NaN-filled workspace: pairs NULL (the finishing launch reads the workspace copy) and pairs given
    ws_bytes = nt.lib().pime_freq_sweep_workspace_bytes(env._h, PN, N_STEPS, SEG)
    assert ws_bytes == 3 * 16 * PN * n * 8
    Kd = np.ascontiguousarray(K, dtype=np.float64)
    ex, wv = _dev(EXCITE), _dev(WAVE)
    sp = np.ascontiguousarray(F.SETPOINTS[kind], dtype=np.float64)
    code, img = (-1, None) if pk is None else (KINDS[pol], pk.packed)
    for with_pairs in (False, True):
        ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
        summary = torch.full((PN, 3, 16, 5), float("nan"), dtype=torch.float64, device=DEV)
        pairs = torch.full((3, 16, PN, n), float("nan"), dtype=torch.float64, device=DEV) if with_pairs else None
        rc, msg = _raw(env, code, md, img, Kd, ex, wv, SEG, PN, N_STEPS, SEG, sp, 3, BAND, TAIL, pairs, summary, None, None, ws)
        assert rc == 0, msg
        assert F.bits_equal(summary.cpu().numpy(), first["summary"]), "a NaN-filled workspace must not change a bit"
        if with_pairs:
            assert F.bits_equal(pairs.cpu().numpy(), first["pairs"])
    after = _lanes(env, kind)
    for k in before:
        assert F.bits_equal(before[k].astype(np.float64), after[k].astype(np.float64)), k
    assert (env._t_all, env._was_reset, env.reset_count) == counters and env._t_lanes is None
    assert torch.equal(env.obs, obs0)
    a = torch.full((n,), 0.25, dtype=torch.float64, device=DEV)
    got, want = env.step(a, auto_reset=False), twin.step(a, auto_reset=False)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), "the next step equals that of an env that never ran the sweep"
    env.close(); twin.close()


@pytest.mark.parametrize("kind,pol,md,state_mode", [("wt", "modular", 128, "mixed"), ("ph", "plain", 64, "f64"), ("wt", "prior", 0, "f64")],
                         ids=lambda v: str(v))
def test_a_tile_alone_gives_the_bits_it_gives_inside_the_grid(kind, pol, md, state_mode):
    big, small = _make_env(kind, state_mode, n=_n(pol)), _make_env(kind, state_mode, n=16)
    for k in FIELDS[kind]:
        if k not in ("t", "episode"):
            assert F.bits_equal(big.get_field(k)[:16], small.get_field(k)), "the same global lanes draw the same state"
    pk, K, _ = _policy(pol, big, md)
    a = _run(big, kind, pk, K)
    for p in (3, 1, 5):      # one row alone (P = 1, N = 16): its table is row 0 of a one-row table
        b = _run(small, kind, pk, K, rows=EXCITE[p:p + 1], wave=WAVE[p:p + 1])
        for k in ("pairs", "actions", "outputs"):
            assert F.bits_equal(a[k][..., p:p + 1, :16], b[k]), (p, k)
    big.close(); small.close()


@pytest.mark.parametrize("kind,pol,md,state_mode,n,per_cu,trace", WALKS, ids=lambda v: str(v))
def test_a_workgroup_walks_more_than_one_quad(kind, pol, md, state_mode, n, per_cu, trace):
    env = _make_env(kind, state_mode, n=n)
    pk, K, _ = _policy(pol, env, md)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    reps = -(-(per_cu * cus + 4) // PN)
    big = _run(env, kind, pk, K, rows=np.tile(EXCITE, (reps, 1)), wave=np.tile(WAVE, (reps, 1, 1)), trace=trace)
    small = _run(env, kind, pk, K, trace=trace)
    axis = dict(summary=0, pairs=2, actions=1, outputs=1)
    assert set(big) == set(small)
    for k in big:        # rows repeated with period 8, each with ITS table: every row p is bit-equal to row p % 8
        assert big[k].shape[axis[k]] == reps * PN
        assert F.bits_equal(big[k], np.take(small[k], np.arange(reps * PN) % PN, axis=axis[k])), f"{k}: a row is not the row of its period"
    env.close()


@pytest.mark.parametrize("kind,pol,md", [("wt", "modular", 128), ("ph", "prior", 0)], ids=lambda v: str(v))
def test_captured_in_a_graph_and_replayed(kind, pol, md):
    import pime_amd.native as nt
    env = _make_env(kind, "mixed", n=_n(pol))
    pk, K, _ = _policy(pol, env, md)
    want = _run(env, kind, pk, K)
    ex, wv = _dev(EXCITE), _dev(WAVE)                                     # uploaded (and validated) before the capture
    graph = torch.cuda.CUDAGraph()
    with nt.capture_guard(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = env.frequency_sweep(pk, K, ex, wv, N_STEPS, setpoints=F.SETPOINTS[kind], seg_len=SEG, band=BAND, tail=TAIL, want_pairs=True,
                                  want_trace=True)
    for x in out.values():
        x.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(F.bits_equal(got[k], want[k]) for k in want)
    env.close()


# ---- 3. the host build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_prior_is_bit_equal_to_the_host_build(kind, ph_table_oracle):
    env = _make_env(kind, "f64", n=N_PRIOR, **({"noise_scale": 0.} if kind == "wt" else {}))
    cfg, keep = _cfg(env, kind, ph_table_oracle)
    lanes = _lanes(env, kind)
    K = np.asarray(-env.K, dtype=np.float64).reshape(-1)
    rec = _run(env, kind, None, K)
    host = F.host_freq(kind, cfg, lanes, rows=EXCITE, wave=WAVE, K=K, n_steps=N_STEPS, seg_len=SEG, band=BAND, tail=TAIL)
    for k in ("pairs", "actions", "outputs", "summary"):
        assert F.bits_equal(rec[k], host[k]), f"{k} is not bit-equal to the host build's"
    env.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_unserved_handles_and_widths_are_refused():
    from pime_amd import gym_control, native
    ex, wv = _dev(EXCITE), _dev(np.tile(WAVE, (1, 3, 1))[:, :N_STEPS])     # seg_len 0: the table has n_steps entries
    ws = torch.zeros(16 * PN * 8, dtype=torch.float64, device=DEV)
    for name, sm, word in ((gym_control.PH_V35, "mixed16", "state_mode"), (gym_control.WT_INTEGRATOR, "mixed16", "state_mode"),
                           (gym_control.WT_STACKING.format(1), "mixed", "Stacking"), (gym_control.WT_STACKING.format(10), "f64", "Stacking")):
        env = gym_control.make_vec(name, 8, device=DEV, state_mode=sm, seed=F.SEED)
        env.reset()
        assert not env.frequency_supported() and native.lib().pime_freq_sweep_supported(env._h, -1, 0) == 0
        assert native.lib().pime_freq_sweep_workspace_bytes(env._h, PN, N_STEPS, 0) == -1
        summary = torch.full((PN, 1, 16, 5), -777.0, dtype=torch.float64, device=DEV)
        K = np.zeros(env.obs_dim)
        rc, msg = _raw(env, -1, 0, None, K, ex, wv, N_STEPS, PN, N_STEPS, 0, None, 0, BAND, TAIL, None, summary, None, None, ws)
        assert rc == -1 and word in msg and "not served" in msg and (summary == -777.0).all(), (name, sm, rc, msg)
        with pytest.raises(native.PimeError):
            env.frequency_sweep(None, K, [[1, 0.1, 0]], np.ones((1, N_STEPS, 2)), N_STEPS)
        env.close()
    env = _make_env("wt", "mixed", n=8)
    img = torch.zeros(16, dtype=torch.float32, device=DEV)
    summary = torch.full((PN, 1, 16, 5), -777.0, dtype=torch.float64, device=DEV)
    for code in (0, 1, 2):
        assert native.lib().pime_freq_sweep_supported(env._h, code, 256) == 0
        rc, msg = _raw(env, code, 256, img, np.zeros(4), ex, wv, N_STEPS, PN, N_STEPS, 0, None, 0, BAND, TAIL, None, summary, None, None, ws)
        assert rc == -1 and "md 256" in msg and (summary == -777.0).all(), (code, rc, msg)
    rc, msg = _raw(env, 7, 64, img, np.zeros(4), ex, wv, N_STEPS, PN, N_STEPS, 0, None, 0, BAND, TAIL, None, summary, None, None, ws)
    assert rc == -1 and "kind 7" in msg
    env.close()


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_argument_errors(kind):
    env = _make_env(kind, "mixed", n=8, reset=False)
    sp = np.ascontiguousarray(F.SETPOINTS[kind], dtype=np.float64)
    K = np.ascontiguousarray(F.PRIOR_K[kind])
    ex, wv = _dev(EXCITE), _dev(WAVE)
    summary = torch.full((PN, 3, 16, 5), -777.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(3 * 16 * PN * 8, dtype=torch.float64, device=DEV)
    base = dict(K=K, ex=ex, wv=wv, wl=SEG, P=PN, n_steps=N_STEPS, seg_len=SEG, sp=sp, n_sp=3, band=BAND, tail=TAIL, summary=summary, ws=ws,
                code=-1, md=0, img=None)
    call = lambda kw: _raw(env, kw["code"], kw["md"], kw["img"], kw["K"], kw["ex"], kw["wv"], kw["wl"], kw["P"], kw["n_steps"], kw["seg_len"],
                           kw["sp"], kw["n_sp"], kw["band"], kw["tail"], None, kw["summary"], None, None, kw["ws"])
    rc, msg = call(base)
    assert rc == -4 and "before pime_env_reset" in msg and (summary == -777.0).all()
    env.reset()
    cases = [("P = 0", dict(P=0)), ("P = -3", dict(P=-3)), ("exceed 2^31 - 1", dict(P=2 ** 28)), ("excite is NULL", dict(ex=None)),
             ("wave is NULL", dict(wv=None)), ("wave_len 23", dict(wl=23)), ("wave_len 60", dict(wl=N_STEPS)),
             ("wave_len 24", dict(seg_len=0, sp=None, n_sp=0)),
             ("summary is NULL", dict(summary=None)), ("workspace is NULL", dict(ws=None)), ("priorK is NULL", dict(K=None)),
             ("packed_actor is NULL", dict(code=2, md=64)), ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))),
             ("band", dict(band=float("inf"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)), ("n_setpoints 17", dict(n_sp=17)),
             ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)), ("set-point schedule", dict(seg_len=-1))]
    bad = []
    for word, over in cases:
        rc, msg = call(dict(base, **over))
        if rc != -1 or word not in msg or "pime_freq_sweep" not in msg or not (summary == -777.0).all():
            bad.append((word, rc, msg))
    assert not bad, bad
    rc, msg = call(base)          # and the good call goes through
    assert rc == 0 and not (summary == -777.0).any(), msg
    for rows, wave in (([[3, 0.1, 0]], np.ones((1, 4, 2))), ([[0, float("nan"), 0]], np.ones((1, 4, 2))), ([[0, 0.1, -1]], np.ones((1, 4, 2))),
                       ([[0, 0.1, 0]], np.ones((1, 5, 2))), ([[0, 0.1, 0]], np.full((1, 4, 2), float("inf")))):
        with pytest.raises(ValueError):
            env.frequency_sweep(None, K, rows, wave, 4)
    env.close()


# ---- 5. train.py -----------------------------------------------------------------------------------------------------------------
def test_train_bode_writes_the_file(tmp_path, capsys):
    import os
    from pime_amd import protocols, train
    common = ["--algo", "ResidualIntegratorModularPPO", "--env", "NonLinearWaterTankChangingParamUniformGoalIntegrator-SquareDistance-v2",
              "--net_dim", "64", "--num_envs", "64", "--target_step", str(64 * 200), "--batch_size", "2048", "--repeat_times", "2",
              "--break_step", str(64 * 200), "--eval_times1", "8", "--eval_times2", "16", "--eval_gap", "1"]
    train.main(common + ["--bode", "--bode_points", "6", "--bode_amplitude", "0.02", "--log_root", str(tmp_path / "a")])
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "frequency_response.npz"]
    assert len(found) == 1
    z = np.load(found[0], allow_pickle=False)
    Fq = len(np.unique(np.rint(np.geomspace(1, 124, 6))))
    assert z["rows"].shape == (2 * Fq, 3) and (z["rows"][:, 1] == 0.02).all() and (z["rows"][:, 2] == 250).all() and int(z["onset"]) == 250
    assert (z["rows"][:Fq, 0] == 0).all() and (z["rows"][Fq:, 0] == 1).all() and z["omega"].shape == (2 * Fq,)
    np.testing.assert_allclose(z["omega"], 2 * np.pi * z["cycles"] / 250, rtol=1e-9)
    np.testing.assert_array_equal(z["plants"], protocols.WT_ROBUST_PLANTS)
    n = len(protocols.WT_ROBUST_PLANTS)
    for who in ("agent", "prior"):
        assert z[f"{who}_pairs"].shape == (5, 16, 2 * Fq, n) and np.isfinite(z[f"{who}_pairs"]).all()
        assert z[f"{who}_T"].shape == z[f"{who}_L"].shape == (2 * Fq, 5, n)
        assert np.isfinite(z[f"{who}_T"][:Fq]).all() and np.isfinite(z[f"{who}_L"][Fq:]).all() and np.isnan(z[f"{who}_L"][:Fq]).all()
        for k in ("gain_margin", "phase_margin", "peak_S", "bandwidth"):
            assert z[f"{who}_{k}"].shape == (5, n), (who, k)
        assert np.isfinite(z[f"{who}_peak_S"]).all()
    assert not F.bits_equal(z["agent_pairs"], z["prior_pairs"]), "the trained residual is not the prior alone"
    out = capsys.readouterr().out
    assert "worst plant gain margin: agent" in out and "worst plant phase margin: agent" in out and ", prior " in out
    import argparse
    from pime_amd import gym_control
    assert train.bode(argparse.Namespace(env=gym_control.WT_STACKING.format(4)), None, str(tmp_path / "b")) is None
    assert "bode skipped" in capsys.readouterr().out
