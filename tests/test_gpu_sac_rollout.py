"""AgentSAC's fused exploration and evaluation (the SAC mode of csrc/rollout_offpolicy.hip / rollout_eval.hip, packed-image kind
PIME_MLP_SAC_ACTOR) against the oracle envs and the float64 actor of tests/sac_oracle.py:

  * one explore call = ONE launch: the stored action is the oracle's tanh(avg + exp(clamp(log_std)) * eps) of the stored observation
    with eps the oracle's Philox stream-2 draw (3e-5), the env side replays through OracleWT / OraclePH on the recorded actions
    (observations and rewards at the mode's 2e-4 / 2e-5, masks and ring slots exact, reset observations bit-equal);
  * the 32-lane forward of the same image (pime_mlp_forward: the mean head) at 3e-5;
  * one evaluation episode = ONE launch: the trace's env action is the oracle's tanh(avg) of the observation the policy saw (3e-5),
    returns agree with the launch-by-launch evaluator;
  * a width-256 actor explores lock-step by lock-step, with one RuntimeWarning."""
import numpy as np
import pytest
import torch

import sac_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _agent(env, md, seed=0):
    from pime_amd.elegantrl.agent_sac import AgentSAC
    torch.manual_seed(seed)
    ag = AgentSAC(device=DEV)
    ag.init(md, env.state_dim, 1)
    with torch.no_grad():   # heads away from their tiny initial scale: a mean that matters, log-stds on both sides of 0
        ag.act.net_a_avg.weight.normal_(0, 0.08)
        ag.act.net_a_std.weight.normal_(0, 0.08)
        ag.act.net_a_std.bias.fill_(-1.0)
    return ag


def _actor_f64(ag):
    return S.f64({k: v.detach().cpu().numpy() for k, v in ag.act.state_dict().items()}, S.ACTOR_KEYS)


@pytest.mark.parametrize("env_name,N,md", [("WT_INTEGRATOR", 4096, 128), ("WT_INTEGRATOR", 4608, 64), ("PH_V35", 2048, 128),
                                            ("PH_V35", 4608, 64)])   # 4 608 lanes: the 16-lane-tile (non-QUAD) instantiation
def test_fused_exploration_replays_through_the_oracle(env_name, N, md):
    import oracle
    from pime_amd import gym_control
    from pime_amd.elegantrl.run import make_buffer
    is_ph = env_name == "PH_V35"
    seed, offset = 11, 8192
    kw = {} if is_ph else dict(reward_type="distance", max_step=40)
    env = gym_control.make_vec(getattr(gym_control, env_name), N, device=DEV, state_mode="mixed", seed=seed, env_offset=offset, **kw)
    T = env.max_step
    steps = T + 12                          # one in-kernel auto-reset (with ensemble resampling) inside the call
    ag = _agent(env, md)
    buf = make_buffer(ag, env, 2 * steps * N)
    assert ag._fused_explore(env) is not None, "this configuration must explore through pime_rollout_offpolicy_sac"
    stepwise = env.step
    env.step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused exploration must not step launch by launch"))
    assert ag.explore_env(env, buf, steps * N, 0.5, 0.98) == steps * N and buf.stored_slots == steps and buf.next_slot == steps
    env.step = stepwise
    torch.cuda.synchronize()
    state, other = buf.state[:steps + 1].cpu().numpy(), buf.other[:steps].cpu().numpy()
    act = _actor_f64(ag)
    for t in range(steps):   # the stored (squashed) action, from the observation the kernel saw and the oracle's draw
        eps = oracle.explore_noise(ag._rollout_seed, offset, N, 1, t)
        f = S.actor_forward(act, state[t].astype(np.float64), eps)
        np.testing.assert_allclose(other[t, :, 2], f["a"][:, 0], rtol=0, atol=3e-5, err_msg=f"stored action, step {t}")
    assert float(np.abs(other[:, :, 2]).max()) < 1.0 and float(other[:, :, 2].std()) > 0.1
    ref = oracle.OraclePH(N, oracle.ph_table(), seed=seed, env_offset=offset) if is_ph else \
        oracle.OracleWT(N, max_steps=T, reward_type="distance", seed=seed, env_offset=offset)
    np.testing.assert_array_equal(state[0], ref.reset())
    tol = 2e-5 if is_ph else 2e-4
    alive = np.ones(N, dtype=bool)          # pH: lanes still in the oracle's titration cell (tests/rollout_replay.py)
    for t in range(steps - 1):              # slot t + 1 is stored for t < steps - 1
        obs, _, rew, d = ref.step(other[t, :, 2].astype(np.float64), auto_reset=True)   # priorK = 0: the env sees the stored action
        assert bool(d.all()) == (t == T - 1) and bool(d.any()) == bool(d.all())
        np.testing.assert_array_equal(other[t, :, 1] == 0, d)                          # masks: 0 where the episode ended
        np.testing.assert_array_equal(other[t, :, 1][~d], np.float32(0.98))
        ok = np.abs(other[t, :, 0] - 0.5 * rew) <= tol * (1.0 + np.abs(0.5 * rew))
        if t == T - 1:      # the slot behind holds the next episode's first observation: the last step shows in its reward only
            assert ok[alive].mean() >= 1.0 - 1e-3 if is_ph else ok.all(), f"reward * scale, step {t}"
            np.testing.assert_array_equal(state[t + 1], obs)    # Philox reset draws + LUT: float32 observation bit-equal
            alive[:] = True
            continue
        if is_ph:
            alive &= np.abs(state[t + 1][:, 0] - obs[:, 0]) <= 1e-5
        assert ok[alive].all(), f"reward * scale, step {t}"
        np.testing.assert_allclose(state[t + 1][alive], obs[alive], rtol=tol, atol=tol, err_msg=f"observation, step {t}")
        if not is_ph:
            for name, col in (("h1", 0), ("h2", 1), ("I", 3)):      # re-sync the fp64 oracle to the kernel's f32 state
                ref.set(name, state[t + 1][:, col].astype(np.float64))
    assert alive.mean() >= 1.0 - 1e-3
    # a second call continues the episodes and the ring
    obs_before = ag._obs.clone()
    assert ag.explore_env(env, buf, 3 * N, 0.5, 0.98) == 3 * N and buf.next_slot == steps + 3 and ag._rollout_epoch == 2
    assert torch.equal(buf.state[steps], obs_before)
    env.close()


@pytest.mark.parametrize("md,D", [(128, 4), (64, 3)])
def test_packed_image_forward_is_the_mean_head(md, D):
    from pime_amd.backend import HipBackend
    from pime_amd.elegantrl.net import ActorSAC
    torch.manual_seed(3)
    act = ActorSAC(md, D, 1).to(DEV)
    with torch.no_grad():
        act.net_a_avg.weight.normal_(0, 0.1)
    pk = HipBackend().packed(act)
    assert pk is not None and pk.kind == "sac_actor"
    x = (torch.rand(1000, D, device=DEV) * 10 - 3).contiguous()
    got = pk(x).cpu().numpy()
    f = S.actor_forward(S.f64({k: v.detach().cpu().numpy() for k, v in act.state_dict().items()}, S.ACTOR_KEYS), x.cpu().numpy().astype(np.float64))
    np.testing.assert_allclose(got, f["avg"][:, 0], rtol=0, atol=3e-5)


@pytest.mark.parametrize("N,md", [(2048, 128), (4608, 64)])
def test_fused_ph_evaluation_from_its_trace(N, md):
    """The kernel's trace mode records every step's observation and env action: the action is tanh(net_a_avg(observation)) of the
    float64 actor (3e-5) at every step, and replaying the recorded actions through OraclePH reproduces rewards and returns (2e-5)."""
    import oracle
    from pime_amd import gym_control
    seed, off = 13, 512
    env = gym_control.make_vec(gym_control.PH_V35, N, device=DEV, state_mode="mixed", seed=seed, env_offset=off)
    ag = _agent(env, md, seed=1)
    fused = ag.fused_eval_policy(env)
    assert fused is not None and env.eval_supported(fused[0], trace=True) and not fused[1].any()
    T = env.max_step
    env.reset()
    ret, tr = env.rollout_eval(fused[0], fused[1], T, want_trace=True)
    torch.cuda.synchronize()
    ret, tr = ret.cpu().numpy(), tr.cpu().numpy()      # tr [T, 6, N]: y, r, I before the step | env action, reward, x after
    ref = oracle.OraclePH(N, oracle.ph_table(), seed=seed, env_offset=off)
    act = _actor_f64(ag)
    ref.reset()
    want_ret = np.zeros(N)
    for t in range(T):
        seen = tr[t, 0:3].T.astype(np.float32)
        want = np.tanh(S.actor_forward(act, seen.astype(np.float64))["avg"][:, 0])
        np.testing.assert_allclose(tr[t, 3], want, rtol=0, atol=3e-5, err_msg=f"tanh(net_a_avg), step {t}")
        _, _, rew, _ = ref.step(tr[t, 3])
        np.testing.assert_allclose(tr[t, 5], ref.get("x"), rtol=1e-12, err_msg=f"plant state x, step {t}")
        np.testing.assert_allclose(tr[t, 4], rew, rtol=2e-5, atol=2e-5, err_msg=f"reward, step {t}")
        want_ret += rew.astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(ret, want_ret, rtol=2e-5, atol=1e-4)
    env.close()


@pytest.mark.parametrize("state_mode", ["mixed", "f64"])
def test_fused_tank_evaluation_matches_the_stepwise_evaluator(state_mode):
    from pime_amd import gym_control
    from pime_amd.elegantrl.run import get_episode_return_vec
    N = 1024
    envs = [gym_control.make_vec(gym_control.WT_INTEGRATOR, N, device=DEV, state_mode=state_mode, seed=5, reward_type="distance",
                                 max_step=60) for _ in range(2)]
    ag = _agent(envs[0], 128, seed=2)
    fused = ag.fused_eval_policy(envs[0])
    assert fused is not None
    stepwise = envs[0].step
    envs[0].step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused evaluation must not step launch by launch"))
    got = get_episode_return_vec(envs[0], ag.act, fused=fused)
    envs[0].step = stepwise
    slow = get_episode_return_vec(envs[1], ag.act)
    np.testing.assert_allclose(got, slow, rtol=1e-4, atol=1e-3)
    for e in envs:
        e.close()


def test_wide_actor_explores_lock_step_with_one_warning():
    import warnings
    from pime_amd import gym_control
    from pime_amd.elegantrl.run import make_buffer
    N = 256
    env = gym_control.make_vec(gym_control.WT_INTEGRATOR, N, device=DEV, state_mode="mixed", seed=3, reward_type="distance", max_step=20)
    ag = _agent(env, 256)
    buf = make_buffer(ag, env, 64 * N)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ag._fused_explore(env) is None and ag.fused_eval_policy(env) is None
        assert ag.explore_env(env, buf, 25 * N, 1.0, 0.99) == 25 * N and buf.stored_slots == 25
    assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == 1
    assert float(buf.other[:25, :, 2].abs().max()) < 1.0 and int((buf.other[:25, :, 1] == 0).sum()) == N
    env.close()
