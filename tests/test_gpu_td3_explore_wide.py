"""Fused TD3 exploration and evaluation at width 256 and on the Stacking observations (csrc/mlp16.hip: rollout16_offpolicy_kernel
and the TD3 instantiation of rollout16_kernel's evaluation mode; csrc/rollout_offpolicy.hip: the ENV 2 variants; csrc/rollout_eval.hip:
KIND = MLP_CRITIC).

  1. the shapes are served at all (AgentOffPolicy._fused_explore, AgentTD3.fused_eval_policy);
  2. one launch against the lock-step path it replaces, the method and tolerance (2e-4) of
     test_gpu_td3.py::test_fused_offpolicy_explore_matches_lock_step_launches: two calls of 12 + 18 lock-steps, 10-step episodes, a
     20-slot ring -- episodes end and the ring wraps inside the test;
  3. pH at width 256 against the oracle: stored actions (oracle.critic_forward + oracle.explore_noise, 5e-5 as
     test_gpu_td3.py::test_config2_...) and the transitions replayed through OraclePH with the cell rule and the 2e-5 of
     tests/rollout_replay.py::replay_through_oracle;
  4. no stray writes (test_gpu_ragged_lanes.py's guarded ring);
  5. hand-over of the Stacking frame ring to the step-per-launch kernels;
  6. tiling independence: test_gpu_rollout_oracle.py::test_quad_and_narrow_tilings_give_the_same_bits establishes BIT equality of the
     QUAD and the 16-lane-tile tilings for the PPO width-256 rollout (("WT_STACKING10", "ResidualPPO", 1000, 256)), so bit-equal ring
     rows are required here;
  7. evaluation against the lock-step evaluator (rtol 1e-4, atol 1e-3: test_gpu_ragged_lanes.py);
  8. refusals."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNKS, MAX_STEP, SLOTS = (12, 18), 10, 20
EXTRA = 7   # a third call that stops MID-episode (step 7 of 10): the hand-over test needs frames that differ from each other


def _env_id(name):
    from pime_amd import gym_control
    return gym_control.WT_STACKING.format(int(name[len("WT_STACKING"):])) if name.startswith("WT_STACKING") else getattr(gym_control, name)


def _make_env(name, N, seed=6, env_offset=0, max_step=MAX_STEP, **kw):
    from pime_amd import gym_control
    if name == "PH_V35":
        kw = dict(max_episode_steps=max_step, **kw)
    else:
        kw = dict(reward_type="distance", max_step=max_step, **kw)
    return gym_control.make_vec(_env_id(name), N, device=DEV, state_mode="mixed", seed=seed, env_offset=env_offset, **kw)


def _make_agent(env, md, residual=True, fused=True):
    from pime_amd.elegantrl.agent import AgentTD3
    from pime_amd.elegantrl.agent_residual import AgentResidualTD3
    torch.manual_seed(0)
    ag = (AgentResidualTD3 if residual else AgentTD3)(device=DEV)
    ag.use_fused_rollout = fused
    ag.init(md, env.state_dim, 1)
    if residual:
        ag.init_residual({"init_K": env.K.reshape(-1, 1)})
    with torch.no_grad():
        ag.act.net[-1].weight.normal_(0, 0.05)   # a non-trivial residual
        ag.act.net[-1].bias.normal_(0, 0.05)
    return ag


# ---- 1. served at all -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("md,env_name", [(256, "WT_STACKING10"), (256, "WT_INTEGRATOR"), (256, "PH_V35"), (128, "WT_STACKING10"),
                                         (64, "WT_STACKING4")])
def test_exploration_is_served(md, env_name):
    from pime_amd.elegantrl.replay import VecReplayBuffer
    N = 33
    env = _make_env(env_name, N)
    ag = _make_agent(env, md)
    assert ag._fused_explore(env) is not None
    buf = VecReplayBuffer(SLOTS * N, N, env.state_dim, 1, DEV)
    stepwise = env.step
    env.step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused exploration must not step launch by launch"))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ag.explore_env(env, buf, 12 * N, 1.0, 0.99) == 12 * N
    env.step = stepwise
    torch.cuda.synchronize()
    assert not [x for x in w if issubclass(x.category, RuntimeWarning)]
    assert buf.stored_slots == 12 and int((buf.other[:12, :, 1] == 0).sum()) == N
    env.close()


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("md,env_name", [(64, "WT_INTEGRATOR"), (256, "WT_STACKING10")])
def test_evaluation_is_served(md, env_name, residual):
    env = _make_env(env_name, 33)
    ag = _make_agent(env, md, residual)
    fused = ag.fused_eval_policy(env)
    assert fused is not None
    pk, k = fused
    assert pk.kind == "critic" and pk.md == md
    if residual:   # the sign and composition of AgentResidualTD3.eval_policy: act(s) + s @ act.priorK, priorK = -K
        np.testing.assert_array_equal(k, -env.K.reshape(-1))
        np.testing.assert_array_equal(k.astype(np.float32), ag.act.priorK.detach().cpu().numpy().reshape(-1))
    else:
        assert k.shape == (env.state_dim,) and not k.any()
    ag.use_fused_rollout = False
    assert ag.fused_eval_policy(env) is None
    env.close()


# ---- 2. / 5. one launch against the lock-step path --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(md, env_name, N):
    """Both paths on twin envs: (fused, lock-step), each a dict of the per-lock-step ring rows of the two calls (+ the third, EXTRA
    lock-steps), the observation the agent holds afterwards, env.observe() and one further step-per-launch env step."""
    from pime_amd.elegantrl.replay import VecReplayBuffer
    chunks = CHUNKS + (EXTRA,)

    def run(fused, noise_from=None):
        env = _make_env(env_name, N)
        ag = _make_agent(env, md, fused=fused)
        buf = VecReplayBuffer(SLOTS * N, N, env.state_dim, 1, DEV)
        orig, it = torch.randn_like, iter(range(sum(chunks)))
        if noise_from is not None:   # eps = (a - tanh(mean)) / 0.1 reproduces the stored action exactly, clipped or not
            f_states, f_other = noise_from

            def replay_noise(a, **k):
                t = next(it)
                return (f_other[t][:, 2].reshape(a.shape) - torch.tanh(ag.act.net(f_states[t]))) / ag.explore_noise
            torch.randn_like = replay_noise
        states, other = [], []
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                for chunk in chunks:
                    base = buf.next_slot
                    assert ag.explore_env(env, buf, chunk * N, 0.5, 0.98) == chunk * N
                    for j in range(chunk):
                        states.append(buf.state[(base + j) % buf.slots].clone())
                        other.append(buf.other[(base + j) % buf.slots].clone())
        finally:
            torch.randn_like = orig
        torch.cuda.synchronize()
        assert buf.slots == SLOTS and buf.if_full and buf.next_slot == sum(chunks) % SLOTS
        assert (ag._fused_explore(env) is not None) == fused
        out = {"states": states, "other": other, "obs": ag._obs.clone(), "observe": env.observe().clone(),
               "warnings": [x for x in w if issubclass(x.category, RuntimeWarning)]}
        nxt, rew, done = env.step(torch.full((N,), 0.3, device=DEV), auto_reset=True)   # a step-per-launch kernel continues
        out["step"] = (nxt.clone(), rew.clone(), done.clone())
        torch.cuda.synchronize()
        env.close()
        return out

    f = run(True)
    return f, run(False, noise_from=(f["states"], f["other"]))


PAIR_CASES = [(256, "WT_STACKING10", 33),     # QUAD, ragged tile
              (256, "WT_STACKING10", 4100),   # 16-lane tiles (one per wave), ragged last tile
              (256, "WT_STACKING4", 33), (256, "WT_STACKING1", 33), (256, "WT_INTEGRATOR", 33),
              (128, "WT_STACKING10", 33),     # QUAD refused: the exchange buffers do not fit behind the image
              (64, "WT_STACKING4", 33), (64, "WT_STACKING1", 4100)]


@pytest.mark.parametrize("md,env_name,N", PAIR_CASES)
def test_one_launch_matches_the_lock_step_path(md, env_name, N):
    f, s = _pair(md, env_name, N)
    assert not f["warnings"]
    n_done = 0
    for t in range(sum(CHUNKS)):
        torch.testing.assert_close(s["states"][t], f["states"][t], rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(s["other"][t], f["other"][t], rtol=2e-4, atol=2e-4)
        assert torch.equal(s["other"][t][:, 1], f["other"][t][:, 1]), "masks (episode ends) must agree exactly"
        n_done += int((f["other"][t][:, 1] == 0).sum())
    assert n_done == 3 * N      # 30 lock-steps of 10-step episodes
    assert float(torch.stack(f["other"])[:, :, 2].std()) > 0.03, "the exploration noise must show in the stored actions"


@pytest.mark.parametrize("md,env_name,N", [(256, "WT_STACKING10", 33), (256, "WT_STACKING4", 33), (128, "WT_STACKING10", 33),
                                           (64, "WT_STACKING4", 33)])
def test_hand_over_to_the_step_per_launch_kernels(md, env_name, N):
    f, s = _pair(md, env_name, N)
    D = f["obs"].shape[1]
    assert torch.equal(f["observe"], f["obs"]), "env.observe() after the launch must be the observation the kernel wrote back"
    assert D >= 12 and not torch.equal(f["obs"][:, D - 3:D - 1], f["obs"][:, D - 6:D - 4])   # mid-episode: the newest frames differ
    torch.testing.assert_close(s["obs"], f["obs"], rtol=2e-4, atol=2e-4)
    for got, want in zip(f["step"][:2], s["step"][:2]):   # the frames and the ring head the launch left behind
        torch.testing.assert_close(got, want, rtol=2e-4, atol=2e-4)
    assert torch.equal(f["step"][2], s["step"][2])
    torch.testing.assert_close(f["step"][0][:, :D - 3], f["obs"][:, 3:], rtol=0, atol=0)   # one frame older, same frames


# ---- 3. pH at width 256 through the oracle ---------------------------------------------------------------------------
def test_ph_width_256_replays_through_the_oracle():
    import oracle
    from pime_amd.elegantrl.replay import VecReplayBuffer
    N, seed, offset, T, steps = 1000, 11, 8192, 20, 30
    env = _make_env("PH_V35", N, seed=seed, env_offset=offset, max_step=T)
    ag = _make_agent(env, 256)
    buf = VecReplayBuffer(steps * N, N, 3, 1, DEV)
    assert ag._fused_explore(env) is not None
    assert ag.explore_env(env, buf, steps * N, 1.0, 0.99) == steps * N and buf.stored_slots == steps
    torch.cuda.synchronize()
    state, other = buf.state[:steps].cpu().numpy(), buf.other[:steps].cpu().numpy()
    sd = {k: v.detach().cpu().numpy() for k, v in ag.act.state_dict().items()}
    for t in range(steps):   # the stored action: clamp(tanh(actor(s)) + 0.1 * eps, -1, 1), eps the oracle's Philox stream-2 draw
        mean = oracle.critic_forward(state[t], sd)[:, 0]
        want = np.clip(np.tanh(mean) + np.float32(0.1) * oracle.explore_noise(ag._rollout_seed, offset, N, 1, t), -1.0, 1.0)
        np.testing.assert_allclose(other[t, :, 2], want, rtol=0, atol=5e-5, err_msg=f"stored action, step {t}")
    assert float(np.abs(other[:, :, 2]).max()) <= 1.0
    # the env side (rollout_replay.py: replay_through_oracle, pH): the env action is the float64 sum the kernel forms
    priorK = ag._rollout_priorK()
    ref = oracle.OraclePH(N, oracle.ph_table(), max_steps=T, seed=seed, env_offset=offset)
    np.testing.assert_array_equal(state[0], ref.reset())
    alive, cell_exact, rtol = np.ones(N, dtype=bool), [], 2e-5
    for t in range(steps - 1):   # slot t + 1 is stored for t < steps - 1
        a_env = other[t, :, 2].astype(np.float64)
        for j in range(3):
            a_env = a_env + state[t][:, j].astype(np.float64) * priorK[j]
        obs, _, rew, d = ref.step(a_env, auto_reset=True)
        assert bool(d.all()) == (t % T == T - 1) and bool(d.any()) == bool(d.all())
        np.testing.assert_array_equal(other[t, :, 1] == 0, d)
        np.testing.assert_array_equal(other[t, :, 1][~d], np.float32(0.99))
        if t % T == T - 1:   # the next slot holds the next episode's first observation: the last step shows in its reward only
            alive &= np.abs(other[t, :, 0] - rew) <= rtol * (1.0 + np.abs(rew))
            cell_exact.append(alive.mean())
            np.testing.assert_array_equal(state[t + 1], obs)
            alive[:] = True
            continue
        alive &= np.abs(state[t + 1][:, 0] - obs[:, 0]) <= 1e-5
        np.testing.assert_allclose(other[t, :, 0][alive], rew[alive], rtol=rtol, atol=rtol)
        np.testing.assert_allclose(state[t + 1][alive], obs[alive], rtol=rtol, atol=rtol)
    cell_exact.append(alive.mean())
    assert min(cell_exact) >= 1.0 - 1e-4, f"only {min(cell_exact):.5f} of the lanes stayed cell-exact over an episode"
    env.close()


# ---- 4. no stray writes ----------------------------------------------------------------------------------------------
def test_guarded_ring_on_stacking10_at_width_256():
    from pime_amd.elegantrl.replay import VecReplayBuffer
    N = 33
    env = _make_env("WT_STACKING10", N, seed=9)
    ag = _make_agent(env, 256)
    buf = VecReplayBuffer(30 * N, N, env.state_dim, 1, DEV)
    big_s = torch.full((buf.state.numel() + 64,), 7.0, device=DEV)
    big_o = torch.full((buf.other.numel() + 64,), 7.0, device=DEV)
    buf.state = big_s[:buf.state.numel()].view(buf.state.shape).zero_()
    buf.other = big_o[:buf.other.numel()].view(buf.other.shape).zero_()
    buf.buf_state, buf.buf_other = buf.state.view(buf.max_len, -1), buf.other.view(buf.max_len, -1)
    assert ag._fused_explore(env) is not None
    assert ag.explore_env(env, buf, 25 * N, 1.0, 0.99) == 25 * N
    torch.cuda.synchronize()
    assert bool((big_s[-64:] == 7).all()) and bool((big_o[-64:] == 7).all()), "stray write behind the ring"
    ended = (buf.other[:25, :, 1] == 0).sum(dim=0)
    assert bool((ended == 2).all()), "every lane ends exactly two 10-step episodes in 25 lock-steps"
    assert bool((buf.other[25:] == 0).all()) and bool((buf.state[25:] == 0).all()), "slots beyond the explored ones must be untouched"
    assert bool((buf.other[:25, :, 2] != 0).all()) and bool((buf.state[:25] != 0).any(dim=2).all()), "every explored row is written"
    env.close()


# ---- 6. tiling independence ------------------------------------------------------------------------------------------
def test_a_lane_does_not_depend_on_the_tiling():
    """The same 48 lanes as one 48-lane env (QUAD: one tile per workgroup) and as the last 48 of a 4 100-lane env (16-lane tiles, one
    per wave, other tile boundaries, the ragged last workgroup): bit-equal ring rows."""
    from pime_amd.elegantrl.replay import VecReplayBuffer
    big_n, n, off, steps = 4100, 48, 1000, 12
    lo = big_n - n
    rows = []
    for N, env_offset in ((n, off + lo), (big_n, off)):
        env = _make_env("WT_INTEGRATOR", N, seed=21, env_offset=env_offset)
        ag = _make_agent(env, 256)
        buf = VecReplayBuffer(SLOTS * N, N, env.state_dim, 1, DEV)
        assert ag._fused_explore(env) is not None
        assert ag.explore_env(env, buf, steps * N, 1.0, 0.99) == steps * N
        torch.cuda.synchronize()
        sl = slice(N - n, N)
        rows.append((buf.state[:steps, sl].clone(), buf.other[:steps, sl].clone(), ag._obs[sl].clone()))
        env.close()
    for a, b, what in zip(rows[0], rows[1], ("ring state", "ring (reward, mask, action)", "observation after the launch")):
        assert torch.equal(a, b), what
    assert int((rows[0][1][:, :, 1] == 0).sum()) == n


# ---- 7. evaluation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("md,env_name,N,residual", [(64, "WT_INTEGRATOR", 33, True), (128, "PH_V35", 33, True),
                                                    (256, "WT_INTEGRATOR", 1000, True), (256, "WT_STACKING10", 33, True),
                                                    (256, "WT_STACKING10", 33, False)])
def test_fused_evaluation_matches_the_lock_step_evaluator(md, env_name, N, residual):
    from pime_amd import native
    from pime_amd.elegantrl.run import Evaluator, get_episode_return_vec
    envs = [_make_env(env_name, N, seed=9, max_step=25) for _ in range(2)]
    ag = _make_agent(envs[0], md, residual)
    policy = Evaluator._policy(ag)
    assert (policy == ag.eval_policy) if residual else (policy is ag.act)
    fused = ag.fused_eval_policy(envs[0])
    assert fused is not None
    stepwise = envs[0].step
    envs[0].step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused evaluation must not step launch by launch"))
    got = get_episode_return_vec(envs[0], policy, fused=fused)
    envs[0].step = stepwise
    slow = get_episode_return_vec(envs[1], policy)
    assert got.shape == (N,) and np.isfinite(got).all() and float(np.std(got)) > 0
    np.testing.assert_allclose(got, slow, rtol=1e-4, atol=1e-3)
    if env_name == "WT_STACKING10":   # returns and trace, but no set-point schedule on a Stacking observation
        assert envs[0].eval_supported(fused[0]) and envs[0].eval_supported(fused[0], trace=True)
        assert not envs[0].eval_supported(fused[0], schedule=True)
        envs[0].reset()
        with pytest.raises(native.PimeError, match="set-point schedule"):
            envs[0].rollout_eval(fused[0], fused[1], 10, setpoints=[3.0, 6.0], seg_len=5)
    else:
        assert envs[0].eval_supported(fused[0], trace=True, schedule=True)
    for e in envs:
        e.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    from pime_amd import gym_control, native
    lib = native.lib()
    N = 33
    two = gym_control.make_vec(gym_control.WT_STACKING.format(4), N, device=DEV, state_mode="mixed", seed=1, reward_type="distance",
                               max_step=MAX_STEP, num_stack=2, P_control_K=np.array([0., 0., 0., 0., 0.4, -0.4]))
    f64 = gym_control.make_vec(gym_control.WT_INTEGRATOR, N, device=DEV, state_mode="f64", seed=1, reward_type="distance", max_step=MAX_STEP)
    for env in (two, f64):
        env.reset()
        D = env.state_dim
        assert D == (6 if env is two else 4)
        for md in (64, 128, 256):
            assert lib.pime_rollout_offpolicy_supported(env._h, md) == 0
        ag = _make_agent(env, 256)
        assert ag._fused_explore(env) is None
        pk = ag._packed_actor().repack()
        obs = torch.zeros((N, D), device=DEV)
        ring_s, ring_o = torch.zeros((4, N, D), device=DEV), torch.zeros((4, N, 3), device=DEV)
        k = np.zeros(D)
        import ctypes as C
        rc = lib.pime_rollout_offpolicy(env._h, 256, native.ptr(pk.packed), native.ptr(k), C.c_float(0.1), C.c_float(0.99), C.c_float(1.0),
                                        2, C.c_uint64(1), C.c_uint32(1), native.ptr(obs), native.ptr(ring_s), native.ptr(ring_o), 0, 4,
                                        env._stream())
        torch.cuda.synchronize()
        assert rc == -1 and "not served" in native.last_error()   # PIME_ERR_ARG, with a message
        assert not ring_s.any() and not ring_o.any()
    # SAC's served shapes did not move: nothing at width 256, nothing on a Stacking observation
    st10 = _make_env("WT_STACKING10", N)
    tank = _make_env("WT_INTEGRATOR", N)
    ph = _make_env("PH_V35", N)
    for env in (st10, tank, ph, two):
        assert lib.pime_rollout_offpolicy_sac_supported(env._h, 256) == 0
    for md in (64, 128):
        assert lib.pime_rollout_offpolicy_sac_supported(st10._h, md) == 0 and lib.pime_rollout_offpolicy_sac_supported(two._h, md) == 0
        assert lib.pime_rollout_offpolicy_sac_supported(tank._h, md) == 1 and lib.pime_rollout_offpolicy_sac_supported(ph._h, md) == 1
    assert lib.pime_sac_supported(4, 1, 256) == 0 and lib.pime_sac_supported(30, 1, 128) == 0 and lib.pime_sac_supported(4, 1, 128) == 1
    assert lib.pime_rollout_eval_supported(st10._h, native.MLP_SAC_ACTOR, 256) == 0
    assert lib.pime_rollout_eval_supported(st10._h, native.MLP_CRITIC, 128) == 0   # Stacking evaluation at widths 64 / 128: unserved
    for env in (two, f64, st10, tank, ph):
        env.close()
