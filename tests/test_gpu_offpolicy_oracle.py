"""Every instantiation of the fused off-policy exploration (`pime_rollout_offpolicy`, `pime_rollout_offpolicy_sac`) and of the fused
evaluation under the TD3 Actor / ActorSAC (`pime_rollout_eval`), replayed lane by lane through the float64 oracle by
tests/offpolicy_replay.py (vetted on the CPU by tests/test_offpolicy_replay_cpu.py: what it checks, with which bar, and which faults it
sees).  The lock-step comparisons of test_gpu_td3.py / test_gpu_td3_explore_wide.py feed the lock-step run with the fused run's own
noise and cannot see the actor or the draw; here both come from the oracle.

Shapes: 81 lanes (16-lane tiling: one full workgroup + a ragged one; QUAD: five full tiles + a single-lane tile) at lane offset 8192,
episodes of 10 steps (14 on Stacking10: a fully distinct 10-frame window occurs), three explore_env calls of (12, 18, 7) lock-steps on
a 20-slot VecReplayBuffer (the ring wraps, episodes end inside calls, the last call stops mid-episode), reward_scale 0.5, gamma 0.98.
The tiling is forced with PIME_ROLLOUT_NARROW = 2 (QUAD) / 1 (16-lane tiles, one per wave).

Test id -> instantiation (T = width / 32; ENV 0 pH, 1 Integrator tank, 2 Stacking tank; S = frames):
  exploration, test_exploration_replays_through_the_oracle[...]
    td3-{64,128}-PH_V35-{quad,narrow}          rollout_offpolicy_kernel<{2,4}, 0, {true,false}, MLP_CRITIC>
    td3-{64,128}-WT_INTEGRATOR-{quad,narrow}   rollout_offpolicy_kernel<{2,4}, 1, {true,false}, MLP_CRITIC>
    td3-{64,128}-WT_STACKING{1,4,10}-{quad,narrow}   rollout_offpolicy_kernel<{2,4}, 2, {true,false}, MLP_CRITIC, {1,4,10}>
        except td3-128-WT_STACKING10-quad: that instantiation is never launched (image + exchange buffers exceed the LDS) --
        td3-128-WT_STACKING10-only runs <4, 2, false, MLP_CRITIC, 10> under the QUAD request and asserts the arithmetic
    td3-256-PH_V35-{quad,narrow}               rollout16_offpolicy_kernel<16, 0, 0, {true,false}>
    td3-256-WT_INTEGRATOR-{quad,narrow}        rollout16_offpolicy_kernel<16, 1, 0, {true,false}>
    td3-256-WT_STACKING{1,4,10}-{quad,narrow}  rollout16_offpolicy_kernel<16, 2, {1,4,10}, {true,false}>
    sac-{64,128}-PH_V35-{quad,narrow}          rollout_offpolicy_kernel<{2,4}, 0, {true,false}, MLP_SAC_ACTOR>
    sac-{64,128}-WT_INTEGRATOR-{quad,narrow}   rollout_offpolicy_kernel<{2,4}, 1, {true,false}, MLP_SAC_ACTOR>
    plain-* (AgentTD3, priorK = 0) and clip-* (sigma 0.8: the clamp at both bounds) re-run one of the instantiations above
  evaluation, test_evaluation_trace_replays_through_the_oracle[...]
    {td3,plain}-{64,128}-{PH_V35,WT_INTEGRATOR}-{quad,narrow}   rollout_eval_kernel<{2,4}, MLP_CRITIC, {0,1}, float, {true,false}>
    sac-{64,128}-{PH_V35,WT_INTEGRATOR}-{quad,narrow}           rollout_eval_kernel<{2,4}, MLP_SAC_ACTOR, {0,1}, float, {true,false}>
    {td3,plain}-256-PH_V35-{quad,narrow}                        rollout16_kernel<16, MLP_CRITIC, 0, 0, {true,false}>, eval_mode
    {td3,plain}-256-WT_INTEGRATOR-{quad,narrow}                 rollout16_kernel<16, MLP_CRITIC, 1, 0, {true,false}>, eval_mode
    {td3,plain}-256-WT_STACKING{1,4,10}-{quad,narrow}           rollout16_kernel<16, MLP_CRITIC, 2, {1,4,10}, {true,false}>, eval_mode
Every test prints one "SHARE" line: the largest used share of each bar, for the record of a GPU run."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import offpolicy_replay as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, OFFSET, SEED, SLOTS = 81, 8192, 6, 20
CHUNKS = (12, 18, 7)
GAMMA, SCALE = 0.98, 0.5
CLIP_SIGMA = 0.8
TORCH_SEED = 0x5EED00000007          # the exploration stream follows torch's seed: both key words non-zero
TILES = {"quad": "2", "narrow": "1", "only": "2"}
ENVS = {"PH_V35": ("ph", 0), "WT_INTEGRATOR": ("integrator", 0), "WT_STACKING1": ("stacking", 1), "WT_STACKING4": ("stacking", 4),
        "WT_STACKING10": ("stacking", 10)}
LDS_LIMIT = 160 * 1024


def _max_step(env_name):
    return 14 if env_name == "WT_STACKING10" else 10


def _make_env(env_name, T):
    from pime_amd import gym_control
    stack = ENVS[env_name][1]
    env_id = gym_control.WT_STACKING.format(stack) if stack else getattr(gym_control, env_name)
    kw = dict(max_episode_steps=T) if env_name == "PH_V35" else dict(reward_type="distance", max_step=T)
    return gym_control.make_vec(env_id, N, device=DEV, state_mode="mixed", seed=SEED, env_offset=OFFSET, **kw)


def _make_agent(agent, env, md):
    """agent: "td3" = AgentResidualTD3 with a non-trivial last layer, "plain" = AgentTD3 (priorK = 0), "sac" = AgentSAC."""
    torch.manual_seed(TORCH_SEED + md)
    if agent == "sac":
        from pime_amd.elegantrl.agent_sac import AgentSAC
        ag = AgentSAC(device=DEV)
        ag.init(md, env.state_dim, 1)
        with torch.no_grad():   # heads away from their tiny initial scale (tests/test_gpu_sac_rollout.py)
            ag.act.net_a_avg.weight.normal_(0, 0.08)
            ag.act.net_a_std.weight.normal_(0, 0.08)
            ag.act.net_a_std.bias.fill_(-1.0)
        return ag
    from pime_amd.elegantrl.agent import AgentTD3
    from pime_amd.elegantrl.agent_residual import AgentResidualTD3
    ag = (AgentResidualTD3 if agent == "td3" else AgentTD3)(device=DEV)
    ag.init(md, env.state_dim, 1)
    if agent == "td3":
        ag.init_residual({"init_K": env.K.reshape(-1, 1)})
    with torch.no_grad():
        ag.act.net[-1].weight.normal_(0, 0.05)
        ag.act.net[-1].bias.normal_(0, 0.05)
    return ag


def _spec(agent, env_name, T, ag, priorK):
    env, stack = ENVS[env_name]
    return {"env": env, "num_stack": stack, "T": T, "seed": SEED, "env_offset": OFFSET, "slots": SLOTS, "gamma": GAMMA, "reward_scale": SCALE,
            "kind": "sac" if agent == "sac" else "td3", "priorK": np.asarray(priorK, dtype=np.float64).reshape(-1),
            "actor": {k: v.detach().cpu().numpy() for k, v in ag.act.state_dict().items()}}


def _family(md, what):
    if what == "explore":
        return "rollout16_offpolicy_kernel" if md == 256 else "rollout_offpolicy_kernel"
    return "rollout16_kernel (evaluation)" if md == 256 else "rollout_eval_kernel"


def _report(family, test_id, used):
    print(f"\nSHARE family={family} id={test_id} action={used['action']:.4f} observation={used['observation']:.4f} "
          f"reward={used['reward']:.4f} lanes_out={used['lanes_out']}")


# ---- exploration ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _recording(agent, md, env_name, tiles, sigma=None):
    """(recording, spec) of three explore_env calls; the caller has set PIME_ROLLOUT_NARROW (the launchers read it per launch)."""
    from pime_amd.elegantrl.replay import VecReplayBuffer
    assert os.environ.get("PIME_ROLLOUT_NARROW") == TILES[tiles]
    T = _max_step(env_name)
    env = _make_env(env_name, T)
    ag = _make_agent(agent, env, md)
    if sigma is not None:
        ag.explore_noise = sigma
    buf = VecReplayBuffer(SLOTS * N, N, env.state_dim, 1, DEV)
    assert buf.slots == SLOTS
    assert ag._fused_explore(env) is not None, "this configuration must explore through the fused kernel"
    stepwise = env.step
    env.step = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused exploration must not step launch by launch"))
    states, other, slots, calls = [], [], [], []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for chunk in CHUNKS:
            base, epoch = buf.next_slot, ag._rollout_epoch
            assert ag.explore_env(env, buf, chunk * N, SCALE, GAMMA) == chunk * N
            assert ag._rollout_epoch == epoch + 1, "one launch per call"
            calls.append((ag._rollout_epoch, chunk, base))
            ring_s, ring_o = buf.state.cpu().numpy(), buf.other.cpu().numpy()
            for j in range(chunk):
                s = (base + j) % SLOTS
                states.append(ring_s[s]); other.append(ring_o[s]); slots.append(s)
    env.step = stepwise
    torch.cuda.synchronize()
    assert not [x for x in w if issubclass(x.category, RuntimeWarning)]
    assert buf.if_full and buf.next_slot == sum(CHUNKS) % SLOTS
    names = ("x", "I", "qww_V", "t", "episode") if env_name == "PH_V35" else ("h1", "h2", "a1", "Kp", "t", "episode")
    rec = {"state": np.stack(states), "other": np.stack(other), "slot": np.array(slots), "held": ag._obs.cpu().numpy(),
           "fields": {f: env.get_field(f) for f in names}}
    if ENVS[env_name][1]:   # the frame ring handed over to the step-per-launch kernels
        assert np.array_equal(env.observe().cpu().numpy(), rec["held"]), "env.observe() after the launch is the observation the kernel wrote back"
    spec = _spec(agent, env_name, T, ag, ag._rollout_priorK())
    spec.update(noise_seed=ag._rollout_seed, calls=calls, sigma=None if agent == "sac" else ag._rollout_sigma())
    assert spec["noise_seed"] >> 32 and spec["noise_seed"] & 0xFFFFFFFF
    env.close()
    return rec, spec


def _quad_fits(kind, md, D):
    """The launcher's rule (csrc/rollout_offpolicy.hip: launch_off_t): QUAD needs the image and two exchange buffers of
    (width / 16) tiles x 64 lanes x 4 floats in the LDS."""
    from pime_amd import native
    image = native.lib().pime_mlp_packed_floats(kind, D, 0, md)
    assert image > 0
    return (image + 2 * (md // 16) * 64 * 4) * 4 <= LDS_LIMIT


EXPLORE = []
for _md in (64, 128, 256):
    for _env in ENVS:
        if (_md, _env) == (128, "WT_STACKING10"):
            EXPLORE.append(("td3", _md, _env, "only", None))
        else:
            EXPLORE += [("td3", _md, _env, t, None) for t in ("quad", "narrow")]
EXPLORE += [("sac", md, env, t, None) for md in (64, 128) for env in ("PH_V35", "WT_INTEGRATOR") for t in ("quad", "narrow")]
EXPLORE += [("plain", 64, "PH_V35", "quad", None), ("plain", 128, "WT_INTEGRATOR", "narrow", None), ("plain", 256, "WT_STACKING10", "quad", None)]
EXPLORE += [("td3", 128, "WT_INTEGRATOR", "quad", CLIP_SIGMA), ("td3", 256, "WT_STACKING4", "narrow", CLIP_SIGMA)]   # one per kernel family


def _explore_id(c):
    agent, md, env, tiles, sigma = c
    return f"{'clip' if sigma else agent}-{md}-{env}-{tiles}"


@pytest.mark.parametrize("case", EXPLORE, ids=_explore_id)
def test_exploration_replays_through_the_oracle(case, monkeypatch):
    from pime_amd import native
    agent, md, env_name, tiles, sigma = case
    monkeypatch.setenv("PIME_ROLLOUT_NARROW", TILES[tiles])
    D = R.obs_dim({"env": ENVS[env_name][0], "num_stack": ENVS[env_name][1]})
    if md < 256:   # which tiling the request gets: QUAD wherever it fits, and it fits everywhere but Stacking10 at width 128
        fits = _quad_fits(native.MLP_SAC_ACTOR if agent == "sac" else native.MLP_CRITIC, md, D)
        assert fits == ((md, env_name) != (128, "WT_STACKING10"))
        assert (tiles == "only") == (not fits)
    rec, spec = _recording(agent, md, env_name, tiles, sigma)
    a = rec["other"][:, :, 2]
    assert (rec["other"][:, :, 1] == 0).sum() == N * (sum(CHUNKS) // spec["T"])
    assert float(a.std()) > 0.03, "the exploration noise must show in the stored actions"
    if sigma:
        assert (a == 1).mean() >= 0.01 and (a == -1).mean() >= 0.01, "the clipping case must clip at both bounds"
    if agent == "plain" or agent == "sac":
        assert not spec["priorK"].any()
    else:
        assert spec["priorK"].any()
    if env_name == "WT_STACKING10":
        assert any(len(np.unique(row[0].reshape(10, 3)[:, 0])) == 10 for row in rec["state"]), "no fully distinct 10-frame window"
    used = R.check_exploration(rec, spec)
    _report(_family(md, "explore") + (" (SAC)" if agent == "sac" else ""), _explore_id(case), used)
    assert used["lanes_out"] == 0


@pytest.mark.parametrize("agent,md,env_name", [("td3", 64, "WT_STACKING4"), ("td3", 256, "WT_STACKING10"), ("td3", 256, "WT_INTEGRATOR")])
def test_quad_and_16_lane_tilings_store_the_same_bits(agent, md, env_name, monkeypatch):
    """The same 81 lanes under QUAD and under 16-lane tiles (one per wave): bit-equal ring rows, held observation and env fields --
    the claim of test_gpu_rollout_oracle.py::test_quad_and_narrow_tilings_give_the_same_bits and of
    test_gpu_td3_explore_wide.py::test_a_lane_does_not_depend_on_the_tiling, here on a Stacking observation in both kernel families."""
    recs = []
    for tiles in ("quad", "narrow"):
        monkeypatch.setenv("PIME_ROLLOUT_NARROW", TILES[tiles])
        recs.append(_recording(agent, md, env_name, tiles, None)[0])
    q, n = recs
    for key in ("state", "other", "held"):
        assert np.array_equal(q[key], n[key]), key
    for f in q["fields"]:
        assert np.array_equal(q["fields"][f], n["fields"][f]), f


# ---- evaluation -------------------------------------------------------------------------------------------------------------
EVAL_SERVED = [(md, env) for md in (64, 128, 256) for env in ENVS if md == 256 or not env.startswith("WT_STACKING")]
EVAL = [(agent, md, env, t) for md, env in EVAL_SERVED for agent in ("td3", "plain") for t in ("quad", "narrow")]
EVAL += [("sac", md, env, t) for md in (64, 128) for env in ("PH_V35", "WT_INTEGRATOR") for t in ("quad", "narrow")]


def test_the_evaluation_cases_are_the_served_shapes():
    from pime_amd import native
    lib = native.lib()
    served_td3, served_sac = [], []
    for env_name in ENVS:
        env = _make_env(env_name, _max_step(env_name))
        for md in (64, 128, 256):
            if lib.pime_rollout_eval_supported(env._h, native.MLP_CRITIC, md):
                served_td3.append((md, env_name))
            if lib.pime_rollout_eval_supported(env._h, native.MLP_SAC_ACTOR, md):
                served_sac.append((md, env_name))
        env.close()
    assert sorted(served_td3) == sorted(EVAL_SERVED)
    assert sorted(served_sac) == sorted({(md, env) for a, md, env, _ in EVAL if a == "sac"})


@pytest.mark.parametrize("case", EVAL, ids=lambda c: "-".join(str(x) for x in c))
def test_evaluation_trace_replays_through_the_oracle(case, monkeypatch):
    """One traced launch of T steps.  On a Stacking observation the trace holds the newest frame (h1, h2, r) after each step, not the
    whole observation: the checker rebuilds what the policy saw from the reset observation and the traced frames."""
    agent, md, env_name, tiles = case
    monkeypatch.setenv("PIME_ROLLOUT_NARROW", TILES[tiles])
    T = _max_step(env_name)
    env = _make_env(env_name, T)
    ag = _make_agent(agent, env, md)
    fused = ag.fused_eval_policy(env)
    assert fused is not None and env.eval_supported(fused[0], trace=True)
    pk, k = fused
    assert pk.kind == ("sac_actor" if agent == "sac" else "critic") and pk.md == md
    assert bool(np.any(k)) == (agent == "td3")
    reset_obs = env.reset().cpu().numpy().copy()
    ret, tr = env.rollout_eval(pk, k, T, want_trace=True)
    torch.cuda.synchronize()
    spec = _spec(agent, env_name, T, ag, k)
    used = R.check_evaluation(tr.cpu().numpy(), ret.cpu().numpy(), reset_obs, spec)
    _report(_family(md, "eval") + (" (SAC)" if agent == "sac" else ""), "-".join(str(x) for x in case), used)
    assert used["lanes_out"] == 0
    env.close()
