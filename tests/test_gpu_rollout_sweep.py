"""Every instantiation of the fused on-policy rollout (`pime_rollout` / `pime_rollout_h`: rollout_kernel of csrc/rollout.hip,
rollout16_kernel of csrc/mlp16.hip at width 256), replayed lane by lane through the float64 oracle by tests/onpolicy_replay.py (vetted
on the CPU by tests/test_onpolicy_replay_cpu.py: what it checks, with which bar, and which faults it sees).
tests/test_gpu_rollout_oracle.py replays whole episodes of the bench's shapes; here the launches are driven through the C ABI the way
VecControlEnv.rollout calls it, but start and stop inside episodes, so that what a launch reloads from and writes back to the handle
(step counter, integrated error -- binary16 in "mixed16" --, last action, on Stacking the frame ring and its head) is under test, and
one launch-by-launch env.step_residual step after the last launch reads it.

Shapes: 81 lanes (32- and 16-lane tilings: one full 64-lane workgroup + a ragged one whose idle waves shadow lane 80; QUAD: five full
tiles + a single-lane tile; rollout16_kernel: one full and one ragged workgroup) at lane offset 8192, episodes of 10 steps (14 on
Stacking10: a fully distinct 10-frame window occurs), three launches of (12, 18, 7) steps with noise epochs 1, 2, 3, a_std_log = -0.7.
The tiling is forced with PIME_ROLLOUT_NARROW = 0 (32-lane tiles) / 1 (16-lane tiles, one per wave) / 2 (QUAD), read per launch.
Output rows are allocated NaN-filled (done: 0xFF): a lane or step the kernel did not write cannot pass.

Test id -> instantiation (T = width / 32; KIND modular = MLP_MODULAR_ACTOR, plain = MLP_PLAIN_ACTOR; ENV 0 pH, 1 Integrator tank,
2 Stacking tank; S = frames; NARROW 0 / 1 / 2 = wide / narrow / quad), test_rollout_replays_through_the_oracle[...]:
    {modular,plain}-{64,128}-PH_V35-{wide,narrow,quad}          rollout_kernel<{2,4}, KIND, 0, 0, {0,1,2}>
    {modular,plain}-{64,128}-WT_INTEGRATOR-{wide,narrow,quad}   rollout_kernel<{2,4}, KIND, 1, 0, {0,1,2}>
    plain-{64,128}-WT_STACKING{1,4,10}-{wide,narrow,quad}       rollout_kernel<{2,4}, plain, 2, {1,4,10}, {0,1,2}>
        except plain-128-WT_STACKING10-quad: rollout_kernel<4, plain, 2, 10, 2> is never launched (the 30-float image plus the exchange
        buffers exceed the 160 KB of LDS, csrc/rollout.hip: tiling) -- plain-128-WT_STACKING10-only runs <4, plain, 2, 10, 1> under the
        QUAD request and asserts the arithmetic.  It is the only such id: 41 of the 42 rollout_kernel instantiations can be launched.
    {modular,plain}-256-PH_V35-{narrow,quad}                    rollout16_kernel<16, KIND, 0, 0, {false,true}, kEvalNone>
    {modular,plain}-256-WT_INTEGRATOR-{narrow,quad}             rollout16_kernel<16, KIND, 1, 0, {false,true}, kEvalNone>
    plain-256-WT_STACKING{1,4,10}-{narrow,quad}                 rollout16_kernel<16, plain, 2, {1,4,10}, {false,true}, kEvalNone>
        (all 14; width 256 has no 32-lane tiling, and its QUAD exchange buffer always fits)
    half-{modular,plain}-{64,128}-{PH_V35,WT_INTEGRATOR}-{wide,narrow,quad}   the run-time h16 branch of rollout_kernel<{2,4}, KIND,
        {0,1}, 0, {0,1,2}> on a "mixed16" handle: binary16 rows (24 runs)
    ppo-* and half-ppo-* (plain PPO: priorK = 0, the env sees tanh(a_pre)) re-run one of the instantiations above.
modular = ResidualIntegratorModularPPO, plain = ResidualPPO, from tests/rollout_replay.py: make_agent.
Every test prints one "SHARE" line: the largest used share of each bar, for the record of a GPU run."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import onpolicy_replay as O
from rollout_replay import DEV, make_agent

pytestmark = pytest.mark.gpu
N, OFFSET, SEED = 81, 8192, 6
CHUNKS = (12, 18, 7)
A_STD_LOG = -0.7
NOISE_SEED = 0x5EED00000007          # both key words non-zero
TILES = {"wide": "0", "narrow": "1", "quad": "2", "only": "2"}
ENVS = {"PH_V35": ("ph", 0), "WT_INTEGRATOR": ("integrator", 0), "WT_STACKING1": ("stacking", 1), "WT_STACKING4": ("stacking", 4),
        "WT_STACKING10": ("stacking", 10)}
ALGO = {"modular": "ResidualIntegratorModularPPO", "plain": "ResidualPPO", "ppo": "PPO"}
LDS_LIMIT = 160 * 1024
NO_QUAD = {(128, "WT_STACKING10")}   # the QUAD request falls back to 16-lane tiles per wave


def _max_step(env_name):
    return 14 if env_name == "WT_STACKING10" else 10


def _make_env(env_name, half, n=N):
    from pime_amd import gym_control
    stack, T = ENVS[env_name][1], _max_step(env_name)
    env_id = gym_control.WT_STACKING.format(stack) if stack else getattr(gym_control, env_name)
    kw = dict(max_episode_steps=T) if env_name == "PH_V35" else dict(reward_type="distance", max_step=T)
    return gym_control.make_vec(env_id, n, device=DEV, state_mode="mixed16" if half else "mixed", seed=SEED, env_offset=OFFSET, **kw)


def _kind(actor):
    from pime_amd import native
    return native.MLP_MODULAR_ACTOR if actor == "modular" else native.MLP_PLAIN_ACTOR


def _quad_fits(actor, md, env_name):
    """The launcher's rule (csrc/rollout.hip: tiling): QUAD needs the image and two exchange buffers of (width / 16) tiles x 64 lanes x
    4 floats in the LDS."""
    from pime_amd import native
    env, stack = ENVS[env_name]
    image = native.lib().pime_mlp_packed_floats(_kind(actor), O.obs_dim({"env": env, "num_stack": stack}), 0 if stack else 1, md)
    assert image > 0
    return (image + 2 * (md // 16) * 64 * 4) * 4 <= LDS_LIMIT


def _family(md, half):
    return "rollout16_kernel" if md == 256 else ("rollout_kernel (binary16 rows)" if half else "rollout_kernel")


def _id(case):
    actor, md, env_name, tiles, half = case
    return f"{'half-' if half else ''}{actor}-{md}-{env_name}-{tiles}"


def _report(case, used):
    print(f"\nSHARE family={_family(case[1], case[4])} id={_id(case)} noise={used['noise']:.4f} mean={used['mean']:.4f} "
          f"observation={used['observation']:.4f} reward={used['reward']:.4f} lanes_out={used['lanes_out']}")


@functools.lru_cache(maxsize=None)
def _recording(actor, md, env_name, tiles, half):
    """(recording, spec) of the three launches and the hand-over step; the caller has set PIME_ROLLOUT_NARROW."""
    from pime_amd import native
    assert os.environ.get("PIME_ROLLOUT_NARROW") == TILES[tiles]
    lib = native.lib()
    env = _make_env(env_name, half)
    T, D = env.max_step, env.obs_dim
    assert T == _max_step(env_name)
    ag = make_agent(ALGO[actor], env, md)
    with torch.no_grad():
        ag.act.a_std_log.fill_(A_STD_LOG)
    ag.weights_changed()
    pk = ag._packed_for("act")
    kind = _kind(actor)
    assert pk is not None and pk.D == D and pk.md == md and (pk.kind == "modular_actor") == (actor == "modular")
    assert lib.pime_rollout_supported(env._h, kind, md) == 1
    priorK = np.ascontiguousarray(np.asarray(ag._rollout_priorK(), dtype=np.float64).reshape(-1))
    assert priorK.shape == (D,) and bool(priorK.any()) == (actor != "ppo")
    a_std = ag.act.a_std_log.detach()
    n = sum(CHUNKS)
    row_t = torch.float16 if half else torch.float32
    state = torch.full((n + 1, N, D), float("nan"), dtype=row_t, device=DEV)
    reward = torch.full((n, N), float("nan"), dtype=row_t, device=DEV)
    action = torch.full((n, N), float("nan"), dtype=torch.float32, device=DEV)
    noise = torch.full((n, N), float("nan"), dtype=torch.float32, device=DEV)
    done = torch.full((n, N), 0xFF, dtype=torch.uint8, device=DEV)
    state[0].copy_(env.reset_h() if half else env.reset())   # slot 0 of a launch: the lanes' current observation
    fn = lib.pime_rollout_h if half else lib.pime_rollout
    calls, t0 = [], 0
    for epoch, c in enumerate(CHUNKS, start=1):   # slot 0 of the next launch is the last row of this one
        native.check(fn(env._h, kind, md, native.ptr(pk.packed), native.ptr(a_std), native.ptr(priorK), c, C.c_uint64(NOISE_SEED),
                        C.c_uint32(epoch), native.ptr(state[t0:t0 + c + 1]), native.ptr(action[t0:t0 + c]), native.ptr(noise[t0:t0 + c]),
                        native.ptr(reward[t0:t0 + c]), native.ptr(done[t0:t0 + c]), env._stream()), "pime_rollout")
        env._t_all = (env._t_all + c) % env.max_step   # the host's step mirror, as VecControlEnv.rollout_offpolicy keeps it
        calls.append((epoch, c))
        t0 += c
    torch.cuda.synchronize()
    env_kind, stack = ENVS[env_name]
    spec = {"env": env_kind, "num_stack": stack, "T": T, "seed": SEED, "env_offset": OFFSET, "noise_seed": NOISE_SEED, "calls": calls,
            "kind": "modular" if actor == "modular" else "plain", "priorK": priorK, "half": half,
            "actor": {k: v.detach().cpu().numpy() for k, v in ag.act.state_dict().items()}}
    fields = {f: env.get_field(f) for f in O.field_names(spec)}
    # hand-over: ONE step of the step-per-launch kernels on what the fused kernel wrote back
    a_tab = torch.linspace(-0.9, 0.9, N, dtype=torch.float32, device=DEV)
    step = env.step_residual_h if half else env.step_residual
    obs, rew, d = step(a_tab, state[n].clone(), priorK, auto_reset=True)
    torch.cuda.synchronize()
    rec = {"state": state.cpu().numpy(), "reward": reward.cpu().numpy(), "action": action.cpu().numpy(), "noise": noise.cpu().numpy(),
           "done": done.cpu().numpy(), "fields": fields,
           "handoff": {"action": a_tab.cpu().numpy(), "obs": obs.cpu().numpy().copy(), "reward": rew.cpu().numpy().copy(),
                       "done": d.cpu().numpy().copy()}}
    env.close()
    return rec, spec


SERVED = [(a, md, e) for md in (64, 128, 256) for a, envs in (("modular", ("PH_V35", "WT_INTEGRATOR")), ("plain", tuple(ENVS))) for e in envs]
SERVED_HALF = [(a, md, e) for md in (64, 128) for a in ("modular", "plain") for e in ("PH_V35", "WT_INTEGRATOR")]
CASES = []
for _a, _md, _e in SERVED:
    for _t in (("narrow", "quad") if _md == 256 else ("wide", "narrow", "quad")):
        CASES.append((_a, _md, _e, "only" if _t == "quad" and (_md, _e) in NO_QUAD else _t, False))
CASES += [(a, md, e, t, True) for a, md, e in SERVED_HALF for t in ("wide", "narrow", "quad")]
CASES += [("ppo", 64, "PH_V35", "quad", False), ("ppo", 128, "WT_STACKING1", "narrow", False), ("ppo", 256, "WT_INTEGRATOR", "quad", False),
          ("ppo", 64, "WT_INTEGRATOR", "wide", True)]


def test_the_id_table_accounts_for_every_instantiation():
    f32 = [c for c in CASES if not c[4] and c[0] != "ppo"]
    assert len([c for c in f32 if c[1] < 256]) == 42 and len([c for c in f32 if c[1] == 256]) == 14
    assert len([c for c in CASES if c[4] and c[0] != "ppo"]) == 24
    assert [c for c in CASES if c[3] == "only"] == [("plain", 128, "WT_STACKING10", "only", False)]
    assert len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rollout_replays_through_the_oracle(case, monkeypatch):
    actor, md, env_name, tiles, half = case
    monkeypatch.setenv("PIME_ROLLOUT_NARROW", TILES[tiles])
    if md < 256:   # which tiling a QUAD request gets: QUAD wherever it fits, and it fits everywhere but Stacking10 at width 128
        fits = _quad_fits("plain" if actor == "ppo" else actor, md, env_name)
        assert fits == ((md, env_name) not in NO_QUAD)
        assert (tiles == "only") == (not fits and TILES[tiles] == "2")
    rec, spec = _recording(actor, md, env_name, tiles, half)
    assert float((rec["noise"] * O.sigma_of(spec)).std()) > 0.03, "the exploration noise must show in the stored actions"
    assert int(rec["done"].any(axis=1).sum()) == sum(CHUNKS) // spec["T"]
    if env_name == "WT_STACKING10":
        assert any(len(np.unique(row[0].reshape(10, 3)[:, 0])) == 10 for row in rec["state"]), "no fully distinct 10-frame window"
    used = O.check_rollout(rec, spec)
    _report(case, used)
    assert used["lanes_out"] == 0


@pytest.mark.parametrize("actor,md,env_name,half", [("modular", 128, "PH_V35", False), ("plain", 64, "WT_INTEGRATOR", False),
                                                    ("plain", 64, "WT_STACKING4", False), ("plain", 256, "PH_V35", False),
                                                    ("modular", 256, "WT_INTEGRATOR", False), ("plain", 256, "WT_STACKING10", False),
                                                    ("modular", 128, "PH_V35", True), ("plain", 64, "WT_INTEGRATOR", True)])
def test_quad_and_narrow_tilings_store_the_same_bits_across_launches(actor, md, env_name, half, monkeypatch):
    """tests/test_gpu_rollout_oracle.py::test_quad_and_narrow_tilings_give_the_same_bits on launches that start and stop inside
    episodes: rows, env fields and the hand-over step are bit-equal under QUAD and under 16-lane tiles (one per wave)."""
    recs = []
    for tiles in ("quad", "narrow"):
        monkeypatch.setenv("PIME_ROLLOUT_NARROW", TILES[tiles])
        recs.append(_recording(actor, md, env_name, tiles, half)[0])
    q, w = recs
    for key in ("state", "reward", "action", "noise", "done"):
        assert np.array_equal(q[key], w[key]), key
    for f in q["fields"]:
        assert np.array_equal(q["fields"][f], w["fields"][f]), f
    for f in q["handoff"]:
        assert np.array_equal(q["handoff"][f], w["handoff"][f]), f


def test_the_library_serves_exactly_the_listed_set():
    """pime_rollout_supported over kind x width {32, 64, 128, 256} x (pH, tank with 0 / 1 / 2 / 4 / 10 frames) x both state modes is
    the set this file lists: "mixed16" is refused on Stacking and at width 256."""
    from pime_amd import native
    from pime_amd.vec_env import VecWaterTank
    lib = native.lib()
    names = {0: "WT_INTEGRATOR", 1: "WT_STACKING1", 4: "WT_STACKING4", 10: "WT_STACKING10"}
    got = {False: set(), True: set()}
    for half in (False, True):
        mode = "mixed16" if half else "mixed"
        envs = [("PH_V35", _make_env("PH_V35", half, n=16))]
        for stack in (0, 1, 2, 4, 10):
            envs.append((names.get(stack, f"WT_STACKING{stack}"), VecWaterTank(16, device=DEV, state_mode=mode, seed=SEED, num_stack=stack,
                                                                                reward_type="distance", max_step=10)))
        for env_name, env in envs:
            for actor in ("modular", "plain"):
                for md in (32, 64, 128, 256):
                    if lib.pime_rollout_supported(env._h, _kind(actor), md):
                        got[half].add((actor, md, env_name))
            assert not lib.pime_rollout_supported(env._h, native.MLP_CRITIC, 128) and not lib.pime_rollout_supported(env._h, native.MLP_SAC_ACTOR, 128)
            env.close()
    assert got[False] == set(SERVED)
    assert got[True] == set(SERVED_HALF)
    assert not [s for s in got[True] if s[1] == 256 or "STACKING" in s[2]]
    assert {(c[0], c[1], c[2]) for c in CASES if c[0] != "ppo" and not c[4]} == set(SERVED)
    assert {(c[0], c[1], c[2]) for c in CASES if c[0] != "ppo" and c[4]} == set(SERVED_HALF)
