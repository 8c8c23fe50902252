"""tests/offpolicy_replay.py vetted without a GPU: recordings synthesised from the oracle itself -- a float32 numpy forward of seeded
weights, oracle.explore_noise, the oracle env rounded to float32 (the tank's state words re-entered as float32 after every step, as the
kernels keep them), the ring written by a few lines of numpy that follow the kernels' loop (csrc/rollout_offpolicy.hip) -- for pH, the
Integrator tank, Stacking4 and Stacking10, with the TD3 Actor and with ActorSAC: three calls of (12, 18, 7) lock-steps, a 20-slot
ring, 81 lanes at a non-zero lane offset, 10-step episodes (14 on Stacking10).

The honest recording must pass with every used share below 0.1 of its bar; every mutant -- the same synthesis with ONE fault -- must
fail, and the test names the assertion it trips (the label the checker's message starts with)."""
import functools

import numpy as np
import pytest

import offpolicy_replay as R
import oracle
import sac_oracle as S

N, OFFSET, SEED, NOISE_SEED, SLOTS = 81, 8192, 6, 1234567, 20
CHUNKS = (12, 18, 7)
ENVS = {"ph": ("ph", 0), "integrator": ("integrator", 0), "stacking4": ("stacking", 4), "stacking10": ("stacking", 10)}
MD = 64


def make_actor(kind, D, md=MD, seed=3):
    """Seeded float32 weights, nn.Linear's default scale; a non-trivial last layer."""
    rng = np.random.default_rng(seed)

    def lin(o, i):
        b = 1.0 / np.sqrt(i)
        return rng.uniform(-b, b, (o, i)).astype(np.float32), rng.uniform(-b, b, o).astype(np.float32)
    sd = {}
    pre = "net" if kind == "td3" else "net_state"
    for idx, (o, i) in zip((0, 2, 4), ((md, D), (md, md), (md, md))):
        sd[f"{pre}.{idx}.weight"], sd[f"{pre}.{idx}.bias"] = lin(o, i)
    if kind == "td3":
        sd["net.6.weight"] = rng.normal(0, 0.05, (1, md)).astype(np.float32)
        sd["net.6.bias"] = rng.normal(0, 0.05, 1).astype(np.float32)
    else:
        sd["net_a_avg.weight"] = rng.normal(0, 0.08, (1, md)).astype(np.float32)
        sd["net_a_avg.bias"] = rng.normal(0, 0.05, 1).astype(np.float32)
        sd["net_a_std.weight"] = rng.normal(0, 0.08, (1, md)).astype(np.float32)
        sd["net_a_std.bias"] = np.full(1, -1.0, dtype=np.float32)
    return sd


def make_spec(env_name, kind, sigma=0.1):
    env, stack = ENVS[env_name]
    spec = {"env": env, "num_stack": stack, "T": 14 if stack == 10 else 10, "seed": SEED, "env_offset": OFFSET, "noise_seed": NOISE_SEED,
            "slots": SLOTS, "kind": kind, "sigma": sigma, "gamma": 0.98, "reward_scale": 0.5}
    D = R.obs_dim(spec)
    calls, slot0 = [], 0
    for epoch, n in enumerate(CHUNKS, start=1):
        calls.append((epoch, n, slot0))
        slot0 = (slot0 + n) % SLOTS
    spec["calls"] = calls
    spec["actor"] = make_actor(kind, D)
    k = np.zeros(D)
    k[-3:] = [0.0, -0.4, 0.4]                       # the tank's prior controller on the newest (h1, h2, r)
    spec["priorK"] = {"ph": np.array([-0.05, 0.05, 0.002]), "integrator": np.array([0.0, -0.4, 0.4, -0.01])}.get(env, k)
    return spec


def stored_action(spec, obs, eps, mutant):
    """float32 numpy forward + the exploration draw: what the kernels store as the action."""
    p = {k: v.copy() for k, v in spec["actor"].items()}
    pre = "net" if spec["kind"] == "td3" else "net_state"
    if mutant == "first_layer_drops_columns_16_up":
        p[f"{pre}.0.weight"][:, 16:] = 0
    if mutant == "bias_units_swapped":   # two hidden units of layer 2's bias land in layer 3's bias slots (a packing fault)
        p[f"{pre}.4.bias"][[0, 1]] = p[f"{pre}.2.bias"][[0, 1]]
    if spec["kind"] == "sac":
        f = S.actor_forward(p, obs, eps)
        return (f["u"] if mutant == "tanh_dropped" else f["a"])[:, 0].astype(np.float32)
    h = obs
    for i in (0, 2, 4):
        h = np.maximum(h @ p[f"net.{i}.weight"].T + p[f"net.{i}.bias"], np.float32(0))
    mean = (h @ p["net.6.weight"].T + p["net.6.bias"])[:, 0]
    assert mean.dtype == np.float32
    noise = np.float32(spec["sigma"]) * eps
    if mutant == "sac_draw_in_td3_mode":
        return np.tanh(mean + noise)
    a = (mean if mutant == "tanh_dropped" else np.tanh(mean)) + noise
    return a if mutant == "unclipped" else np.clip(a, np.float32(-1), np.float32(1))


def synthesize(spec, mutant=None, honest=None):
    """The recording an exploration kernel with the fault `mutant` (None: a correct one) would leave."""
    env_spec = dict(spec, T=spec["T"] + {"episode_one_step_long": 1, "episode_one_step_short": -1}.get(mutant, 0))
    env = R.make_oracle(env_spec, N, resample_every=1000 if mutant == "ensemble_not_resampled" else 1)   # 1000: drawn at episode 0 only
    D, stacking = R.obs_dim(spec), spec["env"] == "stacking"
    priorK = -spec["priorK"] if mutant == "prior_sign" else spec["priorK"]
    gamma, scale = np.float32(spec["gamma"]), np.float32(1.0 if mutant == "reward_unscaled" else spec["reward_scale"])
    ring_s, ring_o = np.zeros((SLOTS, N, D), dtype=np.float32), np.zeros((SLOTS, N, 3), dtype=np.float32)
    obs = env.reset()
    rows_s, rows_o, slots_read, k = [], [], [], 0
    for epoch, n_steps, slot0 in spec["calls"]:
        slot = slot0
        for t in range(n_steps):
            eps = oracle.explore_noise(spec["noise_seed"], 0 if mutant == "noise_of_offset_0" else OFFSET, N,
                                       epoch - 1 if mutant == "noise_of_previous_epoch" else epoch, k if mutant == "noise_t_not_restarted" else t)
            act = stored_action(spec, obs, eps, mutant)
            prior_from = obs
            if mutant == "prior_from_next_observation":   # (the honest trajectory's successor row: exact at the first lock-step)
                prior_from = honest["state"][k + 1] if k + 1 < len(honest["state"]) else honest["held"]
            nxt, _, rew, d = env.step(R.env_action(act, prior_from, priorK), auto_reset=True)
            if stacking:   # the observation registers are the frame deque (oldest first); a reset fills every frame
                new, rst = nxt[:, D - 3:], d[:, None]
                if mutant == "frames_newest_first":
                    nxt = np.where(rst, np.tile(new, (1, D // 3)), np.concatenate([new, obs[:, :D - 3]], axis=1))
                elif mutant == "frame_duplicated":
                    nxt = np.where(rst, np.tile(new, (1, D // 3)), np.concatenate([obs[:, 6:], new, new], axis=1))
                else:
                    shifted = np.concatenate([obs[:, 3:], new], axis=1)
                    nxt = shifted if mutant == "frames_not_refilled" else np.where(rst, np.tile(new, (1, D // 3)), shifted)
            R.resync(env, spec, nxt if not stacking or mutant != "frames_newest_first" else np.concatenate([nxt[:, 3:], nxt[:, :3]], axis=1))
            ring_s[slot] = obs
            ring_o[slot, :, 0] = rew.astype(np.float32) * scale
            ring_o[slot, :, 1] = gamma if mutant == "mask_gamma_at_end" else np.where(d, np.float32(0), gamma)
            ring_o[slot, :, 2] = act
            slot += 1
            if slot == SLOTS:
                slot = 1 if mutant == "ring_shifted_at_wrap" else 0
            held_stale, obs = obs, nxt
            k += 1
        for j in range(n_steps):   # the host reads the call's rows back where the ring's contract puts them
            s = (slot0 + j) % SLOTS
            rows_s.append(ring_s[s].copy()); rows_o.append(ring_o[s].copy()); slots_read.append(s)
    names = ("x", "I", "qww_V", "t", "episode") if spec["env"] == "ph" else ("h1", "h2", "a1", "Kp", "t", "episode")
    return {"state": np.stack(rows_s), "other": np.stack(rows_o), "slot": np.array(slots_read),
            "held": held_stale if mutant == "held_observation_stale" else obs, "fields": {f: env.get(f) for f in names}}


@functools.lru_cache(maxsize=None)
def honest(env_name, kind, sigma=0.1):
    spec = make_spec(env_name, kind, sigma)
    return spec, synthesize(spec)


CASES = [(e, k) for e in ENVS for k in ("td3", "sac")]


@pytest.mark.parametrize("env_name,kind", CASES)
def test_the_honest_recording_passes_far_inside_every_bar(env_name, kind):
    spec, rec = honest(env_name, kind)
    n = sum(CHUNKS)
    assert rec["state"].shape == (n, N, R.obs_dim(spec)) and (rec["other"][:, :, 1] == 0).sum() == N * (n // spec["T"])
    assert n > SLOTS and n % spec["T"] != 0, "the ring must wrap and the last call must stop mid-episode"
    if spec["num_stack"] == 10:   # a fully distinct 10-frame window occurs
        assert any(len(np.unique(row[0].reshape(10, 3)[:, 0])) == 10 for row in rec["state"])
    assert float(rec["other"][:, :, 2].std()) > 0.03, "the exploration noise must show in the stored actions"
    used = R.check_exploration(rec, spec)
    assert used["lanes_out"] == 0
    for what in ("action", "observation", "reward"):
        assert used[what] < 0.1, (what, used)


# mutant -> the assertion it trips (the label the checker's message starts with); {env: label} where it depends on the env
ANY = ("ph", "integrator", "stacking4", "stacking10")
STACKED = ("stacking4", "stacking10")
MUTANTS = {
    "noise_of_offset_0": (ANY, ("td3", "sac"), "stored action"),
    "noise_of_previous_epoch": (ANY, ("td3", "sac"), "stored action"),
    "noise_t_not_restarted": (ANY, ("td3", "sac"), "stored action"),
    "sac_draw_in_td3_mode": (ANY, ("td3",), "stored action"),
    "first_layer_drops_columns_16_up": (("stacking10",), ("td3", "sac"), "stored action"),
    "bias_units_swapped": (ANY, ("td3", "sac"), "stored action"),
    "tanh_dropped": (ANY, ("td3", "sac"), "stored action"),
    "frames_newest_first": (STACKED, ("td3",), "observation"),
    "frames_not_refilled": (STACKED, ("td3",), "reset observation"),
    "frame_duplicated": (STACKED, ("td3",), "observation"),
    "mask_gamma_at_end": (ANY, ("td3", "sac"), "episode end"),
    "episode_one_step_long": (ANY, ("td3",), "episode end"),
    "episode_one_step_short": (ANY, ("td3",), "episode end"),
    "reward_unscaled": (ANY, ("td3", "sac"), "reward"),
    # (the tank's reward is a function of the step's h2 and is compared before the observation; a pH lane that leaves the oracle's
    #  titration cell is set aside without a word and counted when its episode ends)
    "prior_sign": (ANY, ("td3", "sac"), {"ph": "titration cell", None: "reward"}),
    "prior_from_next_observation": (ANY, ("td3", "sac"), {"ph": "titration cell", None: "reward"}),
    "ring_shifted_at_wrap": (ANY, ("td3", "sac"), "ring successor"),
    "held_observation_stale": (ANY, ("td3", "sac"), {"ph": "titration cell", None: "held observation"}),
    "ensemble_not_resampled": (ANY, ("td3",), {"ph": "reset observation", None: "reward"}),   # pH: y of the reset depends on the draw
}
MUTANT_CASES = [(m, e, k) for m, (envs, kinds, _) in MUTANTS.items() for e in envs for k in kinds]


@pytest.mark.parametrize("mutant,env_name,kind", MUTANT_CASES)
def test_every_mutant_fails(mutant, env_name, kind):
    spec, rec = honest(env_name, kind)
    label = MUTANTS[mutant][2]
    if isinstance(label, dict):
        label = label.get(env_name, label[None])
    bad = synthesize(spec, mutant, honest=rec)
    with pytest.raises(AssertionError, match="^" + label):
        R.check_exploration(bad, spec)


def test_the_dropped_columns_do_not_exist_on_stacking4():
    """A first layer that drops the observation's columns 16.. is invisible on a 12-float observation: the fault lives on Stacking10."""
    spec, rec = honest("stacking4", "td3")
    bad = synthesize(spec, "first_layer_drops_columns_16_up")
    assert np.array_equal(bad["other"], rec["other"]) and np.array_equal(bad["state"], rec["state"])


CLIP_SIGMA = 0.8


def test_a_clipping_sigma_clips_and_the_unclipped_action_fails():
    spec, rec = honest("integrator", "td3", CLIP_SIGMA)
    a = rec["other"][:, :, 2]
    assert (a == 1).mean() >= 0.01 and (a == -1).mean() >= 0.01, ((a == 1).mean(), (a == -1).mean())
    used = R.check_exploration(rec, spec)
    assert max(used["action"], used["observation"], used["reward"]) < 0.1
    with pytest.raises(AssertionError, match="stored action"):
        R.check_exploration(synthesize(spec, "unclipped"), spec)
    # (with the usual sigma = 0.1 the clip is never active on these weights: the mutant would pass)
    spec01, rec01 = honest("integrator", "td3")
    assert float(np.abs(rec01["other"][:, :, 2]).max()) < 1.0


# ---- the evaluation checker ---------------------------------------------------------------------------------------------------
def synthesize_eval(spec, mutant=None):
    """(trace, ret, reset_obs) of one traced evaluation launch of T steps, in the kernels' layout (include/pime_hip.h)."""
    env = R.make_oracle(spec, N)
    D, T = R.obs_dim(spec), spec["T"]
    priorK = -spec["priorK"] if mutant == "prior_sign" else spec["priorK"]
    obs = reset_obs = env.reset()
    trace, ret = np.zeros((T, 6, N)), np.zeros(N)
    for t in range(T):
        forward_fault = mutant if mutant in ("tanh_dropped", "bias_units_swapped", "first_layer_drops_columns_16_up") else None
        a = stored_action(dict(spec, sigma=0.0), obs, np.zeros(N, dtype=np.float32), forward_fault)   # no draw: tanh(mean), SAC tanh(avg)
        a_env = R.env_action(a, obs, priorK)
        nxt, _, rew, _ = env.step(a_env)
        rew = rew.astype(np.float32)
        if spec["env"] == "ph":
            trace[t, 0:3], trace[t, 3], trace[t, 4], trace[t, 5] = obs.T, a_env, rew, env.get("x")
        else:
            if spec["env"] == "stacking":
                nxt = np.concatenate([obs[:, 3:], nxt[:, D - 3:]], axis=1)
                trace[t, 0:3] = nxt[:, D - 3:].T
            else:
                trace[t, 0:4] = nxt.T
            trace[t, 4], trace[t, 5] = rew, a_env
            R.resync(env, spec, nxt)
        if not (mutant == "return_misses_a_step" and t == T - 1):
            ret += rew
        obs = nxt
    return trace, ret, reset_obs


@pytest.mark.parametrize("env_name,kind", CASES)
def test_the_honest_evaluation_trace_passes(env_name, kind):
    spec, _ = honest(env_name, kind)
    used = R.check_evaluation(*synthesize_eval(spec), spec)
    assert used["lanes_out"] == 0 and max(used["action"], used["observation"], used["reward"]) < 0.1, used


@pytest.mark.parametrize("mutant,env_name,label", [("tanh_dropped", "ph", "env action"), ("tanh_dropped", "stacking10", "env action"),
                                                   ("prior_sign", "integrator", "env action"), ("bias_units_swapped", "stacking4", "env action"),
                                                   ("first_layer_drops_columns_16_up", "stacking10", "env action"),
                                                   ("return_misses_a_step", "ph", "returned sum")])
@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_every_evaluation_mutant_fails(mutant, env_name, label, kind):
    spec, _ = honest(env_name, kind)
    with pytest.raises(AssertionError, match="^" + label):
        R.check_evaluation(*synthesize_eval(spec, mutant), spec)
