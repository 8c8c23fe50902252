"""tests/onpolicy_replay.py vetted without a GPU: recordings synthesised from the oracle itself -- a float32 numpy forward of seeded
weights (both actor kinds), oracle.explore_noise, the oracle env with the tank's state words re-entered as float32 after every step
(binary16 rows: the integrated error re-entered as the stored binary16 word), the rows written by a few lines of numpy that follow the
loop of rollout_kernel (csrc/rollout.hip) -- for pH, the Integrator tank, Stacking1, Stacking4 and Stacking10: 81 lanes at lane offset
8192, episodes of 10 steps (14 on Stacking10), three launches of (12, 18, 7) steps with noise epochs 1, 2, 3, a_std_log = -0.7, a prior
gain whose last column is non-zero, then one launch-by-launch hand-over step.

With 10-step episodes the second launch starts mid-episode (step 12) and stops at step 30, the end of an episode, so the third starts a
fresh one and stops mid-episode; with 14-step episodes (Stacking10) no launch but the first touches a boundary.  Three episodes end
inside the launches (two of 14 steps on Stacking10).

The honest recording must pass: with float32 rows every used share below 0.1 of its bar and no lane set aside; with binary16 rows one
rounding alone can use a whole bar, and the measured shares are asserted below.  Every mutant -- the same synthesis with ONE fault --
must fail, and the test names the assertion it trips (the label the checker's message starts with)."""
import functools
import inspect

import numpy as np
import pytest

import onpolicy_replay as R
import oracle

N, OFFSET, SEED, NOISE_SEED = 81, 8192, 6, 0x5EED00000007
CHUNKS = (12, 18, 7)
A_STD_LOG = -0.7
MD = 64
ENVS = {"ph": ("ph", 0), "integrator": ("integrator", 0), "stacking1": ("stacking", 1), "stacking4": ("stacking", 4),
        "stacking10": ("stacking", 10)}
F32 = np.float32


def make_actor(kind, D, md=MD, seed=3):
    """Seeded float32 weights, nn.Linear's default scale; a non-trivial last layer (tests/rollout_replay.py: make_agent)."""
    rng = np.random.default_rng(seed)

    def lin(o, i):
        b = 1.0 / np.sqrt(i)
        return rng.uniform(-b, b, (o, i)).astype(F32), rng.uniform(-b, b, o).astype(F32)
    sd = {"a_std_log": np.full((1, 1), A_STD_LOG, dtype=F32)}
    if kind == "plain":
        shapes = (("net.0", md, D), ("net.2", md, md), ("net.4", md, md))
        last = "net.6"
    else:
        shapes = (("other_net.0", md, D - 1), ("other_net.2", md // 2, md), ("integrator_net.0", md, 1), ("integrator_net.2", md // 2, md),
                  ("net.0", md, md))
        last = "net.2"
    for name, o, i in shapes:
        sd[name + ".weight"], sd[name + ".bias"] = lin(o, i)
    sd[last + ".weight"] = rng.normal(0, 0.1, (1, md)).astype(F32)
    sd[last + ".bias"] = rng.normal(0, 0.05, 1).astype(F32)
    return sd


def make_spec(env_name, kind, half=False, chunks=CHUNKS):
    env, stack = ENVS[env_name]
    spec = {"env": env, "num_stack": stack, "T": 14 if stack == 10 else 10, "seed": SEED, "env_offset": OFFSET, "noise_seed": NOISE_SEED,
            "kind": kind, "half": half, "calls": [(epoch, n) for epoch, n in enumerate(chunks, start=1)]}
    D = R.obs_dim(spec)
    spec["actor"] = make_actor(kind, D)
    k = np.zeros(D)
    k[-3:] = [0.0, -0.4, 0.4]                       # the tank's prior controller on the newest (h1, h2, r)
    spec["priorK"] = {"ph": np.array([0.02, -0.02, -0.035]), "integrator": np.array([0.0, -0.4, 0.4, -0.01])}.get(env, k)
    return spec


def forward32(spec, x, mutant=None):
    """float32 numpy forward of the actor's mean: tanh layers, a linear head (oracle/pime_oracle.c: oracle_*_actor_mean)."""
    p = {k: v.copy() for k, v in spec["actor"].items()}

    def dense(name, h, act=True):
        y = h @ p[name + ".weight"].T + p[name + ".bias"]
        return np.tanh(y) if act else y
    if spec["kind"] == "plain":
        if mutant == "first_layer_drops_columns_16_up":
            p["net.0.weight"][:, 16:] = 0
        if mutant == "bias_units_swapped":   # two hidden units of layer 2's bias land in layer 3's bias slots (a packing fault)
            p["net.4.bias"][[0, 1]] = p["net.2.bias"][[0, 1]]
        h = dense("net.4", dense("net.2", dense("net.0", x)))
        mean = dense("net.6", h, act=False)[:, 0]
    else:
        if mutant == "bias_units_swapped":
            p["net.0.bias"][[0, 1]] = p["other_net.0.bias"][[0, 1]]
        Do = x.shape[1] - 1
        xi = x[:, Do - 1:Do] if mutant == "integrator_tower_wrong_column" else x[:, Do:]
        cat = np.concatenate([dense("other_net.2", dense("other_net.0", x[:, :Do])), dense("integrator_net.2", dense("integrator_net.0", xi))], axis=1)
        mean = dense("net.2", dense("net.0", cat), act=False)[:, 0]
    assert mean.dtype == F32
    return mean


HANDOVER_ACTION = np.linspace(-0.9, 0.9, N).astype(F32)


def synthesize(spec, mutant=None, honest=None):
    """The recording a rollout kernel with the fault `mutant` (None: a correct one) would leave."""
    env_spec = dict(spec, T=spec["T"] + {"episode_one_step_long": 1, "episode_one_step_short": -1}.get(mutant, 0))
    env = R.make_oracle(env_spec, N, resample_every=1000 if mutant == "ensemble_not_resampled" else 1)   # 1000: drawn at episode 0 only
    D, stacking, is_ph, half = R.obs_dim(spec), spec["env"] == "stacking", spec["env"] == "ph", spec["half"]
    row_t = np.float16 if half else F32
    priorK = np.array(spec["priorK"], dtype=np.float64)
    if mutant == "prior_sign":
        priorK = -priorK
    if mutant == "prior_last_column_dropped":
        priorK[-1] = 0
    sigma = R.sigma_of(spec)

    def frames(seen, nxt, d):
        """The observation registers are the frame deque (oldest first); a reset fills every frame."""
        new, rst = nxt[:, D - 3:], d[:, None]
        filled = np.tile(new, (1, D // 3))
        if mutant == "frames_newest_first":
            return np.where(rst, filled, np.concatenate([new, seen[:, :D - 3]], axis=1))
        if mutant == "frame_duplicated":
            return np.where(rst, filled, np.concatenate([seen[:, 6:], new, new], axis=1))
        shifted = np.concatenate([seen[:, 3:], new], axis=1)
        return shifted if mutant == "frames_not_refilled" else np.where(rst, filled, shifted)

    def reenter(nxt, row):
        """What the kernel's registers hold behind a step, put into the float64 env: float32 words, binary16 rows: I as stored."""
        if stacking and mutant == "frames_newest_first":
            nxt = np.concatenate([nxt[:, 3:], nxt[:, :3]], axis=1)
        R.resync(env, spec, nxt)
        if half and mutant != "half_I_not_rounded":
            env.set("I", row[:, -1].astype(np.float64))

    unrounded = env.reset()
    row = unrounded.astype(row_t)
    reenter(unrounded, row)
    rows, actions, noises, rewards, dones, k = [row], [], [], [], [], 0
    for epoch, n_steps in spec["calls"]:
        for t in range(n_steps):
            seen = row.astype(F32)
            eps = oracle.explore_noise(spec["noise_seed"], 0 if mutant == "noise_of_offset_0" else OFFSET, N,
                                       epoch - 1 if mutant == "noise_of_previous_epoch" else epoch, k if mutant == "noise_t_not_restarted" else t)
            mean = forward32(spec, unrounded if mutant == "half_policy_sees_unrounded_row" else seen, mutant)
            a_pre = mean + eps * (F32(1) if mutant == "sigma_ignored" else sigma)
            prior_from = seen
            if mutant == "prior_from_next_observation":   # (the honest trajectory's successor row: exact at the first step)
                prior_from = honest["state"][k + 1].astype(F32)
            nxt, o64, rew, d = env.step(oracle.residual_action(a_pre, prior_from, priorK), auto_reset=True)
            if stacking:
                nxt = frames(seen, nxt, d)
            if mutant == "reset_row_holds_the_last_observation":
                nxt = np.where(d[:, None], o64.astype(F32), nxt)   # (o64: the oracle's observation before its auto-reset)
            if mutant == "integrated_error_not_cleared":   # (pH, Integrator: the last column is I)
                nxt[:, -1] = np.where(d, o64[:, -1].astype(F32), nxt[:, -1])
            unrounded = nxt
            row = nxt.astype(row_t)
            reenter(nxt, row)
            rows.append(row)
            actions.append(np.tanh(a_pre) if mutant == "stored_action_post_tanh" else a_pre)
            noises.append(eps * sigma if mutant == "noise_stored_scaled" else eps)
            rewards.append(rew.astype(row_t))
            dones.append(d.astype(np.uint8))
            k += 1
    fields = {f: env.get(f) for f in R.field_names(spec)}
    if mutant == "t_not_written_back":   # the handle keeps the step counter it had before the last launch
        stale = float((k - spec["calls"][-1][1]) % spec["T"])
        fields["t"] = np.full(N, stale)
        env.set("t", stale)
    seen = row.astype(F32)
    nxt, _, rew, d = env.step(oracle.residual_action(HANDOVER_ACTION, seen, spec["priorK"]), auto_reset=True)
    if stacking:   # the step-per-launch kernel reads the frame ring the launch wrote back, oldest at its head
        ring = np.concatenate([seen[:, 3:], seen[:, :3]], axis=1) if mutant == "frame_ring_rotated" else seen
        nxt = np.where(d[:, None], np.tile(nxt[:, D - 3:], (1, D // 3)), np.concatenate([ring[:, 3:], nxt[:, D - 3:]], axis=1))
    handoff = {"action": HANDOVER_ACTION, "obs": nxt.astype(row_t), "reward": rew.astype(row_t), "done": d.astype(np.uint8)}
    return {"state": np.stack(rows), "action": np.stack(actions).astype(F32), "noise": np.stack(noises).astype(F32),
            "reward": np.stack(rewards), "done": np.stack(dones), "fields": fields, "handoff": handoff}


@functools.lru_cache(maxsize=None)
def honest(env_name, kind, half=False, chunks=CHUNKS):
    spec = make_spec(env_name, kind, half, chunks)
    return spec, synthesize(spec)


CASES = [(e, "plain", False) for e in ENVS] + [(e, "modular", False) for e in ("ph", "integrator")]
HALF_CASES = [(e, k, True) for e in ("ph", "integrator") for k in ("modular", "plain")]


def _boundaries(spec):
    """(step at which every launch starts, step at which it ends) with step 0 the fresh reset."""
    ends = np.cumsum([c[1] for c in spec["calls"]])
    return ends - [c[1] for c in spec["calls"]], ends


@pytest.mark.parametrize("env_name,kind,half", CASES + HALF_CASES)
def test_the_inputs_can_show_the_faults(env_name, kind, half):
    spec, rec = honest(env_name, kind, half)
    n, T, D = sum(CHUNKS), spec["T"], R.obs_dim(spec)
    assert rec["state"].shape == (n + 1, N, D)
    starts, ends = _boundaries(spec)
    # the first launch stops and the second starts mid-episode; the last one stops mid-episode
    assert ends[0] % T != 0 and starts[1] % T != 0 and ends[-1] % T != 0
    if T == 14:   # ... and with 14-step episodes no launch but the first touches an episode boundary (with 10: step 30 is one)
        assert all(s % T != 0 for s in starts[1:]) and all(e % T != 0 for e in ends)
    inside = int(rec["done"].any(axis=1).sum())
    assert inside == n // T and inside >= (2 if T == 14 else 3) and (rec["done"].sum(axis=1) % N == 0).all()
    frames = rec["state"].astype(np.float64).reshape(n + 1, N, -1, 3) if spec["env"] == "stacking" else None
    if spec["num_stack"] == 10:   # a fully distinct ten-frame window occurs
        assert any(len(np.unique(row[0, :, 0])) == 10 for row in frames)
    if spec["num_stack"] >= 4:    # the state handed over mid-episode: the newest frames differ (but on a lane whose tanks ran empty)
        last = frames[n]
        assert (last[:, -1, :2] != last[:, -2, :2]).any(axis=1).mean() > 0.9 and (last[:, -2, :2] != last[:, -3, :2]).any(axis=1).mean() > 0.9
    assert R.sigma_of(spec) not in (1.0, F32(np.exp(-0.5)))
    assert float((rec["noise"] * R.sigma_of(spec)).std()) > 0.03, "the exploration noise must show in the stored actions"
    assert spec["priorK"][-1] != 0
    prior = np.abs(rec["state"][:n].astype(np.float64) @ spec["priorK"])
    assert (prior > 10 * R.ENV_TOL[spec["env"]]).mean() >= 0.5, "the prior term must move the env action"


@pytest.mark.parametrize("env_name,kind,half", CASES)
def test_the_honest_float32_recording_passes_far_inside_every_bar(env_name, kind, half):
    spec, rec = honest(env_name, kind, half)
    used = R.check_rollout(rec, spec)
    assert used["lanes_out"] == 0
    for what in ("noise", "mean", "observation", "reward"):
        assert used[what] < 0.1, (what, used)


# the largest used share of each bar of the honest binary16 recordings, MEASURED on this synthesis (one rounding to binary16 can use a
# whole H: these are no claim about the kernels, they pin that the synthesis and the checker round where the kernel does)
HALF_SHARES = {("ph", "modular"): (0.994, 0.461), ("ph", "plain"): (0.981, 0.454),          # (observation, reward)
               ("integrator", "modular"): (0.821, 0.351), ("integrator", "plain"): (0.848, 0.344)}


@pytest.mark.parametrize("env_name,kind,half", HALF_CASES)
def test_the_honest_binary16_recording_passes(env_name, kind, half):
    spec, rec = honest(env_name, kind, half)
    assert rec["state"].dtype == rec["reward"].dtype == np.float16
    used = R.check_rollout(rec, spec)
    assert used["lanes_out"] == 0 and used["noise"] == 0 and used["mean"] < 0.1, used
    obs_share, rew_share = HALF_SHARES[env_name, kind]
    assert used["observation"] <= obs_share and used["reward"] <= rew_share, used
    assert used["observation"] > 0.5 * obs_share, used   # (the measured figure, not a slack one)


# mutant -> (envs, row formats, the assertion it trips: the label the checker's message starts with; {env: label} where it depends)
ANY = tuple(ENVS)
WITH_I = ("ph", "integrator")
STACKED = ("stacking4", "stacking10")
BOTH, FLOAT, HALF = (False, True), (False,), (True,)
# (the tank's reward is a function of the step's h2 and is compared before the observation; a pH lane with float32 rows that leaves the
#  oracle's titration cell is set aside without a word and counted when its episode ends; with binary16 rows the reward is judged first)
ENV_SIDE = {("ph", False): "titration cell", None: "reward"}
MUTANTS = {
    "noise_of_offset_0": (ANY, BOTH, "exploration noise"),                 # keyed by the local lane
    "noise_of_previous_epoch": (ANY, BOTH, "exploration noise"),
    "noise_t_not_restarted": (ANY, BOTH, "exploration noise"),             # the counter's t runs on across launches
    "noise_stored_scaled": (ANY, BOTH, "exploration noise"),               # the noise row holds eps * sigma
    "sigma_ignored": (ANY, BOTH, "policy mean"),
    "stored_action_post_tanh": (ANY, BOTH, "policy mean"),
    "bias_units_swapped": (ANY, BOTH, "policy mean"),
    "first_layer_drops_columns_16_up": (("stacking10",), FLOAT, "policy mean"),
    "integrator_tower_wrong_column": (WITH_I, BOTH, "policy mean"),       # (modular actor only)
    "prior_sign": (ANY, BOTH, ENV_SIDE),
    "prior_from_next_observation": (ANY, BOTH, ENV_SIDE),
    "prior_last_column_dropped": (ANY, BOTH, {**ENV_SIDE, ("integrator", True, "modular"): "observation"}),
    "episode_one_step_long": (ANY, BOTH, "episode end"),
    "episode_one_step_short": (ANY, BOTH, "episode end"),
    "reset_row_holds_the_last_observation": (ANY, BOTH, "reset observation"),
    "ensemble_not_resampled": (ANY, BOTH, {("ph", False): "reset observation", ("ph", True): "reset observation", None: "reward"}),
    "integrated_error_not_cleared": (WITH_I, BOTH, "reset observation"),
    "frames_newest_first": (STACKED, FLOAT, "observation"),
    "frames_not_refilled": (STACKED, FLOAT, "reset observation"),
    "frame_duplicated": (STACKED, FLOAT, "observation"),
    "t_not_written_back": (ANY, BOTH, "env field"),
    "frame_ring_rotated": (STACKED, FLOAT, "hand-over"),
    "half_I_not_rounded": (WITH_I, HALF, "observation"),                   # I carried in float32 between steps, rounded in the rows only
    "half_policy_sees_unrounded_row": (WITH_I, HALF, "policy mean"),
}
ALL_CASES = CASES + HALF_CASES
MUTANT_CASES = [(m, e, k, h) for m, (envs, halves, _) in MUTANTS.items() for e, k, h in ALL_CASES
                if e in envs and h in halves and (k == "modular" or m != "integrator_tower_wrong_column")]


def test_every_label_is_tripped_by_some_mutant():
    tripped = set()
    for _, _, label in MUTANTS.values():
        tripped |= set(label.values()) if isinstance(label, dict) else {label}
    assert tripped == set(R.LABELS)


@pytest.mark.parametrize("mutant,env_name,kind,half", MUTANT_CASES)
def test_every_mutant_fails(mutant, env_name, kind, half):
    spec, rec = honest(env_name, kind, half)
    label = MUTANTS[mutant][2]
    if isinstance(label, dict):
        label = label.get((env_name, half, kind)) or label.get((env_name, half)) or label[None]
    bad = synthesize(spec, mutant, honest=rec)
    with pytest.raises(AssertionError, match="^" + label):
        R.check_rollout(bad, spec)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("state", "action", "noise", "reward", "done")) and \
        all(np.array_equal(a["fields"][f], b["fields"][f]) for f in a["fields"]) and \
        all(np.array_equal(a["handoff"][f], b["handoff"][f]) for f in a["handoff"])


def test_the_dropped_columns_do_not_exist_on_stacking4():
    """A first layer that drops the observation's columns 16.. is invisible on a 12-float observation: the fault lives on Stacking10."""
    spec, rec = honest("stacking4", "plain")
    assert _same(synthesize(spec, "first_layer_drops_columns_16_up"), rec)


@pytest.mark.parametrize("env_name", STACKED)
def test_a_rotated_frame_ring_hides_behind_an_episode_boundary(env_name):
    """The frame ring written back rotated by one slot shows in the hand-over step only while the frames differ: when the last launch
    stops at the end of an episode every frame is the reset frame, and the fault is invisible -- which is why every whole-episode test
    (tests/test_gpu_rollout_oracle.py) is blind to the slot order of the write-back."""
    T = 14 if env_name == "stacking10" else 10
    chunks = CHUNKS[:2] + (2 * T - sum(CHUNKS[:2]) % T,) if sum(CHUNKS[:2]) % T else CHUNKS[:2] + (T,)
    spec, rec = honest(env_name, "plain", False, chunks)
    assert sum(chunks) % T == 0 and rec["done"][-1].all()
    R.check_rollout(rec, spec)
    assert _same(synthesize(spec, "frame_ring_rotated"), rec)
    spec, rec = honest(env_name, "plain")   # mid-episode it shows (and test_every_mutant_fails names the label)
    assert not np.array_equal(synthesize(spec, "frame_ring_rotated")["handoff"]["obs"], rec["handoff"]["obs"])


def test_the_hand_over_reward_does_not_depend_on_the_last_action():
    """`last_a` is the pH env's previous action, read by the action-change punishment only (csrc/env_device.hpp: has_punish); the
    registered envs have none and the tank has no such word.  So a `last_a` that is not written back cannot show in the hand-over step:
    two pH envs that reach the same state behind different last actions take the same next step."""
    spec, _ = honest("ph", "plain")
    a, b = R.make_oracle(spec, N), R.make_oracle(spec, N)
    assert np.array_equal(a.reset(), b.reset())
    a.step(np.full(N, 0.3)); b.step(np.full(N, -0.2))
    for f in ("x", "I", "y"):
        b.set(f, a.get(f))
    oa, _, ra, _ = a.step(np.full(N, 0.1))
    ob, _, rb, _ = b.step(np.full(N, 0.1))
    assert np.array_equal(oa, ob) and np.array_equal(ra, rb)


def test_the_bars_are_the_established_ones():
    """No bar of the checker is its own: the float32-row bars are the literals of rollout_replay.replay_through_oracle, the env bars and
    the cell rule are offpolicy_replay's objects, the binary16 bars the literals of test_gpu_config5._replay_half."""
    import offpolicy_replay
    import rollout_replay
    import test_gpu_config5
    src = inspect.getsource(rollout_replay.replay_through_oracle)
    assert "rtol=1.2e-7, atol=0" in src and "neq.mean() <= 1e-4" in src and "rtol=3e-5, atol=3e-5" in src
    assert "rtol = 2e-5 if is_ph else 2e-4" in src and "<= 1e-5" in src and "1.0 - 1e-4" in src
    assert (R.NOISE_RTOL, R.NOISE_SHARE, R.MEAN_TOL) == (1.2e-7, 1e-4, 3e-5)
    assert R.ENV_TOL is offpolicy_replay.ENV_TOL and (R.CELL, R.CELL_SHARE) == (offpolicy_replay.CELL, offpolicy_replay.CELL_SHARE) == (1e-5, 1e-4)
    assert R.ENV_TOL == {"ph": 2e-5, "integrator": 2e-4, "stacking": 2e-4}
    half = inspect.getsource(test_gpu_config5._replay_half)
    assert R.H == test_gpu_config5.H
    for literal in ("rtol=2 * H, atol=3e-3", "H * np.abs(obs[:, 0]) + 1e-6", "got[:, 1], obs[:, 1], rtol=H, atol=0", "got[:, 2], obs[:, 2], rtol=H, atol=1e-5",
                    "got[:, :3], obs[:, :3], rtol=H, atol=2e-3", "got[:, 3], obs[:, 3], rtol=H, atol=2e-3 + 1e-5"):
        assert literal in half, literal
    assert (R.HALF_REWARD, R.HALF_PH_Y, R.HALF_PH_R, R.HALF_PH_I) == ((2 * R.H, 3e-3), (R.H, 1e-6), (R.H, 0.0), (R.H, 1e-5))
    assert (R.HALF_WT_LEVEL, R.HALF_WT_I) == ((R.H, 2e-3), (R.H, 2e-3 + 1e-5))
