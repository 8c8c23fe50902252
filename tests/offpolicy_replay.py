"""Replay of what the fused off-policy exploration (`pime_rollout_offpolicy` / `pime_rollout_offpolicy_sac`) wrote into the device
ring, and of what the fused evaluation (`pime_rollout_eval`, TD3 kind) traced, through the float64 oracle.  Pure numpy + `oracle`:
no torch, no GPU -- tests/test_offpolicy_replay_cpu.py vets it on recordings synthesised from the oracle itself (one honest, the
others each with one fault), tests/test_gpu_offpolicy_oracle.py feeds it what the kernels stored.

A RECORDING is a dict:
  state  float32 [n, N, D]   the ring's state row of every lock-step, all calls in call order
  other  float32 [n, N, 3]   (reward * scale, mask, stored action) of the same rows
  slot   int [n]             the ring slot each row was read from
  held   float32 [N, D]      the observation the agent holds after the last call
  fields {name: float64 [N]} env fields read back after the last call: tank h1 h2 a1 Kp t episode, pH x I qww_V t episode

A SPEC is a dict:
  env "ph" | "integrator" | "stacking", num_stack, T (max steps), seed, env_offset, noise_seed, calls [(epoch, n_steps, slot0)],
  slots (ring size), actor (numpy state dict), kind "td3" | "sac", priorK float64 [D], sigma, gamma, reward_scale

Bars (none of them this module's own):
  stored action   TD3 5e-5 absolute (tests/test_gpu_td3.py), SAC 3e-5 absolute (tests/test_gpu_sac_rollout.py)
  observation and reward * scale   |got - want| <= tol * (1 + |want|), tol = 2e-5 on pH, 2e-4 on the tank (tests/rollout_replay.py)
  pH titration cell: a lane whose y leaves the oracle's by more than 1e-5 is out until its episode ends; at most 1e-4 of the lanes may
  be out at an episode's end (or at the end of the recording), the others are compared at every step.
Every assertion message starts with a label from LABELS: the mutant tests name the one they trip."""
import functools

import numpy as np

import oracle
import sac_oracle as S

LABELS = ("ring slot", "ring successor", "stored action", "episode end", "mask", "reward", "observation", "reset observation",
          "titration cell", "held observation", "env field", "env action", "traced state", "returned sum")
ACTION_ATOL = {"td3": 5e-5, "sac": 3e-5}
ENV_TOL = {"ph": 2e-5, "integrator": 2e-4, "stacking": 2e-4}
EVAL_ACTION_ATOL = 3e-5      # the bar of the PPO and SAC trace tests
CELL, CELL_SHARE = 1e-5, 1e-4


def obs_dim(spec):
    return {"ph": 3, "integrator": 4}.get(spec["env"]) or 3 * spec["num_stack"]


def setpoint_col(spec):
    """Column of the episode's set-point r: pH [y, r, I], Integrator [h1, h2, r, I], Stacking: the newest frame's (h1, h2, r)."""
    return {"ph": 1, "integrator": 2}.get(spec["env"], obs_dim(spec) - 1)


@functools.lru_cache(maxsize=None)
def _ph_table():
    return oracle.ph_table()


def make_oracle(spec, n, **kw):
    if spec["env"] == "ph":
        return oracle.OraclePH(n, _ph_table(), max_steps=spec["T"], seed=spec["seed"], env_offset=spec["env_offset"], **kw)
    return oracle.OracleWT(n, max_steps=spec["T"], reward_type="distance", num_stack=spec.get("num_stack", 0) if spec["env"] == "stacking" else 0,
                           seed=spec["seed"], env_offset=spec["env_offset"], **kw)


def resync(ref, spec, obs):
    """The float64 oracle continues from ITS state: put it on the recorded float32 state so one step's error does not compound."""
    if spec["env"] == "ph":
        return
    D = obs.shape[1]
    cols = (("h1", D - 3), ("h2", D - 2)) if spec["env"] == "stacking" else (("h1", 0), ("h2", 1), ("I", 3))
    for name, col in cols:
        ref.set(name, obs[:, col].astype(np.float64))


def oracle_action(spec, state, epoch, t, n):
    """float64-accumulated stored action of the rows `state` at lock-step t of the call with noise epoch `epoch`."""
    eps = oracle.explore_noise(spec["noise_seed"], spec["env_offset"], n, epoch, t)
    if spec["kind"] == "sac":
        act = S.f64(spec["actor"], S.ACTOR_KEYS)
        return S.actor_forward(act, state.astype(np.float64), eps)["a"][:, 0]
    mean = oracle.critic_forward(state, spec["actor"])[:, 0]
    return np.clip(np.tanh(mean.astype(np.float64)) + np.float64(np.float32(spec["sigma"])) * eps, -1.0, 1.0)


def env_action(stored, state, priorK):
    """a_env as the kernels form it: the float32 stored action widened, then + state[j] * priorK[j] in float64, j ascending."""
    a = stored.astype(np.float64)
    for j in range(state.shape[1]):
        a = a + state[:, j].astype(np.float64) * priorK[j]
    return a


def _share(label, got, want, tol, where, rel=True):
    """Largest used share of the bar |got - want| <= tol * (1 + |want|) (rel) or tol; asserts it is at most 1."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    bar = tol * (1.0 + np.abs(want)) if rel else tol
    used = np.abs(got - want) / bar
    worst = float(np.nanmax(used)) if np.isfinite(used).all() else float("inf")
    assert worst <= 1.0, f"{label}: {worst:.3g} of the bar {tol:g} at {where} (lane/column {np.unravel_index(np.argmax(used), used.shape)})"
    return worst


def check_exploration(rec, spec):
    """Assert everything the module docstring lists; returns the largest used share of each bar and the pH lanes out of cell."""
    state, other, held = rec["state"], rec["other"], rec["held"]
    n, N, D = state.shape
    assert D == obs_dim(spec) and other.shape == (n, N, 3) and held.shape == (N, D) and state.dtype == other.dtype == np.float32
    calls, slots, T = spec["calls"], spec["slots"], spec["T"]
    assert sum(c[1] for c in calls) == n and len(rec["slot"]) == n
    priorK = np.asarray(spec["priorK"], dtype=np.float64).reshape(-1)
    assert priorK.shape == (D,)
    is_ph, tol = spec["env"] == "ph", ENV_TOL[spec["env"]]
    gamma32, scale = np.float32(spec["gamma"]), float(spec["reward_scale"])
    rc = setpoint_col(spec)

    # ---- ring: row j of a call sits in slot (slot0 + j) % slots; each row's successor continues the trajectory (the episode's set-point
    # travels unchanged from a row to its successor -- the next row, or the held observation -- inside an episode)
    k = 0
    for epoch, n_steps, slot0 in calls:
        assert 1 <= n_steps <= slots
        for j in range(n_steps):
            assert int(rec["slot"][k]) == (slot0 + j) % slots, f"ring slot: row {j} of the call with epoch {epoch} read from slot {rec['slot'][k]}"
            k += 1
    for k in range(n):
        succ = state[k + 1] if k + 1 < n else held
        cont = (other[k, :, 1] != 0) & ((k + 1) % T != 0)   # (where mask and step count disagree, "episode end" below says so)
        assert np.array_equal(succ[cont, rc], state[k][cont, rc]), f"ring successor: the set-point changes behind lock-step {k} inside an episode"

    ref = make_oracle(spec, N)
    obs = ref.reset()
    assert np.array_equal(state[0], obs), "reset observation: the first stored row is not the oracle's reset observation"
    used = {"action": 0.0, "observation": 0.0, "reward": 0.0}
    alive, cell_exact = np.ones(N, dtype=bool), []
    k = 0
    for epoch, n_steps, _ in calls:
        for t in range(n_steps):
            where = f"lock-step {k} (step {t} of the call with epoch {epoch})"
            s, o = state[k], other[k]
            # stored action: the oracle's forward of the state the kernel saw + the oracle's draw of (global lane, epoch, t in call)
            want = oracle_action(spec, s, epoch, t, N)
            used["action"] = max(used["action"], _share("stored action", o[:, 2], want, ACTION_ATOL[spec["kind"]], where, rel=False))
            assert float(np.abs(o[:, 2]).max()) <= 1.0, f"stored action: outside [-1, 1] at {where}"
            # env side
            nxt_got = state[k + 1] if k + 1 < n else held
            nxt, _, rew, d = ref.step(env_action(o[:, 2], s, priorK), auto_reset=True)
            end = (k + 1) % T == 0
            assert bool(d.all()) == end and bool(d.any()) == end, f"episode end: the oracle's episodes end at multiples of {T}, not at {where}"
            assert np.array_equal(o[:, 1] == 0, d), f"episode end: mask 0 on {int((o[:, 1] == 0).sum())} lanes at {where}, oracle {int(d.sum())}"
            assert np.array_equal(o[:, 1][~d], np.full(int((~d).sum()), gamma32)), f"mask: not float32(gamma) inside an episode at {where}"
            want_r = rew * scale
            if end:   # the successor holds the next episode's first observation: the last step shows in its reward only
                if is_ph:
                    alive &= np.abs(o[:, 0] - want_r) <= tol * (1.0 + np.abs(want_r))
                    cell_exact.append(alive.mean())
                else:
                    used["reward"] = max(used["reward"], _share("reward", o[:, 0], want_r, tol, where))
                label = "reset observation" if k + 1 < n else "held observation"
                assert np.array_equal(nxt_got, nxt), f"{label}: not bit-equal to the oracle's reset observation behind {where}"
                if spec["env"] == "stacking":
                    assert np.array_equal(nxt_got, np.tile(nxt_got[:, D - 3:], (1, D // 3))), f"reset observation: frames differ behind {where}"
                alive[:] = True
            else:
                if is_ph:
                    alive &= np.abs(nxt_got[:, 0] - nxt[:, 0]) <= CELL
                used["reward"] = max(used["reward"], _share("reward", o[:, 0][alive], want_r[alive], tol, where))
                label = "observation" if k + 1 < n else "held observation"
                used["observation"] = max(used["observation"], _share(label, nxt_got[alive], nxt[alive], tol, where))
                if k + 1 < n:
                    resync(ref, spec, nxt_got)
            k += 1
    cell_exact.append(alive.mean())
    assert min(cell_exact) >= 1.0 - CELL_SHARE, f"titration cell: only {min(cell_exact):.5f} of the lanes stayed cell-exact over an episode"

    # ---- after the last call (the oracle was not re-synced behind the last step: it holds its own float64 successor state)
    f = rec["fields"]
    t_now = float(n % T)
    for name, want in (("t", np.full(N, t_now)), ("episode", ref.get("episode"))):
        assert np.array_equal(f[name], want), f"env field: {name} {np.unique(f[name])} != {np.unique(want)}"
    if is_ph:
        _share("env field x", f["x"][alive], ref.get("x")[alive], 1e-12, "the end of the last call")
        _share("env field I", f["I"][alive], ref.get("I")[alive], tol, "the end of the last call")
        assert np.array_equal(f["qww_V"], ref.get("qww_V")), "env field: qww_V (ensemble parameter of the running episode)"
    else:
        for name in ("h1", "h2"):
            _share("env field " + name, f[name], ref.get(name), tol, "the end of the last call")
        for name in ("a1", "Kp"):
            want = ref.get(name)
            assert (np.abs(f[name] - want) <= 1e-7 * np.abs(want)).all(), f"env field: {name} (ensemble parameter of the running episode)"
    used["lanes_out"] = int(round((1.0 - min(cell_exact)) * N))
    return used


def check_evaluation(trace, ret, reset_obs, spec):
    """One traced evaluation launch of n_steps <= T steps from a fresh reset (no noise, no auto-reset) under the TD3 Actor (kind "sac":
    ActorSAC's mean head):
    trace float64 [n_steps, 6, N] -- pH: (y, r, I before the step | env action, reward, x after); tank: (h1, h2, r, I after the step |
    reward, env action); ret float64 [N] the returned sums; reset_obs float32 [N, D] what env.reset() returned.
    On a Stacking observation the trace holds the newest frame (h1, h2, r) after each step, not the whole observation: `seen` is rebuilt
    here from the reset observation and the traced frames (deque append, oldest first).
    Asserts: the env action is tanh(oracle.critic_forward(seen)) + seen @ priorK (3e-5; SAC: tanh(avg) of tests/sac_oracle.py); the
    recorded actions replayed through the oracle reproduce the traced state and reward within the mode's bars; the returned sum is the
    trace's reward column."""
    n_steps, six, N = trace.shape
    D = obs_dim(spec)
    assert six == 6 and reset_obs.shape == (N, D) and n_steps <= spec["T"]
    is_ph, tol = spec["env"] == "ph", ENV_TOL[spec["env"]]
    priorK = np.asarray(spec["priorK"], dtype=np.float64).reshape(-1)
    ref = make_oracle(spec, N)
    obs = ref.reset()
    assert np.array_equal(reset_obs, obs), "reset observation: env.reset() is not the oracle's"
    used = {"action": 0.0, "observation": 0.0, "reward": 0.0}
    seen = reset_obs.copy()
    alive = np.ones(N, dtype=bool)
    a_col, r_col = (3, 4) if is_ph else (5, 4)
    nxt = obs
    for t in range(n_steps):
        where = f"step {t}"
        if is_ph:   # the trace holds what the policy saw: the observation the step before left (cell-exact lanes only)
            seen = trace[t, 0:3].T.astype(np.float32)
            assert np.array_equal(seen.astype(np.float64), trace[t, 0:3].T), f"traced state: not float32 values before {where}"
            if t == 0:
                assert np.array_equal(seen, reset_obs), "traced state: the first step does not see the reset observation"
            else:
                alive &= np.abs(seen[:, 0] - nxt[:, 0]) <= CELL
                used["observation"] = max(used["observation"], _share("traced state", seen[alive], nxt[alive], tol, where))
        if spec["kind"] == "sac":   # ActorSAC.forward: tanh(net_a_avg(net_state(s)))
            mean = S.actor_forward(S.f64(spec["actor"], S.ACTOR_KEYS), seen.astype(np.float64))["avg"][:, 0]
        else:
            mean = oracle.critic_forward(seen, spec["actor"])[:, 0]
        dot = np.zeros(N)
        for j in range(D):
            dot = dot + seen[:, j].astype(np.float64) * priorK[j]
        want = np.tanh(mean.astype(np.float64)) + dot
        used["action"] = max(used["action"], _share("env action", trace[t, a_col], want, EVAL_ACTION_ATOL, where, rel=False))
        nxt, _, rew, _ = ref.step(trace[t, a_col])
        if is_ph:
            x = ref.get("x")
            alive &= np.abs(trace[t, 5] - x) <= 1e-12 * np.abs(x)      # cell-exact lanes carry the oracle's plant state
        else:
            w = 3 if spec["env"] == "stacking" else 4
            after = trace[t, 0:w].T.astype(np.float32)
            assert np.array_equal(after.astype(np.float64), trace[t, 0:w].T), f"traced state: not float32 values after {where}"
            seen = np.concatenate([seen[:, 3:], after], axis=1) if spec["env"] == "stacking" else after
            used["observation"] = max(used["observation"], _share("traced state", seen, nxt, tol, where))
            resync(ref, spec, seen)
        used["reward"] = max(used["reward"], _share("reward", trace[t, r_col][alive], rew[alive], tol, where))
    assert alive.mean() >= 1.0 - CELL_SHARE, f"titration cell: only {alive.mean():.5f} of the lanes stayed cell-exact"
    # the kernel adds float32 rewards into a float64 sum, in step order
    _share("returned sum", ret, trace[:, r_col].sum(axis=0), 1e-12, "the end of the launch")
    used["lanes_out"] = int((~alive).sum())
    return used
