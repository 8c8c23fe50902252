"""Replay of what the fused on-policy rollout (`pime_rollout` / `pime_rollout_h`: rollout_kernel of csrc/rollout.hip, rollout16_kernel of
csrc/mlp16.hip) stored, through the float64 oracle.  Pure numpy + `oracle`: no torch, no GPU -- tests/test_onpolicy_replay_cpu.py vets it
on recordings synthesised from the oracle itself (one honest, the others each with one fault), tests/test_gpu_rollout_sweep.py feeds it
what every instantiation of the kernels stored over launches that start and stop inside episodes.

A RECORDING is a dict:
  state   float32 | float16 [n + 1, N, D]   slot 0 the observation before the first launch, then the row behind every step
  reward  float32 | float16 [n, N]          (float16: `pime_rollout_h`, the binary16 rows of state_mode "mixed16")
  action  float32 [n, N]                    the stored pre-tanh action a_pre = mean + eps * sigma
  noise   float32 [n, N]                    the stored draw eps
  done    uint8 [n, N]
  fields  {name: float64 [N]}   env fields read back after the last launch, before the hand-over step:
                                pH x I r qww_V qc_V t episode; tank h1 h2 r I a1 a2 Kp t episode (Stacking: no I, the variant
                                has no integrated error)
  handoff {action float32 [N], obs [N, D], reward [N], done uint8 [N]}   ONE launch-by-launch step (env.step_residual /
                                step_residual_h, auto-reset on) taken after the last launch on the last stored row with `action`
n = the steps of all launches, in launch order.

A SPEC is a dict:
  env "ph" | "integrator" | "stacking", num_stack, T (max steps), seed, env_offset, noise_seed, calls [(epoch, n_steps)],
  kind "plain" | "modular", actor (numpy state dict with a_std_log), priorK float64 [D], half (binary16 rows)

Bars (none of them this module's own):
  float32 rows (tests/rollout_replay.py: replay_through_oracle): the draw within one float32 ulp (rtol 1.2e-7) and at most 1e-4 of the
    recording's draws unequal at all; policy mean 3e-5 * (1 + |want|); observation and reward tol * (1 + |want|), tol = 2e-5 on pH and
    2e-4 on the tank; the pH cell rule: a lane whose y leaves the oracle's by more than 1e-5 is set aside until its episode ends, and at
    most 1e-4 of the lanes may be.  Plant state x of a cell-exact lane 1e-12 (tests/offpolicy_replay.py), ensemble parameters bit-equal
    on pH and 1e-7 on the tank (tests/test_gpu_rollout_oracle.py).
  binary16 rows (tests/test_gpu_config5.py: _replay_half): H = 2^-11 per stored word with that function's absolute terms -- reward
    2 H + 3e-3; pH y inside H |y| + 1e-6 of the oracle's cell (no lane-step outside), r H, I H + 1e-5; tank levels and set-point
    H + 2e-3, I H + 2e-3 + 1e-5 -- and the oracle's I re-synchronised to the stored value after every step.
The tank's levels are re-synchronised to the recorded float32 rows as in offpolicy_replay.resync.
Every assertion message starts with a label from LABELS: the mutant tests name the one they trip."""
import numpy as np

import oracle
from offpolicy_replay import CELL, CELL_SHARE, ENV_TOL, make_oracle, obs_dim, resync

LABELS = ("exploration noise", "policy mean", "episode end", "reward", "observation", "reset observation", "titration cell", "env field",
          "hand-over")
NOISE_RTOL, NOISE_SHARE = 1.2e-7, 1e-4   # tests/rollout_replay.py: one float32 ulp, on at most one draw in 10^4
MEAN_TOL = 3e-5                          # tests/rollout_replay.py: rtol = atol = 3e-5
X_RTOL = 1e-12                           # tests/offpolicy_replay.py: the float64 plant state of a cell-exact pH lane
PARAM_RTOL = 1e-7                        # tests/test_gpu_rollout_oracle.py: the tank's ensemble parameters (float32 words)
H = 2.0 ** -11                           # tests/test_gpu_config5.py: one rounding to binary16
HALF_REWARD = (2 * H, 3e-3)              # (rtol, atol) of _replay_half, as are the following
HALF_PH_Y, HALF_PH_R, HALF_PH_I = (H, 1e-6), (H, 0.0), (H, 1e-5)
HALF_WT_LEVEL, HALF_WT_I = (H, 2e-3), (H, 2e-3 + 1e-5)
FIELDS = {"ph": ("x", "I", "r", "qww_V", "qc_V", "t", "episode"), "tank": ("h1", "h2", "r", "I", "a1", "a2", "Kp", "t", "episode")}


def field_names(spec):
    names = FIELDS["ph" if spec["env"] == "ph" else "tank"]
    return tuple(f for f in names if f != "I") if spec["env"] == "stacking" else names


def actor_mean(spec, rows):
    f = oracle.modular_actor_mean if spec["kind"] == "modular" else oracle.plain_actor_mean
    return f(np.ascontiguousarray(rows, dtype=np.float32), spec["actor"])[:, 0]


def sigma_of(spec):
    return np.float32(np.exp(np.asarray(spec["actor"]["a_std_log"], dtype=np.float32).reshape(-1)[0]))


def _share(label, got, want, bar, where):
    """Largest used share of |got - want| <= bar (an array like want, or a scalar); asserts it is at most 1."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    used = np.abs(got - want) / bar
    worst = float(np.nanmax(used)) if np.isfinite(used).all() else float("inf")
    assert worst <= 1.0, f"{label}: {worst:.3g} of the bar at {where} (lane/column {np.unravel_index(np.argmax(used), used.shape)})"
    return worst


def _bar(want, rtol_atol):
    return rtol_atol[0] * np.abs(np.asarray(want, dtype=np.float64)) + rtol_atol[1]


class _Judge:
    """One step's stored reward and successor row against the oracle's, under the bars of the row format."""

    def __init__(self, spec, N):
        self.spec, self.N = spec, N
        self.is_ph, self.stacking, self.half = spec["env"] == "ph", spec["env"] == "stacking", bool(spec.get("half"))
        self.tol, self.D = ENV_TOL[spec["env"]], obs_dim(spec)
        self.used = {"noise": 0.0, "mean": 0.0, "observation": 0.0, "reward": 0.0}
        self.alive, self.cell_exact, self.off_cell = np.ones(N, dtype=bool), [], 0

    def _max(self, what, share):
        self.used[what] = max(self.used[what], share)

    def step(self, seen_rows, got_next, got_rew, nxt, rew, end, where, handover=False):
        """seen_rows: the stored row the step started from (row format); got_next / got_rew: what was stored behind the step; nxt, rew:
        the oracle's float32 successor observation and float64 reward; end: the step ends an episode (got_next is a reset row)."""
        lab = (lambda s: "hand-over") if handover else (lambda s: s)
        D, alive = self.D, self.alive
        got64, rew64 = got_next.astype(np.float64), got_rew.astype(np.float64)
        rbar = _bar(rew, HALF_REWARD) if self.half else self.tol * (1.0 + np.abs(rew))
        if end:   # the successor holds the next episode's first observation: the last step shows in its reward only
            if self.is_ph and not self.half:
                alive &= np.abs(rew64 - rew) <= rbar
                self.cell_exact.append(alive.mean())
            else:
                self._max("reward", _share(lab("reward"), rew64, rew, rbar, where))
            want_row = nxt.astype(np.float16) if self.half else nxt
            assert np.array_equal(got_next, want_row), f"{lab('reset observation')}: not bit-equal to the oracle's reset observation behind {where}"
            if self.stacking:
                assert np.array_equal(got_next, np.tile(got_next[:, D - 3:], (1, D // 3))), \
                    f"{lab('reset observation')}: the frames of a reset row differ behind {where}"
            alive[:] = True
            return
        if self.half:
            self._max("reward", _share(lab("reward"), rew64, rew, rbar, where))
            if self.is_ph:
                self.off_cell += int((np.abs(got64[:, 0] - nxt[:, 0]) > _bar(nxt[:, 0], HALF_PH_Y)).sum())
                bars, cols = np.stack([_bar(nxt[:, 1], HALF_PH_R) + 1e-300, _bar(nxt[:, 2], HALF_PH_I)], axis=1), slice(1, 3)
            else:
                bars = np.concatenate([_bar(nxt[:, :3], HALF_WT_LEVEL), _bar(nxt[:, 3:], HALF_WT_I)], axis=1)
                cols = slice(0, 4)
            self._max("observation", _share(lab("observation"), got64[:, cols], nxt[:, cols], bars, where))
            return
        if self.is_ph:
            alive &= np.abs(got64[:, 0] - nxt[:, 0]) <= CELL
        self._max("reward", _share(lab("reward"), rew64[alive], rew[alive], rbar[alive], where))
        if self.stacking:   # the deque: every older frame is the row's next-newer one, bit for bit
            assert np.array_equal(got_next[:, :D - 3], seen_rows[:, 3:]), f"{lab('observation')}: the frames are not the last row's shifted by one, oldest first, behind {where}"
        self._max("observation", _share(lab("observation"), got64[alive], nxt[alive], self.tol * (1.0 + np.abs(nxt[alive])), where))


def check_rollout(rec, spec):
    """Assert everything the module docstring lists; returns the largest used share of each bar (noise, mean, observation, reward) and
    the lanes set aside (binary16 rows: the pH lane-steps outside the oracle's cell)."""
    state, reward, action, noise, done = rec["state"], rec["reward"], rec["action"], rec["noise"], rec["done"]
    n, N, D = state.shape[0] - 1, state.shape[1], state.shape[2]
    half = bool(spec.get("half"))
    row_t = np.float16 if half else np.float32
    assert D == obs_dim(spec) and state.dtype == reward.dtype == row_t and action.dtype == noise.dtype == np.float32 and done.dtype == np.uint8
    assert reward.shape == action.shape == noise.shape == done.shape == (n, N)
    assert not half or spec["env"] != "stacking", "binary16 rows: pH and the Integrator tank"
    calls, T = spec["calls"], spec["T"]
    assert sum(c[1] for c in calls) == n
    priorK = np.asarray(spec["priorK"], dtype=np.float64).reshape(-1)
    assert priorK.shape == (D,)
    is_ph = spec["env"] == "ph"
    sigma = sigma_of(spec)
    J = _Judge(spec, N)

    ref = make_oracle(spec, N)
    obs = ref.reset()
    assert np.array_equal(state[0], obs.astype(row_t)), "reset observation: slot 0 is not the oracle's reset observation"
    if half:
        ref.set("I", state[0][:, -1].astype(np.float64))
    unequal, k = 0, 0
    for epoch, n_steps in calls:
        for t in range(n_steps):
            tt = k % T
            where = f"step {k} (step {t} of the launch with epoch {epoch}, step {tt} of its episode)"
            seen = state[k].astype(np.float32)   # the row the policy and the prior term saw (binary16 rows: widened)
            # exploration noise: the draw of (global lane, the launch's epoch, the step index inside the launch)
            want_eps = oracle.explore_noise(spec["noise_seed"], spec["env_offset"], N, epoch, t)
            unequal += int((noise[k] != want_eps).sum())
            J._max("noise", _share("exploration noise", noise[k], want_eps, NOISE_RTOL * np.abs(want_eps) + 1e-300, where))
            # policy mean on the row the kernel saw, at every step
            want = actor_mean(spec, seen)
            J._max("mean", _share("policy mean", action[k] - noise[k] * sigma, want, MEAN_TOL * (1.0 + np.abs(want)), where))
            # env step of the reference composition on the RECORDED action and row
            nxt, _, rew, d = ref.step(oracle.residual_action(action[k], seen, priorK), auto_reset=True)
            end = tt == T - 1
            assert bool(d.all()) == end and bool(d.any()) == end, f"episode end: the oracle's episodes end at step {T - 1}, not at {where}"
            assert np.array_equal(done[k], d.astype(np.uint8)), f"episode end: done on {int((done[k] != 0).sum())} lanes at {where}, oracle {int(d.sum())}"
            J.step(state[k], state[k + 1], reward[k], nxt, rew, end, where)
            if half:
                ref.set("I", state[k + 1][:, -1].astype(np.float64))   # the device continues from the STORED (rounded) integrator
            elif not end and k + 1 < n:
                resync(ref, spec, state[k + 1])
            k += 1
    assert unequal <= NOISE_SHARE * n * N, f"exploration noise: {unequal} of {n * N} draws are not bit-equal to the oracle's"
    J.cell_exact.append(J.alive.mean())
    assert min(J.cell_exact) >= 1.0 - CELL_SHARE, f"titration cell: only {min(J.cell_exact):.5f} of the lanes stayed cell-exact over an episode"
    assert J.off_cell == 0, f"titration cell: {J.off_cell} pH lane-steps read another titration cell than the oracle"

    # ---- what the launch wrote back (float32 rows: the oracle was not re-synced behind the last step, it holds its own successor state)
    f, alive = rec["fields"], J.alive
    where = "the end of the last launch"
    assert set(f) >= set(field_names(spec)), f"env field: missing {set(field_names(spec)) - set(f)}"
    for name, want in (("t", np.full(N, float(n % T))), ("episode", ref.get("episode"))):
        assert np.array_equal(f[name], want), f"env field: {name} {np.unique(f[name])} != {np.unique(want)}"
    if is_ph:
        _share("env field x", f["x"][alive], ref.get("x")[alive], X_RTOL * np.abs(ref.get("x")[alive]) + 1e-300, where)
        for name in ("qww_V", "qc_V"):
            assert np.array_equal(f[name], ref.get(name)), f"env field: {name} (ensemble parameter of the running episode)"
        cols = (("r", _bar(ref.get("r"), HALF_PH_R) + 1e-300), ("I", _bar(ref.get("I"), HALF_PH_I))) if half else \
            (("r", None), ("I", None))
    else:
        for name in ("a1", "a2", "Kp"):
            want = ref.get(name)
            assert (np.abs(f[name] - want) <= PARAM_RTOL * np.abs(want)).all(), f"env field: {name} (ensemble parameter of the running episode)"
        level = (lambda name: _bar(ref.get(name), HALF_WT_LEVEL)) if half else (lambda name: None)
        cols = (("h1", level("h1")), ("h2", level("h2")), ("r", level("r")), ("I", _bar(ref.get("I"), HALF_WT_I) if half else None))
        cols = cols[:3] if spec["env"] == "stacking" else cols
    for name, bar in cols:
        want = ref.get(name)
        _share("env field " + name, f[name][alive], want[alive], (J.tol * (1.0 + np.abs(want)) if bar is None else bar)[alive], where)
    if half:
        assert np.array_equal(f["I"], f["I"].astype(np.float16).astype(np.float64)), "env field: the handle's I is not a binary16 value"

    # ---- one launch-by-launch step on what the launch wrote back: t, I, last_a, on Stacking the frame ring and head
    ho = rec["handoff"]
    last = state[n]
    if not half:
        resync(ref, spec, last)
    tt = n % T
    nxt, _, rew, d = ref.step(oracle.residual_action(np.asarray(ho["action"], dtype=np.float32), last.astype(np.float32), priorK), auto_reset=True)
    end = tt == T - 1
    assert bool(d.all()) == end and bool(d.any()) == end
    assert ho["obs"].dtype == row_t and ho["reward"].dtype == row_t and ho["obs"].shape == (N, D)
    assert np.array_equal(np.asarray(ho["done"], dtype=np.uint8), d.astype(np.uint8)), \
        f"hand-over: done on {int((np.asarray(ho['done']) != 0).sum())} lanes behind the step after the last launch (step {tt} of its episode), oracle {int(d.sum())}"
    J.step(last, ho["obs"], ho["reward"], nxt, rew, end, "the step after the last launch", handover=True)
    assert J.off_cell == 0, f"hand-over: {J.off_cell} pH lanes read another titration cell than the oracle"
    if is_ph and not half and not end:
        assert J.alive.mean() >= 1.0 - CELL_SHARE, f"hand-over: only {J.alive.mean():.5f} of the lanes stayed cell-exact"
    used = dict(J.used)
    used["lanes_out"] = J.off_cell if half else int(round((1.0 - min(J.cell_exact)) * N))
    return used
