"""Batched evaluation protocols: the reference's fixed set-point step responses and robustness sweeps, run for a whole
grid of plants at once (one env lane per plant) instead of one Python loop per plant.

replaces (protocols only, not the matplotlib plotting around them):
  pH          test_ph_policy_uniform_integrator   /root/reference/utils/test.py:1369-1407  (r = 10,6,3,8,5 x 50 steps)
              params_ph[1] plant grid             utils/test.py:1225-1236
  water tank  test_policy_uniform_integrator      utils/test.py:209-349                    (r = 3,6,9,4,2 x max_step)
              robust_test_nonlinear_watertank     utils/robust_test.py:4-46                (3 plants, max_step 500)

`policy` maps a float32 observation batch [N, D] to env actions [N]; None selects the prior controller -obs @ K
(the reference's `get_linear_action`).  All lanes share the set-point sequence; each lane keeps its own plant.

With `policy=None` (prior controller) or `agent=<a residual PPO agent>` the whole protocol is ONE launch of the fused evaluation
kernel (csrc/rollout_eval.hip, `pime_rollout_eval` with a set-point schedule: no per-step launches, no per-step device-to-host
reads; round 2 read four state fields back per step); an arbitrary `policy` callable keeps the step-per-launch loop.

`step_response_metrics` / `robust_grid` return the QUALITY of the responses instead of the responses: per plant and set-point
segment the eight control indices of `METRIC_NAMES` (error integrals, overshoot, settling step, steady-state error, return, action
variation; definitions in include/pime_hip.h), reduced on the device while the protocol runs (`pime_rollout_eval_metrics`: one
launch, no trace) -- a dense robustness map costs 64 bytes per plant and segment instead of 48 bytes per plant and STEP.

`step_response_band` returns the response of a whole ENSEMBLE as a band: per step and lane group the mean, standard deviation,
minimum and maximum of the controlled output, the error, the action and the reward over the group's plants, and a histogram of
the output (`band_quantiles` turns it into a percentile fan) -- reduced across lanes on the device while the protocol runs
(`pime_rollout_eval_band`: one launch, no trace; 128 bytes + 4 bytes per bin leave the device per step and group).

`identify_plants` turns the grid around: instead of scoring a policy on a grid of plants it scores the PLANTS against recorded runs
(`records_from_physical`: measured data; `records_from_trace`: a fused evaluation's trace, for sim-to-sim studies) -- every (plant,
record) pair replayed and its output error reduced in one launch (`pime_env_replay_error`) -- and `ensemble_ranges` reads the
plausible ensemble bounds off the result: the check that the training ensemble brackets the real plant.

`tune_prior` asks the question that comes next: which PRIOR GAIN is best over that whole ensemble, and how bad is it on its worst
plant?  A grid of gains (`gain_box`) x the plants in the env's lanes, every pair's step response reduced to the control indices and
each index across the plants in one call (`pime_prior_sweep`), a few numbers per gain coming back.

Sign convention.  The env classes hold K with a = -obs @ K (the reference's `get_linear_action`); the kernels take priorK = -env.K
with a = obs @ priorK.  `tune_prior` and `VecControlEnv.prior_sweep` take and return gains in the KERNELS' sign (priorK);
`gain_box` scales whatever it is given and keeps its sign; `train.py --prior_K` reads `best_gain` in the ENV's sign (env.K).
"""
from collections import OrderedDict

import numpy as np
import torch

from .native import ACT_ROW_NAMES, BAND_SIGNALS, BAND_STATS, DISTURB_ROW_NAMES, ENV_PH, FREQ_POINTS, FREQ_ROW_NAMES, METRIC_NAMES, REPLAY_ROW_NAMES, SWEEP_STATS

PH_SETPOINTS = (10., 6., 3., 8., 5.)
WT_SETPOINTS = (3., 6., 9., 4., 2.)
PH_PARAM_GRID = ((0.005, 0.0025), (0.005, 0.0015), (0.015, 0.0025), (0.015, 0.0015), (0.001, 0.002), (0.001, 0.0022),
                 (0.001, 0.0018), (0.0007, 0.002), (0.0013, 0.002))          # utils/test.py:1225-1236 (qww_V, qc_V)
WT_ROBUST_PLANTS = ((0.0024, 0.0019, 0.12), (0.0024, 0.0015, 0.12), (0.0024, 0.0015, 0.07))  # robust_test.py:13-44


def _prior(env):
    k = torch.as_tensor(-env.K, dtype=torch.float64, device=env.device)
    return lambda obs: obs.double() @ k


def _fused_policy(env, policy, agent):
    """(packed actor or None, priorK) when the fused evaluation kernel can run the protocol, else None."""
    if policy is not None or not hasattr(env, "eval_supported"):
        return None
    if agent is None:
        return (None, -env.K) if env.eval_supported(None, trace=True, schedule=True) else None
    fused = agent.fused_eval_policy(env) if hasattr(agent, "fused_eval_policy") else None
    return fused if fused is not None and env.eval_supported(fused[0], trace=True, schedule=True) else None


def ph_step_response(env, policy=None, setpoints=PH_SETPOINTS, steps=50, plants=None, agent=None):
    """env: VecPH.  plants: optional [N, 2] (qww_V, qc_V) written before the run (the plant IS rebuilt, unlike the
    reference's set_params -- SURVEY.md App. C.3).  Returns dict of [len(setpoints)*steps, N] float64 arrays
    y, r, I, action, reward (and x) exactly in the order the reference protocol appends them."""
    fused = _fused_policy(env, policy, agent)
    env.set_reset_all(False)
    env.set_max_step(2 ** 30)                      # the protocol ignores TimeLimit's done and runs `steps` per segment
    if plants is not None:
        plants = np.asarray(plants, dtype=np.float64)
        env.set_params(plants[:, 0], plants[:, 1])
    if fused is not None and len(setpoints) <= 16:
        env.reset()
        env.set_field("x", np.zeros(env.num_envs))          # the protocol starts from state 0 (utils/test.py:1375)
        _, tr = env.rollout_eval(fused[0], fused[1], len(setpoints) * steps, setpoints=setpoints, seg_len=steps, want_trace=True)
        tr = tr.cpu().numpy()
        return {"y": tr[:, 0], "r": tr[:, 1], "I": tr[:, 2], "action": tr[:, 3], "reward": tr[:, 4], "x": tr[:, 5]}
    policy = policy or (agent.act if agent is not None else _prior(env))
    out = {k: [] for k in ("y", "r", "I", "action", "reward", "x")}
    last_x = np.zeros(env.num_envs)
    for r in setpoints:
        env.reset()
        env.set_field("x", last_x)
        env.set_field("r", float(r))
        obs = env.observe().clone()
        for _ in range(steps):
            a = policy(obs)
            out["y"].append(env.get_field("y")); out["r"].append(env.get_field("r")); out["I"].append(env.get_field("I"))
            out["action"].append(a.detach().double().cpu().numpy().reshape(-1))
            nxt, rew, _ = env.step(a.detach(), auto_reset=False)
            out["reward"].append(rew.double().cpu().numpy()); out["x"].append(env.get_field("x"))
            obs = nxt.clone()
        last_x = env.get_field("x")
    return {k: np.stack(v) for k, v in out.items()}


def wt_step_response(env, policy=None, setpoints=WT_SETPOINTS, steps=None, plants=None, agent=None):
    """env: VecWaterTank (Integrator observation).  plants: optional [N, 3] (a1, a2, Kp).  Returns obs [S*steps, N, D],
    action and reward [S*steps, N]; tank levels are carried from one set-point segment to the next."""
    fused = _fused_policy(env, policy, agent)
    steps = steps or env.max_step
    env.set_reset_all(False)
    env.set_max_step(max(steps, env.max_step))
    if plants is not None:
        plants = np.asarray(plants, dtype=np.float64)
        env.reset_changable_parameters(plants[:, 0], plants[:, 1], plants[:, 2])
    if fused is not None and len(setpoints) <= 16 and env.num_stack == 0:
        env.reset()
        env.set_field("h1", np.zeros(env.num_envs)); env.set_field("h2", np.zeros(env.num_envs))   # utils/test.py:219-221
        _, tr = env.rollout_eval(fused[0], fused[1], len(setpoints) * steps, setpoints=setpoints, seg_len=steps, want_trace=True)
        tr = tr.cpu().numpy()
        return {"obs": np.ascontiguousarray(np.transpose(tr[:, :4], (0, 2, 1))), "reward": tr[:, 4], "action": tr[:, 5]}
    policy = policy or (agent.act if agent is not None else _prior(env))
    out = {k: [] for k in ("obs", "action", "reward")}
    h1 = h2 = np.zeros(env.num_envs)
    for r in setpoints:
        env.reset()
        env.set_field("h1", h1); env.set_field("h2", h2); env.set_field("r", float(r))
        obs = env.observe().clone()
        for _ in range(steps):
            a = policy(obs)
            nxt, rew, _ = env.step(a.detach(), auto_reset=False)
            out["action"].append(a.detach().double().cpu().numpy().reshape(-1))
            out["obs"].append(np.stack([env.get_field(f) for f in ("h1", "h2", "r", "I")], axis=1))
            out["reward"].append(rew.double().cpu().numpy())
            obs = nxt.clone()
        h1, h2 = env.get_field("h1"), env.get_field("h2")
    return {k: np.stack(v) for k, v in out.items()}


def metrics_from_records(y_after, r, action, reward, y_start, seg_len=0, band=0.05, tail=10):
    """The eight rows of `pime_rollout_eval_metrics` from step-by-step records, in numpy -- for the paths the fused kernel does not
    serve (an arbitrary `policy` callable, draw injection).  y_after [T, N]: the controlled output AFTER each step (pH: y, tank:
    h2); r [T, N] or [T]: the set-point of each step; action, reward [T, N]; y_start [n_segments, N]: the output before each
    segment's first step; seg_len 0: one segment.  Returns dict name -> float64 [n_segments, N].  Sums run in ascending step order
    (np.cumsum adds sequentially), rewards are rounded to float32 before they are widened, as the kernel's are."""
    y = np.asarray(y_after, dtype=np.float64)
    T, N = y.shape
    r = np.broadcast_to(np.asarray(r, dtype=np.float64).reshape(T, -1), (T, N))
    a = np.asarray(action, dtype=np.float64).reshape(T, N)
    rew = np.asarray(reward).reshape(T, N).astype(np.float32).astype(np.float64)
    y_start = np.asarray(y_start, dtype=np.float64).reshape(-1, N)
    L0 = int(seg_len) if seg_len > 0 else T
    n_seg = -(-T // L0)
    assert y_start.shape[0] == n_seg and band >= 0 and tail >= 1
    out = {name: np.zeros((n_seg, N)) for name in METRIC_NAMES}
    last = lambda terms: np.cumsum(terms, axis=0)[-1]
    for s in range(n_seg):
        sl = slice(s * L0, min((s + 1) * L0, T))
        ys, rs, as_ = y[sl], r[sl][0], a[sl]
        L = ys.shape[0]
        e = rs - ys
        k1 = np.arange(1, L + 1, dtype=np.float64)[:, None]
        out["iae"][s] = last(np.abs(e))
        out["ise"][s] = last(e * e)
        out["itae"][s] = last(k1 * np.abs(e))
        d = np.where(rs >= y_start[s], 1.0, -1.0)
        out["overshoot"][s] = np.maximum(0.0, (d * (ys - rs)).max(axis=0))
        outside = np.abs(e) > band
        out["settling_step"][s] = np.where(outside.any(axis=0), L - np.argmax(outside[::-1], axis=0), 0)
        w = min(int(tail), L)
        out["steady_state_error"][s] = last(e[L - w:]) / w
        out["return"][s] = last(rew[sl])
        out["action_variation"][s] = last(np.abs(np.diff(as_, axis=0))) if L > 1 else 0.0
    return out


def _protocol_start(env, is_ph, steps, plants):
    """What the fused protocols do before their one launch: the plants written, a reset, the plant state at 0."""
    env.set_reset_all(False)
    if is_ph:
        env.set_max_step(2 ** 30)
        if plants is not None:
            plants = np.asarray(plants, dtype=np.float64)
            env.set_params(plants[:, 0], plants[:, 1])
        env.reset()
        env.set_field("x", np.zeros(env.num_envs))
    else:
        env.set_max_step(max(steps, env.max_step))
        if plants is not None:
            plants = np.asarray(plants, dtype=np.float64)
            env.reset_changable_parameters(plants[:, 0], plants[:, 1], plants[:, 2])
        env.reset()
        env.set_field("h1", np.zeros(env.num_envs)); env.set_field("h2", np.zeros(env.num_envs))


def _protocol_records(env, is_ph, policy, setpoints, steps, plants, agent):
    """The step-per-launch protocol as records: (y_after, r, action, reward, y_before), each [T, N]."""
    if is_ph:
        res = ph_step_response(env, policy=policy, setpoints=setpoints, steps=steps, plants=plants, agent=agent)
        y_before = res["y"]                                              # y BEFORE each step; the plant state is carried over
        y_after = np.concatenate([y_before[1:], env.get_field("y")[None]])
        r, action = res["r"], res["action"]
    else:
        res = wt_step_response(env, policy=policy, setpoints=setpoints, steps=steps, plants=plants, agent=agent)
        y_after = res["obs"][:, :, 1]
        y_before = np.concatenate([np.zeros((1, env.num_envs)), y_after[:-1]])   # the protocol starts from empty tanks
        r, action = res["obs"][:, :, 2], res["action"]
    return y_after, r, action, res["reward"], y_before


def step_response_metrics(env, agent=None, policy=None, setpoints=None, steps=None, plants=None, band=None, tail=10):
    """The step-response protocol of `env` (pH: `ph_step_response`, r = 10,6,3,8,5 x 50 steps; Integrator tank:
    `wt_step_response`, r = 3,6,9,4,2 x max_step) reduced to its control indices: dict of metric name (`METRIC_NAMES`) ->
    float64 [len(setpoints), N].  band: the settling band on |r - y| (default 0.05 for pH -- the reference's sparse-reward
    threshold -- and 0.05 for the tank); tail: the steady-state window in steps.  With the prior controller (agent and policy None)
    or an agent the fused evaluation kernel serves this is ONE launch and no trace; otherwise the step-per-launch protocol runs and
    `metrics_from_records` reduces its records."""
    is_ph = env.kind == ENV_PH
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    fused = _fused_policy(env, policy, agent)
    if fused is not None and len(setpoints) <= 16 and (is_ph or env.num_stack == 0):
        _protocol_start(env, is_ph, steps, plants)
        _, m, _ = env.rollout_eval_metrics(fused[0], fused[1], len(setpoints) * steps, setpoints=setpoints, seg_len=steps, band=band,
                                           tail=tail)
        m = m.cpu().numpy()
        return {name: np.ascontiguousarray(m[:, j]) for j, name in enumerate(METRIC_NAMES)}
    y_after, r, action, reward, y_before = _protocol_records(env, is_ph, policy, setpoints, steps, plants, agent)
    return metrics_from_records(y_after, r, action, reward, y_before[::steps], seg_len=steps, band=band, tail=tail)


def _grid(env, axes, who):
    """(names, axes as an OrderedDict of float64 arrays, shape, plants [n, P] in C order) -- the grid of `robust_grid`."""
    names = ("qww_V", "qc_V") if env.kind == ENV_PH else ("a1", "a2", "Kp")
    axes = OrderedDict((k, np.asarray(v, dtype=np.float64).reshape(-1)) for k, v in axes.items())
    if sorted(axes) != sorted(names):
        raise ValueError(f"{who}: axes {list(axes)} must name exactly {names}")
    shape = tuple(len(v) for v in axes.values())
    if int(np.prod(shape)) != env.num_envs:
        raise ValueError(f"{who}: the grid has {int(np.prod(shape))} plants, the env {env.num_envs} lanes")
    mesh = dict(zip(axes, np.meshgrid(*axes.values(), indexing="ij")))
    return names, axes, shape, np.stack([mesh[k].reshape(-1) for k in names], axis=1)


def robust_grid(env, axes, agent=None, policy=None, setpoints=None, steps=None, band=None, tail=10):
    """A dense robustness map: the step-response metrics over the Cartesian product of plant parameters.  axes: ordered mapping
    of plant parameter -> 1-D values (pH: qww_V, qc_V; tank: a1, a2, Kp -- all of them, in any order); env.num_envs must equal the
    product of their lengths; lane = the C-order index into the grid.  Returns (dict of metric name -> float64 [n_segments, *axis
    lengths], axes as an OrderedDict of float64 arrays)."""
    _, axes, shape, plants = _grid(env, axes, "robust_grid")
    m = step_response_metrics(env, agent=agent, policy=policy, setpoints=setpoints, steps=steps, plants=plants, band=band, tail=tail)
    return {k: v.reshape(v.shape[0], *shape) for k, v in m.items()}, axes


def band_from_records(y_after, r, action, reward, group_lanes=None, hist=None):
    """The rows of `pime_rollout_eval_band` from step-by-step records, in numpy -- for the paths the fused kernel does not serve
    (an arbitrary `policy` callable, draw injection).  y_after [T, N]: the controlled output AFTER each step; r [T, N] or [T]: the
    set-point of each step; action, reward [T, N] (rewards are rounded to float32 before they are widened, as the kernel's are).
    Lane i belongs to group i // group_lanes (None or >= N: one group).  hist: None or (bins, lo, hi).  Returns a dict: stats
    float64 [T, 16, G] with row 4 * signal + stat over BAND_SIGNALS x BAND_STATS, count int64 [G], hist int64 [T, G, bins] or None."""
    y = np.asarray(y_after, dtype=np.float64)
    T, N = y.shape
    r = np.broadcast_to(np.asarray(r, dtype=np.float64).reshape(T, -1), (T, N))
    a = np.asarray(action, dtype=np.float64).reshape(T, N)
    rew = np.asarray(reward).reshape(T, N).astype(np.float32).astype(np.float64)
    gl = N if group_lanes is None or group_lanes >= N else int(group_lanes)
    if gl <= 0 or (gl < N and gl % 16):
        raise ValueError(f"band_from_records: group_lanes {group_lanes} (a positive multiple of 16, or >= the {N} lanes)")
    G = -(-N // gl)
    stats = np.empty((T, len(BAND_SIGNALS) * len(BAND_STATS), G))
    count = np.array([min(gl, N - g * gl) for g in range(G)], dtype=np.int64)
    counts = None
    if hist is not None:
        bins, lo, hi = int(hist[0]), float(hist[1]), float(hist[2])
        if not (1 <= bins <= 256 and np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError(f"band_from_records: hist {hist} (1 <= bins <= 256, finite lo < hi)")
        scale = float(bins) / (hi - lo)
        with np.errstate(invalid="ignore"):
            inside = np.minimum(np.floor((np.clip(y, lo, hi) - lo) * scale), bins - 1).astype(np.int64)
            b = np.where(~(y >= lo), 0, np.where(y >= hi, bins - 1, inside))
        counts = np.zeros((T, G, bins), dtype=np.int64)
    for g in range(G):
        sl = slice(g * gl, min((g + 1) * gl, N))
        for j, x in enumerate((y[:, sl], (r - y)[:, sl], a[:, sl], rew[:, sl])):
            stats[:, 4 * j, g] = x.sum(axis=1)
            stats[:, 4 * j + 1, g] = (x * x).sum(axis=1)
            stats[:, 4 * j + 2, g] = x.min(axis=1)
            stats[:, 4 * j + 3, g] = x.max(axis=1)
        if counts is not None:
            for t in range(T):
                counts[t, g] = np.bincount(b[t, sl], minlength=bins)
    return {"stats": stats, "count": count, "hist": counts}


def _band_result(stats, count, counts, hist, metrics):
    """stats [T, 16, G] -> the band: mean / std / min / max per signal as [T, G] (std: the population's, from sum and sum of squares)."""
    n = count.astype(np.float64)[None, :]
    out = {"mean": {}, "std": {}, "min": {}, "max": {}, "count": count, "hist": counts, "edges": None, "metrics": metrics}
    for j, name in enumerate(BAND_SIGNALS):
        mean = stats[:, 4 * j + BAND_STATS.index("sum")] / n
        out["mean"][name] = mean
        out["std"][name] = np.sqrt(np.maximum(stats[:, 4 * j + BAND_STATS.index("sumsq")] / n - mean * mean, 0.0))
        out["min"][name] = np.ascontiguousarray(stats[:, 4 * j + BAND_STATS.index("min")])
        out["max"][name] = np.ascontiguousarray(stats[:, 4 * j + BAND_STATS.index("max")])
    if hist is not None:
        out["edges"] = np.linspace(float(hist[1]), float(hist[2]), int(hist[0]) + 1)
    return out


def step_response_band(env, agent=None, policy=None, setpoints=None, steps=None, plants=None, group_lanes=None, hist=None, band=None,
                       tail=10):
    """The step-response protocol of `env` (as `step_response_metrics`) over an ensemble of plants, reduced to a band per step:
    returns a dict with mean / std / min / max -> {signal in BAND_SIGNALS: float64 [T, G]} over the lanes of each group of
    `group_lanes` consecutive lanes (None: all lanes are one group), count int64 [G], hist (counts [T, G, bins] of the controlled
    output, for hist=(bins, lo, hi); values outside [lo, hi) count in the outer bins) with its bin edges [bins + 1], and metrics
    (the dict of `step_response_metrics`).  plants None: every lane keeps the plant its reset draws from the registered ranges.
    One launch and no trace where the fused evaluation kernel serves the configuration; otherwise the step-per-launch protocol runs
    and `band_from_records` / `metrics_from_records` reduce its records."""
    is_ph = env.kind == ENV_PH
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    fused = _fused_policy(env, policy, agent)
    if fused is not None and len(setpoints) <= 16 and (is_ph or env.num_stack == 0):
        _protocol_start(env, is_ph, steps, plants)
        _, m, stats, counts, _ = env.rollout_eval_band(fused[0], fused[1], len(setpoints) * steps, setpoints=setpoints, seg_len=steps,
                                                       band=band, tail=tail, group_lanes=group_lanes, hist=hist)
        m, stats = m.cpu().numpy(), stats.cpu().numpy()
        gl = env.num_envs if group_lanes is None or group_lanes >= env.num_envs else int(group_lanes)
        count = np.array([min(gl, env.num_envs - g * gl) for g in range(stats.shape[2])], dtype=np.int64)
        counts = None if counts is None else counts.cpu().numpy().view(np.uint32).astype(np.int64)
        metrics = {name: np.ascontiguousarray(m[:, j]) for j, name in enumerate(METRIC_NAMES)}
        return _band_result(stats, count, counts, hist, metrics)
    y_after, r, action, reward, y_before = _protocol_records(env, is_ph, policy, setpoints, steps, plants, agent)
    metrics = metrics_from_records(y_after, r, action, reward, y_before[::steps], seg_len=steps, band=band, tail=tail)
    b = band_from_records(y_after, r, action, reward, group_lanes=group_lanes, hist=hist)
    return _band_result(b["stats"], b["count"], b["hist"], hist, metrics)


def band_quantiles(hist, edges, q):
    """Percentiles of the controlled output from a band's histogram: hist [..., bins] counts, edges [bins + 1], q in [0, 1] (scalar
    or 1-D) -> float64 [..., len(q)], by linear interpolation inside the bin that holds the q-th share of the counts (the counts of
    a bin are taken as spread evenly over it).  The outer bins also hold what fell outside [edges[0], edges[-1]): a quantile
    there is only known to lie beyond the edge.  A histogram without counts gives NaN."""
    h = np.asarray(hist, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    bins = h.shape[-1]
    assert edges.shape == (bins + 1,) and ((q >= 0) & (q <= 1)).all()
    c = np.cumsum(h, axis=-1)
    total = c[..., -1]
    out = np.empty(h.shape[:-1] + (q.size,))
    for j, qj in enumerate(q):
        target = qj * total
        b = np.minimum(((c < target[..., None]) | (c == 0)).sum(axis=-1), bins - 1)   # the first non-empty bin whose cumulative count reaches the target
        before = np.where(b > 0, np.take_along_axis(c, np.maximum(b - 1, 0)[..., None], axis=-1)[..., 0], 0.0)
        inside = np.take_along_axis(h, b[..., None], axis=-1)[..., 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(inside > 0, (target - before) / inside, 0.0)
        out[..., j] = np.where(total > 0, edges[b] + frac * (edges[b + 1] - edges[b]), np.nan)
    return out


# ------------------------------------------------------------------------------------------------ plant identification
def records_from_trace(trace, kind, lanes=None, first=None, y_last=None):
    """Records for `identify_plants` from the trace of a fused evaluation (`rollout_eval(..., want_trace=True)`, float64
    [n_steps, 6, N]): every lane in `lanes` (default: all) becomes one record of its env actions and outputs.  kind: ENV_PH / ENV_WT
    (or "ph" / "wt").  The trace holds the tank's levels AFTER each step and the pH's y BEFORE it, so without more the first step
    (tank) or the first and last step (pH) only supply the starting row; first -- tank: [2, N] the levels (h1, h2) before step 0 --
    and y_last -- pH: [N] the output after the last step -- recover them.  pH records carry state0 (x after step 0, from the trace);
    drop the key to identify with x hidden.  A set-point schedule needs no care: it acts through the recorded action alone."""
    tr = np.asarray(trace.detach().cpu().numpy() if hasattr(trace, "detach") else trace, dtype=np.float64)
    lanes = np.arange(tr.shape[2]) if lanes is None else np.asarray(lanes, dtype=np.int64).reshape(-1)
    if kind in (ENV_PH, "ph"):
        y = tr[1:, 0][:, lanes]                                  # y before steps 1 .. n-1 = after steps 0 .. n-2
        action = tr[1:, 3][:, lanes]
        if y_last is None:
            action = action[:-1]
        else:
            y = np.concatenate([y, np.asarray(y_last, dtype=np.float64).reshape(-1)[lanes][None]])
        return dict(action=np.ascontiguousarray(action.T), output=np.ascontiguousarray(y.T[:, :, None]),
                    state0=np.ascontiguousarray(tr[0, 5][lanes]))
    h = tr[:, 0:2][:, :, lanes]                                  # [n, 2, E]: the levels after each step
    action = tr[:, 5][:, lanes]
    if first is None:
        action = action[1:]
    else:
        h = np.concatenate([np.asarray(first, dtype=np.float64).reshape(2, -1)[:, lanes][None], h])
    return dict(action=np.ascontiguousarray(action.T), output=np.ascontiguousarray(h.transpose(2, 0, 1)))


def records_from_physical(u, y, kind):
    """Records from measured data in physical units.  u [E, T]: the plant input -- the tank's pump signal u = 5 a + 5 (action_P with
    P_max_action 10), the pH's flow u = 0.75 (a + 1) (the action map onto [0, 1.5]) -- converted back to the env action a; y
    [E, T + 1, C] (pH: [E, T + 1] will do) the measured outputs, row 0 before the first input, NaN where a sample is missing."""
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    if kind in (ENV_PH, "ph"):
        action = u / 0.75 - 1.0
        y = y.reshape(u.shape[0], -1, 1)
    else:
        action = (u - 5.0) / 5.0
        y = y.reshape(u.shape[0], -1, 2)
    if y.shape[1] != u.shape[1] + 1:
        raise ValueError(f"records_from_physical: {u.shape[1]} inputs need {u.shape[1] + 1} output rows, got {y.shape[1]}")
    return dict(action=np.ascontiguousarray(action), output=np.ascontiguousarray(y))


def identify_plants(env, records, axes, mode="simulate", skip=0, weights=None):
    """Scores a dense plant grid against recorded runs.  axes: as `robust_grid` (every plant parameter -> 1-D values; env.num_envs =
    the product of their lengths; lane = the C-order index); records: see `VecControlEnv.replay_error`; mode "simulate" (free run
    from the first row) or "predict" (tank: every step from the measured state); skip: burn-in steps that are not counted;
    weights: per output channel the scale its error is divided by (default 1).  The grid is written into the env's lanes and ONE
    `replay_error` launch replays every (plant, record) pair; the env is not stepped.  Returns a dict:
      axes, plants [n, P]           the grid
      cost [*shape]                 sum over records e and channels c of SSE[e, c] / weights[c]^2
      count [*shape]                the number of measurements that entered it (gaps and the burn-in do not)
      rmse [*shape]                 sqrt(cost / count)
      max_error [C, *shape]         per channel the largest |simulated - measured| over all records (unweighted)
      best_index, best              the C-order lane of the smallest cost and its plant as an OrderedDict name -> value"""
    names, axes, shape, plants = _grid(env, axes, "identify_plants")
    if env.kind == ENV_PH:
        env.set_params(plants[:, 0], plants[:, 1])
    else:
        env.reset_changable_parameters(plants[:, 0], plants[:, 1], plants[:, 2])
    err, _ = env.replay_error(records, mode=mode, skip=skip)
    err = err.cpu().numpy()
    row = {name: j for j, name in enumerate(REPLAY_ROW_NAMES)}
    n_ch = 1 if env.kind == ENV_PH else 2
    w = np.ones(n_ch) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (n_ch,) or not (w > 0).all():
        raise ValueError(f"identify_plants: weights must be {n_ch} positive numbers")
    cost = sum(err[:, row[f"sse{c}"]].sum(axis=0) / w[c] ** 2 for c in range(n_ch))
    count = err[:, row["count"]].sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rmse = np.sqrt(cost / count)
    best = int(np.nanargmin(cost))
    return dict(axes=axes, plants=plants, cost=cost.reshape(shape), count=count.reshape(shape), rmse=rmse.reshape(shape),
                max_error=np.stack([err[:, row[f"max{c}"]].max(axis=0).reshape(shape) for c in range(n_ch)]),
                best_index=best, best=OrderedDict((k, float(plants[best, j])) for j, k in enumerate(names)))


def ensemble_ranges(result, factor=2.0):
    """The bounding box, per axis, of the plants of an `identify_plants` result whose rmse is <= factor x the best rmse: the
    ensemble the records find plausible -- OrderedDict axis name -> (low, high).  The training ranges should contain it."""
    rmse = np.asarray(result["rmse"], dtype=np.float64)
    keep = np.argwhere(rmse <= factor * np.nanmin(rmse))
    return OrderedDict((k, (float(v[keep[:, j]].min()), float(v[keep[:, j]].max()))) for j, (k, v) in enumerate(result["axes"].items()))


# ------------------------------------------------------------------------------------------------ prior-gain sweep
def gain_box(K, factors):
    """The Cartesian grid [G, D] of K[j] * factors[j][...] in C order (the last component varies fastest).  K: a gain [D], in either
    sign -- the grid keeps it: pass -env.K for `tune_prior`.  factors: one list of numbers, applied to every NON-ZERO component of K
    (a zero component stays zero and adds no axis), or D lists, one per component."""
    K = np.asarray(K, dtype=np.float64).reshape(-1)
    scalar = len(factors) > 0 and all(np.ndim(f) == 0 for f in factors)
    if scalar:
        f = np.asarray(factors, dtype=np.float64).reshape(-1)
        per = [f if k != 0.0 else np.ones(1) for k in K]
    else:
        per = [np.asarray(f, dtype=np.float64).reshape(-1) for f in factors]
    if len(per) != K.size or any(f.size < 1 for f in per):
        raise ValueError(f"gain_box: factors must be one non-empty list of numbers or {K.size} non-empty lists")
    mesh = np.meshgrid(*[K[j] * per[j] for j in range(K.size)], indexing="ij")
    return np.ascontiguousarray(np.stack([m.reshape(-1) for m in mesh], axis=1))


def tune_prior(env, gains, axes=None, plants=None, setpoints=None, steps=None, band=None, tail=10, cost="itae", robust="worst"):
    """Robust tuning of the prior controller: the step-response protocol of `env` (as `step_response_metrics`) under a_env = obs @
    gains[g] for every gain row, over the plants in the env's lanes, in ONE sweep (`VecControlEnv.prior_sweep`).  gains float64
    [G, D] in the KERNELS' sign (priorK = -env.K; `gain_box(-env.K, factors)`).  axes: a plant grid as `robust_grid` takes it, or
    plants [N, P]: written into the lanes; neither: every lane keeps the plant its reset draws.  cost: a name of `METRIC_NAMES`;
    robust "worst": the cost of a gain is the sum over segments of the row's MAXIMUM over the plants, "mean": of its mean over
    the plants.  A gain with a non-finite value on any plant, segment or row costs +inf.  Returns a dict:
      gains [G, D], summary [G, n_segments, 8, 5] (stats `SWEEP_STATS`), cost [G]
      worst_plant int64 [G, n_segments]   the lane with the largest value of the cost row
      settled_all bool [G]                every plant is inside `band` at the end of every segment
      best_index, best_gain               the first gain of the smallest cost, in the kernels' sign"""
    if cost not in METRIC_NAMES or robust not in ("worst", "mean"):
        raise ValueError(f"tune_prior: cost {cost!r} must be one of {METRIC_NAMES} and robust {robust!r} 'worst' or 'mean'")
    is_ph = env.kind == ENV_PH
    if axes is not None:
        plants = _grid(env, axes, "tune_prior")[3]
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    gains = np.ascontiguousarray(np.asarray(gains, dtype=np.float64).reshape(-1, env.obs_dim))
    _protocol_start(env, is_ph, steps, plants)
    summary = env.prior_sweep(gains, len(setpoints) * steps, setpoints=setpoints, seg_len=steps, band=band, tail=tail).cpu().numpy()
    st = {name: j for j, name in enumerate(SWEEP_STATS)}
    row = METRIC_NAMES.index(cost)
    if robust == "worst":
        c = summary[:, :, row, st["max"]].sum(axis=1)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (summary[:, :, row, st["sum"]] / summary[:, :, row, st["finite"]]).sum(axis=1)
    whole = (summary[:, :, :, st["finite"]] == env.num_envs).all(axis=(1, 2))
    c = np.where(whole, c, np.inf)
    settled = whole & (summary[:, :, METRIC_NAMES.index("settling_step"), st["max"]] < steps).all(axis=1)
    best = int(np.argmin(c))
    return dict(gains=gains, summary=summary, cost=c, worst_plant=summary[:, :, row, st["argmax"]].astype(np.int64), settled_all=settled,
                best_index=best, best_gain=gains[best].copy())


# ------------------------------------------------------------------------------------------------ policy sweep
def policy_sweep(env, policies, axes=None, plants=None, setpoints=None, steps=None, band=None, tail=10, want_pairs=False):
    """Which of these controllers is best on its worst plant?  The step-response protocol of `env` (as `step_response_metrics`: the
    same start, set-points, steps, band and tail) under every row of `policies` (an `ops.PackedPolicies` stack: P packed actors of
    one class, each with its own prior gain), over the plants in the env's lanes, in ONE call (`VecControlEnv.policy_sweep`).  axes:
    a plant grid as `robust_grid` takes it, or plants [N, P]: written into the lanes; neither: every lane keeps the plant its reset
    draws.  Returns a dict for `select_policy`: summary [P, n_segments, 8, 5] (stats `SWEEP_STATS`), settled int64 [P] (the plants
    of a row that are finite in every metric row and inside `band` at the end of every segment; counted on the device), pairs
    [n_segments, 8, P, N] or None, steps, setpoints, band, tail, n (the plants)."""
    is_ph = env.kind == ENV_PH
    if axes is not None:
        plants = _grid(env, axes, "policy_sweep")[3]
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    if not hasattr(env, "policy_supported") or not env.policy_supported(policies):
        raise ValueError("policy_sweep: the policy sweep does not serve this env / stack of actors (VecControlEnv.policy_supported)")
    _protocol_start(env, is_ph, steps, plants)
    out = env.policy_sweep(policies, len(setpoints) * steps, setpoints=setpoints, seg_len=steps, band=band, tail=tail, want_pairs=True)
    pairs = out["pairs"]
    fit = torch.isfinite(pairs).all(dim=1) & (pairs[:, METRIC_NAMES.index("settling_step")] < steps)    # [S, P, N]
    settled = fit.all(dim=0).sum(dim=1).cpu().numpy().astype(np.int64)
    return dict(summary=out["summary"].cpu().numpy(), settled=settled, pairs=pairs.cpu().numpy() if want_pairs else None, steps=int(steps),
                setpoints=setpoints, band=band, tail=tail, n=int(env.num_envs))


def select_policy(result, cost="itae", robust="worst"):
    """The row of a `policy_sweep` result to deploy, in the vocabulary of `tune_prior`.  cost: a name of `METRIC_NAMES`; robust
    "worst": a policy costs the sum over segments of the row's MAXIMUM over the plants, "mean": of its mean over the plants.  A
    policy is FIT when every plant is finite in every segment and metric row and settles in every segment (result["settled"] ==
    result["n"]); an unfit policy ranks behind every fit one, whatever its cost, and among policies of one kind the smaller cost
    wins, a non-finite cost counting as +inf; ties go to the lowest row.  Returns a dict:
      best_index                     the chosen row
      nominal_index                  the row the same rule chooses with the plant-MEAN cost: what a nominal ranking would deploy
      cost [P]                       the cost the choice ranked (worst_cost or mean_cost)
      mean_cost, worst_cost [P]      both costs of every policy
      worst_plant int64 [P, n_segments]   the lane with the largest value of the cost row
      settled int64 [P], fit bool [P]
      order int64 [P]                every row, best first"""
    if cost not in METRIC_NAMES or robust not in ("worst", "mean"):
        raise ValueError(f"select_policy: cost {cost!r} must be one of {METRIC_NAMES} and robust {robust!r} 'worst' or 'mean'")
    summary = np.asarray(result["summary"], dtype=np.float64)
    n, settled = int(result["n"]), np.asarray(result["settled"], dtype=np.int64).reshape(-1)
    st = {name: j for j, name in enumerate(SWEEP_STATS)}
    row = METRIC_NAMES.index(cost)
    worst = summary[:, :, row, st["max"]].sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (summary[:, :, row, st["sum"]] / summary[:, :, row, st["finite"]]).sum(axis=1)
    fit = (summary[:, :, :, st["finite"]] == n).all(axis=(1, 2)) & (settled == n)

    def rank(c):
        c = np.where(np.isfinite(c), c, np.inf)
        return np.lexsort((np.arange(len(c)), c, ~fit))     # unfit last, then the cost, then the row
    order = rank(worst if robust == "worst" else mean)
    return dict(best_index=int(order[0]), nominal_index=int(rank(mean)[0]), cost=(worst if robust == "worst" else mean).copy(),
                mean_cost=mean, worst_cost=worst, worst_plant=summary[:, :, row, st["argmax"]].astype(np.int64), settled=settled, fit=fit,
                order=order.astype(np.int64))


# ------------------------------------------------------------------------------------------------ receding-horizon baseline
def mpc_baseline(env, plants=None, setpoints=None, steps=None, horizon=20, passes=2, rho=0.0, model=None, band=None, tail=10, trace=False):
    """How good could ANY controller be on each plant?  The step-response protocol of `env` (as `step_response_metrics`: the same
    start, set-points, steps, band and tail) under a non-linear receding-horizon controller on the plant's own model
    (`VecControlEnv.mpc_eval`: 64 constant-action candidates per pass over `horizon` noise-free steps, cost sum (y - r)^2 +
    rho (u - u_prev)^2), every plant in ONE launch.  plants [N, P]: written into the lanes; None: every lane keeps the plant its
    reset draws.  model (tank only): None -- every plant is controlled on its own model --, one plant row (a1, a2, Kp) broadcast to
    all lanes, or [N, 3]: certainty-equivalent control on, e.g., the best plant of `identify_plants`.  Returns the dict of
    `step_response_metrics` (metric name -> float64 [len(setpoints), N]) and, with `trace`, "actions" / "outputs" [T, N]."""
    is_ph = env.kind == ENV_PH
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    if model is not None:
        model = np.asarray(model, dtype=np.float64)
        if model.shape == (3,):
            model = np.broadcast_to(model, (env.num_envs, 3))
        model = np.ascontiguousarray(model)
    _protocol_start(env, is_ph, steps, plants)
    out = env.mpc_eval(horizon, passes=passes, rho=rho, model_plants=model, n_steps=len(setpoints) * steps, seg_len=steps,
                       setpoints=setpoints, band=band, tail=tail, trace=trace)
    m = (out[0] if trace else out).cpu().numpy()
    res = {name: np.ascontiguousarray(m[:, j]) for j, name in enumerate(METRIC_NAMES)}
    if trace:
        res["actions"], res["outputs"] = out[1].cpu().numpy(), out[2].cpu().numpy()
    return res


def regret(metrics, baseline, name="itae"):
    """A controller's metric against a baseline's (`mpc_baseline`) on the same plants and segments: (difference, ratio) =
    (metrics[name] - baseline[name], metrics[name] / baseline[name]), element-wise; the ratio is NaN where the baseline is 0."""
    a, b = np.asarray(metrics[name], dtype=np.float64), np.asarray(baseline[name], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b == 0.0, np.nan, a / b)
    return a - b, ratio


# ------------------------------------------------------------------------------------------------ loop margins
def perturbation_grid(gains=(1.,), delays=(0,), sigmas=(0.,)):
    """The rows of `loop_sweep` / `VecControlEnv.margin_sweep` for every combination of loop gains, dead times (sample periods) and
    sensor-noise scales: float64 [P, 3], columns (gain, delay, sigma), in C order -- the gain outermost, sigma innermost."""
    g, d, s = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (gains, delays, sigmas))
    if g.size < 1 or d.size < 1 or s.size < 1:
        raise ValueError("perturbation_grid: every axis needs at least one value")
    mesh = np.meshgrid(g, d, s, indexing="ij")
    return np.ascontiguousarray(np.stack([m.reshape(-1) for m in mesh], axis=1))


def loop_sweep(env, perturb, agent=None, axes=None, plants=None, setpoints=None, steps=None, band=None, tail=10, seed=0, want_pairs=False):
    """How much dead time, loop-gain error and sensor noise does the closed loop tolerate?  The step-response protocol of `env` (as
    `step_response_metrics`: the same start, set-points, steps, band and tail) under every row (gain, delay, sigma) of `perturb`
    [P, 3] (`perturbation_grid`), over the plants in the env's lanes, in ONE call (`VecControlEnv.margin_sweep`): the plant receives
    gain x the controller's output of `delay` steps ago, the controller reads the plant outputs plus sigma x a standard normal keyed
    on the lane (every row meets the same noise sequence; `seed` keys it).  agent None: the prior controller alone, else an agent the
    fused evaluation serves.  axes: a plant grid as `robust_grid` takes it, or plants [N, P]: written into the lanes; neither: every
    lane keeps the plant its reset draws.  Returns a dict for `loop_margins`: perturb [P, 3], summary [P, n_segments, 8, 5] (stats
    `SWEEP_STATS`), pairs [n_segments, 8, P, N] or None, steps, setpoints, band, tail, n (the plants)."""
    from .vec_env import check_perturb
    is_ph = env.kind == ENV_PH
    rows = check_perturb(perturb)
    if axes is not None:
        plants = _grid(env, axes, "loop_sweep")[3]
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    fused = _fused_policy(env, None, agent)
    if fused is None or not hasattr(env, "margin_supported") or not env.margin_supported(fused[0]):
        raise ValueError("loop_sweep: the loop-perturbation sweep does not serve this env / agent (VecControlEnv.margin_supported)")
    _protocol_start(env, is_ph, steps, plants)
    out = env.margin_sweep(fused[0], fused[1], rows, len(setpoints) * steps, setpoints=setpoints, seg_len=steps, band=band, tail=tail,
                           noise_seed=seed, want_pairs=want_pairs)
    summary, pairs = (out["summary"], out["pairs"]) if want_pairs else (out, None)
    return dict(perturb=rows, summary=summary.cpu().numpy(), pairs=None if pairs is None else pairs.cpu().numpy(), steps=int(steps),
                setpoints=setpoints, band=band, tail=tail, n=int(env.num_envs))


def _last_ok(values, ok):
    """values ascending away from the nominal one (first): the last value before the first failure; NaN if the nominal row fails."""
    last = np.nan
    for v, good in zip(values, ok):
        if not good:
            break
        last = v
    return float(last)


def loop_margins(result, cost="itae", factor=2.0):
    """Margins from a `loop_sweep` result.  A row is ACCEPTABLE when every plant settles in every segment (the settling step's
    maximum < the segment's length, every value finite) and the worst-plant `cost` (a name of `METRIC_NAMES`; summed over the
    segments) stays <= factor x its value on the nominal row (1, 0, 0), which the grid must hold.  Along each perturbation axis, the
    other two columns nominal, the margin is the LAST value, walking away from the nominal one, up to which every row is acceptable
    (NaN: the nominal row itself is not).  Returns a dict: nominal (row index), acceptable bool [P], cost [P], delay_margin,
    gain_margin (upwards from 1), gain_margin_low (downwards), sigma_margin, sigma_slope (the least-squares slope of the plant-mean
    action variation, summed over the segments, against sigma; NaN with fewer than two sigma rows) and, when the result holds
    `pairs`, the same per plant: plant_delay_margin, plant_gain_margin, plant_gain_margin_low, plant_sigma_margin, each [N]."""
    if cost not in METRIC_NAMES:
        raise ValueError(f"loop_margins: cost {cost!r} must be one of {METRIC_NAMES}")
    rows, summary = np.asarray(result["perturb"], dtype=np.float64), np.asarray(result["summary"], dtype=np.float64)
    P, S = summary.shape[0], summary.shape[1]
    N, steps = int(result["n"]), int(result["steps"])
    g, d, sg = rows[:, 0], rows[:, 1], rows[:, 2]
    nominal = np.flatnonzero((g == 1.0) & (d == 0.0) & (sg == 0.0))
    if nominal.size < 1:
        raise ValueError("loop_margins: the grid holds no nominal row (gain 1, delay 0, sigma 0)")
    nom = int(nominal[0])
    st = {name: j for j, name in enumerate(SWEEP_STATS)}
    row, settle, av = METRIC_NAMES.index(cost), METRIC_NAMES.index("settling_step"), METRIC_NAMES.index("action_variation")
    seg_steps = np.full(S, steps, dtype=np.float64)   # (loop_sweep runs whole segments)
    whole = (summary[:, :, :, st["finite"]] == N).all(axis=(1, 2))
    settled = (summary[:, :, settle, st["max"]] < seg_steps[None, :]).all(axis=1)
    c = summary[:, :, row, st["max"]].sum(axis=1)
    with np.errstate(invalid="ignore"):
        ok = whole & settled & (c <= factor * c[nom])
    axes = {"delay": ((g == 1.0) & (sg == 0.0), d, +1), "gain": ((d == 0.0) & (sg == 0.0) & (g >= 1.0), g, +1),
            "gain_low": ((d == 0.0) & (sg == 0.0) & (g <= 1.0), g, -1), "sigma": ((g == 1.0) & (d == 0.0), sg, +1)}
    out = dict(nominal=nom, acceptable=ok, cost=c)
    order = {}
    for name, (mask, vals, sign) in axes.items():
        idx = np.flatnonzero(mask)
        idx = idx[np.argsort(sign * vals[idx], kind="stable")]
        order[name] = idx
        out[name + "_margin" if name != "gain_low" else "gain_margin_low"] = _last_ok(vals[idx], ok[idx])
    idx = order["sigma"]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_av = (summary[:, :, av, st["sum"]] / summary[:, :, av, st["finite"]]).sum(axis=1)
    fit = np.isfinite(mean_av[idx])
    out["sigma_slope"] = float(np.polyfit(sg[idx][fit], mean_av[idx][fit], 1)[0]) if np.unique(sg[idx][fit]).size >= 2 else float("nan")
    pairs = result.get("pairs")
    if pairs is not None:
        pairs = np.asarray(pairs, dtype=np.float64)                      # [S, 8, P, N]
        finite = np.isfinite(pairs).all(axis=(0, 1))                     # [P, N]
        settled_p = (pairs[:, settle] < seg_steps[:, None, None]).all(axis=0)
        cp = pairs[:, row].sum(axis=0)
        with np.errstate(invalid="ignore"):
            ok_p = finite & settled_p & (cp <= factor * cp[nom][None, :])
        for name, (mask, vals, sign) in axes.items():
            idx = order[name]
            key = "plant_" + (name + "_margin" if name != "gain_low" else "gain_margin_low")
            out[key] = np.array([_last_ok(vals[idx], ok_p[idx, i]) for i in range(ok_p.shape[1])])
    return out


# ------------------------------------------------------------------------------------------------ disturbance rejection
def disturbance_grid(onset, loads=(), m0=(), m1=(), m2=(), length=0):
    """The rows of `disturbance_rejection` / `VecControlEnv.disturbance_sweep`: the nominal row (onset, length, 0, 1, 1, 1) first, then
    one row per value, one axis at a time -- the loads, then the multipliers of the first, second and third plant parameter (pH:
    qww_V, qc_V; tank: a1, a2, Kp) -- every other column nominal.  float64 [P, 6], columns native.DISTURB_COL_NAMES."""
    rows = [[onset, length, 0.0, 1.0, 1.0, 1.0]]
    for col, values in ((2, loads), (3, m0), (4, m1), (5, m2)):
        for v in np.asarray(values, dtype=np.float64).reshape(-1):
            row = [onset, length, 0.0, 1.0, 1.0, 1.0]
            row[col] = float(v)
            rows.append(row)
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64))


def disturbance_rejection(env, rows, agent=None, axes=None, plants=None, setpoints=None, steps=None, band=None, tail=10, want_pairs=False):
    """How well does the closed loop reject a load at the plant input or a step of the plant's parameters?  The step-response
    protocol of `env` (as `step_response_metrics`: the same start, set-points, steps, band and tail) under every row (onset, length,
    load, m0, m1, m2) of `rows` [P, 6] (`disturbance_grid`), over the plants in the env's lanes, in ONE call
    (`VecControlEnv.disturbance_sweep`): the disturbance comes back at step `onset` of every set-point segment.  agent None: the prior
    controller alone, else an agent the fused evaluation serves.  axes: a plant grid as `robust_grid` takes it, or plants [N, P]:
    written into the lanes; neither: every lane keeps the plant its reset draws.  Returns a dict for `rejection_summary`: rows
    [P, 6], summary [P, n_segments, 15, 5] (rows `METRIC_NAMES` then `DISTURB_ROW_NAMES`, stats `SWEEP_STATS`), pairs
    [n_segments, 15, P, N] and actions, outputs [T, P, N], or None, steps, setpoints, band, tail, n (the plants)."""
    from .vec_env import check_disturb
    is_ph = env.kind == ENV_PH
    rows = check_disturb(rows, is_ph)
    if axes is not None:
        plants = _grid(env, axes, "disturbance_rejection")[3]
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    fused = _fused_policy(env, None, agent)
    if fused is None or not hasattr(env, "disturbance_supported") or not env.disturbance_supported(fused[0]):
        raise ValueError("disturbance_rejection: the disturbance sweep does not serve this env / agent (VecControlEnv.disturbance_supported)")
    _protocol_start(env, is_ph, steps, plants)
    out = env.disturbance_sweep(fused[0], fused[1], rows, len(setpoints) * steps, setpoints=setpoints, seg_len=steps, band=band,
                                tail=tail, want_pairs=want_pairs, want_trace=want_pairs)
    host = lambda v: None if v is None else v.cpu().numpy()
    summary, pairs, actions, outputs = (out["summary"], out["pairs"], out["actions"], out["outputs"]) if want_pairs else (out, None, None, None)
    return dict(rows=rows, summary=host(summary), pairs=host(pairs), actions=host(actions), outputs=host(outputs), steps=int(steps),
                setpoints=setpoints, band=band, tail=tail, n=int(env.num_envs))


def rejection_summary(result):
    """A `disturbance_rejection` result per row, over the plants and the segments the row starts in: dict of float64 [P] --
      worst_peak, worst_recovery, worst_iae   the worst plant's peak error, recovery step and IAE from the onset (the largest over the
                                              segments);
      recovered                               the share of (plant, segment) pairs whose recovery step is smaller than the window's length
                                              (needs `pairs`; without them 1.0 / 0.0 from the worst plant per segment);
      worst_e0                                the largest |error| a disturbance met at its onset: had the loop settled?
    NaN where the row starts in no segment."""
    summary = np.asarray(result["summary"], dtype=np.float64)
    rows, steps = np.asarray(result["rows"], dtype=np.float64), int(result["steps"])
    st = {name: j for j, name in enumerate(SWEEP_STATS)}
    at = {name: len(METRIC_NAMES) + j for j, name in enumerate(DISTURB_ROW_NAMES)}
    P = summary.shape[0]
    window = np.maximum(steps - rows[:, 0], 0.0)                                  # [P] (disturbance_rejection runs whole segments)
    seen = summary[:, :, at["peak"], st["finite"]] > 0                            # [P, S]
    worst = lambda name: np.where(seen.any(axis=1), np.where(seen, summary[:, :, at[name], st["max"]], -np.inf).max(axis=1), np.nan)
    e0 = np.maximum(np.abs(summary[:, :, at["e0"], st["min"]]), np.abs(summary[:, :, at["e0"], st["max"]]))
    out = dict(worst_peak=worst("peak"), worst_recovery=worst("recovery"), worst_iae=worst("iae"),
               worst_e0=np.where(seen.any(axis=1), np.where(seen, e0, -np.inf).max(axis=1), np.nan))
    pairs = result.get("pairs")
    if pairs is not None:
        rec = np.asarray(pairs, dtype=np.float64)[:, at["recovery"]]              # [S, P, N]
        counted = np.isfinite(rec)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["recovered"] = (counted & (rec < window[None, :, None])).sum(axis=(0, 2)) / counted.sum(axis=(0, 2))
    else:
        ok = np.where(seen, summary[:, :, at["recovery"], st["max"]] < window[:, None], False)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["recovered"] = np.where(seen.any(axis=1), ok.sum(axis=1) / seen.sum(axis=1), np.nan)
    assert all(v.shape == (P,) for v in out.values())
    return out


# ------------------------------------------------------------------------------------------------ actuator and sensor limits
ACT_OFF = (-np.inf, np.inf, np.inf, 0.0, 0.0, 0.0)      # a row with every stage off (columns native.ACT_COL_NAMES)
# the reference rig (gym_control/envs/real_watertank.py): a 0 .. 10 V pump, a DAC byte (256 levels), an ADC at 10 / 504 V per count
RIG_VOLTS, RIG_DAC_LEVELS, RIG_ADC_COUNTS = 10.0, 256, 504


def actuator_grid(limits=(), rates=(), deadbands=(), qu=(), qy=()):
    """The rows of `actuator_sweep` / `VecControlEnv.actuator_sweep`: the PRODUCT of the five axes, each axis led by its "off" value
    -- limits: (lo, hi) pairs; rates, deadbands, qu, qy: scalars -- with `limits` the slowest and `qy` the fastest index, so row 0 is
    always the all-off row `ACT_OFF`.  float64 [P, 6], P = the product of (1 + len(axis)), columns native.ACT_COL_NAMES."""
    lim = [ACT_OFF[:2]] + [tuple(float(x) for x in v) for v in np.asarray(limits, dtype=np.float64).reshape(-1, 2)]
    ax = [[off] + [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)] for off, v in zip(ACT_OFF[2:], (rates, deadbands, qu, qy))]
    rows = [[l[0], l[1], r, d, a, y] for l in lim for r in ax[0] for d in ax[1] for a in ax[2] for y in ax[3]]
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64))


def rig_row(p_max_action=10.0):
    """ONE row for the reference rig.  A command a in [-1, 1] becomes a * P_max / 2 + P_max / 2 volts, clipped to 0 .. 10 V and
    floored onto 256 DAC levels; the levels come back through a 10-bit ADC at 10 / 504 V per count.  In normalised action units:
    0 V is a = -1, 10 V is a = 20 / P_max - 1; one DAC level is (10 / 256) V = (10 / 256) / (P_max / 2) = 20 / (256 P_max).  The rig's
    observation IS the ADC's volt reading (no level calibration in between) and a policy moves over reading those numbers where it
    read the simulated levels, so one count is 10 / 504 observation units.  No rate limit, no dead-band.  float64 [6]."""
    p = float(p_max_action)
    if not (np.isfinite(p) and p > 0):
        raise ValueError("rig_row: p_max_action must be finite and > 0")
    return np.array([-1.0, 2.0 * RIG_VOLTS / p - 1.0, np.inf, 0.0, 2.0 * RIG_VOLTS / (RIG_DAC_LEVELS * p), RIG_VOLTS / RIG_ADC_COUNTS],
                    dtype=np.float64)


def actuator_sweep(env, rows, agent=None, axes=None, plants=None, setpoints=None, steps=None, band=None, tail=10, want_pairs=False):
    """What do a real actuator and a real sensor do to the closed loop?  The step-response protocol of `env` (as
    `disturbance_rejection`: the same start, set-points, steps, band and tail) under every row (lo, hi, rate, deadband, qu, qy) of
    `rows` [P, 6] (`actuator_grid`, `rig_row`), over the plants in the env's lanes, in ONE call (`VecControlEnv.actuator_sweep`).
    agent None: the prior controller alone, else an agent the fused evaluation serves.  axes / plants: as `disturbance_rejection`.
    Returns a dict for `actuator_summary`: rows [P, 6], summary [P, n_segments, 16, 5] (rows `METRIC_NAMES` then `ACT_ROW_NAMES`,
    stats `SWEEP_STATS`), pairs [n_segments, 16, P, N] and actions, commands, outputs [T, P, N], or None, steps, setpoints, band,
    tail, n (the plants)."""
    from .vec_env import check_actuator
    is_ph = env.kind == ENV_PH
    rows = check_actuator(rows)
    if axes is not None:
        plants = _grid(env, axes, "actuator_sweep")[3]
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    band = 0.05 if band is None else band
    fused = _fused_policy(env, None, agent)
    if fused is None or not hasattr(env, "actuator_supported") or not env.actuator_supported(fused[0]):
        raise ValueError("actuator_sweep: the actuator sweep does not serve this env / agent (VecControlEnv.actuator_supported)")
    _protocol_start(env, is_ph, steps, plants)
    out = env.actuator_sweep(fused[0], fused[1], rows, len(setpoints) * steps, setpoints=setpoints, seg_len=steps, band=band, tail=tail,
                             want_pairs=want_pairs, want_trace=want_pairs)
    host = lambda v: None if v is None else v.cpu().numpy()
    got = out if want_pairs else {"summary": out}
    return dict(rows=rows, summary=host(got["summary"]), pairs=host(got.get("pairs")), actions=host(got.get("actions")),
                commands=host(got.get("commands")), outputs=host(got.get("outputs")), steps=int(steps), setpoints=setpoints, band=band,
                tail=tail, n=int(env.num_envs))


def _act_axis_rows(rows):
    """axis name -> (row indices, a value per row ascending in harshness) of the rows with exactly that axis on."""
    rows = np.asarray(rows, dtype=np.float64)
    on = np.stack([np.isfinite(rows[:, 0]) | np.isfinite(rows[:, 1]), (rows[:, 2] > 0) & np.isfinite(rows[:, 2]), rows[:, 3] > 0,
                   rows[:, 4] > 0, rows[:, 5] > 0], axis=1)
    # harshness: a narrower span, a smaller rate, a wider dead-band, a coarser quantum
    value = np.stack([rows[:, 1] - rows[:, 0], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]], axis=1)
    out = {}
    for j, (name, sign) in enumerate((("limits", -1.0), ("rate", -1.0), ("deadband", 1.0), ("qu", 1.0), ("qy", 1.0))):
        idx = np.flatnonzero(on[:, j] & (on.sum(axis=1) == 1))
        idx = idx[np.argsort(sign * value[idx, j], kind="stable")]
        out[name] = (idx, value[idx, j])
    return out


def actuator_summary(result):
    """An `actuator_sweep` result.  Per row, dict of float64 [P] --
      itae_ratio    the worst plant's ITAE (the largest over the segments) over that of row 0, which must be the all-off row;
      limit_cycle   the share of (plant, segment) pairs whose TAIL_Y_P2P exceeds the band: the output still swings at the segment's end
                    (needs `pairs`; without them the share of segments whose worst plant does);
      reversals     the median REVERSALS over the (plant, segment) pairs (needs `pairs`; NaN without them);
    and per axis -- "limits" (the span hi - lo), "rate", "deadband", "qu", "qy" -- over the rows that have this axis alone on,
    walking from the mildest value (the widest span, the largest rate, the smallest dead-band or quantum) to the harshest: the LAST
    value up to which no plant limit-cycles, i.e. the tightest limit / the largest quantum the loop tolerates (key `<axis>_tolerated`;
    NaN: the mildest value already cycles, or the grid has no such row)."""
    summary = np.asarray(result["summary"], dtype=np.float64)
    rows, band = np.asarray(result["rows"], dtype=np.float64), float(result["band"])
    if np.isfinite(rows[0, :2]).any() or (rows[0, 2] > 0 and np.isfinite(rows[0, 2])) or (rows[0, 3:] > 0).any():
        raise ValueError("actuator_summary: row 0 must be the all-off row (actuator_grid puts it there)")
    st = {name: j for j, name in enumerate(SWEEP_STATS)}
    at = {name: len(METRIC_NAMES) + j for j, name in enumerate(ACT_ROW_NAMES)}
    itae = summary[:, :, METRIC_NAMES.index("itae"), st["max"]].max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(itae_ratio=itae / itae[0])
    pairs = result.get("pairs")
    if pairs is not None:
        pairs = np.asarray(pairs, dtype=np.float64)
        out["limit_cycle"] = (pairs[:, at["tail_y_p2p"]] > band).mean(axis=(0, 2))
        out["reversals"] = np.median(pairs[:, at["reversals"]], axis=(0, 2))
    else:
        out["limit_cycle"] = (summary[:, :, at["tail_y_p2p"], st["max"]] > band).mean(axis=1)
        out["reversals"] = np.full(len(rows), np.nan)
    for name, (idx, vals) in _act_axis_rows(rows).items():
        out[name + "_tolerated"] = _last_ok(vals, out["limit_cycle"][idx] == 0.0) if len(idx) else float("nan")
    return out


# ------------------------------------------------------------------------------------------------ frequency response
def excitation_grid(cycles, amplitude, point, seg_len, onset):
    """The rows and the table of `frequency_sweep` / `VecControlEnv.frequency_sweep`: one row per entry of `cycles`, `amplitude`,
    `point` and `onset` (a scalar serves every row; point: 0 / 1 / 2 or a name of native.FREQ_POINTS).  Row p holds an INTEGER
    number m = cycles[p] of cycles in its correlation window of W = seg_len - onset steps, so that c and s are orthogonal over it and to a
    constant: c_k = cos(2 pi m (k - onset) / W), s_k = sin(2 pi m (k - onset) / W) for every k of the segment (the steps before the
    onset run the same sinusoid: the loop is in its periodic state when the window opens).  m = W / 2 is the Nyquist rate, where s
    vanishes and nothing is excited.  Returns (rows float64 [P, 3], wave float64 [P, seg_len, 2]).  ValueError: a point that is not
    served, a value that is not finite, an onset that is not an integer in 0 .. seg_len - 1, cycles that are not an integer in
    0 .. W / 2."""
    L = int(seg_len)
    pts = [FREQ_POINTS.get(v, np.nan) if isinstance(v, str) else v for v in np.atleast_1d(np.asarray(point, dtype=object)).reshape(-1)]
    try:
        m, amp, pt, k0 = (np.array(a, dtype=np.float64) for a in np.broadcast_arrays(
            *(np.atleast_1d(np.asarray(v, dtype=np.float64)).reshape(-1) for v in (cycles, amplitude, pts, onset))))
    except (TypeError, ValueError):
        raise ValueError("excitation_grid: cycles, amplitude, point and onset must be scalars or of one length") from None
    P = m.size
    if P < 1 or L < 1:
        raise ValueError("excitation_grid: no cycles or seg_len < 1")
    if not np.all(np.isin(pt, tuple(float(v) for v in FREQ_POINTS.values()))):
        raise ValueError(f"excitation_grid: point must be one of {FREQ_POINTS}")
    if not (np.all(np.isfinite(m)) and np.all(np.isfinite(amp)) and np.all(np.isfinite(k0))):
        raise ValueError("excitation_grid: cycles, amplitude and onset must be finite")
    if np.any(k0 != np.rint(k0)) or np.any(k0 < 0) or np.any(k0 >= L):
        raise ValueError(f"excitation_grid: onset must be an integer in 0 .. seg_len - 1 = {L - 1}")
    W = L - k0
    if np.any(m != np.rint(m)) or np.any(m < 0) or np.any(m > W / 2):
        raise ValueError("excitation_grid: cycles must be an integer in 0 .. (seg_len - onset) / 2")
    k = np.arange(L, dtype=np.float64)[None, :]
    theta = 2.0 * np.pi * m[:, None] * (k - k0[:, None]) / W[:, None]
    wave = np.stack([np.cos(theta), np.sin(theta)], axis=-1)
    rows = np.column_stack([pt, amp, k0])
    return np.ascontiguousarray(rows, dtype=np.float64), np.ascontiguousarray(wave, dtype=np.float64)


def frequency_sweep(env, rows, wave, agent=None, axes=None, plants=None, setpoints=None, steps=None, band=None, tail=10, want_trace=False):
    """The step-response protocol of `env` (as `step_response_metrics`: the same start, set-points, steps, band and tail) under every
    excitation row of `rows` [P, 3] with its table `wave` [P, steps, 2] (`excitation_grid` with seg_len = steps), over the plants in
    the env's lanes, in ONE call (`VecControlEnv.frequency_sweep`): the excitation restarts with every set-point segment.  agent None:
    the prior controller alone, else an agent the fused evaluation serves.  axes / plants: as `disturbance_rejection`.  Returns a dict
    for `frequency_response`: rows, wave, summary [P, n_segments, 16, 5], pairs [n_segments, 16, P, N] (rows `METRIC_NAMES` then
    `FREQ_ROW_NAMES`), actions and outputs [T, P, N] or None, n_steps, seg_len, steps, setpoints, band, tail, n (the plants)."""
    from .vec_env import check_excite
    is_ph = env.kind == ENV_PH
    setpoints = tuple(setpoints if setpoints is not None else (PH_SETPOINTS if is_ph else WT_SETPOINTS))
    steps = steps or (50 if is_ph else env.max_step)
    rows, wave = check_excite(rows, wave, steps)
    if axes is not None:
        plants = _grid(env, axes, "frequency_sweep")[3]
    band = 0.05 if band is None else band
    fused = _fused_policy(env, None, agent)
    if fused is None or not hasattr(env, "frequency_supported") or not env.frequency_supported(fused[0]):
        raise ValueError("frequency_sweep: the frequency-response sweep does not serve this env / agent (VecControlEnv.frequency_supported)")
    _protocol_start(env, is_ph, steps, plants)
    out = env.frequency_sweep(fused[0], fused[1], rows, wave, len(setpoints) * steps, setpoints=setpoints, seg_len=steps, band=band,
                              tail=tail, want_pairs=True, want_trace=want_trace)
    host = lambda v: None if v is None else v.cpu().numpy()
    return dict(rows=rows, wave=wave, summary=host(out["summary"]), pairs=host(out["pairs"]), actions=host(out["actions"]),
                outputs=host(out["outputs"]), n_steps=len(setpoints) * int(steps), seg_len=int(steps), steps=int(steps), setpoints=setpoints,
                band=band, tail=tail, n=int(env.num_envs))


def frequency_response(result):
    """Transfer-function estimates from the lock-in rows of a `frequency_sweep` result (or any dict with rows [P, 3], wave [P, L, 2],
    pairs [n_segments, 16, P, N] and, for a ragged last segment, n_steps).  Per (row p, segment s) the window is k = k0 .. len_s - 1;
    a signal x with sums (X0, XC, XS) over it is fitted by least squares with x_k ~ d + b c_k + a s_k -- the normal equations are the
    table's own sums, so any table serves and a window that is not a whole number of cycles is handled -- and its phasor against the
    reference s is X = a + j b (x_k = Im(X e^{j theta_k}) for a sinusoid).  E is the same fit of e_k = A s_k, from the table itself.
    Returns a dict, complex [P, n_segments, N] unless said:
      Y, U, E        the phasors of the controlled output, the controller's output a_c and the excitation (E [P, n_segments])
      T              Y / E on SETPOINT rows: the complementary sensitivity (NaN elsewhere)
      L, S           on LOAD rows the loop transfer function L = -U / (U + E) (a_env = a_c + e carries the same step index) and the
                     sensitivity S = 1 / (1 + L)
      N              Y / E on MEASUREMENT rows: the noise sensitivity (-T for a linear loop)
      share          float64: the share of y's variance over the window that the fitted fundamental explains -- below 1 where the
                     plant answers with harmonics: a per-plant index of non-linearity
      omega          float64 [P]: rad per sample, from the phase the table advances by at the onset
      point          int [P]
    NaN where the segment never reaches the onset, and in the ratios where nothing is excited (A = 0, the Nyquist rate)."""
    rows = np.asarray(result["rows"], dtype=np.float64)
    wave = np.asarray(result["wave"], dtype=np.float64)
    pairs = np.asarray(result["pairs"], dtype=np.float64)
    S_, R, P, N = pairs.shape
    base = len(METRIC_NAMES)
    assert R == base + len(FREQ_ROW_NAMES) and rows.shape == (P, 3) and wave.shape[0] == P and wave.shape[2] == 2, (pairs.shape, rows.shape, wave.shape)
    L0 = wave.shape[1]
    n_steps = int(result.get("n_steps", S_ * L0))
    at = {name: base + j for j, name in enumerate(FREQ_ROW_NAMES)}
    point = np.clip(np.nan_to_num(np.rint(rows[:, 0]), nan=0.0), 0, 2).astype(int)
    nan = np.full((P, S_, N), np.nan + 0j)
    Y, U = nan.copy(), nan.copy()
    E = np.full((P, S_), np.nan + 0j)
    share = np.full((P, S_, N), np.nan)
    om = np.full(P, np.nan)
    for p in range(P):
        k0 = rows[p, 2]
        if not np.isfinite(k0):
            continue
        k0 = int(min(max(np.rint(k0), 0), 2 ** 30))
        if k0 + 1 < L0:
            (c0, s0), (c1, s1) = wave[p, k0], wave[p, k0 + 1]
            om[p] = abs(np.arctan2(s1 * c0 - c1 * s0, c1 * c0 + s1 * s0))
        for s in range(S_):
            length = min(L0, n_steps - s * L0)
            if k0 >= length:
                continue
            c, sn = wave[p, k0:length, 0], wave[p, k0:length, 1]
            W = float(length - k0)
            G = np.array([[W, c.sum(), sn.sum()], [c.sum(), (c * c).sum(), (c * sn).sum()], [sn.sum(), (c * sn).sum(), (sn * sn).sum()]])
            Gi = np.linalg.pinv(G, rcond=1e-9, hermitian=True)
            fit = lambda x0, xc, xs: Gi @ np.stack([x0, xc, xs])                      # (d, b, a) per plant
            fy = fit(pairs[s, at["y0"], p], pairs[s, at["yc"], p], pairs[s, at["ys"], p])
            fu = fit(pairs[s, at["u0"], p], pairs[s, at["uc"], p], pairs[s, at["us"], p])
            fe = Gi @ (rows[p, 1] * G[:, 2])
            Y[p, s], U[p, s], E[p, s] = fy[2] + 1j * fy[1], fu[2] + 1j * fu[1], fe[2] + 1j * fe[1]
            y0, y2 = pairs[s, at["y0"], p], pairs[s, at["y2"], p]
            explained = fy[1] * (pairs[s, at["yc"], p] - G[0, 1] * y0 / W) + fy[2] * (pairs[s, at["ys"], p] - G[0, 2] * y0 / W)
            total = y2 - y0 * y0 / W
            with np.errstate(divide="ignore", invalid="ignore"):
                share[p, s] = np.where(total > 0, explained / total, np.nan)
    Eb = E[:, :, None]
    quiet = ~(np.abs(Eb) > 1e-9 * np.maximum(np.abs(rows[:, 1])[:, None, None], 1e-300))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(quiet, np.nan, Y / Eb)
        loop = np.where(quiet, np.nan, -U / (U + Eb))
        sens = 1.0 / (1.0 + loop)
    is_pt = lambda v: (point == v)[:, None, None]
    return dict(Y=Y, U=U, E=E, T=np.where(is_pt(FREQ_POINTS["setpoint"]), ratio, np.nan), L=np.where(is_pt(FREQ_POINTS["load"]), loop, np.nan),
                S=np.where(is_pt(FREQ_POINTS["load"]), sens, np.nan), N=np.where(is_pt(FREQ_POINTS["measurement"]), ratio, np.nan),
                share=share, omega=om, point=point)


def _log_interp(w0, w1, f0, f1, level, v0, v1):
    """f crosses `level` between (w0, f0) and (w1, f1), linearly in log w: (the crossing's w, v there, linear in log w as well)."""
    x = (level - f0) / (f1 - f0)
    return float(np.exp(np.log(w0) + x * (np.log(w1) - np.log(w0)))), float(v0 + x * (v1 - v0))


def _margins_of(w, L, wt, T):
    """One plant and segment: (gain margin, phase margin in degrees, peak |S|, bandwidth) from L at ascending w and T at ascending wt."""
    gm = pm = peak = bw = np.nan
    ok = np.isfinite(L)
    w, L = w[ok], L[ok]
    if w.size >= 1:
        mag, ph = np.log(np.abs(L)), np.unwrap(np.angle(L))
        for i in range(w.size - 1):                    # gain crossover: |L| falls through 1
            if np.isnan(pm) and mag[i] > 0.0 >= mag[i + 1]:
                pm = np.degrees(_log_interp(w[i], w[i + 1], mag[i], mag[i + 1], 0.0, ph[i], ph[i + 1])[1] + np.pi)
            if np.isnan(gm) and ph[i] > -np.pi >= ph[i + 1]:   # phase crossover: arg L falls through -180 degrees
                gm = float(np.exp(-_log_interp(w[i], w[i + 1], ph[i], ph[i + 1], -np.pi, mag[i], mag[i + 1])[1]))
        s = np.abs(1.0 / (1.0 + L))
        j = int(np.argmax(s))
        peak = float(s[j])
        if 0 < j < w.size - 1:                         # an interior maximum: the parabola through its three points in log w
            x = np.log(w[j - 1:j + 2]) - np.log(w[j])
            a, b, _ = np.polyfit(x, s[j - 1:j + 2], 2)
            if a < 0:
                peak = float(s[j] - b * b / (4 * a))
    ok = np.isfinite(T)
    wt, T = wt[ok], np.abs(T[ok])
    for i in range(wt.size - 1):                       # bandwidth: |T| falls through 1 / sqrt 2
        if T[i] > np.sqrt(0.5) >= T[i + 1]:
            bw = _log_interp(wt[i], wt[i + 1], T[i], T[i + 1], np.sqrt(0.5), 0.0, 0.0)[0]
            break
    return gm, pm, peak, bw


def stability_margins(response):
    """Classical margins from a `frequency_response`: per segment and plant, float64 [n_segments, N] each --
      gain_margin   1 / |L| where arg L first falls through -180 degrees (the unwrapped phase over the LOAD rows in ascending omega)
      phase_margin  180 degrees + arg L where |L| first falls through 1, in degrees
      peak_S        the largest |S| = |1 / (1 + L)| over the LOAD rows, refined by the parabola through the three points around an
                    interior maximum
      bandwidth     omega (rad per sample) where |T| first falls through 1 / sqrt 2 over the SETPOINT rows
    Crossings are interpolated linearly in log omega between the two rows that bracket them (log |L| and the phase for the margins,
    |T| for the bandwidth) and are NaN where the grid brackets none; rows where nothing was excited are left out."""
    om, point = np.asarray(response["omega"], dtype=np.float64), np.asarray(response["point"])
    L, T = np.asarray(response["L"]), np.asarray(response["T"])
    _, S_, N = L.shape
    pick = lambda v: (lambda idx: idx[np.argsort(om[idx], kind="stable")])(np.flatnonzero((point == v) & np.isfinite(om) & (om > 0)))
    il, it = pick(FREQ_POINTS["load"]), pick(FREQ_POINTS["setpoint"])
    out = {k: np.full((S_, N), np.nan) for k in ("gain_margin", "phase_margin", "peak_S", "bandwidth")}
    for s in range(S_):
        for i in range(N):
            g, ph, pk, bw = _margins_of(om[il], L[il, s, i], om[it], T[it, s, i])
            out["gain_margin"][s, i], out["phase_margin"][s, i], out["peak_S"][s, i], out["bandwidth"][s, i] = g, ph, pk, bw
    return out
