"""Checker of the receding-horizon benchmark controller (`pime_mpc_eval`, csrc/mpc_eval.hpp) and the ctypes binding of its host build
(libpime_mpc_host.so, include/pime_mpc_host.h).  Shared by tests/test_mpc_eval_cpu.py and tests/test_gpu_mpc_eval.py.  TEST
INFRASTRUCTURE: the pime_amd package never loads the host library.

`check_recording` takes what a launch left -- actions, outputs, metrics -- and the lane state it started from:
  [trajectory] the true plant replayed under the RECORDED actions through the float64 oracle (OraclePH / OracleWT: set-point
               boundaries as r set, I and t zeroed, a new episode beyond the first; the tank's process noise from the oracle's own
               Philox stream) reproduces the recorded outputs at the bars of tests/rollout_replay.py: pH within 1e-5 (the same
               titration cell), tank within 2e-4 * (1 + |y|);
  [metrics]    protocols.metrics_from_records of (actions, outputs) gives every row of `metrics` bit for bit -- except the return,
               which is a sum of rewards the launch does not record: that row is held to the oracle's rewards at the trajectory bar;
  [grid]       every applied action lies on the final grid around a pass-0 grid point;
  [optimal] / [tie]  every step of every plant is optimal: in a float64 numpy restatement of candidates and cost (below; written from
               include/pime_hip.h, not from mpc_eval.hpp) at the oracle's state, no candidate of the final pass's grid or of pass 0's
               grid costs less than the applied action by more than OPT_BAR relative, and no candidate of the final grid with a
               smaller index and a different action ties it exactly.
OPT_BAR is 10 x the largest relative gap of the host build in FLOAT32 state against the float64 restatement on the test shapes
(profiles/mpc_eval_bars.txt, measured by tests/test_mpc_eval_cpu.py::test_the_measured_bar; the GPU build is never its source).
`numpy_mpc` is the restatement in closed loop; it takes one named fault (FAULTS) and the checker is vetted on those."""
import ctypes as C
import os

import numpy as np

import prior_sweep as P

HOST_LIB_PATH = os.path.join(P.PKG, "libpime_mpc_host.so")
HOST_EXPORTS = ("pime_mpc_eval_host", "pime_mpc_host_last_error")
FAULTS = ("horizon_short", "rho_ignored", "u_prev_stale", "model_noise", "prior_added", "setpoint_stale", "refine_from_zero",
          "tie_larger", "unclipped", "model_neighbour")
# the shapes of the issue: 70 plants at a lane offset (18 workgroups, the last half empty), three segments, the last one ragged
N, OFFSET, SEED = 70, 4096, 3
N_STEPS, SEG, TAIL, BAND = 24, 10, 4, 0.05
HORIZON, PASSES = 5, 2
SETPOINTS = P.SETPOINTS
PH_CELL, WT_RTOL = 1e-5, 2e-4                     # tests/rollout_replay.py
OPT_MEASURED = 6.02e-5                            # profiles/mpc_eval_bars.txt
OPT_BAR = 10 * OPT_MEASURED
J_FLOOR = 1e-300
REWARD_NAMES = {0: "distance", 1: "square_distance", 2: "sparse"}


def bits_equal(a, b):
    return P.bits_equal(a, b)


# ------------------------------------------------------------------------------------------------ candidates and cost, in numpy
def grid0():
    return np.clip(-1.0 + np.arange(64, dtype=np.float64) * (2.0 / 63.0), -1.0, 1.0)


def grid_step(p):
    s = 2.0 / 63.0
    for _ in range(p):
        s = s / 32.0
    return s


def grid_around(center, p, clipped=True):
    """[..., 64] the candidates of pass p >= 1 around `center` [...]."""
    u = np.asarray(center, dtype=np.float64)[..., None] + (np.arange(64, dtype=np.float64) - 32.0) * grid_step(p)
    return np.clip(u, -1.0, 1.0) if clipped else u


def reachable(passes):
    """Every action `passes` passes can end on: the final grids around every pass-0 grid point (sorted, unique)."""
    s = grid0()
    for p in range(1, passes):
        s = np.unique(grid_around(s, p).reshape(-1))
    return s


def wt_cost(cfg, st, r, u, u_prev, H, rho, noise=None):
    """Tank: J [N, C] of the constant actions u [N, C] from st = (h1, h2, a1, a2, kp), each [N]; noise: None or [H, 2, N]."""
    h1, h2, a1, a2, kp = (np.asarray(v, dtype=np.float64)[:, None] + np.zeros_like(u) for v in st)
    A1, A2, G, dt, pmax = cfg.wt_A1, cfg.wt_A2, cfg.wt_G, cfg.wt_dt, cfg.wt_pmax
    up = u * pmax / 2.0 + pmax / 2.0
    J = np.zeros_like(u)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(H):
            for _ in range(cfg.wt_n_discrete):
                s1, s2 = np.sqrt(2 * G * h1), np.sqrt(2 * G * h2)
                n1 = h1 + (-a1 / A1 * s1 + kp / A1 * up) * dt
                n2 = h2 + (a1 / A2 * s1 - a2 / A2 * s2) * dt
                h1, h2 = np.maximum(n1, 0.0), np.maximum(n2, 0.0)
            if noise is not None:
                h1, h2 = np.maximum(h1 + noise[k, 0][:, None], 0.0), np.maximum(h2 + noise[k, 1][:, None], 0.0)
            e = h2 - r[:, None]
            J = J + e * e
        du = u - u_prev[:, None]
        return J + rho * (du * du)


def ph_cost(cfg, table, st, r, u, u_prev, H, rho):
    """pH: J [N, C] from st = (x, A, B, C), each [N]."""
    x, A, B, Cc = (np.asarray(v, dtype=np.float64)[:, None] + np.zeros_like(u) for v in st)
    a = np.clip(u, -1.0, 1.0)
    uu = cfg.ph_u_low + (cfg.ph_u_high - cfg.ph_u_low) * ((a + 1.0) / 2.0)
    J = np.zeros_like(u)
    for k in range(H):
        x = A * x + B * uu
        idx = np.clip(np.rint(Cc * x * cfg.ph_table_scale), 0, len(table) - 1).astype(np.int64)
        e = table[idx] - r[:, None]
        J = J + e * e
    du = u - u_prev[:, None]
    return J + rho * (du * du)


def pick(J, larger_on_tie=False):
    """The choice rule over the last axis: the smallest finite J, the smaller index on a tie, index 0 if none is finite."""
    Jf = np.where(np.isfinite(J), J, np.inf)
    if larger_on_tie:
        return J.shape[-1] - 1 - np.argmin(Jf[..., ::-1], axis=-1)
    return np.argmin(Jf, axis=-1)


# ------------------------------------------------------------------------------------------------ the true plant: the oracle
class Plant:
    """The float64 oracle holding the lane state `lanes` (P.twin_lanes / the handle's fields)."""

    def __init__(self, kind, cfg, lanes, table):
        import oracle
        self.kind, n = kind, len(lanes["r"])
        if kind == "ph":
            self.o = oracle.OraclePH(n, table, max_steps=2 ** 30, reward_type=REWARD_NAMES[cfg.reward_type],
                                     integral_bound=bool(cfg.integral_bound), resample_every=0, seed=cfg.seed, env_offset=cfg.env_offset)
            self.o.set_punish(cfg.integral_punish, cfg.action_punish, cfg.action_change_punish)
            names = ("A", "B", "C", "x", "r", "I", "t", "episode")
        else:
            self.o = oracle.OracleWT(n, max_steps=2 ** 30, reward_type=REWARD_NAMES[cfg.reward_type], num_stack=0, resample_every=0,
                                     noise_scale=cfg.wt_noise_scale, seed=cfg.seed, env_offset=cfg.env_offset)
            self.o.set_punish(cfg.integral_punish)
            names = ("a1", "a2", "Kp", "h1", "h2", "r", "I", "t", "episode")
        self.o.reset()
        for k in names:
            self.o.set(k, np.asarray(lanes[k], dtype=np.float64))

    def boundary(self, sp, bump):
        self.o.set("r", sp); self.o.set("I", 0.0); self.o.set("t", 0.0)
        if bump:
            self.o.set("episode", self.o.get("episode") + 1)

    def state(self):
        if self.kind == "ph":
            return tuple(self.o.get(k) for k in ("x", "A", "B", "C"))
        return tuple(self.o.get(k) for k in ("h1", "h2", "a1", "a2", "Kp"))

    def y(self):
        return self.o.get("y") if self.kind == "ph" else self.o.get("h2")

    def obs(self):
        if self.kind == "ph":
            return np.column_stack([self.y(), self.o.get("r"), self.o.get("I")])
        return np.column_stack([self.o.get(k) for k in ("h1", "h2", "r", "I")])

    def step(self, a):
        _, _, rew, _ = self.o.step(a, auto_reset=False)
        return self.y(), rew


def n_segments(n_steps, seg_len):
    return P.n_segments(n_steps, seg_len)


def _cost(kind, cfg, table, st, r, u, u_prev, H, rho, noise=None):
    return ph_cost(cfg, table, st, r, u, u_prev, H, rho) if kind == "ph" else wt_cost(cfg, st, r, u, u_prev, H, rho, noise)


# ------------------------------------------------------------------------------------------------ the restatement in closed loop
def numpy_mpc(kind, cfg, lanes, table, horizon=HORIZON, passes=PASSES, rho=0.0, n_steps=N_STEPS, seg_len=SEG, setpoints=None,
              band=BAND, tail=TAIL, model=None, fault=None):
    """The controller of include/pime_hip.h in float64 numpy on the oracle as the true plant.  Returns a dict: actions, outputs
    [T, N], metrics [S, 8, N], index [T, N] (the final pass's winner), margin [T, N] (the smallest relative distance of a runner-up's
    cost over all passes; inf where every other candidate repeats the winner's action), pass_costs [T, passes, N]."""
    from pime_amd import protocols
    assert fault is None or fault in FAULTS
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    n = len(lanes["r"])
    plant = Plant(kind, cfg, lanes, table)
    rng = np.random.default_rng(9)
    H = horizon - 1 if fault == "horizon_short" else horizon
    rho_c = 0.0 if fault == "rho_ignored" else rho
    u_prev, r_ctl = np.zeros(n), plant.o.get("r")
    acts, ys, rews, y_start, rs = [], [], [], [], []
    index, margin, pcost = np.zeros((n_steps, n), dtype=np.int64), np.full((n_steps, n), np.inf), np.zeros((n_steps, passes, n))
    K = P.PRIOR_K[kind]
    for t in range(n_steps):
        if seg_len > 0 and t % seg_len == 0:
            plant.boundary(sp[t // seg_len], t > 0)
            if not (fault == "setpoint_stale" and t > 0):
                r_ctl = plant.o.get("r")
        elif seg_len == 0 and t == 0:
            r_ctl = plant.o.get("r")
        if t % (seg_len if seg_len > 0 else n_steps) == 0:
            y_start.append(plant.y())
        st = plant.state()
        if kind == "wt" and model is not None:
            m = np.asarray(model, dtype=np.float64)
            if fault == "model_neighbour":
                m = np.roll(m, -1, axis=0)
            st = st[:2] + (m[:, 0], m[:, 1], m[:, 2])
        noise = cfg.wt_noise_scale * rng.standard_normal((H, 2, n)) if fault == "model_noise" else None
        ustar = np.zeros(n)
        for p in range(passes):
            if p == 0:
                u = np.broadcast_to(grid0(), (n, 64)).copy()
                if fault == "unclipped":
                    u = u * 1.25
            else:
                center = np.full(n, grid0()[0]) if fault == "refine_from_zero" else ustar
                u = grid_around(center, p, clipped=fault != "unclipped")
            J = _cost(kind, cfg, table, st, r_ctl, u, u_prev, H, rho_c, noise)
            c = pick(J, larger_on_tie=fault == "tie_larger")
            ustar = u[np.arange(n), c]
            Jc = J[np.arange(n), c]
            other = np.where(u != ustar[:, None], np.where(np.isfinite(J), J, np.inf), np.inf)
            with np.errstate(invalid="ignore"):
                margin[t] = np.minimum(margin[t], (other.min(axis=1) - Jc) / np.maximum(Jc, J_FLOOR))
            index[t], pcost[t, p] = c, Jc
        applied = ustar + plant.obs() @ K if fault == "prior_added" else ustar
        y, rew = plant.step(applied)
        acts.append(ustar); ys.append(y); rews.append(rew); rs.append(plant.o.get("r"))
        if fault != "u_prev_stale":
            u_prev = ustar
    m = protocols.metrics_from_records(np.stack(ys), np.stack(rs), np.stack(acts), np.stack(rews), np.stack(y_start), seg_len=seg_len,
                                       band=band, tail=tail)
    metrics = np.stack([m[name] for name in protocols.METRIC_NAMES], axis=1)
    return dict(actions=np.stack(acts), outputs=np.stack(ys), metrics=metrics, index=index, margin=margin, pass_costs=pcost)


# ------------------------------------------------------------------------------------------------ the checker
def optimality_gaps(kind, cfg, lanes, table, actions, horizon, passes, rho, n_steps, seg_len, setpoints, model=None):
    """Replays the true plant under `actions` through the oracle and, at every step, restates the costs.  Returns (outputs [T, N],
    rewards [T, N], y_start [S, N], r [T, N], gap [T, N], tie [T, N] bool, on_grid [T, N] bool): gap = (J(applied) - min J over
    pass 0's grid and the final grid) / max(min J, J_FLOOR); tie: a final-grid candidate of smaller index and another action has
    exactly the applied action's cost."""
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    n = actions.shape[1]
    plant = Plant(kind, cfg, lanes, table)
    u_prev = np.zeros(n)
    ys, rews, y_start, rs = [], [], [], []
    gap, tie, on_grid = np.zeros((n_steps, n)), np.zeros((n_steps, n), dtype=bool), np.zeros((n_steps, n), dtype=bool)
    rows = np.arange(n)
    for t in range(n_steps):
        if seg_len > 0 and t % seg_len == 0:
            plant.boundary(sp[t // seg_len], t > 0)
        if t % (seg_len if seg_len > 0 else n_steps) == 0:
            y_start.append(plant.y())
        r = plant.o.get("r")
        st = plant.state()
        if kind == "wt" and model is not None:
            m = np.asarray(model, dtype=np.float64)
            st = st[:2] + (m[:, 0], m[:, 1], m[:, 2])
        cost = lambda u: _cost(kind, cfg, table, st, r, u, u_prev, horizon, rho)
        a = actions[t]
        Ja = cost(a[:, None])[:, 0]
        g0 = np.broadcast_to(grid0(), (n, 64))
        J0 = cost(g0.copy())
        best = np.where(np.isfinite(J0), J0, np.inf).min(axis=1)
        # the final grid: the one the restatement's own earlier passes lead to where the applied action lies on it, otherwise any
        # grid around a reachable centre that holds the applied action
        ustar = g0[rows, pick(J0)]
        for p in range(1, passes - 1):
            u = grid_around(ustar, p)
            ustar = u[rows, pick(cost(u))]
        if passes > 1:
            final = grid_around(ustar, passes - 1)
            miss = np.flatnonzero(~(final == a[:, None]).any(axis=1))
            if len(miss):
                centres = reachable(passes - 1)
                for i in miss:
                    cand = grid_around(centres, passes - 1)
                    hit = np.flatnonzero((cand == a[i]).any(axis=1))
                    if len(hit):
                        final[i] = cand[hit[np.argmin(np.abs(centres[hit] - ustar[i]))]]
            on_grid[t] = (final == a[:, None]).any(axis=1)
            Jf = cost(final)
            best = np.minimum(best, np.where(np.isfinite(Jf), Jf, np.inf).min(axis=1))
            where = np.argmax(final == a[:, None], axis=1)
        else:
            final, Jf = g0, J0
            on_grid[t] = (g0 == a[:, None]).any(axis=1)
            where = np.argmax(g0 == a[:, None], axis=1)
        earlier = np.arange(64)[None, :] < where[:, None]
        tie[t] = (earlier & (Jf == Ja[:, None]) & (final != a[:, None])).any(axis=1) & on_grid[t]
        with np.errstate(invalid="ignore"):
            gap[t] = np.where(np.isfinite(Ja), (Ja - best) / np.maximum(best, J_FLOOR), np.where(np.isfinite(best), np.inf, 0.0))
        y, rew = plant.step(a)
        ys.append(y); rews.append(rew); rs.append(r)
        u_prev = a
    return np.stack(ys), np.stack(rews), np.stack(y_start), np.stack(rs), gap, tie, on_grid


def check_recording(kind, cfg, lanes, table, rec, horizon=HORIZON, passes=PASSES, rho=0.0, n_steps=N_STEPS, seg_len=SEG, setpoints=None,
                    band=BAND, tail=TAIL, model=None, opt_bar=OPT_BAR, tag=""):
    """rec: dict with actions, outputs [T, N] and metrics [S, 8, N] of one launch from the lane state `lanes`.  Returns the share of
    each bar the recording uses: dict trajectory / return / optimal."""
    from pime_amd import protocols
    actions, outputs, metrics = (np.asarray(rec[k], dtype=np.float64) for k in ("actions", "outputs", "metrics"))
    n = actions.shape[1]
    assert actions.shape == outputs.shape == (n_steps, n) and metrics.shape == (n_segments(n_steps, seg_len), 8, n)
    assert np.isfinite(actions).all() and (np.abs(actions) <= 1.0).all(), f"[grid] an applied action is outside [-1, 1] {tag}"
    y, rew, y_start, r, gap, tie, on_grid = optimality_gaps(kind, cfg, lanes, table, actions, horizon, passes, rho, n_steps, seg_len,
                                                            setpoints, model)
    # 1. the true plant under the recorded actions
    err = np.abs(outputs - y)
    bar = np.full_like(y, PH_CELL) if kind == "ph" else WT_RTOL * (1.0 + np.abs(y))
    use_traj = float((err / bar).max())
    assert use_traj <= 1.0, f"[trajectory] the recorded outputs leave the oracle's replay of the recorded actions {tag}: {use_traj:.3g} of the bar at {np.argwhere(err > bar)[:3].tolist()}"
    # 2. the metrics from the launch's own records; the return from the oracle's rewards
    m = protocols.metrics_from_records(outputs, r, actions, rew, y_start_recorded(outputs, y_start, seg_len), seg_len=seg_len, band=band, tail=tail)
    use_ret = 0.0
    for j, name in enumerate(protocols.METRIC_NAMES):
        if name == "return":
            L0 = seg_len if seg_len > 0 else n_steps
            rtol = 2e-5 if kind == "ph" else WT_RTOL
            for s in range(metrics.shape[0]):
                rs_ = rew[s * L0:(s + 1) * L0].astype(np.float32).astype(np.float64)
                room = rtol * (len(rs_) + np.abs(rs_).sum(axis=0))
                use_ret = max(use_ret, float((np.abs(metrics[s, j] - m[name][s]) / room).max()))
            assert use_ret <= 1.0, f"[metrics] the return row leaves the oracle's rewards {tag}: {use_ret:.3g} of the bar"
        else:
            assert bits_equal(metrics[:, j], m[name]), f"[metrics] row {name} is not what metrics_from_records makes of the launch's own actions and outputs {tag}"
    # 3. every step of every plant
    assert on_grid.all(), f"[grid] an applied action is on no final grid around a pass-0 grid point {tag}: {np.argwhere(~on_grid)[:3].tolist()}"
    use_opt = float(gap.max()) / opt_bar
    assert use_opt <= 1.0, f"[optimal] a candidate costs less than the applied action {tag}: relative gap {gap.max():.3g} (bar {opt_bar:.3g}) at {np.argwhere(gap > opt_bar)[:3].tolist()}"
    assert not tie.any(), f"[tie] a candidate of smaller index ties the applied action's cost {tag}: {np.argwhere(tie)[:3].tolist()}"
    return dict(trajectory=use_traj, ret=use_ret, optimal=use_opt, gap=float(gap.max()))


def y_start_recorded(outputs, y_start, seg_len):
    """The output before each segment's first step: the recorded output of the step before it (the plant state is carried over a
    boundary); before the launch's first step only the oracle knows it."""
    out = np.array(y_start, dtype=np.float64)
    L0 = seg_len if seg_len > 0 else len(outputs)
    for s in range(1, out.shape[0]):
        out[s] = outputs[s * L0 - 1]
    return out


# ------------------------------------------------------------------------------------------------ host library
def host_lib():
    return P.load_host(HOST_LIB_PATH, HOST_EXPORTS[0],
                       [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p,
                        C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], HOST_EXPORTS[1])


def host_raw(kind, cfg, lanes, N_, model, horizon, passes, rho, n_steps, seg_len, sp, n_sp, band, tail, metrics, actions, outputs,
             pass_costs=None):
    """The raw call: returns (status, message)."""
    s, keep = (None, None) if lanes is None else P._lanes_struct(kind, lanes)
    rc = host_lib().pime_mpc_eval_host(C.byref(cfg), None if s is None else C.byref(s), N_, P._p(model), horizon, passes, rho, n_steps,
                                       seg_len, P._p(sp), n_sp, band, tail, P._p(metrics), P._p(actions), P._p(outputs), P._p(pass_costs))
    del keep
    return rc, host_lib().pime_mpc_host_last_error().decode()


def host_mpc(kind, cfg, lanes, horizon=HORIZON, passes=PASSES, rho=0.0, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND,
             tail=TAIL, model=None, trace=True):
    """The host build from the lane state `lanes`, in the state precision cfg.state_mode names: dict actions, outputs, metrics,
    pass_costs."""
    n = len(lanes["r"])
    sp = np.ascontiguousarray(setpoints if setpoints is not None else SETPOINTS[kind], dtype=np.float64)
    metrics = np.full((n_segments(n_steps, seg_len), 8, n), -777.0)
    actions, outputs = (np.full((n_steps, n), -777.0), np.full((n_steps, n), -777.0)) if trace else (None, None)
    pc = np.full((n_steps, passes, n), -777.0) if trace else None
    model = None if model is None else np.ascontiguousarray(model, dtype=np.float64)
    rc, msg = host_raw(kind, cfg, lanes, n, model, horizon, passes, rho, n_steps, seg_len, sp if seg_len > 0 else None,
                       len(sp) if seg_len > 0 else 0, band, tail, metrics, actions, outputs, pc)
    assert rc == 0, f"pime_mpc_eval_host failed ({rc}): {msg}"
    return dict(actions=actions, outputs=outputs, metrics=metrics, pass_costs=pc)


def twin_case(kind, n, table, state_mode="f64", noise=0.01, seed=SEED, offset=OFFSET, draws_seed=5):
    """(cfg, keep, lanes): the configuration and a lane state of `n` plants spread over the registered ensemble ranges, from the CPU
    twin.  With float32 state the lane words are rounded as a MIXED handle holds them (the tank's all, pH's r and I)."""
    import pime_amd.native as nt
    over = {} if kind == "ph" else {"wt_noise_scale": noise}
    draws = P.case_draws(kind, n, SETPOINTS[kind][0], seed=draws_seed)
    twin = P.make_twin(kind, n, table, seed, offset, over, draws)
    lanes = P.twin_lanes(twin)
    twin.close()
    cfg, keep = P.host_cfg(kind, n, table, seed, offset, **over)
    if state_mode != "f64":
        cfg.state_mode = nt.STATE_MIXED
        for k in (("r", "I") if kind == "ph" else ("h1", "h2", "a1", "a2", "Kp", "r", "I")):
            lanes[k] = lanes[k].astype(np.float32).astype(np.float64)
    return cfg, keep, lanes

