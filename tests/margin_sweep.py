"""Checker of the loop-perturbation sweep (`pime_margin_sweep`, csrc/margin_sweep.hpp) and the ctypes binding of its host build
(libpime_margin_host.so, include/pime_margin_host.h).  Shared by tests/test_margin_sweep_cpu.py and tests/test_gpu_margin_sweep.py.
TEST INFRASTRUCTURE: the pime_amd package never loads the host library.

`check_recording` takes what a call left -- actions, outputs [T, P, N] and pairs [S, 8, P, N] -- and the lane state it started from,
and replays EVERY pair open-loop through the float64 oracle (OraclePH / OracleWT, tests/mpc_eval.py: Plant), fed the recorded
applied actions; no pair, step or row is left out:
  [trajectory] the oracle reproduces the recorded outputs at the bars of tests/rollout_replay.py: pH within 1e-5 (the same titration
               cell), tank within 2e-4 * (1 + |y|);
  [zero]       the applied action of step t < d is exactly 0.0;
  [action]     the applied action of step t >= d is g x the float64 controller output of step t - d -- the prior term summed in
               ascending j, plus the policy's tanh term -- on the oracle's observation of that step plus sigma x the Philox stream-3
               Box-Muller draw keyed on the PLANT (oracle.binding.philox_uniform_pair: cosine -> column 0, sine -> column 1), within
               ACT_BAR * (1 + |wanted|).  The controller's history runs across segment boundaries;
  [metrics]    protocols.metrics_from_records of the recorded (applied actions, outputs) gives seven rows of `pairs` bit for bit; the
               return row is held to the oracle's rewards at the trajectory bar (rewards are not recorded: the departure
               tests/mpc_eval.py documents).
ACT_BAR is 10 x the largest gap a FLOAT32 numpy restatement of the loop (float32 observation, noise and policy, the state a MIXED
handle holds in float32: the tank's Euler sub-steps, pH's r and I) shows against this float64 check on the test shapes -- measured on
the CPU with no kernel involved, the tank's process noise off (profiles/margin_sweep_bars.txt; tests/test_margin_sweep_cpu.py::test_the_measured_bar re-measures it).
`numpy_loop` is that restatement in closed loop on the oracle; it takes one named fault (FAULTS) and the checker is vetted on those."""
import ctypes as C
import os

import numpy as np

import mpc_eval as M
import prior_sweep as P

HOST_LIB_PATH = os.path.join(P.PKG, "libpime_margin_host.so")
HOST_EXPORTS = ("pime_margin_sweep_host", "pime_margin_host_last_error")
FAULTS = ("delay_off_by_one", "line_cleared", "first_held", "gain_residual_only", "noise_pair", "noise_on_setpoint",
          "sigma_ignored_delayed", "sincos_swapped", "noise_into_plant", "commanded_in_variation", "setpoint_stale", "transposed")
# the shapes of the tests: 81 plants at a lane offset, 23 steps in segments of 9 (the last one ragged), tail 4
N, OFFSET, SEED = 81, 1000, 3
N_STEPS, SEG, TAIL, BAND = 23, 9, 4, 0.05
NOISE_SEED, NOISE_EPOCH = 0x5EED1234ABCD, 7
STREAM_MEASURE = 3
MAX_DELAY = 8
SETPOINTS = P.SETPOINTS
PRIOR_K = P.PRIOR_K
PH_CELL, WT_RTOL = M.PH_CELL, M.WT_RTOL          # tests/rollout_replay.py
ACT_MEASURED = 2.7e-6                            # profiles/margin_sweep_bars.txt
ACT_BAR = 10 * ACT_MEASURED
# P = 5, the nominal row first and last; delays {0, 1, 3, 8}, gains {0.5, 2}, sigma {0, 0.05}
PERTURB = np.array([[1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [2.0, 3.0, 0.05], [1.0, 8.0, 0.05], [1.0, 0.0, 0.0]])


def bits_equal(a, b):
    return P.bits_equal(a, b)


def n_segments(n_steps, seg_len):
    return P.n_segments(n_steps, seg_len)


def decode_row(row):
    """(g, d, sigma) as pime_margin_sweep reads a row: d = rint clamped into 0 .. 8, NaN -> 0."""
    d = np.rint(row[1])
    d = 0 if not d >= 0 else int(min(d, MAX_DELAY))
    return float(row[0]), d, float(row[2])


_noise_cache = {}


def measure_noise(seed, epoch, gids, n_steps):
    """float64 [n_steps, len(gids), 2]: the standard normals (cosine branch, sine branch) of every step for the global lanes `gids`."""
    import oracle
    key = (seed, epoch, tuple(int(g) for g in gids), n_steps)
    if key not in _noise_cache:
        u = np.array([[oracle.philox_uniform_pair(seed, int(g), epoch, t, STREAM_MEASURE) for g in gids] for t in range(n_steps)])
        rad, ang = np.sqrt(-2.0 * np.log(1.0 - u[..., 0])), 2.0 * np.pi * u[..., 1]
        _noise_cache[key] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1)
    return _noise_cache[key]


class NumpyPolicy:
    """A plain tanh actor D -> md -> md -> md -> 1 in numpy, float64 weights that are exact float32 values: `term(obs, dtype)` is the
    residual's tanh term in that precision (float32: every layer in float32, the float64 tanh of the mean rounded once)."""

    def __init__(self, D, md=64, seed=11):
        rng = np.random.default_rng(seed)
        dims = [D, md, md, md, 1]
        self.W = [(rng.standard_normal((dims[k + 1], dims[k])) / np.sqrt(dims[k]) * (0.1 if k == 3 else 1.0)).astype(np.float32)
                  for k in range(4)]
        self.b = [(0.05 * rng.standard_normal(dims[k + 1])).astype(np.float32) for k in range(4)]

    def term(self, obs, dtype=np.float64):
        h = np.asarray(obs, dtype=dtype)
        for k in range(4):
            h = h @ self.W[k].astype(dtype).T + self.b[k].astype(dtype)
            if k < 3:
                h = np.tanh(h)
        mean = h[:, 0]
        if dtype == np.float32:
            return np.tanh(mean.astype(np.float64)).astype(np.float32).astype(np.float64)
        return np.tanh(mean)


def controller(om, K, policy=None, dtype=np.float64):
    """a_c [N] from the measured observation om [N, D]: the prior term in double, ascending j from 0.0, the policy's tanh term added."""
    a = np.zeros(om.shape[0])
    for j in range(om.shape[1]):
        a = a + om[:, j].astype(np.float64) * K[j]
    if policy is None:
        return a, np.zeros_like(a)
    term = policy(om) if dtype == np.float64 else policy(om, np.float32)
    return term + a, term


def _measured_cols(kind):
    return (0,) if kind == "ph" else (0, 1)


def _mixed_words(kind):
    return ("r", "I") if kind == "ph" else ("h1", "h2", "r", "I")


class TankF32:
    """The Integrator tank with FLOAT32 state in numpy, process noise off: the arithmetic of a MIXED handle's lane step (every Euler
    sub-step rounds to float32), restated from include/pime_hip.h and the env class -- the plant of the bar's measurement only."""

    def __init__(self, cfg, lanes):
        assert cfg.wt_noise_scale == 0.0
        f = np.float32
        self.cfg = cfg
        self.h1, self.h2, self.a1, self.a2, self.kp, self.r, self.I = (np.asarray(lanes[k], dtype=np.float64).astype(f)
                                                                       for k in ("h1", "h2", "a1", "a2", "Kp", "r", "I"))

    def boundary(self, sp, bump):
        self.r = np.full_like(self.r, np.float32(sp)); self.I = np.zeros_like(self.I)

    def setpoint(self):
        return self.r.astype(np.float64)

    def y(self):
        return self.h2.astype(np.float64)

    def obs(self):
        return np.column_stack([self.h1, self.h2, self.r, self.I]).astype(np.float64)

    def step(self, a):
        c, f = self.cfg, np.float32
        u = (np.asarray(a, dtype=np.float64) * c.wt_pmax / 2.0 + c.wt_pmax / 2.0).astype(f)
        A1, A2, G, dt = f(c.wt_A1), f(c.wt_A2), f(c.wt_G), f(c.wt_dt)
        h1, h2 = self.h1, self.h2
        with np.errstate(invalid="ignore", over="ignore"):
            for _ in range(c.wt_n_discrete):
                s1, s2 = np.sqrt(f(2) * G * h1), np.sqrt(f(2) * G * h2)
                n1 = h1 + (-self.a1 / A1 * s1 + self.kp / A1 * u) * dt
                n2 = h2 + (self.a1 / A2 * s1 - self.a2 / A2 * s2) * dt
                h1, h2 = np.maximum(n1, f(0)), np.maximum(n2, f(0))
            self.h1, self.h2 = h1, h2
            dist = np.abs(h2 - self.r)
            rew = {0: -dist, 1: -(dist * dist), 2: np.where(dist > f(c.distance_threshold), f(-1), f(0))}[int(c.reward_type)]
            if int(c.reward_type) != 2:
                rew = rew * f(c.wt_z1)
            I_raw = self.I + (self.r - h2)
            rew = rew + -f(c.integral_punish) * np.abs(I_raw)
            self.I = np.minimum(np.maximum(I_raw, f(-c.integral_max)), f(c.integral_max))
        return self.y(), rew.astype(np.float64)


def _setpoint(plant):
    return plant.setpoint() if isinstance(plant, TankF32) else plant.o.get("r")


# ------------------------------------------------------------------------------------------------ the restatement in closed loop
def numpy_loop(kind, cfg, lanes, table, perturb=PERTURB, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND,
               tail=TAIL, seed=NOISE_SEED, epoch=NOISE_EPOCH, dtype=np.float64, fault=None):
    """The loop of include/pime_hip.h in numpy on the oracle as the plant.  policy: None or an object with term(obs, dtype).
    The observation and the noise sum are float32 as the env's observation is.  dtype float32 (no faults): the policy in float32 as
    well and the state as a MIXED handle holds it -- pH: the oracle with r and I rounded to float32 after every step; tank: TankF32,
    every Euler sub-step in float32, which needs cfg.wt_noise_scale == 0.  Returns dict actions, outputs [T, P, N], pairs [S, 8, P, N]."""
    from pime_amd import protocols
    assert fault is None or fault in FAULTS
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    perturb = np.asarray(perturb, dtype=np.float64)
    n, Pn, S = len(lanes["r"]), len(perturb), n_segments(n_steps, seg_len)
    f32 = dtype == np.float32
    pol = None if policy is None else policy.term
    actions, outputs, pairs = np.zeros((n_steps, Pn, n)), np.zeros((n_steps, Pn, n)), np.zeros((S, 8, Pn, n))
    sp_col = 1 if kind == "ph" else 2
    for p in range(Pn):
        g, d, sigma = decode_row(perturb[p])
        if fault == "delay_off_by_one":
            d = d + 1
        if fault == "sigma_ignored_delayed" and d > 0:
            sigma = 0.0
        gids = cfg.env_offset + np.arange(n) + (p * n if fault == "noise_pair" else 0)
        nz = measure_noise(seed, epoch, gids, n_steps)
        if fault == "sincos_swapped":
            nz = nz[..., ::-1]
        plant = TankF32(cfg, lanes) if f32 and kind == "wt" else M.Plant(kind, cfg, lanes, table)

        def to_f32():                       # pH in MIXED state: x, A, B, C stay float64; r and I are float32 words
            if f32 and kind == "ph":
                for k in _mixed_words(kind):
                    plant.o.set(k, plant.o.get(k).astype(np.float32).astype(np.float64))
        hist, terms, acts, cmds, ys, rews, rs, y_start = [], [], [], [], [], [], [], []
        r_stale = None
        for t in range(n_steps):
            if seg_len > 0 and t % seg_len == 0:
                r_stale = _setpoint(plant).copy()
                plant.boundary(sp[t // seg_len], t > 0)
                to_f32()
                if fault == "line_cleared" and t > 0:
                    hist, terms = [np.zeros(n)] * len(hist), [np.zeros(n)] * len(terms)
            if t % (seg_len if seg_len > 0 else n_steps) == 0:
                y_start.append(plant.y())
            obs = plant.obs()
            if fault == "setpoint_stale" and seg_len > 0 and t % seg_len == 0 and t > 0:
                obs[:, sp_col] = r_stale
            om = obs.astype(np.float32)           # the env's observation is float32 in every state mode; the noise is added in float32
            if sigma != 0.0:
                for c in _measured_cols(kind):
                    om[:, c] = om[:, c] + np.float32(sigma) * nz[t, :, c].astype(np.float32)
                if fault == "noise_on_setpoint":
                    om[:, sp_col] = om[:, sp_col] + np.float32(sigma) * nz[t, :, 0].astype(np.float32)
                if fault == "noise_into_plant" and kind == "wt":
                    plant.o.set("h1", np.maximum(om[:, 0].astype(np.float64), 0.0)); plant.o.set("h2", np.maximum(om[:, 1].astype(np.float64), 0.0))
            a_c, term = controller(om, K, pol, dtype)
            hist.append(a_c); terms.append(term)
            if t >= d:
                a_env = g * hist[t - d]
                if fault == "gain_residual_only":
                    a_env = g * terms[t - d] + (hist[t - d] - terms[t - d])
            else:
                a_env = g * hist[0] if fault == "first_held" else np.zeros(n)
            y, rew = plant.step(a_env)
            to_f32()
            y = plant.y()
            acts.append(a_env); cmds.append(a_c); ys.append(y); rews.append(rew); rs.append(_setpoint(plant))
        acts, ys = np.stack(acts), np.stack(ys)
        shown = np.stack(cmds) if fault == "commanded_in_variation" else acts
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(ys, np.stack(rs), shown, np.stack(rews), np.stack(y_start), seg_len=seg_len, band=band, tail=tail)
            if fault == "commanded_in_variation":
                m2 = protocols.metrics_from_records(ys, np.stack(rs), acts, np.stack(rews), np.stack(y_start), seg_len=seg_len, band=band, tail=tail)
                m = dict(m2, action_variation=m["action_variation"])
        actions[:, p], outputs[:, p] = acts, ys
        for j, name in enumerate(protocols.METRIC_NAMES):
            pairs[:, j, p] = m[name]
    if fault == "transposed":   # column i * P + p in place of p * N + i
        tr = lambda a: np.ascontiguousarray(np.swapaxes(a, -1, -2)).reshape(a.shape)
        actions, outputs, pairs = tr(actions), tr(outputs), tr(pairs)
    return dict(actions=actions, outputs=outputs, pairs=pairs)


# ------------------------------------------------------------------------------------------------ the checker
def check_recording(kind, cfg, lanes, table, rec, perturb=PERTURB, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None,
                    band=BAND, tail=TAIL, seed=NOISE_SEED, epoch=NOISE_EPOCH, act_bar=ACT_BAR, rows=None, tag=""):
    """rec: dict with actions, outputs [T, P, N] and pairs [S, 8, P, N] of one call from the lane state `lanes`.  policy: None or a
    callable obs float64 [N, D] -> the float64 tanh term [N].  rows: the rows to check (None: every row).  Returns the share of each
    bar the recording uses: dict trajectory / ret / action, and `gap`, the largest |got - wanted| / (1 + |wanted|)."""
    from pime_amd import protocols
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    perturb = np.asarray(perturb, dtype=np.float64)
    actions, outputs, pairs = (np.asarray(rec[k], dtype=np.float64) for k in ("actions", "outputs", "pairs"))
    n, Pn, S = len(lanes["r"]), len(perturb), n_segments(n_steps, seg_len)
    assert actions.shape == outputs.shape == (n_steps, Pn, n) and pairs.shape == (S, 8, Pn, n), (actions.shape, pairs.shape)
    use_traj = use_ret = gap = 0.0
    for p in (range(Pn) if rows is None else rows):
        g, d, sigma = decode_row(perturb[p])
        where = f"{tag} row {p} (g {g}, d {d}, sigma {sigma})"
        nz = measure_noise(seed, epoch, cfg.env_offset + np.arange(n), n_steps)
        plant = M.Plant(kind, cfg, lanes, table)
        hist, ys, rews, rs, y_start = [], [], [], [], []
        for t in range(n_steps):
            if seg_len > 0 and t % seg_len == 0:
                plant.boundary(sp[t // seg_len], t > 0)
            if t % (seg_len if seg_len > 0 else n_steps) == 0:
                y_start.append(plant.y())
            om = plant.obs()
            if sigma != 0.0:
                for c in _measured_cols(kind):
                    om[:, c] = om[:, c] + sigma * nz[t, :, c]
            hist.append(controller(om, K, policy)[0])
            got = actions[t, p]
            if t < d:
                assert (got == 0.0).all(), f"[zero] an applied action before the delay has passed is not 0.0 {where}: step {t}, plants {np.flatnonzero(got != 0.0)[:4].tolist()}"
            else:
                want = g * hist[t - d]
                with np.errstate(invalid="ignore"):
                    e = np.abs(got - want) / (1.0 + np.abs(want))
                e = np.where(np.isfinite(want), e, np.where(bits_equal(got, want), 0.0, np.inf))
                gap = max(gap, float(np.nanmax(e)))
                assert not np.isnan(e).any() and gap <= act_bar, f"[action] the applied action is not g x the controller's output of step t - d {where}: step {t}, {float(np.nanmax(e)):.3g} (bar {act_bar:.3g}) at plants {np.flatnonzero(~(e <= act_bar))[:4].tolist()}"
            y, rew = plant.step(got)
            err = np.abs(outputs[t, p] - y)
            bar = np.full_like(y, PH_CELL) if kind == "ph" else WT_RTOL * (1.0 + np.abs(y))
            use_traj = max(use_traj, float((err / bar).max()))
            assert use_traj <= 1.0, f"[trajectory] the recorded outputs leave the oracle's replay of the recorded actions {where}: step {t}, {use_traj:.3g} of the bar at plants {np.flatnonzero(err > bar)[:4].tolist()}"
            ys.append(y); rews.append(rew); rs.append(plant.o.get("r"))
        rew = np.stack(rews)
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(outputs[:, p], np.stack(rs), actions[:, p], rew,
                                               M.y_start_recorded(outputs[:, p], np.stack(y_start), seg_len), seg_len=seg_len, band=band, tail=tail)
        for j, name in enumerate(protocols.METRIC_NAMES):
            if name == "return":
                L0 = seg_len if seg_len > 0 else n_steps
                rtol = 2e-5 if kind == "ph" else WT_RTOL
                for s in range(S):
                    rs_ = rew[s * L0:(s + 1) * L0].astype(np.float32).astype(np.float64)
                    room = rtol * (len(rs_) + np.abs(rs_).sum(axis=0))
                    use_ret = max(use_ret, float((np.abs(pairs[s, j, p] - m[name][s]) / room).max()))
                assert use_ret <= 1.0, f"[metrics] the return row leaves the oracle's rewards {where}: {use_ret:.3g} of the bar"
            else:
                assert bits_equal(pairs[:, j, p], m[name]), f"[metrics] row {name} is not what metrics_from_records makes of the call's own applied actions and outputs {where}"
    return dict(trajectory=use_traj, ret=use_ret, action=gap / act_bar, gap=gap)


# ------------------------------------------------------------------------------------------------ host library
def host_lib():
    return P.load_host(HOST_LIB_PATH, HOST_EXPORTS[0],
                       [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32,
                        C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], HOST_EXPORTS[1])


def host_raw(kind, cfg, lanes, N_, K, perturb, Pn, seed, epoch, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, outputs):
    """The raw call: returns (status, message)."""
    s, keep = (None, None) if lanes is None else P._lanes_struct(kind, lanes)
    rc = host_lib().pime_margin_sweep_host(C.byref(cfg), None if s is None else C.byref(s), N_, P._p(K), P._p(perturb), Pn, seed, epoch,
                                           n_steps, seg_len, P._p(sp), n_sp, band, tail, P._p(pairs), P._p(summary), P._p(actions),
                                           P._p(outputs))
    del keep
    return rc, host_lib().pime_margin_host_last_error().decode()


def host_margin(kind, cfg, lanes, perturb=PERTURB, K=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND, tail=TAIL,
                seed=NOISE_SEED, epoch=NOISE_EPOCH, trace=True, want_pairs=True):
    """The host build (the prior controller alone) from the lane state `lanes`, in the state precision cfg.state_mode names: dict
    summary [P, S, 8, 5], pairs [S, 8, P, N], actions, outputs [T, P, N]."""
    n = len(lanes["r"])
    K = np.ascontiguousarray(PRIOR_K[kind] if K is None else K, dtype=np.float64)
    perturb = np.ascontiguousarray(perturb, dtype=np.float64)
    Pn, S = len(perturb), n_segments(n_steps, seg_len)
    sp = np.ascontiguousarray(setpoints if setpoints is not None else SETPOINTS[kind], dtype=np.float64)
    summary = np.full((Pn, S, 8, 5), -777.0)
    pairs = np.full((S, 8, Pn, n), -777.0) if want_pairs else None
    actions, outputs = (np.full((n_steps, Pn, n), -777.0), np.full((n_steps, Pn, n), -777.0)) if trace else (None, None)
    rc, msg = host_raw(kind, cfg, lanes, n, K, perturb, Pn, seed, epoch, n_steps, seg_len, sp if seg_len > 0 else None,
                       len(sp) if seg_len > 0 else 0, band, tail, pairs, summary, actions, outputs)
    assert rc == 0, f"pime_margin_sweep_host failed ({rc}): {msg}"
    return dict(summary=summary, pairs=pairs, actions=actions, outputs=outputs)


def twin_case(kind, n, table, state_mode="f64", noise=0.01, seed=SEED, offset=OFFSET):
    """(cfg, keep, lanes) as tests/mpc_eval.py builds them, at this module's lane offset."""
    return M.twin_case(kind, n, table, state_mode, noise=noise, seed=seed, offset=offset)
