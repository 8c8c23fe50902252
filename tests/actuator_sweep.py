"""Checker of the actuator-limits sweep (`pime_actuator_sweep`, csrc/actuator_sweep.hpp) and the ctypes binding of its host build
(libpime_actuator_host.so, include/pime_actuator_host.h).  Shared by tests/test_actuator_sweep_cpu.py and
tests/test_gpu_actuator_sweep.py.  TEST INFRASTRUCTURE: the pime_amd package never loads the host library.

`check_recording` takes what a call left -- actions (the APPLIED u), commands (the controller's a_c), outputs [T, P, N] and pairs
[S, 16, P, N] -- and the lane state it started from; no pair, step or row is left out:
  [chain]      `chain`, a numpy restatement of the four actuator stages, run on the recorded commands and the recorded previous applied
               action (0.0 before the launch's first step, carried over segment boundaries), gives `actions` bit for bit;
  [trajectory] every pair replayed open-loop through the float64 oracle (OraclePH / OracleWT, tests/mpc_eval.py: Plant) under u
               reproduces the recorded outputs at the bars of tests/rollout_replay.py: pH within 1e-5 (the same titration cell), tank
               within 2e-4 * (1 + |y|);
  [action]     every recorded a_c is the float64 controller output -- the prior term summed in ascending j, plus the policy's tanh term
               -- on the oracle's observation of that step with the sensor stage restated in numpy (measured columns on the levels
               QY * rint(obs / QY)), within tests/margin_sweep.py's ACT_BAR * (1 + |wanted|) (profiles/margin_sweep_bars.txt).  Where
               the oracle's obs / QY lies within TIE of a rounding tie the controller at EITHER neighbouring level is accepted; no
               step is excluded;
  [metrics]    protocols.metrics_from_records of the recorded (u, outputs) gives seven of the first eight rows of `pairs` bit for bit;
               the return row is held to the oracle's rewards at the trajectory bar (rewards are not recorded);
  [actuator]   `actuator_rows` of the three traces -- the chain's flags, the gap, the reversals, the tail windows -- gives the eight
               actuator rows bit for bit.
`numpy_loop` is a restatement of the whole loop in closed loop on the oracle; it takes one named fault (FAULTS) and the checker is
vetted on those."""
import ctypes as C
import itertools
import os

import numpy as np

import margin_sweep as G
import mpc_eval as M
import prior_sweep as P

HOST_LIB_PATH = os.path.join(P.PKG, "libpime_actuator_host.so")
HOST_EXPORTS = ("pime_actuator_sweep_host", "pime_actuator_host_last_error")
FAULTS = ("clamp_before_quantise", "slew_from_command", "uprev_cleared", "deadband_strict", "round_half_up", "qy_on_setpoint",
          "qy_truncates", "metrics_fed_command", "reversals_count_zero", "tail_off_by_one", "sat_counts_unchanged",
          "gap_iae_descending", "off_stage_rewrites")
# the shapes of the tests: 81 plants at a lane offset, 23 steps in segments of 9 (the last one ragged), tail 4
N, OFFSET, SEED = G.N, G.OFFSET, G.SEED
N_STEPS, SEG, TAIL, BAND = 23, 9, 4, 0.05
SETPOINTS = P.SETPOINTS
PRIOR_K = P.PRIOR_K
PH_CELL, WT_RTOL = M.PH_CELL, M.WT_RTOL          # tests/rollout_replay.py
ACT_BAR = G.ACT_BAR                              # tests/margin_sweep.py (profiles/margin_sweep_bars.txt)
TIE = 1e-4                                       # level units: how near a rounding tie either neighbour is accepted
COLS, ROWS, AROWS = 6, 16, 8
LO, HI, RATE, DEADBAND, QU, QY = range(6)
SAT_STEPS, RATE_STEPS, HOLD_STEPS, GAP_PEAK, GAP_IAE, REVERSALS, TAIL_Y_P2P, TAIL_U_P2P = range(8, 16)
_INF = np.inf
OFF = (-_INF, _INF, _INF, 0.0, 0.0, 0.0)


def _grid(lo, hi, rate, db, qu, qy):
    """all-off; each stage alone; clamp + quantise (neither limit a multiple of QU: the clamp-last order matters); dead-band + slew;
    everything on; all-off again"""
    return np.array([OFF, (lo, hi, _INF, 0, 0, 0), (-_INF, _INF, rate, 0, 0, 0), (-_INF, _INF, _INF, db, 0, 0), (-_INF, _INF, _INF, 0, qu, 0),
                     (-_INF, _INF, _INF, 0, 0, qy), (lo, hi, _INF, 0, qu, 0), (-_INF, _INF, rate, db, 0, 0), (lo, hi, rate, db, qu, qy), OFF],
                    dtype=np.float64)


# the prior's command spans about -2.8 .. 1.2 on the tank (0.4 (r - h2)) and +-0.15 on pH: every limit sits inside that range
ACT = {"wt": _grid(-0.35, 0.5, 0.15, 0.05, 0.12, 0.5), "ph": _grid(-0.035, 0.05, 0.02, 0.01, 0.015, 0.25)}
ALL_OFF = (0, 9)


def bits_equal(a, b):
    return P.bits_equal(a, b)


def n_segments(n_steps, seg_len):
    return P.n_segments(n_steps, seg_len)


def stages(row):
    """Which stages a row switches on, as pime_actuator_sweep decodes it: dict clamp / slew / hold / quant / sense."""
    lo, hi, rate, db, qu, qy = (float(v) for v in row)
    return dict(clamp=lo > -_INF or hi < _INF, slew=0.0 < rate < _INF, hold=db > 0.0, quant=qu > 0.0, sense=qy > 0.0)


def chain(row, a_c, u_prev, fault=None, a_prev=None):
    """The applied action [N] and the flags (held, slewed, clamped) of one step from the commands a_c [N] and the previous applied
    action u_prev [N]: csrc/actuator_sweep.hpp's act_apply in numpy float64.  A stage that is off touches nothing."""
    lo, hi, rate, db, qu, _ = (float(v) for v in row)
    on = stages(row)
    n = len(a_c)
    v = np.array(a_c, dtype=np.float64)
    held = slewed = clamped = np.zeros(n, dtype=bool)
    rewrite = fault == "off_stage_rewrites"

    def clamp(v):
        c1 = v < lo
        v = np.where(c1, lo, v)
        c2 = v > hi
        return np.where(c2, hi, v), c1 | c2

    def quantise(v):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return qu * (np.floor(v / qu + 0.5) if fault == "round_half_up" else np.rint(v / qu))
    with np.errstate(invalid="ignore", over="ignore"):
        if on["hold"]:
            gap = np.abs(v - u_prev)
            held = gap < db if fault == "deadband_strict" else gap <= db
            v = np.where(held, u_prev, v)
        elif rewrite:
            v = v + 0.0
        if on["slew"]:
            ref = a_prev if fault == "slew_from_command" else u_prev
            d = v - ref
            dc = np.where(d < -rate, -rate, d)
            dc = np.where(dc > rate, rate, dc)
            slewed = dc != d
            v = ref + dc
        if fault == "clamp_before_quantise":
            if on["clamp"]:
                v, clamped = clamp(v)
            if on["quant"]:
                v = quantise(v)
        else:
            if on["quant"]:
                v = quantise(v)
            if on["clamp"]:
                v, clamped = clamp(v)
    return v, (held, slewed, clamped)


def replay_chain(row, commands, u0=None, fault=None):
    """`chain` over the recorded commands [T, N]: the applied actions [T, N] and the flags [3, T, N].  u_prev is carried from step to
    step and over segment boundaries, 0.0 before the first."""
    T, n = commands.shape
    u_prev = np.zeros(n) if u0 is None else u0
    us, flags = [], []
    for t in range(T):
        u, f = chain(row, commands[t], u_prev, fault=fault, a_prev=commands[t - 1] if t > 0 else np.zeros(n))
        us.append(u); flags.append(np.stack(f))
        u_prev = u
    return np.stack(us), np.stack(flags, axis=1)


def actuator_rows(row, commands, actions, outputs, seg_len, tail, fault=None):
    """The eight actuator rows [S, 8, N] from a pair's three traces [T, N], sequential as csrc/actuator_sweep.hpp's ActMetrics
    accumulates them; the flags come from `chain` on (commands[t], actions[t - 1])."""
    T, n = outputs.shape
    S, L0 = n_segments(T, seg_len), (seg_len if seg_len > 0 else T)
    out = np.zeros((S, AROWS, n))
    on = stages(row)
    for s in range(S):
        lo, hi = s * L0, min((s + 1) * L0, T)
        sat, rate, hold, rev = (np.zeros(n) for _ in range(4))
        peak, iae, last = np.zeros(n), np.zeros(n), np.zeros(n)
        gaps = []
        for t in range(lo, hi):
            u_prev = actions[t - 1] if t > 0 else np.zeros(n)
            _, (held, slewed, clamped) = chain(row, commands[t], u_prev)
            if fault == "sat_counts_unchanged" and on["clamp"]:
                clamped = np.ones(n, dtype=bool)
            sat, rate, hold = sat + clamped, rate + slewed, hold + held
            g = np.abs(commands[t] - actions[t])
            peak = np.where(g > peak, g, peak)
            gaps.append(g)
            m = actions[t] - u_prev
            sg = np.where(m > 0, 1.0, np.where(m < 0, -1.0, 0.0))
            if fault == "reversals_count_zero":
                turned = (sg != last) & (t > lo)
                rev, last = rev + turned, sg
            else:
                moved = sg != 0
                rev = rev + (moved & (last != 0) & (sg != last))
                last = np.where(moved, sg, last)
        for g in (reversed(gaps) if fault == "gap_iae_descending" else gaps):
            iae = iae + g
        length = hi - lo
        first = length - min(tail, length) - (1 if fault == "tail_off_by_one" else 0)
        win = slice(lo + max(first, 0), hi)
        out[s] = np.stack([sat, rate, hold, peak, iae, rev, outputs[win].max(axis=0) - outputs[win].min(axis=0),
                           actions[win].max(axis=0) - actions[win].min(axis=0)])
    return out


def sense(kind, row, obs, dtype=np.float32, fault=None):
    """The measured observation of csrc/actuator_sweep.hpp's act_measure from the env's observation obs [N, D] (float32 as the env's)."""
    om = np.array(obs, dtype=dtype)
    qy = float(row[QY])
    if stages(row)["sense"]:
        cols = G._measured_cols(kind) + (((1 if kind == "ph" else 2),) if fault == "qy_on_setpoint" else ())
        for c in cols:
            lv = om[:, c].astype(np.float64) / qy
            om[:, c] = (qy * (np.floor(lv) if fault == "qy_truncates" else np.rint(lv))).astype(dtype)
    return om


class ConstPolicy:
    """A policy whose tanh term is the constant c: with zero prior gains the command is exactly c at every step (ties on purpose)."""

    def __init__(self, c):
        self.c = float(c)

    def term(self, obs, dtype=np.float64):
        return np.full(len(obs), self.c)


# ------------------------------------------------------------------------------------------------ the restatement in closed loop
def numpy_loop(kind, cfg, lanes, table, rows=None, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND,
               tail=TAIL, fault=None, negzero=False):
    """The loop of include/pime_hip.h in numpy on the oracle as the plant (float64 state).  policy: None or an object with
    term(obs, dtype).  negzero: a zero command is emitted as -0.0 (IEEE addition from +0.0 never makes one; this is the only way to
    show that an idle stage keeps the sign).  Returns dict actions (u), commands (a_c), outputs [T, P, N], pairs [S, 16, P, N]."""
    from pime_amd import protocols
    assert fault is None or fault in FAULTS
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    rows = np.asarray(ACT[kind] if rows is None else rows, dtype=np.float64)
    n, Pn, S = len(lanes["r"]), len(rows), n_segments(n_steps, seg_len)
    L0 = seg_len if seg_len > 0 else n_steps
    pol = None if policy is None else policy.term
    actions, commands, outputs = (np.zeros((n_steps, Pn, n)) for _ in range(3))
    pairs = np.zeros((S, ROWS, Pn, n))
    row_faults = ("reversals_count_zero", "tail_off_by_one", "sat_counts_unchanged", "gap_iae_descending")
    for p in range(Pn):
        plant = M.Plant(kind, cfg, lanes, table)
        us, cmds, ys, rews, rs, y_start = [], [], [], [], [], []
        u_prev, a_prev = np.zeros(n), np.zeros(n)
        for t in range(n_steps):
            if seg_len > 0 and t % seg_len == 0:
                plant.boundary(sp[t // seg_len], t > 0)
                if fault == "uprev_cleared" and t > 0:
                    u_prev = np.zeros(n)
            if t % L0 == 0:
                y_start.append(plant.y())
            om = sense(kind, rows[p], plant.obs().astype(np.float32), fault=fault)
            a_c = G.controller(om, K, pol)[0]
            if negzero:
                a_c = np.where(a_c == 0.0, -0.0, a_c)
            u, _ = chain(rows[p], a_c, u_prev, fault=fault, a_prev=a_prev)
            y, rew = plant.step(u)
            us.append(u); cmds.append(a_c); ys.append(y); rews.append(rew); rs.append(plant.o.get("r"))
            u_prev, a_prev = u, a_c
        us, cmds, ys = np.stack(us), np.stack(cmds), np.stack(ys)
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(ys, np.stack(rs), cmds if fault == "metrics_fed_command" else us, np.stack(rews),
                                               np.stack(y_start), seg_len=seg_len, band=band, tail=tail)
        actions[:, p], commands[:, p], outputs[:, p] = us, cmds, ys
        for j, name in enumerate(protocols.METRIC_NAMES):
            pairs[:, j, p] = m[name]
        pairs[:, 8:, p] = actuator_rows(rows[p], cmds, us, ys, seg_len, tail, fault=fault if fault in row_faults else None)
    return dict(actions=actions, commands=commands, outputs=outputs, pairs=pairs)


# ------------------------------------------------------------------------------------------------ the checker
def _wanted_commands(kind, row, obs, K, policy):
    """The float64 controller on the oracle's observation obs [N, D] behind the sensor stage: a list of candidates [N] -- one, or,
    with QY on, one per choice of neighbouring level for the measured columns (only the lanes within TIE of a tie differ)."""
    qy = float(row[QY])
    if not stages(row)["sense"]:
        return [G.controller(obs, K, policy)[0]]
    cols = G._measured_cols(kind)
    out = []
    for up in itertools.product((0.0, 1.0), repeat=len(cols)):
        om = obs.copy()
        for c, bit in zip(cols, up):
            lv = obs[:, c] / qy
            near = np.abs(lv - np.floor(lv) - 0.5) <= TIE
            om[:, c] = qy * np.where(near, np.floor(lv) + bit, np.rint(lv))
        out.append(G.controller(om, K, policy)[0])
    return out


def check_recording(kind, cfg, lanes, table, rec, rows=None, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND,
                    tail=TAIL, act_bar=ACT_BAR, only=None, tag=""):
    """rec: dict with actions, commands, outputs [T, P, N] and pairs [S, 16, P, N] of one call from the lane state `lanes`.  policy:
    None or a callable obs float64 [N, D] -> the float64 tanh term [N].  only: the rows to check (None: every row).  Returns the share
    of each bar the recording uses: dict trajectory / ret / action, and `gap`."""
    from pime_amd import protocols
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    rows = np.asarray(ACT[kind] if rows is None else rows, dtype=np.float64)
    actions, commands, outputs, pairs = (np.asarray(rec[k], dtype=np.float64) for k in ("actions", "commands", "outputs", "pairs"))
    n, Pn, S = len(lanes["r"]), len(rows), n_segments(n_steps, seg_len)
    L0 = seg_len if seg_len > 0 else n_steps
    assert actions.shape == commands.shape == outputs.shape == (n_steps, Pn, n) and pairs.shape == (S, ROWS, Pn, n), (actions.shape, pairs.shape)
    use_traj = use_ret = gap = 0.0
    for p in (range(Pn) if only is None else only):
        where = f"{tag} row {p} {rows[p].tolist()}"
        want_u, _ = replay_chain(rows[p], commands[:, p])
        # (step by step from the RECORDED previous action as well: one wrong step must not hide behind the next)
        for t in range(n_steps):
            u_t, _ = chain(rows[p], commands[t, p], actions[t - 1, p] if t > 0 else np.zeros(n))
            assert bits_equal(actions[t, p], u_t), f"[chain] the applied action is not what dead-band, slew, quantise, clamp make of the recorded command and the recorded previous action {where}: step {t}, plants {np.flatnonzero(actions[t, p].view(np.uint64) != u_t.view(np.uint64))[:4].tolist()}"
        assert bits_equal(actions[:, p], want_u), f"[chain] the applied actions are not the chain's over the recorded commands {where}"
        plant = M.Plant(kind, cfg, lanes, table)
        rews, rs, y_start = [], [], []
        for t in range(n_steps):
            if seg_len > 0 and t % seg_len == 0:
                plant.boundary(sp[t // seg_len], t > 0)
            if t % L0 == 0:
                y_start.append(plant.y())
            got = commands[t, p]
            e = None
            for want in _wanted_commands(kind, rows[p], plant.obs(), K, policy):
                with np.errstate(invalid="ignore"):
                    ew = np.abs(got - want) / (1.0 + np.abs(want))
                ew = np.where(np.isfinite(want), ew, np.where(bits_equal(got, want), 0.0, np.inf))
                e = ew if e is None else np.fmin(e, ew)
            gap = max(gap, float(np.nanmax(e)))
            assert not np.isnan(e).any() and gap <= act_bar, f"[action] the recorded command is not the controller's output on the sensor's reading of the true observation {where}: step {t}, {float(np.nanmax(e)):.3g} (bar {act_bar:.3g}) at plants {np.flatnonzero(~(e <= act_bar))[:4].tolist()}"
            y, rew = plant.step(actions[t, p])
            err = np.abs(outputs[t, p] - y)
            bar = np.full_like(y, PH_CELL) if kind == "ph" else WT_RTOL * (1.0 + np.abs(y))
            use_traj = max(use_traj, float((err / bar).max()))
            assert use_traj <= 1.0, f"[trajectory] the recorded outputs leave the oracle's replay of the applied actions {where}: step {t}, {use_traj:.3g} of the bar at plants {np.flatnonzero(err > bar)[:4].tolist()}"
            rews.append(rew); rs.append(plant.o.get("r"))
        rew, rs = np.stack(rews), np.stack(rs)
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(outputs[:, p], rs, actions[:, p], rew, M.y_start_recorded(outputs[:, p], np.stack(y_start), seg_len),
                                               seg_len=seg_len, band=band, tail=tail)
        for j, name in enumerate(protocols.METRIC_NAMES):
            if name == "return":
                rtol = 2e-5 if kind == "ph" else WT_RTOL
                for s in range(S):
                    rs_ = rew[s * L0:(s + 1) * L0].astype(np.float32).astype(np.float64)
                    room = rtol * (len(rs_) + np.abs(rs_).sum(axis=0))
                    use_ret = max(use_ret, float((np.abs(pairs[s, j, p] - m[name][s]) / room).max()))
                assert use_ret <= 1.0, f"[metrics] the return row leaves the oracle's rewards {where}: {use_ret:.3g} of the bar"
            else:
                assert bits_equal(pairs[:, j, p], m[name]), f"[metrics] row {name} is not what metrics_from_records makes of the call's own applied actions and outputs {where}"
        want = actuator_rows(rows[p], commands[:, p], actions[:, p], outputs[:, p], seg_len, tail)
        for j, name in enumerate(protocols.ACT_ROW_NAMES):
            assert bits_equal(pairs[:, 8 + j, p], want[:, j]), f"[actuator] row {name} is not what the three traces give {where}: segments {np.flatnonzero((pairs[:, 8 + j, p] != want[:, j]).any(axis=1)).tolist()}"
    return dict(trajectory=use_traj, ret=use_ret, action=gap / act_bar, gap=gap)


# ------------------------------------------------------------------------------------------------ host library
def host_lib():
    return P.load_host(HOST_LIB_PATH, HOST_EXPORTS[0],
                       [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                        C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], HOST_EXPORTS[1])


def host_raw(kind, cfg, lanes, N_, K, rows, Pn, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, commands, outputs):
    """The raw call: returns (status, message)."""
    s, keep = (None, None) if lanes is None else P._lanes_struct(kind, lanes)
    rc = host_lib().pime_actuator_sweep_host(C.byref(cfg), None if s is None else C.byref(s), N_, P._p(K), P._p(rows), Pn, n_steps, seg_len,
                                             P._p(sp), n_sp, band, tail, P._p(pairs), P._p(summary), P._p(actions), P._p(commands),
                                             P._p(outputs))
    del keep
    return rc, host_lib().pime_actuator_host_last_error().decode()


def host_actuator(kind, cfg, lanes, rows=None, K=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND, tail=TAIL, trace=True,
                  want_pairs=True):
    """The host build (the prior controller alone) from the lane state `lanes`, in the state precision cfg.state_mode names: dict
    summary [P, S, 16, 5], pairs [S, 16, P, N], actions, commands, outputs [T, P, N]."""
    n = len(lanes["r"])
    K = np.ascontiguousarray(PRIOR_K[kind] if K is None else K, dtype=np.float64)
    rows = np.ascontiguousarray(ACT[kind] if rows is None else rows, dtype=np.float64)
    Pn, S = len(rows), n_segments(n_steps, seg_len)
    sp = np.ascontiguousarray(setpoints if setpoints is not None else SETPOINTS[kind], dtype=np.float64)
    summary = np.full((Pn, S, ROWS, 5), -777.0)
    pairs = np.full((S, ROWS, Pn, n), -777.0) if want_pairs else None
    actions, commands, outputs = (np.full((n_steps, Pn, n), -777.0) for _ in range(3)) if trace else (None, None, None)
    rc, msg = host_raw(kind, cfg, lanes, n, K, rows, Pn, n_steps, seg_len, sp if seg_len > 0 else None, len(sp) if seg_len > 0 else 0, band,
                       tail, pairs, summary, actions, commands, outputs)
    assert rc == 0, f"pime_actuator_sweep_host failed ({rc}): {msg}"
    return dict(summary=summary, pairs=pairs, actions=actions, commands=commands, outputs=outputs)


def twin_case(kind, n, table, state_mode="f64", noise=0.01, seed=SEED, offset=OFFSET):
    """(cfg, keep, lanes) as tests/mpc_eval.py builds them, at this module's lane offset."""
    return M.twin_case(kind, n, table, state_mode, noise=noise, seed=seed, offset=offset)
