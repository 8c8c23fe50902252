"""Checker of the disturbance-rejection sweep (`pime_disturb_sweep`, csrc/disturb_sweep.hpp) and the ctypes binding of its host build
(libpime_disturb_host.so, include/pime_disturb_host.h).  Shared by tests/test_disturb_sweep_cpu.py and tests/test_gpu_disturb_sweep.py.
TEST INFRASTRUCTURE: the pime_amd package never loads the host library.

`check_recording` takes what a call left -- actions (the CONTROLLER's outputs a_c), outputs [T, P, N] and pairs [S, 15, P, N] -- and
the lane state it started from (pH: with the stored qww_V and qc_V), and replays EVERY pair open-loop through the float64 oracle
(OraclePH / OracleWT, tests/mpc_eval.py: Plant).  The oracle's plant words are switched with `set` at the onset, at the end of a pulse
and at segment boundaries (pH: A', B' from np.exp / np.expm1 of qww_V * M0, C' = qc_V * M1; a unit multiplier keeps the stored word),
and the oracle is fed a_c + d_u while the row is active, a_c otherwise; no pair, step or row is left out:
  [action]     every recorded a_c is the float64 controller output -- the prior term summed in ascending j, plus the policy's tanh term
               -- on the oracle's observation of that step, within tests/margin_sweep.py's ACT_BAR * (1 + |wanted|): the same
               controller arithmetic with sigma 0, the project's own bar;
  [trajectory] the oracle reproduces the recorded outputs at the bars of tests/rollout_replay.py: pH within 1e-5 (the same titration
               cell), tank within 2e-4 * (1 + |y|);
  [metrics]    protocols.metrics_from_records of the recorded (a_c, outputs) gives seven of the first eight rows of `pairs` bit for
               bit; the return row is held to the oracle's rewards at the trajectory bar (rewards are not recorded);
  [nan]        the seven rejection rows are NaN exactly in the segments the row never starts in;
  [rejection]  `rejection_rows` of the recorded traces -- a sequential numpy restatement of the window rows -- gives the seven
               rejection rows bit for bit;
  [nominal]    before the first onset, actions and outputs are bit-equal to those of the nominal row.
`numpy_loop` is a restatement of the whole loop in closed loop on the oracle; it takes one named fault (FAULTS) and the checker is
vetted on those."""
import ctypes as C
import os

import numpy as np

import margin_sweep as G
import mpc_eval as M
import prior_sweep as P

HOST_LIB_PATH = os.path.join(P.PKG, "libpime_disturb_host.so")
HOST_EXPORTS = ("pime_disturb_sweep_host", "pime_disturb_host_last_error")
FAULTS = ("onset_off_by_one", "pulse_long", "pulse_short", "kept_over_boundary", "load_behind_clip", "load_recorded",
          "multiplier_wrong_parameter", "A_rebuilt_B_kept", "C_scaled_by_M0", "e0_after_step", "peak_step_from_segment",
          "recovery_from_segment", "window_from_segment", "finite_for_nan")
# the shapes of the tests: 81 plants at a lane offset, 23 steps in segments of 9 (the last one ragged), tail 4
N, OFFSET, SEED = G.N, G.OFFSET, G.SEED
N_STEPS, SEG, TAIL, BAND = 23, 9, 4, 0.05
SETPOINTS = P.SETPOINTS
PRIOR_K = P.PRIOR_K
PH_CELL, WT_RTOL = M.PH_CELL, M.WT_RTOL          # tests/rollout_replay.py
ACT_BAR = G.ACT_BAR                              # tests/margin_sweep.py
COLS, ROWS, DROWS = 6, 15, 7
E0, PEAK, PEAK_STEP, RECOVERY, IAE, ITAE, ACTION_PEAK = range(8, 15)
MAX_STEPS = 2 ** 30
# columns (k0, L, d_u, M0, M1, M2): nominal; load step; pulse from the first step; plant step; onset beyond the ragged segment with a
# load and a plant step; a pulse the boundary cuts to one step; nominal with a finite window
_COMMON = [(0, 0, 0, 1, 1, 1), (3, 0, 0.3, 1, 1, 1), (0, 2, -0.5, 1, 1, 1), (4, 0, 0, 1.5, 0.7, 1), None, (8, 5, 0.1, 1, 1, 1), (2, 0, 0, 1, 1, 1)]
DISTURB = {"wt": np.array([r if r is not None else (6, 0, 0.2, 1, 1, 0.8) for r in _COMMON], dtype=np.float64),
           "ph": np.array([r if r is not None else (6, 0, 0.2, 1, 1.2, 1) for r in _COMMON], dtype=np.float64)}


def bits_equal(a, b):
    return P.bits_equal(a, b)


def n_segments(n_steps, seg_len):
    return P.n_segments(n_steps, seg_len)


def decode_row(row):
    """(k0, L, d_u, M0, M1, M2) as pime_disturb_sweep reads a row: k0 and L rint, clamped into 0 .. 2^30; NaN: never / 0."""
    k0, L = np.rint(row[0]), np.rint(row[1])
    k0 = None if np.isnan(k0) else int(min(max(k0, 0), MAX_STEPS))
    L = 0 if np.isnan(L) else int(min(max(L, 0), MAX_STEPS))
    return k0, L, float(row[2]), float(row[3]), float(row[4]), float(row[5])


def is_active(k, k0, L):
    return k0 is not None and k >= k0 and (L == 0 or k < k0 + L)


def plant_sets(kind, cfg, lanes, m0, m1, m2):
    """(names, nominal, disturbed): the plant words the oracle is switched between; a unit multiplier keeps the stored word."""
    if kind == "wt":
        nom = tuple(np.asarray(lanes[k], dtype=np.float64) for k in ("a1", "a2", "Kp"))
        return ("a1", "a2", "Kp"), nom, (nom[0] * m0, nom[1] * m1, nom[2] * m2)
    A, B, Cc = (np.asarray(lanes[k], dtype=np.float64) for k in ("A", "B", "C"))
    Ad, Bd, Cd = A, B, Cc
    if m0 != 1.0:
        q = np.asarray(lanes["qww_V"], dtype=np.float64) * m0
        e = -q * cfg.ph_sample_t
        Ad, Bd = np.exp(e), -np.expm1(e) / q
    if m1 != 1.0:
        Cd = np.asarray(lanes["qc_V"], dtype=np.float64) * m1
    return ("A", "B", "C"), (A, B, Cc), (Ad, Bd, Cd)


def _set_plant(plant, names, values):
    for k, v in zip(names, values):
        plant.o.set(k, v)


def _y_start(kind, plant, table, nominal):
    """The controlled output under the NOMINAL plant before a segment's first step (pH: the oracle's stored y is the last step's,
    under whatever C that step ran on)."""
    if kind == "wt":
        return plant.o.get("h2")
    return P._ph_y(np.asarray(table, dtype=np.float64), nominal[2], plant.o.get("x"))


def rejection_rows(actions, outputs, r, y_start, k0, seg_len, band, fault=None):
    """The seven rejection rows [S, 7, N] from a pair's traces: actions (a_c), outputs, r [T, N], y_start [S, N].  Sequential, as
    csrc/disturb_sweep.hpp's DistMetrics accumulates them."""
    T, n = outputs.shape
    S, L0 = n_segments(T, seg_len), (seg_len if seg_len > 0 else T)
    out = np.full((S, DROWS, n), np.nan)
    for s in range(S):
        lo, hi = s * L0, min((s + 1) * L0, T)
        if k0 is None or k0 >= hi - lo:
            if fault == "finite_for_nan":
                out[s] = 0.0
            continue
        first = 0 if fault == "window_from_segment" else k0
        base = 0 if fault in ("peak_step_from_segment", "recovery_from_segment", "window_from_segment") else k0
        y_before = y_start[s] if k0 == 0 else outputs[lo + k0 - 1]
        if fault == "e0_after_step":
            y_before = outputs[lo + k0]
        a_ref = np.zeros(n) if k0 == 0 else actions[lo + k0 - 1]
        rr = r[lo + k0]
        e0 = rr - y_before
        peak, peak_step, recovery = None, np.zeros(n), np.zeros(n)
        iae, itae, apeak = np.zeros(n), np.zeros(n), None
        for k in range(first, hi - lo):
            ae = np.abs(r[lo + k] - outputs[lo + k])
            w = k - k0 + 1
            da = np.abs(actions[lo + k] - a_ref)
            if peak is None:
                peak, peak_step, apeak = ae.copy(), np.full(n, float(k - (base if fault == "peak_step_from_segment" else k0) + 1)), da.copy()
            else:
                up = ae > peak
                peak = np.where(up, ae, peak)
                peak_step = np.where(up, float(k - (base if fault == "peak_step_from_segment" else k0) + 1), peak_step)
                apeak = np.where(da > apeak, da, apeak)
            iae = iae + ae
            itae = itae + float(w) * ae
            recovery = np.where(ae > band, float(k - (base if fault == "recovery_from_segment" else k0) + 1), recovery)
        out[s] = np.stack([e0, peak, peak_step, recovery, iae, itae, apeak])
    return out


# ------------------------------------------------------------------------------------------------ the restatement in closed loop
def numpy_loop(kind, cfg, lanes, table, rows=None, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND,
               tail=TAIL, fault=None):
    """The loop of include/pime_hip.h in numpy on the oracle as the plant (float64 state).  policy: None or an object with
    term(obs, dtype).  Returns dict actions (a_c), outputs [T, P, N], pairs [S, 15, P, N]."""
    from pime_amd import protocols
    assert fault is None or fault in FAULTS
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    rows = np.asarray(DISTURB[kind] if rows is None else rows, dtype=np.float64)
    n, Pn, S = len(lanes["r"]), len(rows), n_segments(n_steps, seg_len)
    L0 = seg_len if seg_len > 0 else n_steps
    pol = None if policy is None else policy.term
    actions, outputs, pairs = np.zeros((n_steps, Pn, n)), np.zeros((n_steps, Pn, n)), np.zeros((S, ROWS, Pn, n))
    for p in range(Pn):
        k0, L, du, m0, m1, m2 = decode_row(rows[p])
        if fault == "multiplier_wrong_parameter":
            m0, m1 = m1, m0
        names, nominal, disturbed = plant_sets(kind, cfg, lanes, m0, m1, m2)
        if kind == "ph" and fault == "A_rebuilt_B_kept":
            disturbed = (disturbed[0], nominal[1], disturbed[2])
        if kind == "ph" and fault == "C_scaled_by_M0" and m0 != 1.0:
            disturbed = (disturbed[0], disturbed[1], np.asarray(lanes["qc_V"], dtype=np.float64) * m0)
        k0_run = k0 if fault != "onset_off_by_one" or k0 is None else k0 + 1
        L_run = L + (1 if fault == "pulse_long" else -1 if fault == "pulse_short" else 0) if L > 0 else L
        plant = M.Plant(kind, cfg, lanes, table)
        cmds, ys, rews, rs, y_start = [], [], [], [], []
        on = False
        for t in range(n_steps):
            k = t % L0
            if seg_len > 0 and t % seg_len == 0:
                plant.boundary(sp[t // seg_len], t > 0)
            if k == 0:
                y_start.append(_y_start(kind, plant, table, nominal))
            kept = fault == "kept_over_boundary" and on and t > 0 and k < (k0_run or 0)
            on = is_active(k, k0_run, L_run) or kept
            _set_plant(plant, names, disturbed if on else nominal)
            a_c = G.controller(plant.obs().astype(np.float32), K, pol)[0]
            a_env = a_c + du if on else a_c
            if fault == "load_behind_clip" and on:
                a_env = np.clip(a_c, -1.0, 1.0) + du
            y, rew = plant.step(a_env)
            cmds.append(a_env if fault == "load_recorded" else a_c); ys.append(y); rews.append(rew); rs.append(plant.o.get("r"))
        cmds, ys, rs, y_start = np.stack(cmds), np.stack(ys), np.stack(rs), np.stack(y_start)
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(ys, rs, cmds, np.stack(rews), y_start, seg_len=seg_len, band=band, tail=tail)
        actions[:, p], outputs[:, p] = cmds, ys
        for j, name in enumerate(protocols.METRIC_NAMES):
            pairs[:, j, p] = m[name]
        pairs[:, 8:, p] = rejection_rows(cmds, ys, rs, y_start, k0, seg_len, band, fault=fault)
    return dict(actions=actions, outputs=outputs, pairs=pairs)


# ------------------------------------------------------------------------------------------------ the checker
def check_recording(kind, cfg, lanes, table, rec, rows=None, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND,
                    tail=TAIL, act_bar=ACT_BAR, nominal_row=0, only=None, tag=""):
    """rec: dict with actions, outputs [T, P, N] and pairs [S, 15, P, N] of one call from the lane state `lanes`.  policy: None or a
    callable obs float64 [N, D] -> the float64 tanh term [N].  nominal_row: a row with zero load and unit multipliers the others are
    compared with before their first onset (None: skip).  only: the rows to check (None: every row).  Returns the share of each bar the
    recording uses: dict trajectory / ret / action, and `gap`."""
    from pime_amd import protocols
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    rows = np.asarray(DISTURB[kind] if rows is None else rows, dtype=np.float64)
    actions, outputs, pairs = (np.asarray(rec[k], dtype=np.float64) for k in ("actions", "outputs", "pairs"))
    n, Pn, S = len(lanes["r"]), len(rows), n_segments(n_steps, seg_len)
    L0 = seg_len if seg_len > 0 else n_steps
    assert actions.shape == outputs.shape == (n_steps, Pn, n) and pairs.shape == (S, ROWS, Pn, n), (actions.shape, pairs.shape)
    use_traj = use_ret = gap = 0.0
    for p in (range(Pn) if only is None else only):
        k0, L, du, m0, m1, m2 = decode_row(rows[p])
        where = f"{tag} row {p} {rows[p].tolist()}"
        names, nominal, disturbed = plant_sets(kind, cfg, lanes, m0, m1, m2)
        plant = M.Plant(kind, cfg, lanes, table)
        rews, rs, y_start, loose = [], [], [], []
        on = False
        for t in range(n_steps):
            k = t % L0
            if seg_len > 0 and t % seg_len == 0:
                plant.boundary(sp[t // seg_len], t > 0)
            if k == 0:
                # the output the segment starts from: the recorded one where the step before ran on the nominal C (the plant state is
                # carried over a boundary), otherwise only the oracle knows it
                exact = t > 0 and (kind == "wt" or not on or m1 == 1.0)
                y_start.append(outputs[t - 1, p] if exact else _y_start(kind, plant, table, nominal))
                loose.append(not exact)
            on = is_active(k, k0, L)
            _set_plant(plant, names, disturbed if on else nominal)
            want = G.controller(plant.obs(), K, policy)[0]
            got = actions[t, p]
            with np.errstate(invalid="ignore"):
                e = np.abs(got - want) / (1.0 + np.abs(want))
            e = np.where(np.isfinite(want), e, np.where(bits_equal(got, want), 0.0, np.inf))
            gap = max(gap, float(np.nanmax(e)))
            assert not np.isnan(e).any() and gap <= act_bar, f"[action] the recorded action is not the controller's output on the true observation {where}: step {t}, {float(np.nanmax(e)):.3g} (bar {act_bar:.3g}) at plants {np.flatnonzero(~(e <= act_bar))[:4].tolist()}"
            y, rew = plant.step(got + du if on else got)
            err = np.abs(outputs[t, p] - y)
            bar = np.full_like(y, PH_CELL) if kind == "ph" else WT_RTOL * (1.0 + np.abs(y))
            use_traj = max(use_traj, float((err / bar).max()))
            assert use_traj <= 1.0, f"[trajectory] the recorded outputs leave the oracle's replay of the recorded actions plus the row's disturbance {where}: step {t}, {use_traj:.3g} of the bar at plants {np.flatnonzero(err > bar)[:4].tolist()}"
            rews.append(rew); rs.append(plant.o.get("r"))
        rew, rs, y_start = np.stack(rews), np.stack(rs), np.stack(y_start)
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(outputs[:, p], rs, actions[:, p], rew, y_start, seg_len=seg_len, band=band, tail=tail)
        for j, name in enumerate(protocols.METRIC_NAMES):
            if name == "return":
                rtol = 2e-5 if kind == "ph" else WT_RTOL
                for s in range(S):
                    rs_ = rew[s * L0:(s + 1) * L0].astype(np.float32).astype(np.float64)
                    room = rtol * (len(rs_) + np.abs(rs_).sum(axis=0))
                    use_ret = max(use_ret, float((np.abs(pairs[s, j, p] - m[name][s]) / room).max()))
                assert use_ret <= 1.0, f"[metrics] the return row leaves the oracle's rewards {where}: {use_ret:.3g} of the bar"
            else:
                assert bits_equal(pairs[:, j, p], m[name]), f"[metrics] row {name} is not what metrics_from_records makes of the call's own actions and outputs {where}"
        want = rejection_rows(actions[:, p], outputs[:, p], rs, y_start, k0, seg_len, band)
        got = pairs[:, 8:, p]
        assert (np.isnan(got) == np.isnan(want)).all(), f"[nan] the rejection rows are not NaN exactly where the row never starts {where}: segments {np.flatnonzero((np.isnan(got) != np.isnan(want)).any(axis=(1, 2))).tolist()}"
        for s in range(S):
            if np.isnan(want[s]).all():
                continue
            for j, name in enumerate(protocols.DISTURB_ROW_NAMES):
                if name == "e0" and k0 == 0 and loose[s]:     # (y_start from the oracle: the trajectory bar)
                    room = PH_CELL if kind == "ph" else WT_RTOL * (1.0 + np.abs(y_start[s]))
                    assert (np.abs(got[s, j] - want[s, j]) <= room).all(), f"[rejection] row e0 leaves the oracle's start of segment {s} {where}"
                else:
                    assert bits_equal(got[s, j], want[s, j]), f"[rejection] row {name} of segment {s} is not what the window from the onset makes of the call's own actions and outputs {where}"
        if nominal_row is not None and p != nominal_row:
            first = n_steps if k0 is None else min(k0, n_steps)
            for k in ("actions", "outputs"):
                assert bits_equal(rec[k][:first, p], rec[k][:first, nominal_row]), f"[nominal] {k} before the first onset are not those of the nominal row {where}"
    return dict(trajectory=use_traj, ret=use_ret, action=gap / act_bar, gap=gap)


# ------------------------------------------------------------------------------------------------ host library
def host_lib():
    return P.load_host(HOST_LIB_PATH, HOST_EXPORTS[0],
                       [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                        C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], HOST_EXPORTS[1])


def host_raw(kind, cfg, lanes, N_, qww, qc, K, rows, Pn, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, outputs):
    """The raw call: returns (status, message)."""
    s, keep = (None, None) if lanes is None else P._lanes_struct(kind, lanes)
    rc = host_lib().pime_disturb_sweep_host(C.byref(cfg), None if s is None else C.byref(s), N_, P._p(qww), P._p(qc), P._p(K), P._p(rows), Pn,
                                            n_steps, seg_len, P._p(sp), n_sp, band, tail, P._p(pairs), P._p(summary), P._p(actions),
                                            P._p(outputs))
    del keep
    return rc, host_lib().pime_disturb_host_last_error().decode()


def host_disturb(kind, cfg, lanes, rows=None, K=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND, tail=TAIL, trace=True,
                 want_pairs=True):
    """The host build (the prior controller alone) from the lane state `lanes`, in the state precision cfg.state_mode names: dict
    summary [P, S, 15, 5], pairs [S, 15, P, N], actions, outputs [T, P, N]."""
    n = len(lanes["r"])
    K = np.ascontiguousarray(PRIOR_K[kind] if K is None else K, dtype=np.float64)
    rows = np.ascontiguousarray(DISTURB[kind] if rows is None else rows, dtype=np.float64)
    Pn, S = len(rows), n_segments(n_steps, seg_len)
    sp = np.ascontiguousarray(setpoints if setpoints is not None else SETPOINTS[kind], dtype=np.float64)
    summary = np.full((Pn, S, ROWS, 5), -777.0)
    pairs = np.full((S, ROWS, Pn, n), -777.0) if want_pairs else None
    actions, outputs = (np.full((n_steps, Pn, n), -777.0), np.full((n_steps, Pn, n), -777.0)) if trace else (None, None)
    qww, qc = (None, None) if kind == "wt" else (np.ascontiguousarray(lanes["qww_V"], dtype=np.float64),
                                                  np.ascontiguousarray(lanes["qc_V"], dtype=np.float64))
    rc, msg = host_raw(kind, cfg, lanes, n, qww, qc, K, rows, Pn, n_steps, seg_len, sp if seg_len > 0 else None,
                       len(sp) if seg_len > 0 else 0, band, tail, pairs, summary, actions, outputs)
    assert rc == 0, f"pime_disturb_sweep_host failed ({rc}): {msg}"
    return dict(summary=summary, pairs=pairs, actions=actions, outputs=outputs)


def twin_case(kind, n, table, state_mode="f64", noise=0.01, seed=SEED, offset=OFFSET):
    """(cfg, keep, lanes) as tests/mpc_eval.py builds them, at this module's lane offset; pH: with the stored qww_V and qc_V the
    plants were built from (the first two reset draws)."""
    cfg, keep, lanes = M.twin_case(kind, n, table, state_mode, noise=noise, seed=seed, offset=offset)
    if kind == "ph":
        draws = P.case_draws(kind, n, SETPOINTS[kind][0], seed=5)
        lanes["qww_V"], lanes["qc_V"] = np.ascontiguousarray(draws[:, 0]), np.ascontiguousarray(draws[:, 1])
    return cfg, keep, lanes
