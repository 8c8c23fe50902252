"""Checker of the frequency-response sweep (`pime_freq_sweep`, csrc/freq_sweep.hpp) and the ctypes binding of its host build
(libpime_freq_host.so, include/pime_freq_host.h).  Shared by tests/test_freq_sweep_cpu.py and tests/test_gpu_freq_sweep.py.
TEST INFRASTRUCTURE: the pime_amd package never loads the host library.

`check_recording` takes what a call left -- actions (the CONTROLLER's outputs a_c), outputs [T, P, N] and pairs [S, 16, P, N] -- the
rows, the table and the lane state it started from, and replays EVERY pair open-loop through the float64 oracle (OraclePH / OracleWT,
tests/mpc_eval.py: Plant) with the excitation e_k = A * wave[p, k, 1] of the step WITHIN the segment injected at the row's point: the
oracle's set-point word is sp + e_k (SETPOINT), the oracle is fed a_c + e_k (LOAD), or the controller is evaluated on the oracle's
observation with e_k added to the controlled output's column (MEASUREMENT).  No pair, step or row is left out:
  [action]     every recorded a_c is the float64 controller output -- the prior term summed in ascending j, plus the policy's tanh term
               -- on the (excited) observation of that step, within tests/margin_sweep.py's ACT_BAR * (1 + |wanted|);
  [trajectory] the oracle reproduces the recorded outputs at the bars of tests/rollout_replay.py: pH within 1e-5 (the same titration
               cell), tank within 2e-4 * (1 + |y|);
  [metrics]    protocols.metrics_from_records of the recorded (a_c, outputs) with the segment's NOMINAL set-point gives seven of the
               first eight rows of `pairs` bit for bit; the return row is held to the oracle's rewards at the trajectory bar;
  [nan]        the eight lock-in rows are NaN exactly in the segments that never reach the onset;
  [lockin]     `lockin_rows` of the recorded traces -- a sequential numpy restatement of the window sums -- gives the eight lock-in rows
               bit for bit;
  [nominal]    a row with A == 0 leaves the actions and outputs of the nominal row, bit for bit.
`numpy_loop` is a restatement of the whole loop in closed loop on the oracle; it takes one named fault (FAULTS) and the checker is
vetted on those."""
import ctypes as C
import os

import numpy as np

import margin_sweep as G
import mpc_eval as M
import prior_sweep as P

HOST_LIB_PATH = os.path.join(P.PKG, "libpime_freq_host.so")
HOST_EXPORTS = ("pime_freq_sweep_host", "pime_freq_host_last_error")
FAULTS = ("window_early", "window_late", "table_by_launch_step", "neighbour_table", "cs_swapped", "amplitude_on_reference",
          "load_behind_clip", "setpoint_not_integrated", "measure_h1", "measure_into_integrator", "a_env_recorded", "finite_for_nan")
# the shapes of the CPU tests: 81 plants at a lane offset, 23 steps in segments of 9 (the last one ragged: 5 steps), tail 4
N, OFFSET, SEED = G.N, G.OFFSET, G.SEED
N_STEPS, SEG, TAIL, BAND = 23, 9, 4, 0.05
SETPOINTS = P.SETPOINTS
PRIOR_K = P.PRIOR_K
PH_CELL, WT_RTOL = M.PH_CELL, M.WT_RTOL          # tests/rollout_replay.py
ACT_BAR = G.ACT_BAR                              # tests/margin_sweep.py
COLS, ROWS, FROWS = 3, 16, 8
YC, YS, UC, US, Y0, U0, Y2, U2 = range(8, 16)
SETPOINT, LOAD, MEASUREMENT = 0, 1, 2
MAX_STEPS = 2 ** 30


def sinusoids(cycles, onsets, seg_len):
    """wave [P, seg_len, 2]: c_k = cos(2 pi m (k - k0) / W), s_k = sin(...), W = seg_len - k0 (numpy, independent of protocols)."""
    out = np.zeros((len(cycles), seg_len, 2))
    for p, (m, k0) in enumerate(zip(cycles, onsets)):
        k0 = min(int(k0), seg_len - 1)
        th = 2.0 * np.pi * m * (np.arange(seg_len) - k0) / (seg_len - k0)
        out[p, :, 0], out[p, :, 1] = np.cos(th), np.sin(th)
    return out


# columns (POINT, A, k0): nominal; set-point, 1 cycle in the window of 5 (s_0 != 0); load, 2 cycles; measurement, 1 cycle; load with an onset beyond
# the ragged segment (NaN there); nominal amplitude on a MEASUREMENT row with a late onset; set-point from the first step
EXCITE = np.array([(0, 0.0, 3), (0, 0.5, 4), (1, 0.3, 3), (2, 0.2, 3), (1, -0.25, 6), (2, 0.0, 7), (0, 0.4, 0)], dtype=np.float64)
WAVE = sinusoids((1, 1, 2, 1, 1, 1, 2), EXCITE[:, 2], SEG)


def bits_equal(a, b):
    return P.bits_equal(a, b)


def n_segments(n_steps, seg_len):
    return P.n_segments(n_steps, seg_len)


def decode_row(row):
    """(point, A, k0) as pime_freq_sweep reads a row: point rint clamped into 0 .. 2 (NaN: 0); k0 rint clamped into 0 .. 2^30 (NaN:
    never, None)."""
    pt, k0 = np.rint(row[0]), np.rint(row[2])
    pt = 0 if not pt >= 0 else int(min(pt, 2))
    k0 = None if np.isnan(k0) else int(min(max(k0, 0), MAX_STEPS))
    return pt, float(row[1]), k0


def out_col(kind):
    return 0 if kind == "ph" else 1


def _lockin(actions, outputs, cs, L0, k0, fault=None):
    """lockin_rows with the table given per LAUNCH step: cs [T, 2]."""
    T, n = outputs.shape
    S = -(-T // L0)
    out = np.full((S, FROWS, n), np.nan)
    for s in range(S):
        lo, hi = s * L0, min((s + 1) * L0, T)
        if k0 is None or k0 >= hi - lo:
            if fault == "finite_for_nan":
                out[s] = 0.0
            continue
        first = k0 - 1 if fault == "window_early" and k0 > 0 else k0 + 1 if fault == "window_late" else k0
        acc = [np.zeros(n) for _ in range(FROWS)]
        for k in range(first, hi - lo):
            y, u, c, sn = outputs[lo + k], actions[lo + k], cs[lo + k, 0], cs[lo + k, 1]
            for j, term in enumerate((y * c, y * sn, u * c, u * sn, y, u, y * y, u * u)):
                acc[j] = acc[j] + term
        out[s] = np.stack(acc)
    return out


def lockin_rows(actions, outputs, wave, k0):
    """The eight lock-in rows [S, 8, N] from a pair's traces: actions (a_c) and outputs [T, N], the row's table wave [L, 2] (L is the
    segment length: the table restarts with every segment), the onset k0 (None: never).  Sequential from 0.0 in ascending k, each
    product rounded before it is added, as csrc/freq_sweep.hpp's FreqMetrics accumulates them."""
    T, L0 = outputs.shape[0], wave.shape[0]
    return _lockin(actions, outputs, np.tile(wave, (-(-T // L0), 1))[:T], L0, k0)


def _segment_setpoint(sp, lanes, seg_len, t):
    return float(sp[t // seg_len]) if seg_len > 0 else np.asarray(lanes["r"], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the restatement in closed loop
def numpy_loop(kind, cfg, lanes, table, rows=None, wave=None, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND,
               tail=TAIL, fault=None):
    """The loop of include/pime_hip.h in numpy on the oracle as the plant (float64 state).  policy: None or an object with
    term(obs, dtype).  Returns dict actions (a_c), outputs [T, P, N], pairs [S, 16, P, N]."""
    from pime_amd import protocols
    assert fault is None or fault in FAULTS
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    rows = np.asarray(EXCITE if rows is None else rows, dtype=np.float64)
    wave = np.asarray(WAVE if wave is None else wave, dtype=np.float64)
    n, Pn, S = len(lanes["r"]), len(rows), n_segments(n_steps, seg_len)
    L0 = seg_len if seg_len > 0 else n_steps
    assert wave.shape == (Pn, L0, 2)
    flat = wave.reshape(Pn * L0, 2)
    pol = None if policy is None else policy.term
    col, sp_col = out_col(kind), (1 if kind == "ph" else 2)
    actions, outputs, pairs = np.zeros((n_steps, Pn, n)), np.zeros((n_steps, Pn, n)), np.zeros((S, ROWS, Pn, n))
    for p in range(Pn):
        pt, A, k0 = decode_row(rows[p])
        w = wave[(p + 1) % Pn] if fault == "neighbour_table" else wave[p]
        if fault == "cs_swapped":
            w = w[:, ::-1]
        if fault == "table_by_launch_step":                 # wave[2 * t] runs on into the next row's table
            w_of = lambda t, k: flat[(p * L0 + t) % (Pn * L0)]
        else:
            w_of = lambda t, k: w[k]
        plant = M.Plant(kind, cfg, lanes, table)
        cmds, ys, rews, rs, y_start, used = [], [], [], [], [], []
        for t in range(n_steps):
            k = t % L0
            if seg_len > 0 and t % seg_len == 0:
                plant.boundary(sp[t // seg_len], t > 0)
            r_nom = _segment_setpoint(sp, lanes, seg_len, t)
            if k == 0:
                y_start.append(plant.y())
            c, sn = w_of(t, k)
            used.append((c, sn))
            e = A * sn
            on = A != 0.0
            if on and pt == SETPOINT and fault != "setpoint_not_integrated":
                plant.o.set("r", r_nom + e)
            om = plant.obs().astype(np.float32)
            if on and pt == SETPOINT and fault == "setpoint_not_integrated":
                om[:, sp_col] = (r_nom + e) * np.ones(n, dtype=np.float64)
            if on and pt == MEASUREMENT:
                mc = 0 if fault == "measure_h1" else col
                om[:, mc] = om[:, mc] + np.float32(e)
            a_c = G.controller(om, K, pol)[0]
            a_env = a_c + e if on and pt == LOAD else a_c
            if fault == "load_behind_clip" and on and pt == LOAD:
                a_env = np.clip(a_c, -1.0, 1.0) + e
            y, rew = plant.step(a_env)
            if fault == "measure_into_integrator" and on and pt == MEASUREMENT:
                plant.o.set("I", plant.o.get("I") - e)
            cmds.append(a_env if fault == "a_env_recorded" else a_c); ys.append(y); rews.append(rew)
            rs.append((r_nom + e if fault == "amplitude_on_reference" and on and pt == SETPOINT else r_nom) * np.ones(n))
        cmds, ys, rs, y_start = np.stack(cmds), np.stack(ys), np.stack(rs), np.stack(y_start)
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(ys, rs, cmds, np.stack(rews), y_start, seg_len=seg_len, band=band, tail=tail)
        actions[:, p], outputs[:, p] = cmds, ys
        for j, name in enumerate(protocols.METRIC_NAMES):
            pairs[:, j, p] = m[name]
        lock = _lockin(cmds, ys, np.array(used), L0, k0, fault=fault)     # the kernel correlates with the pairs it excited with
        pairs[:, 8:, p] = lock
    return dict(actions=actions, outputs=outputs, pairs=pairs)


# ------------------------------------------------------------------------------------------------ the checker
def check_recording(kind, cfg, lanes, table, rec, rows=None, wave=None, K=None, policy=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None,
                    band=BAND, tail=TAIL, act_bar=ACT_BAR, nominal_row=0, only=None, tag=""):
    """rec: dict with actions, outputs [T, P, N] and pairs [S, 16, P, N] of one call from the lane state `lanes`.  policy: None or a
    callable obs float64 [N, D] -> the float64 tanh term [N].  nominal_row: a row with A == 0 every other such row is compared with
    (None: skip).  only: the rows to check (None: every row).  Returns the share of each bar the recording uses: dict trajectory / ret /
    action, and `gap`."""
    from pime_amd import protocols
    K = PRIOR_K[kind] if K is None else np.asarray(K, dtype=np.float64).reshape(-1)
    sp = list(setpoints if setpoints is not None else SETPOINTS[kind])
    rows = np.asarray(EXCITE if rows is None else rows, dtype=np.float64)
    wave = np.asarray(WAVE if wave is None else wave, dtype=np.float64)
    actions, outputs, pairs = (np.asarray(rec[k], dtype=np.float64) for k in ("actions", "outputs", "pairs"))
    n, Pn, S = len(lanes["r"]), len(rows), n_segments(n_steps, seg_len)
    L0 = seg_len if seg_len > 0 else n_steps
    assert wave.shape == (Pn, L0, 2), wave.shape
    assert actions.shape == outputs.shape == (n_steps, Pn, n) and pairs.shape == (S, ROWS, Pn, n), (actions.shape, pairs.shape)
    col = out_col(kind)
    use_traj = use_ret = gap = 0.0
    for p in (range(Pn) if only is None else only):
        pt, A, k0 = decode_row(rows[p])
        where = f"{tag} row {p} {rows[p].tolist()}"
        on = A != 0.0
        plant = M.Plant(kind, cfg, lanes, table)
        rews, rs, y_start = [], [], []
        for t in range(n_steps):
            k = t % L0
            if seg_len > 0 and t % seg_len == 0:
                plant.boundary(sp[t // seg_len], t > 0)
            r_nom = _segment_setpoint(sp, lanes, seg_len, t)
            if k == 0:
                y_start.append(plant.y())
            e = A * wave[p, k, 1]
            if on and pt == SETPOINT:
                plant.o.set("r", r_nom + e)
            om = plant.obs()
            if on and pt == MEASUREMENT:
                om[:, col] = om[:, col] + e
            want = G.controller(om, K, policy)[0]
            got = actions[t, p]
            with np.errstate(invalid="ignore"):
                err = np.abs(got - want) / (1.0 + np.abs(want))
            err = np.where(np.isfinite(want), err, np.where(bits_equal(got, want), 0.0, np.inf))
            gap = max(gap, float(np.nanmax(err)))
            assert not np.isnan(err).any() and gap <= act_bar, f"[action] the recorded action is not the controller's output on the observation the row's excitation leaves {where}: step {t}, {float(np.nanmax(err)):.3g} (bar {act_bar:.3g}) at plants {np.flatnonzero(~(err <= act_bar))[:4].tolist()}"
            y, rew = plant.step(got + e if on and pt == LOAD else got)
            err = np.abs(outputs[t, p] - y)
            bar = np.full_like(y, PH_CELL) if kind == "ph" else WT_RTOL * (1.0 + np.abs(y))
            use_traj = max(use_traj, float((err / bar).max()))
            assert use_traj <= 1.0, f"[trajectory] the recorded outputs leave the oracle's replay of the recorded actions under the row's excitation {where}: step {t}, {use_traj:.3g} of the bar at plants {np.flatnonzero(err > bar)[:4].tolist()}"
            rews.append(rew); rs.append(r_nom * np.ones(n))
        rew = np.stack(rews)
        with np.errstate(invalid="ignore", over="ignore"):
            m = protocols.metrics_from_records(outputs[:, p], np.stack(rs), actions[:, p], rew,
                                               M.y_start_recorded(outputs[:, p], np.stack(y_start), seg_len), seg_len=seg_len, band=band, tail=tail)
        for j, name in enumerate(protocols.METRIC_NAMES):
            if name == "return":
                rtol = 2e-5 if kind == "ph" else WT_RTOL
                for s in range(S):
                    rs_ = rew[s * L0:(s + 1) * L0].astype(np.float32).astype(np.float64)
                    room = rtol * (len(rs_) + np.abs(rs_).sum(axis=0))
                    use_ret = max(use_ret, float((np.abs(pairs[s, j, p] - m[name][s]) / room).max()))
                assert use_ret <= 1.0, f"[metrics] the return row leaves the oracle's rewards {where}: {use_ret:.3g} of the bar"
            else:
                assert bits_equal(pairs[:, j, p], m[name]), f"[metrics] row {name} is not what metrics_from_records makes of the call's own actions and outputs against the nominal set-point {where}"
        want = lockin_rows(actions[:, p], outputs[:, p], wave[p], k0)
        got = pairs[:, 8:, p]
        assert (np.isnan(got) == np.isnan(want)).all(), f"[nan] the lock-in rows are not NaN exactly where the segment never reaches the onset {where}: segments {np.flatnonzero((np.isnan(got) != np.isnan(want)).any(axis=(1, 2))).tolist()}"
        for j, name in enumerate(protocols.FREQ_ROW_NAMES):
            assert bits_equal(got[:, j], want[:, j]), f"[lockin] row {name} is not what the window from the onset makes of the call's own actions and outputs and the row's table {where}"
        if nominal_row is not None and p != nominal_row and not on:
            for key in ("actions", "outputs"):
                assert bits_equal(rec[key][:, p], rec[key][:, nominal_row]), f"[nominal] {key} of a row with zero amplitude are not those of the nominal row {where}"
    return dict(trajectory=use_traj, ret=use_ret, action=gap / act_bar, gap=gap)


# ------------------------------------------------------------------------------------------------ host library
def host_lib():
    return P.load_host(HOST_LIB_PATH, HOST_EXPORTS[0],
                       [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                        C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], HOST_EXPORTS[1])


def host_raw(kind, cfg, lanes, N_, K, rows, wave, wave_len, Pn, n_steps, seg_len, sp, n_sp, band, tail, pairs, summary, actions, outputs):
    """The raw call: returns (status, message)."""
    s, keep = (None, None) if lanes is None else P._lanes_struct(kind, lanes)
    rc = host_lib().pime_freq_sweep_host(C.byref(cfg), None if s is None else C.byref(s), N_, P._p(K), P._p(rows), P._p(wave), wave_len, Pn,
                                         n_steps, seg_len, P._p(sp), n_sp, band, tail, P._p(pairs), P._p(summary), P._p(actions),
                                         P._p(outputs))
    del keep
    return rc, host_lib().pime_freq_host_last_error().decode()


def host_freq(kind, cfg, lanes, rows=None, wave=None, K=None, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND, tail=TAIL, trace=True,
              want_pairs=True):
    """The host build (the prior controller alone) from the lane state `lanes`, in the state precision cfg.state_mode names: dict
    summary [P, S, 16, 5], pairs [S, 16, P, N], actions, outputs [T, P, N]."""
    n = len(lanes["r"])
    K = np.ascontiguousarray(PRIOR_K[kind] if K is None else K, dtype=np.float64)
    rows = np.ascontiguousarray(EXCITE if rows is None else rows, dtype=np.float64)
    wave = np.ascontiguousarray(WAVE if wave is None else wave, dtype=np.float64)
    Pn, S = len(rows), n_segments(n_steps, seg_len)
    assert wave.shape == (Pn, seg_len if seg_len > 0 else n_steps, 2)
    sp = np.ascontiguousarray(setpoints if setpoints is not None else SETPOINTS[kind], dtype=np.float64)
    summary = np.full((Pn, S, ROWS, 5), -777.0)
    pairs = np.full((S, ROWS, Pn, n), -777.0) if want_pairs else None
    actions, outputs = (np.full((n_steps, Pn, n), -777.0), np.full((n_steps, Pn, n), -777.0)) if trace else (None, None)
    rc, msg = host_raw(kind, cfg, lanes, n, K, rows, wave, wave.shape[1], Pn, n_steps, seg_len, sp if seg_len > 0 else None,
                       len(sp) if seg_len > 0 else 0, band, tail, pairs, summary, actions, outputs)
    assert rc == 0, f"pime_freq_sweep_host failed ({rc}): {msg}"
    return dict(summary=summary, pairs=pairs, actions=actions, outputs=outputs)


def twin_case(kind, n, table, state_mode="f64", noise=0.01, seed=SEED, offset=OFFSET):
    """(cfg, keep, lanes) as tests/mpc_eval.py builds them, at this module's lane offset."""
    return M.twin_case(kind, n, table, state_mode, noise=noise, seed=seed, offset=offset)
