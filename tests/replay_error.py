"""Checker of the fused replay of recorded runs (`pime_env_replay_error`, csrc/replay_error.hpp) and the ctypes binding of its host
build (libpime_replay_host.so, include/pime_replay_host.h).  Shared by tests/test_replay_error_cpu.py and
tests/test_gpu_replay_error.py.  TEST INFRASTRUCTURE: the pime_amd package never loads the host library.

Everything is float64 numpy around oracle.binding.OraclePH / OracleWT:
  * plants are placed by injected reset draws, with noise_scale 0 and a huge max_steps (no reset ever happens);
  * PREDICT is `set('h1' / 'h2', measured)` before each step;
  * the pH inverse lookup is np.searchsorted(-table, -y0, side="left"), clamped to the table.
`check_recording` holds one recording (err, sim) to it and raises `ReplayMismatch` with the NAME of the property that failed:
  sim     a simulated output differs from the oracle's by more than the bar: 1e-12 (1 + |ref|) with float64 state (the float64 bar
          of tests/rollout_replay.py); float32 tank levels 2e-5 (1 + |ref|) against ONE oracle step from the recording's own
          previous state (re-synchronised every step as rollout_replay.py does, so that rounding does not compound); pH in mixed
          mode must be the float32 rounding of the oracle's table cell exactly (x is float64 in both modes)
  sse0 / sse1 / max0 / max1 / count
          an error row is not BIT-equal to the numpy reduction of the recording's own sim, in the kernel's order
  nosim   err of the call without sim is not bit-equal to err of the call with it
`synthesize` builds a recording from the oracle alone, optionally with one named fault: the checker is vetted on those."""
import ctypes as C
import os

import numpy as np

from prior_sweep import load_host

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pime-robust-non-linear-set-point-control-with-reinforcement-learning_amd")
HOST_LIB_PATH = os.path.join(PKG, "libpime_replay_host.so")
HOST_EXPORTS = ("pime_replay_error_host", "pime_replay_host_last_error")
SSE0, MAX0, SSE1, MAX1, COUNT, ROWS = 0, 1, 2, 3, 4, 5
ROW_NAMES = ("sse0", "max0", "sse1", "max1", "count")
MODES = {"simulate": 0, "predict": 1}
BAR_F64, BAR_MIXED = 1e-12, 2e-5
TABLE_SCALE = 1e5
FAULTS = ("action_shift", "skip_off", "row_t", "h2_vs_h1", "noise_on", "predict_from_sim", "x0_other_C", "k0_off", "nan_counted",
          "max_last")
# registered ensemble ranges (gym_control/__init__.py: the defaults of pime_env_cfg_default) and the two 81-plant grids
WT_AXES = dict(a1=np.linspace(0.0015, 0.0024, 3), a2=np.linspace(0.0015, 0.0024, 3), Kp=np.linspace(0.07, 0.17, 9))
PH_AXES = dict(qww_V=np.linspace(0.005, 0.015, 9), qc_V=np.linspace(0.0015, 0.0025, 9))
WT_TRUE, PH_TRUE = (1, 2, 5), (3, 6)      # the grid points the identification records are generated from


class ReplayMismatch(AssertionError):
    def __init__(self, name, msg):
        super().__init__(f"[{name}] {msg}")
        self.name = name


def grid_plants(axes):
    """[n, P] plants of the Cartesian product in C order (lane = the C-order index, as protocols.robust_grid)."""
    mesh = np.meshgrid(*axes.values(), indexing="ij")
    return np.stack([m.reshape(-1) for m in mesh], axis=1)


def true_lane(kind):
    axes, idx = (PH_AXES, PH_TRUE) if kind == "ph" else (WT_AXES, WT_TRUE)
    return int(np.ravel_multi_index(idx, tuple(len(v) for v in axes.values())))


# ------------------------------------------------------------------------------------------------ host library
def host_lib():
    return load_host(HOST_LIB_PATH, HOST_EXPORTS[0],
                     [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32],
                     HOST_EXPORTS[1])


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_cfg(kind, n, table=None):
    """pime_env_cfg_default's configuration (libpime_hip.so fills the struct; no GPU call).  Returns (cfg, keep-alive)."""
    import pime_amd.native as nt
    cfg = nt.EnvCfg()
    nt.check(nt.lib().pime_env_cfg_default(nt.ENV_PH if kind == "ph" else nt.ENV_WT, C.byref(cfg)))
    cfg.n_envs, cfg.state_mode = int(n), nt.STATE_F64
    keep = None
    if kind == "ph":
        keep = np.ascontiguousarray(table, dtype=np.float64)
        cfg.ph_table = keep.ctypes.data_as(C.POINTER(C.c_double))
        cfg.ph_table_len = len(keep)
    return cfg, keep


def host_replay_raw(kind, plants, action, output, state0, E, T, mode, skip, err, sim, threads=1, table=None):
    """The raw call: returns (status, message)."""
    import pime_amd.native as nt
    plants = np.ascontiguousarray(plants, dtype=np.float64)
    cfg, keep = host_cfg(kind, len(plants), table)
    rec = nt.ReplayRecords(None if action is None else action.ctypes.data, None if output is None else output.ctypes.data,
                           None if state0 is None else state0.ctypes.data, E, T)
    rc = host_lib().pime_replay_error_host(C.byref(cfg), _p(plants), len(plants), C.byref(rec), mode, skip, _p(err), _p(sim), threads)
    del keep
    return rc, host_lib().pime_replay_host_last_error().decode()


def host_replay(kind, plants, rec, mode="simulate", skip=0, want_sim=True, threads=1, table=None):
    """(err [E, 5, N], sim [E, T, C, N] or None) of the host build."""
    act = np.ascontiguousarray(rec["action"], dtype=np.float64)
    out = np.ascontiguousarray(rec["output"], dtype=np.float64)
    st0 = None if rec.get("state0") is None else np.ascontiguousarray(rec["state0"], dtype=np.float64)
    E, T = act.shape
    N, Cn = len(plants), out.shape[2]
    err = np.full((E, ROWS, N), np.nan)
    sim = np.full((E, T, Cn, N), np.nan) if want_sim else None
    rc, msg = host_replay_raw(kind, plants, act, out, st0, E, T, MODES[mode], skip, err, sim, threads, table)
    assert rc == 0, f"pime_replay_error_host failed ({rc}): {msg}"
    return err, sim


# ------------------------------------------------------------------------------------------------ the oracle's replay
def ph_k0(table, y0):
    """The smallest index whose entry is <= y0 in the table's own precision, clamped to the table."""
    k = int(np.searchsorted(-table, -table.dtype.type(y0), side="left"))
    return min(k, len(table) - 1)


def oracle_sim(kind, plants, rec, mode="simulate", table=None, fault=None, resync=None, state32=False, round_steps=False):
    """sim [E, T, C, N]: the records replayed by the oracle.  resync: a recording's own sim -- the state before step t > 0 is taken
    from it (one oracle step per recorded step).  state32: measured states enter rounded to float32 (PIME_STATE_MIXED tank), the
    pH inverse lookup runs on the float32 table.  round_steps: the tank levels are rounded to float32 after every step and the run
    goes on from the rounded ones.  fault: one of FAULTS that acts on the simulation."""
    import oracle
    act, out, st0 = np.asarray(rec["action"], float), np.asarray(rec["output"], float), rec.get("state0")
    plants = np.asarray(plants, dtype=np.float64)
    E, T = act.shape
    N = len(plants)
    r32 = (lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)) if state32 else (lambda v: np.asarray(v, dtype=np.float64))
    a_of = lambda e, t: act[e, t - 1 if (fault == "action_shift" and t > 0) else t]
    if kind == "ph":
        ref = oracle.OraclePH(N, table, max_steps=2 ** 30, resample_every=1)
        search = table.astype(np.float32) if state32 else table
        sim = np.empty((E, T, 1, N))
        for e in range(E):
            ref.reset(draws=np.column_stack([plants[:, 0], plants[:, 1], np.zeros(N), np.full(N, 7.0)]))
            if st0 is not None:
                x0 = np.full(N, float(st0[e]))
            else:
                k0 = ph_k0(search, out[e, 0, 0]) + (1 if fault == "k0_off" else 0)
                Cq = ref.get("C")
                x0 = float(k0) / ((np.roll(Cq, 1) if fault == "x0_other_C" else Cq) * TABLE_SCALE)
            ref.set("x", x0)
            for t in range(T):
                sim[e, t, 0] = ref.step(np.full(N, a_of(e, t)))[1][:, 0]
        return sim
    ref = oracle.OracleWT(N, max_steps=2 ** 30, reward_type="distance", resample_every=1, noise_scale=0.01 if fault == "noise_on" else 0.0)
    sim = np.empty((E, T, 2, N))
    for e in range(E):
        h0 = r32(out[e, 0])
        ref.reset(draws=np.column_stack([plants, np.full(N, h0[0]), np.full(N, h0[1]), np.zeros(N)]))
        for t in range(T):
            if resync is not None and t > 0:
                ref.set("h1", resync[e, t - 1, 0]); ref.set("h2", resync[e, t - 1, 1])
            if mode == "predict" and fault != "predict_from_sim":
                for c, name in enumerate(("h1", "h2")):
                    if not np.isnan(out[e, t, c]):
                        ref.set(name, r32(out[e, t, c]))
            o64 = ref.step(np.full(N, a_of(e, t)), noise=None if fault == "noise_on" else np.zeros((N, 2)))[1]
            sim[e, t, 0], sim[e, t, 1] = o64[:, 0], o64[:, 1]
            if round_steps:
                sim[e, t] = sim[e, t].astype(np.float32).astype(np.float64)
                ref.set("h1", sim[e, t, 0]); ref.set("h2", sim[e, t, 1])
    return sim


def reduce_err(sim, output, skip, fault=None):
    """err [E, 5, N] from sim in the kernel's order: steps ascending, channel 0 before channel 1, each d * d rounded before it is
    added; a NaN measurement is no term.  fault: one of FAULTS that acts on the reduction."""
    E, T, Cn, N = sim.shape
    out = np.asarray(output, dtype=np.float64)
    err = np.zeros((E, ROWS, N))
    first = skip + 1 if fault == "skip_off" else skip
    for e in range(E):
        for t in range(first, T):
            for c in range(Cn):
                m = out[e, t if fault == "row_t" else t + 1, 0 if (fault == "h2_vs_h1" and c == 1) else c]
                if np.isnan(m) and fault != "nan_counted":
                    continue
                d = sim[e, t, c] - m
                ad = np.abs(d)
                err[e, 2 * c] = err[e, 2 * c] + d * d
                with np.errstate(invalid="ignore"):
                    err[e, 2 * c + 1] = ad if fault == "max_last" else np.where(ad > err[e, 2 * c + 1], ad, err[e, 2 * c + 1])
                err[e, COUNT] += 1.0
    return err


def synthesize(kind, plants, rec, mode="simulate", skip=0, table=None, fault=None, state32=False):
    """A recording (err, sim) built from the oracle alone.  state32: the tank levels are rounded to float32 after every step, as a
    float32 state would hold them (an honest PIME_STATE_MIXED recording, to the rounding of the arithmetic in between)."""
    sim = oracle_sim(kind, plants, rec, mode, table, fault, state32=state32, round_steps=state32)
    if state32:
        sim = sim.astype(np.float32).astype(np.float64)
    return reduce_err(sim, rec["output"], skip, fault), sim


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def check_recording(kind, plants, rec, mode, skip, err, sim, state_mode="f64", table=None, err_nosim=None, tag=""):
    """Holds one recording to the oracle (module docstring); returns {"sim": the largest used share of the sim bar}."""
    out = np.asarray(rec["output"], dtype=np.float64)
    mixed = state_mode == "mixed"
    E, T = np.asarray(rec["action"]).shape
    Cn = 1 if kind == "ph" else 2
    if sim.shape != (E, T, Cn, len(plants)) or err.shape != (E, ROWS, len(plants)):
        raise ReplayMismatch("shape", f"{tag}: sim {sim.shape}, err {err.shape}")
    if np.isnan(sim).any():
        raise ReplayMismatch("sim", f"{tag}: {int(np.isnan(sim).sum())} simulated outputs are NaN (unwritten?)")
    if kind == "ph":
        want = oracle_sim(kind, plants, rec, mode, table, state32=mixed)
        if mixed:   # x is float64 in both modes: the oracle's cell on every lane and step, read from the float32 table
            bad = sim != want.astype(np.float32).astype(np.float64)
            share = float(bad.any())
            if bad.any():
                raise ReplayMismatch("sim", f"{tag}: {int(bad.sum())} of {bad.size} pH outputs are not the oracle's titration cell")
        else:
            bar = BAR_F64 * (1.0 + np.abs(want))
            share = float((np.abs(sim - want) / bar).max())
    else:
        want = oracle_sim(kind, plants, rec, mode, table, resync=sim if mixed else None, state32=mixed)
        bar = (BAR_MIXED if mixed else BAR_F64) * (1.0 + np.abs(want))
        share = float((np.abs(sim - want) / bar).max())
    if not share <= 1.0:
        e, t, c, i = np.unravel_index(int(np.argmax(np.abs(sim - want))), sim.shape)
        raise ReplayMismatch("sim", f"{tag}: record {e} step {t} channel {c} lane {i}: {sim[e, t, c, i]!r} against the oracle's "
                                    f"{want[e, t, c, i]!r} ({share:.3g} of the bar)")
    ref = reduce_err(sim, out, skip)
    for row in (COUNT, SSE0, SSE1, MAX0, MAX1):
        if not _bits_equal(err[:, row], ref[:, row]):
            bad = np.argwhere(~((err[:, row] == ref[:, row]) | (np.isnan(err[:, row]) & np.isnan(ref[:, row]))))
            at = tuple(bad[0]) if len(bad) else (0, 0)
            raise ReplayMismatch(ROW_NAMES[row], f"{tag}: row {ROW_NAMES[row]} is not the reduction of the recording's own sim: record "
                                                 f"{at[0]} lane {at[1]}: {err[at[0], row, at[1]]!r} against {ref[at[0], row, at[1]]!r}")
    if err_nosim is not None and not _bits_equal(err_nosim, err):
        raise ReplayMismatch("nosim", f"{tag}: err of the call without sim differs from err of the call with it")
    return {"sim": share}


# ------------------------------------------------------------------------------------------------ records
def make_records(kind, plant, E, T, seed, table=None, gaps=0):
    """E records of T steps generated by the ORACLE from one plant: actions U(-1, 1), a random start, zero process noise.  gaps: that
    many measurement words after row 0 are replaced by NaN.  pH records carry state0 (drop the key for the hidden-x case)."""
    import oracle
    rs = np.random.RandomState(seed)
    act = rs.uniform(-1.0, 1.0, (E, T))
    plant = np.asarray(plant, dtype=np.float64).reshape(1, -1)
    if kind == "ph":
        x0 = rs.uniform(0.0, 50.0, E)
        ref = oracle.OraclePH(1, table, max_steps=2 ** 30, resample_every=1)
        out = np.empty((E, T + 1, 1))
        for e in range(E):
            ref.reset(draws=np.array([[plant[0, 0], plant[0, 1], x0[e], 7.0]]))
            out[e, 0, 0] = ref.get("y")[0]
            for t in range(T):
                out[e, t + 1, 0] = ref.step(act[e, t:t + 1])[1][0, 0]
        rec = dict(action=act, output=out, state0=x0)
    else:
        h0 = rs.uniform(0.0, 10.0, (E, 2))
        out = np.empty((E, T + 1, 2))
        out[:, 0] = h0
        sim = oracle_sim("wt", plant, dict(action=act, output=out), "simulate")
        out[:, 1:] = sim[:, :, :, 0]
        rec = dict(action=act, output=out)
    if gaps:
        flat = rec["output"][:, 1:].reshape(E, -1)
        for e in range(E):
            flat_e = flat[e].copy()
            flat_e[rs.choice(flat_e.size, gaps, replace=False)] = np.nan
            rec["output"][e, 1:] = flat_e.reshape(rec["output"][e, 1:].shape)
    return rec


def cost_of(err, weights=None):
    """cost[i] = sum_e sum_c SSE[e, c, i] / weights[c]^2 (what protocols.identify_plants returns)."""
    w = np.ones(2) if weights is None else np.asarray(weights, dtype=np.float64)
    return (err[:, SSE0] / w[0] ** 2 + err[:, SSE1] / w[1] ** 2).sum(axis=0)
