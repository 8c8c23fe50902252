"""Checker of the prior-gain sweep (`pime_prior_sweep`, csrc/prior_sweep.hpp) and the ctypes binding of its host build
(libpime_sweep_host.so, include/pime_sweep_host.h).  Shared by tests/test_prior_sweep_cpu.py and tests/test_gpu_prior_sweep.py.
TEST INFRASTRUCTURE: the pime_amd package never loads the host library.

  * `summary_from_pairs` restates the summary in numpy: which values count (the finite ones), the five stats, and the ORDER of the
    sum -- blocks of 64 consecutive plants, absent plants and uncounted values +0.0, inside a block the balanced pairwise tree over
    the index bits (level 0 adds elements 2j and 2j + 1, ...), the block sums added in ascending block order from block 0's sum.
  * `twin_pairs` is the reference loop: every gain row over the lanes of the CPU twin (oracle/twin.py: pime_env_step_cpu, one
    launch per step), the set-point boundaries as injected resets (plant and plant state kept, r set, I and t zeroed, a new
    episode beyond the first), a_env summed in numpy in ascending j, the records reduced by protocols.metrics_from_records.
Both take one named fault (FAULTS): the checkers `check_summary` / `check_pairs` are vetted on those."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pime-robust-non-linear-set-point-control-with-reinforcement-learning_amd")
HOST_LIB_PATH = os.path.join(PKG, "libpime_sweep_host.so")
HOST_EXPORTS = ("pime_prior_sweep_host", "pime_sweep_host_last_error")
SUM, MIN, MAX, ARGMAX, FINITE, STATS = 0, 1, 2, 3, 4, 5
STAT_NAMES = ("sum", "min", "max", "argmax", "finite")
ROWS = 8
BLOCK = 64
FAULTS = ("plain_sum", "blocks32", "argmax_last", "nan_counted", "noise_pair")
TABLE_SCALE = 1e5
SETPOINTS = {"ph": (10.0, 6.0, 3.0), "wt": (3.0, 6.0, 9.0)}
PRIOR_K = {"ph": np.array([0.02, -0.02, -0.035]), "wt": np.array([0.0, -0.4, 0.4, 0.0])}   # -K of the env classes


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def gain_rows(kind):
    """The G = 3 rows of the tests: the env's own -K, the same scaled by 1.7, and one with the error gain's sign flipped (the
    components on the controlled output and the set-point)."""
    k = PRIOR_K[kind]
    flipped = k.copy()
    flipped[[0, 1] if kind == "ph" else [1, 2]] *= -1.0
    return np.ascontiguousarray(np.stack([k, 1.7 * k, flipped]))


def n_segments(n_steps, seg_len):
    return -(-n_steps // seg_len) if seg_len > 0 else 1


# ------------------------------------------------------------------------------------------------ the summary in numpy
def summary_from_pairs(pairs, fault=None):
    """pairs float64 [n_segments, 8, G, N] -> summary float64 [G, n_segments, 8, 5], bit for bit what pime_prior_sweep writes."""
    x = np.ascontiguousarray(np.moveaxis(np.asarray(pairs, dtype=np.float64), 2, 0))      # [G, S, R, N]
    N = x.shape[-1]
    counted = np.isfinite(x)
    if fault == "nan_counted":
        counted = counted | np.isnan(x)
    out = np.empty(x.shape[:-1] + (STATS,))
    block = 32 if fault == "blocks32" else BLOCK
    nb = -(-N // block)
    w = np.zeros(x.shape[:-1] + (nb * block,))
    w[..., :N] = np.where(counted, x, 0.0)
    if fault == "plain_sum":
        total = np.cumsum(w, axis=-1)[..., -1]                      # sequential, ascending
    else:
        w = w.reshape(x.shape[:-1] + (nb, block))
        while w.shape[-1] > 1:
            w = w[..., 0::2] + w[..., 1::2]
        sums = w[..., 0]
        total = sums[..., 0].copy()
        for b in range(1, nb):
            total = total + sums[..., b]
    lo = np.where(counted, x, np.inf)
    hi = np.where(counted, x, -np.inf)
    out[..., SUM] = total
    out[..., MIN] = lo.min(axis=-1)
    out[..., MAX] = hi.max(axis=-1)
    arg = np.argmax(hi, axis=-1) if fault != "argmax_last" else N - 1 - np.argmax(hi[..., ::-1], axis=-1)
    out[..., ARGMAX] = np.where(counted.any(axis=-1), arg, -1)
    out[..., FINITE] = counted.sum(axis=-1)
    return out


def check_summary(summary, pairs, tag=""):
    want = summary_from_pairs(pairs)
    for j, name in sorted(enumerate(STAT_NAMES), reverse=True):   # what counts first, the order of the sum last
        assert bits_equal(summary[..., j], want[..., j]), f"[{name}] summary differs from the numpy restatement of the call's own pairs {tag}"


def check_pairs(pairs, want, tag=""):
    assert bits_equal(pairs, want), f"[pairs] differ from the reference loop {tag}: {np.argwhere(pairs.view(np.uint64) != want.view(np.uint64))[:4]}"


# ------------------------------------------------------------------------------------------------ the reference loop
def case_draws(kind, N, sp0, seed=5):
    """Injected reset draws [N, 4 | 6] of a case: plants spread over the registered ensemble ranges, a plant state, r = sp0."""
    rng = np.random.default_rng(seed)
    if kind == "ph":
        return np.column_stack([rng.uniform(0.005, 0.015, N), rng.uniform(0.0015, 0.0025, N), rng.uniform(5.0, 40.0, N), np.full(N, sp0)])
    return np.column_stack([rng.uniform(0.0015, 0.0024, N), rng.uniform(0.0015, 0.0024, N), rng.uniform(0.07, 0.17, N),
                            rng.uniform(1.0, 8.0, N), rng.uniform(1.0, 8.0, N), np.full(N, sp0)])


def make_twin(kind, N, table, seed, env_offset, cfg_over, draws):
    from oracle.twin import TwinEnv
    env = TwinEnv(kind, N, table=table, seed=seed, env_offset=env_offset, resample_every=1, **cfg_over)
    env.reset(draws=draws)
    return env


def twin_lanes(env):
    """The lane state of a twin as the host build takes it."""
    names = ("x", "A", "B", "C", "r", "I", "t", "episode") if env.kind == "ph" else ("h1", "h2", "a1", "a2", "Kp", "r", "I", "t", "episode")
    out = {k: np.ascontiguousarray(env.get(k)) for k in names}
    out["t"], out["episode"] = out["t"].astype(np.int32), out["episode"].astype(np.int32)
    return out


def _ph_y(table, C_, x):
    k = np.clip(np.rint(C_ * x * TABLE_SCALE), 0, len(table) - 1).astype(np.int64)
    return table[k]


def twin_pairs(kind, N, gains, n_steps, seg_len, setpoints, band, tail, table=None, seed=3, env_offset=0, cfg_over=None, draws=None,
               fault=None):
    """pairs [n_segments, 8, G, N] by the reference loop.  fault "noise_pair": the process noise keyed on the pair index."""
    from pime_amd import protocols
    cfg_over = dict(cfg_over or {})
    gains = np.asarray(gains, dtype=np.float64)
    G, S = len(gains), n_segments(n_steps, seg_len)
    sp = list(setpoints)
    draws = case_draws(kind, N, sp[0]) if draws is None else draws
    out = np.empty((S, ROWS, G, N))
    for g in range(G):
        offset = env_offset + (g * N if fault == "noise_pair" else 0)
        env = make_twin(kind, N, table, seed, offset, cfg_over, draws)
        plant = draws[:, :2] if kind == "ph" else draws[:, :3]
        state = (lambda: env.get("x")[:, None]) if kind == "ph" else (lambda: np.column_stack([env.get("h1"), env.get("h2")]))
        out_y = (lambda: _ph_y(env._table, env.get("C"), env.get("x"))) if kind == "ph" else (lambda: env.get("h2"))
        obs = np.column_stack([out_y(), env.get("r"), env.get("I")]).astype(np.float32) if kind == "ph" else \
            np.column_stack([env.get("h1"), env.get("h2"), env.get("r"), env.get("I")]).astype(np.float32)
        ys, rs, acts, rews, y_start = [], [], [], [], []
        for t in range(n_steps):
            if seg_len > 0 and t % seg_len == 0 and t > 0:   # (the boundary at t = 0 is the injected reset the case starts from)
                obs = env.reset(draws=np.column_stack([plant, state(), np.full(N, sp[t // seg_len])]))
            if t % (seg_len if seg_len > 0 else n_steps) == 0:
                y_start.append(out_y())
            a = np.zeros(N)
            for j in range(obs.shape[1]):
                a = a + obs[:, j].astype(np.float64) * gains[g, j]
            obs, rew, _ = env.step(a, auto_reset=False)
            ys.append(out_y()); rs.append(env.get("r")); acts.append(a); rews.append(rew)
        env.close()
        with np.errstate(invalid="ignore"):
            m = protocols.metrics_from_records(np.stack(ys), np.stack(rs), np.stack(acts), np.stack(rews), np.stack(y_start),
                                               seg_len=seg_len, band=band, tail=tail)
        for j, name in enumerate(protocols.METRIC_NAMES):
            out[:, j, g] = m[name]
    return out


# ------------------------------------------------------------------------------------------------ host library
class SweepLanes(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ph_x", "ph_A", "ph_B", "ph_C", "ph_last_a", "wt_h1", "wt_h2", "wt_a1", "wt_a2", "wt_kp",
                                          "r", "I", "t", "episode")]


_hosts = {}


def load_host(path, entry, argtypes, last_error):
    """The host library at `path`, loaded once (also for mpc_eval, margin_sweep and replay_error): `entry` takes `argtypes` and
    returns int, `last_error` returns the message of its last failure."""
    if path not in _hosts:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C {PKG}/csrc` (or __graft_entry__.build())")
        h = C.CDLL(path)
        getattr(h, entry).restype = C.c_int
        getattr(h, entry).argtypes = argtypes
        getattr(h, last_error).restype = C.c_char_p
        _hosts[path] = h
    return _hosts[path]


def host_lib():
    return load_host(HOST_LIB_PATH, HOST_EXPORTS[0],
                     [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                      C.c_int32, C.c_void_p, C.c_void_p], HOST_EXPORTS[1])


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_cfg(kind, n, table=None, seed=3, env_offset=0, **over):
    """pime_env_cfg_default's configuration (libpime_hip.so fills the struct; no GPU call), as oracle.twin.TwinEnv overrides it."""
    import pime_amd.native as nt
    cfg = nt.EnvCfg()
    nt.check(nt.lib().pime_env_cfg_default(nt.ENV_PH if kind == "ph" else nt.ENV_WT, C.byref(cfg)))
    cfg.n_envs, cfg.state_mode, cfg.seed, cfg.env_offset = int(n), nt.STATE_F64, seed, env_offset
    for k, v in over.items():
        setattr(cfg, k, v)
    keep = None
    if kind == "ph":
        keep = np.ascontiguousarray(table, dtype=np.float64)
        cfg.ph_table = keep.ctypes.data_as(C.POINTER(C.c_double))
        cfg.ph_table_len = len(keep)
    return cfg, keep


def _lanes_struct(kind, lanes):
    f = {k: np.ascontiguousarray(v) for k, v in lanes.items()}
    g = lambda k: None if k not in f else f[k].ctypes.data
    if kind == "ph":
        s = SweepLanes(g("x"), g("A"), g("B"), g("C"), None, None, None, None, None, None, g("r"), g("I"), g("t"), g("episode"))
    else:
        s = SweepLanes(None, None, None, None, None, g("h1"), g("h2"), g("a1"), g("a2"), g("Kp"), g("r"), g("I"), g("t"), g("episode"))
    return s, f


def host_sweep_raw(kind, cfg, lanes, N, gains, G, n_steps, seg_len, setpoints, n_setpoints, band, tail, pairs, summary):
    """The raw call: returns (status, message)."""
    s, keep = (None, None) if lanes is None else _lanes_struct(kind, lanes)
    rc = host_lib().pime_prior_sweep_host(C.byref(cfg), None if s is None else C.byref(s), N, _p(gains), G, n_steps, seg_len,
                                          _p(setpoints), n_setpoints, band, tail, _p(pairs), _p(summary))
    del keep
    return rc, host_lib().pime_sweep_host_last_error().decode()


def host_sweep(kind, lanes, gains, n_steps, seg_len, setpoints, band, tail, want_pairs=True, table=None, seed=3, env_offset=0,
               cfg_over=None):
    """(summary [G, S, 8, 5], pairs [S, 8, G, N] or None) of the host build, from the lane state `lanes` (twin_lanes)."""
    gains = np.ascontiguousarray(gains, dtype=np.float64)
    N, G, S = len(lanes["r"]), len(gains), n_segments(n_steps, seg_len)
    cfg, keep = host_cfg(kind, N, table, seed, env_offset, **(cfg_over or {}))
    sp = np.ascontiguousarray(setpoints, dtype=np.float64)
    summary = np.full((G, S, ROWS, STATS), -777.0)
    pairs = np.full((S, ROWS, G, N), -777.0) if want_pairs else None
    rc, msg = host_sweep_raw(kind, cfg, lanes, N, gains, G, n_steps, seg_len, sp if seg_len > 0 else None, len(sp) if seg_len > 0 else 0,
                             band, tail, pairs, summary)
    del keep
    assert rc == 0, f"pime_prior_sweep_host failed ({rc}): {msg}"
    return summary, pairs
