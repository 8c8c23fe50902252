"""Every instantiation of the env step / reset / observe kernels (csrc/env_kernels.hip) against the float64 oracle: the case table, the
scripted scenario that drives a device through it, and the checker.  tests/test_env_cases_cpu.py vets all three without a GPU (on a numpy
`FakeDevice`, on the product's host build, and by mutation); tests/test_gpu_env_sweep.py runs the table on the device.

A *device* is anything with
    N, D, half, has_head                           lanes, observation width, binary16 rows?, is the ring head readable?
    new_buf(shape, kind)                           kind "obs" / "reward" (the entry form's row type), "observe" (float32), "done" (uint8)
    reset(mask, out)                               mask None or uint8 [N]
    step(action, residual, auto_reset, out_obs, out_reward, out_done)
                                                   action float32 / float64 [N]; residual None or (obs_in rows, priorK float64 [D])
    observe(out)
    field(name) -> float64 [N]
and a buffer is a `HostBuf` (or the GPU test's twin of it): `rows` is what a launch writes, `host()` the whole allocation with its guard.

The scenario (`run_scenario`), max_step 7, resample_every 2, in-kernel Philox draws, a non-zero env_offset:
    1  reset all lanes                              5  observe() into a fresh buffer
    2  five steps, auto_reset off                   6  one step, auto_reset off: group B's episode ends and is NOT reset
    3  masked reset of group A (lane 0 in, lane N - 1 out): from here A and B are out of lock-step, their ring heads differ
    4  n_auto steps, auto_reset on: B ends on steps 2, 9, 16, A on 7, 14, 21 (n_auto = 22; 8: one end each)
Every launch writes into fresh buffers filled with 0xFF bytes (a NaN in float32 and binary16) with GUARD words behind them.

Bars (the ones of tests/test_gpu_env_parity.py; none is tightened here)
    f64       state 1e-12, pH observation bit-equal, tank observation one float32 ulp, reward 1e-6
    mixed     observation, reward and float32 state words 3e-5 (pH) / 2e-4 (tank), rtol = atol; pH x 1e-12
    mixed16   a float32 word: the mixed bar.  A binary16 word h (a row of the *_h entry points, or the stored I) against the oracle's w
              with the mixed bar tol of that quantity: accepted iff float16(w - tol) <= h <= float16(w + tol) -- rounding is monotone, so
              this is exactly "some value within tol of w rounds to h".  The oracle continues from the device's stored I (and, on the
              tank, its levels) after every step, so one step's rounding is judged at a time.  The I of a float32 row is the stored
              word too (exactly a binary16 value, judged as one): it is what the next step continues from and observe() returns.
    always    done, t, episode, the plant fields, the titration cell rint(C x 1e5) on every lane, rows of a reset bit-equal to the oracle's,
              the Stacking row oldest-first (a step shifts it by one frame, its last frame is the lane's state), all frames equal after
              a reset, head == t mod num_stack."""
import os
import re
from collections import namedtuple

import numpy as np

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PKG = os.path.join(ROOT, "pime-robust-non-linear-set-point-control-with-reinforcement-learning_amd")
KERNELS = os.path.join(_PKG, "csrc", "env_kernels.hip")
HEADER = os.path.join(ROOT, "include", "pime_hip.h")

GUARD = 64
F16, F32, F64 = np.float16, np.float32, np.float64

# ------------------------------------------------------------------------------------------------ the case table
Case = namedtuple("Case", "env num_stack entry action")
HANDLES = (("ph", 0), ("wt", 0), ("wt", 1), ("wt", 4), ("wt", 10))
_ENTRY = {("double", "double", "float"): "f64", ("float", "float", "float"): "mixed", ("float", "half_t", "float"): "mixed16",
          ("float", "half_t", "half_t"): "mixed16_h"}
_ACTION = {("double", "false"): "a64", ("float", "false"): "a32", ("float", "true"): "residual"}


def instantiations():
    """The (S, SI, OT) triples of PIME_INST in csrc/env_kernels.hip."""
    with open(KERNELS) as f:
        src = f.read()
    return [tuple(w.strip() for w in m) for m in re.findall(r"^PIME_INST\(([^,()]+),([^,()]+),([^,()]+)\)", src, re.M)]


def step_forms():
    """The (ActT, RESIDUAL) pairs the step launchers instantiate, the same for both envs."""
    with open(KERNELS) as f:
        src = f.read()
    forms = {env: sorted(set(re.findall(env + r"_step_kernel<S, SI, (\w+), OT, (true|false)>", src))) for env in ("ph", "wt")}
    assert forms["ph"] == forms["wt"] and forms["ph"], forms
    return forms["ph"]


def half_takes_float64_action():
    """Does the ABI of pime_env_step_h take an action dtype?  (It takes `const float* action`.)"""
    with open(HEADER) as f:
        sig = re.search(r"int pime_env_step_h\(([^;]*)\);", f.read()).group(1)
    assert "const float* action" in sig
    return "action_dtype" in sig


def cases():
    out = []
    for env, ns in HANDLES:
        for triple in instantiations():
            entry = _ENTRY[triple]
            for act_t, residual in step_forms():
                if triple[2] == "half_t" and act_t == "double" and not half_takes_float64_action():
                    continue
                out.append(Case(env, ns, entry, _ACTION[act_t, residual]))
    return out


def case_id(c):
    return f"{c.env}{'-s%d' % c.num_stack if c.num_stack else ''}-{c.entry}-{c.action}"


def mode_of(c):
    return "mixed16" if c.entry.startswith("mixed16") else c.entry


def obs_dim(c):
    return 3 if c.env == "ph" else (3 * c.num_stack if c.num_stack else 4)


def has_I(c):
    return c.env == "ph" or c.num_stack == 0


def prior_gain(c):
    """priorK of the residual composition in the kernels' sign (= -env.K)."""
    if c.env == "ph":
        return -np.array([-0.02, 0.02, 0.035])
    if c.num_stack == 0:
        return -np.array([0., 0.4, -0.4, 0.])
    k = np.zeros(3 * c.num_stack)
    k[-3:] = [0., 0.4, -0.4]
    return -k


# ------------------------------------------------------------------------------------------------ the scenario
Scenario = namedtuple("Scenario", "N env_offset seed max_step resample_every n_auto window env_kw")


def scenario(N=193, n_auto=22, window=None, env_offset=1000, seed=20240607, **env_kw):
    """window (g0, n): the device holds the lanes g0 .. g0 + n - 1 of the N-lane scenario (at env_offset + g0) and gets their slice of
    its actions and mask."""
    return Scenario(N, env_offset, seed, 7, 2, n_auto, window or (0, N), tuple(sorted(env_kw.items())))


N_FREE = 5   # steps before the masked reset


def lane_mask(sc):
    m = (np.random.RandomState(sc.seed % 65521).uniform(size=sc.N) < 0.5).astype(np.uint8)
    m[0], m[-1] = 1, 0
    return m


def make_oracle(c, sc, table):
    g0, n = sc.window
    kw = dict(sc.env_kw)
    if c.env == "ph":
        ref = oracle.OraclePH(n, table, max_steps=sc.max_step, reward_type=kw.get("reward_type", "square_distance"),
                              integral_bound=kw.get("integral_bound", True), resample_every=sc.resample_every, seed=sc.seed,
                              env_offset=sc.env_offset + g0)
        ref.set_punish(kw.get("integral_punish", 0.0), kw.get("action_punishment", 0.0), kw.get("action_change_punishment", 0.0))
    else:
        ref = oracle.OracleWT(n, max_steps=sc.max_step, reward_type=kw.get("reward_type", "distance"), num_stack=c.num_stack,
                              resample_every=sc.resample_every, seed=sc.seed, env_offset=sc.env_offset + g0)
        ref.set_punish(kw.get("integral_punish", 0.0))
    return ref


def make_vec_env(c, sc, device, **over):
    """The product's env of a case (needs a GPU)."""
    from pime_amd.vec_env import VecPH, VecWaterTank
    g0, n = sc.window
    kw = dict(sc.env_kw)
    common = dict(device=device, state_mode=mode_of(c), seed=sc.seed, env_offset=sc.env_offset + g0, resample_every=sc.resample_every)
    if c.env == "ph":
        kw.setdefault("reward_type", "square_distance")
        return VecPH(n, max_episode_steps=sc.max_step, **common, **kw, **over)
    kw.setdefault("reward_type", "distance")
    return VecWaterTank(n, max_step=sc.max_step, num_stack=c.num_stack, **common, **kw, **over)


class HostBuf:
    def __init__(self, shape, dtype):
        self.shape, self.size = tuple(shape), int(np.prod(shape))
        self.full = np.empty(self.size + GUARD, dtype=dtype)
        self.full.view(np.uint8)[:] = 0xFF
        self.rows = self.full[:self.size].reshape(self.shape)

    def host(self):
        return self.full


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def poisoned(a):
    return bits(a) == np.iinfo(bits(a).dtype).max


# ------------------------------------------------------------------------------------------------ the checker
def _share(got, want, rtol, atol):
    """|got - want| as a share of atol + rtol |want|, per element (NaN counts as infinite)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err == 0, 0.0, err / (atol + rtol * np.abs(want)))
    return np.where(np.isnan(s), np.inf, s)


def half_interval(w, rtol, atol):
    w = np.asarray(w, F64)
    tol = atol + rtol * np.abs(w)
    return (w - tol).astype(F16), (w + tol).astype(F16)


def _half_share(h, w, rtol, atol):
    """The interval criterion: inf where the binary16 word h is outside [float16(w - tol), float16(w + tol)]; inside, |h - w| as a share of
    the farthest an accepted word can lie from w, tol + half a binary16 step."""
    w = np.asarray(w, F64)
    h = np.asarray(h, F16)
    lo, hi = half_interval(w, rtol, atol)
    ok = (lo <= h) & (h <= hi)
    s = np.abs(h.astype(F64) - w) / (atol + rtol * np.abs(w) + 0.5 * np.abs(np.spacing(h).astype(F64)))
    return np.where(ok, np.minimum(s, 1.0), np.inf)


class Checker:
    PH_FIELDS = ("x", "I", "r", "A", "B", "C", "qww_V", "qc_V", "t", "episode")
    WT_FIELDS = ("h1", "h2", "r", "a1", "a2", "Kp", "t", "episode")

    def __init__(self, dev, ref, c, sc):
        self.dev, self.ref, self.c, self.sc = dev, ref, c, sc
        self.mode, self.ph = mode_of(c), c.env == "ph"
        self.bar = 3e-5 if self.ph else 2e-4
        self.share = {}
        self.fields = None
        self.rows = None      # the rows the device holds for every lane, as last written (device dtype)
        self.where = ""
        names = self.PH_FIELDS if self.ph else self.WT_FIELDS + (("I",) if c.num_stack == 0 else ()) + (
            ("head",) if c.num_stack and dev.has_head else ())
        self.names = names

    # -- bookkeeping ---------------------------------------------------------------------------------------------------------------------
    def _use(self, key, s, what):
        m = float(np.max(s)) if np.size(s) else 0.0
        self.share[key] = max(self.share.get(key, 0.0), m)
        assert m <= 1.0, f"{self.where}: {what}: {m:.3g} of the bar at lane {int(np.argmax(np.max(np.reshape(s, (len(s), -1)), axis=1)))}"

    def _same(self, got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        if got.size == 0 and want.size == 0:
            return
        bad = np.nonzero(np.reshape(got != want, (len(got), -1)).any(axis=1))[0]
        assert bad.size == 0, f"{self.where}: {what}: lanes {bad[:8].tolist()} differ (got {got[bad[0]]}, want {want[bad[0]]})"

    def _buffers(self, written, *bufs):
        """Guards intact; every word of a written row written; every other row still poison."""
        for name, b in bufs:
            full = b.host()
            assert poisoned(full[b.size:]).all(), f"{self.where}: {name}: a word behind the buffer was written"
            p = poisoned(full[:b.size]).reshape(b.shape[0], -1)
            holes = np.nonzero(p[written].any(axis=1))[0]
            assert holes.size == 0, f"{self.where}: {name}: unwritten words in written rows (row {np.nonzero(written)[0][holes[0]]})"
            stray = np.nonzero((~p[~written]).any(axis=1))[0]
            assert stray.size == 0, f"{self.where}: {name}: a row that must stay untouched was written (row {np.nonzero(~written)[0][stray[0]]})"

    def _word(self, key, got, want, what, rtol=None, atol=None):
        """A float32 or binary16 word of a row against the oracle's float64 value, with the mode's bar."""
        rtol = self.bar if rtol is None else rtol
        atol = self.bar if atol is None else atol
        if np.asarray(got).dtype == F16:
            self._use(key + "16", _half_share(got, want, rtol, atol), what + " (binary16 interval)")
        else:
            self._use(key, _share(got, want, rtol, atol), what)

    # -- state ---------------------------------------------------------------------------------------------------------------------------
    def _state(self):
        dev, ref, f64 = self.dev, self.ref, self.mode == "f64"
        got = {k: dev.field(k) for k in self.names}
        r32 = (lambda v: v) if f64 else (lambda v: v.astype(F32).astype(F64))
        for k in ("t", "episode"):
            self._same(got[k], ref.get(k), k)
        if self.ph:
            self._same(got["qww_V"], ref.get("qww_V"), "qww_V")
            self._same(got["qc_V"], ref.get("qc_V"), "qc_V")
            self._same(got["C"], ref.get("C"), "C")
            self._use("plant", _share(got["A"], ref.get("A"), 4e-16, 0), "A")
            self._use("plant", _share(got["B"], ref.get("B"), 2e-15, 0), "B")
            self._use("x", _share(got["x"], ref.get("x"), 1e-12, 1e-12), "x")
            cell = lambda C, x: np.rint(C * x * 1e5)   # noqa: E731
            self._same(cell(got["C"], got["x"]), cell(ref.get("C"), ref.get("x")), "titration cell")
        else:
            for k in ("a1", "a2", "Kp"):
                self._same(got[k], r32(ref.get(k)), k)
            for k in ("h1", "h2"):
                self._use("state", _share(got[k], ref.get(k), *((1e-12, 1e-12) if f64 else (self.bar, self.bar))), k)
            if "head" in got:
                self._same(got["head"], ref.get("t") % self.c.num_stack, "ring head")
        self._same(got["r"], r32(ref.get("r")), "r")
        if "I" in got:
            I = ref.get("I")
            if f64:
                self._use("state", _share(got["I"], I, 1e-12, 1e-12), "I")
            elif self.mode == "mixed":
                self._use("state", _share(got["I"], I, self.bar, self.bar), "I")
            else:
                h = got["I"].astype(F16)
                self._same(h.astype(F64), got["I"], "the stored I is a binary16 word")
                self._use("I16", _half_share(h, I, self.bar, self.bar), "stored I (binary16 interval)")
        return got

    def _resync(self, got):
        if self.mode != "mixed16":
            return
        if "I" in got:
            self.ref.set("I", got["I"])
        if not self.ph:
            self.ref.set("h1", got["h1"])
            self.ref.set("h2", got["h2"])

    def _frames_equal(self, rows, lanes, what):
        if self.c.num_stack:
            fr = bits(rows).reshape(len(rows), self.c.num_stack, 3)
            self._same(fr[lanes], np.broadcast_to(fr[lanes][:, :1], fr[lanes].shape), what + ": every frame is the first frame")

    # -- launches ------------------------------------------------------------------------------------------------------------------------
    def after_reset(self, where, buf, want, sel):
        self.where = where
        sel = np.asarray(sel, bool)
        self._buffers(sel, ("obs", buf))
        rows = buf.host()[:buf.size].reshape(buf.shape)
        self._same(bits(rows[sel]), bits(want.astype(rows.dtype)[sel]), "the reset rows")
        self._frames_equal(rows, sel, "reset")
        before = self.fields
        got = self._state()
        if before is not None:   # a masked reset: the other lanes keep their state bit for bit
            for k in self.names:
                self._same(bits(got[k][~sel]), bits(before[k][~sel]), f"{k} of an unselected lane")
        self.fields = got
        if self.rows is None:
            assert sel.all()
            self.rows = rows.copy()
        else:
            self.rows[sel] = rows[sel]
        return self.rows

    def after_step(self, where, obs, rew, done, w_obs, w_obs64, w_rew, w_done, auto):
        self.where = where
        n, c, f64 = len(w_done), self.c, self.mode == "f64"
        every = np.ones(n, bool)
        self._buffers(every, ("obs", obs), ("reward", rew), ("done", done))
        rows = obs.host()[:obs.size].reshape(obs.shape)
        g_rew, g_done = rew.host()[:rew.size], done.host()[:done.size]
        self._same(g_done, w_done.astype(np.uint8), "done")
        fresh = w_done & bool(auto)      # lanes the launch reset: their row is the new episode's first
        self._same(bits(rows[fresh]), bits(w_obs.astype(rows.dtype)[fresh]), "the rows of an auto-reset")
        self._frames_equal(rows, fresh, "auto-reset")
        run = ~fresh
        if f64:
            if self.ph:
                self._same(bits(rows[run]), bits(w_obs[run]), "the float64 pH observation (bit-equal)")
            else:
                self._use("obs", _share(rows[run], w_obs[run], 1.2e-7, 0), "observation (one float32 ulp)")
            self._use("reward", _share(g_rew, w_rew, 1e-6, 1e-6), "reward")
        else:
            wide, want = rows[run], w_obs64[run]
            if self.mode == "mixed16" and rows.dtype == F32 and has_I(c):   # the float row carries I as stored: a binary16 word
                h = wide[:, -1].astype(F16)
                self._same(bits(h.astype(F32)), bits(wide[:, -1]), "I of a float32 row is the stored binary16 word")
                self._word("obs", h, want[:, -1], "I of the observation")
                wide, want = wide[:, :-1], want[:, :-1]
            self._word("obs", wide, want, "observation")
            self._word("reward", g_rew, w_rew, "reward")
        if c.num_stack:   # oldest first: a step drops the oldest frame and appends the lane's new state
            self._same(bits(rows[run][:, :-3]), bits(self.rows[run][:, 3:]), "the Stacking row shifted by one frame")
        got = self._state()
        if c.num_stack:
            last = np.stack([got["h1"], got["h2"], got["r"]], axis=1).astype(F32).astype(rows.dtype)
            self._same(bits(rows[:, -3:]), bits(last), "the newest frame is the lane's state")
        elif not self.ph:
            cur = np.stack([got["h1"], got["h2"], got["r"], got["I"]], axis=1).astype(F32).astype(rows.dtype)
            self._same(bits(rows), bits(cur), "the row is the lane's state")
        else:
            self._same(bits(rows[:, 1:]), bits(np.stack([got["r"], got["I"]], axis=1).astype(F32).astype(rows.dtype)), "r, I of the row")
        self.fields = got
        self._resync(got)
        self.rows = rows.copy()
        return self.rows

    def after_observe(self, where, buf):
        self.where = where
        self._buffers(np.ones(buf.shape[0], bool), ("observe", buf))
        rows = buf.host()[:buf.size].reshape(buf.shape)
        assert rows.dtype == F32
        self._same(bits(rows.astype(self.rows.dtype)), bits(self.rows), "observe() repeats the last written rows")
        if self.rows.dtype == F16 and has_I(self.c):   # I is stored as binary16: observe() reads that very word
            self._same(bits(rows[:, -1]), bits(self.rows[:, -1].astype(F32)), "I of observe() is the stored binary16 word")


def share_line(c, sc, share):
    keys = " ".join(f"{k}={v:.4f}" for k, v in sorted(share.items()))
    return f"SHARE env id={case_id(c)} N={sc.window[1]} {keys}"


# ------------------------------------------------------------------------------------------------ the driver
class InjectedDraws:
    """Host-made draws for a device built on them (vec_env.CallbackDraws) and for the oracle: the driver names the launch, both sides read
    the same rows.  A device whose host path hands the kernel a row for a lane that does not end must not show it: `episode_fn` serves
    the lanes that are asked for, everything else is up to the device's draw source (the GPU test poisons it)."""

    def __init__(self, c, sc):
        self.c, self.sc, self.launch = c, sc, 0

    def _rng(self, salt):
        return np.random.RandomState((self.sc.seed + 7919 * self.launch + salt) % (2 ** 31))

    def episode(self):
        """float64 [n, 4 | 6]: this launch's reset row of every lane."""
        n = self.sc.window[1]
        lo, hi = (((0.005, 0.0015, 0., 3.), (0.015, 0.0025, 50., 11.)) if self.c.env == "ph"
                  else ((0.0015, 0.0015, 0.07, 0., 0., 0.), (0.0024, 0.0024, 0.17, 10., 10., 10.)))
        return self._rng(1).uniform(lo, hi, (n, len(lo)))

    def noise(self):
        return None if self.c.env == "ph" else 0.01 * self._rng(2).standard_normal((self.sc.window[1], 2))

    def episode_fn(self, i):
        return tuple(self.episode()[i])

    def noise_fn(self, i):
        return tuple(self.noise()[i])


def run_scenario(dev, c, sc, table, record=None, draws=None):
    """Drive `dev` through the scenario, checking every launch against the oracle; returns the largest used share of each bar.  `record`
    (a list) receives one dict per launch: what the device wrote and what the oracle says happened.  draws: the InjectedDraws the device
    was built on (None: in-kernel Philox on both sides)."""
    ref = make_oracle(c, sc, table)
    chk = Checker(dev, ref, c, sc)
    g0, n = sc.window
    win = slice(g0, g0 + n)
    assert dev.N == n and dev.D == obs_dim(c) and dev.half == (c.entry == "mixed16_h")
    rng = np.random.RandomState(sc.seed % 9973)
    mask = lane_mask(sc)[win]
    K = prior_gain(c)
    amp = 1.3 if c.env == "ph" else 1.5
    launch = [0]

    def note(kind, **kw):
        if record is not None:
            record.append(dict(kind=kind, launch=launch[0], plant=ref.get("qww_V" if c.env == "ph" else "a1"), **kw))
        launch[0] += 1

    def reset(where, m):
        t0, ep0 = ref.get("t"), ref.get("episode")
        buf = dev.new_buf((n, dev.D), "obs")
        if draws is not None:
            draws.launch = launch[0]
        dev.reset(m, buf)
        want = ref.reset(mask=m, draws=None if draws is None else draws.episode())
        sel = np.ones(n, bool) if m is None else m.astype(bool)
        rows = chk.after_reset(where, buf, want, sel)
        note("reset", obs=rows.copy(), selected=sel, t_before=t0, episode=ref.get("episode"), episode_before=ep0)
        return rows

    def step(where, cur, auto):
        t0, ep0 = ref.get("t"), ref.get("episode")
        if c.action == "residual":
            a = (rng.standard_normal(sc.N) * 0.6).astype(F32)[win]
            a_env = oracle.residual_action(a, cur.astype(F32), K)
            residual = (cur, K)
        else:
            a = rng.uniform(-amp, amp, sc.N)[win]
            a = a.astype(F32) if c.action == "a32" else a
            a_env, residual = a.astype(F64), None
        bufs = dev.new_buf((n, dev.D), "obs"), dev.new_buf((n,), "reward"), dev.new_buf((n,), "done")
        if draws is not None:
            draws.launch = launch[0]
        dev.step(a, residual, auto, *bufs)
        inj = {} if draws is None else dict(reset_draws=draws.episode(), **({} if c.env == "ph" else dict(noise=draws.noise())))
        w = ref.step(a_env, auto_reset=auto, **inj)
        rows = chk.after_step(where, *bufs, *w, auto)
        note("step", obs=rows.copy(), reward=bufs[1].host()[:n].copy(), done=w[3].copy(), want64=w[1].copy(), want_reward=w[2].copy(), auto=auto, t_before=t0, episode=ref.get("episode"),
             episode_before=ep0)
        return rows

    cur = reset("reset", None)
    for k in range(N_FREE):
        cur = step(f"free step {k}", cur, False)
    cur = reset("masked reset", mask)
    for k in range(sc.n_auto):
        cur = step(f"auto step {k + 1}", cur, True)
    buf = dev.new_buf((n, dev.D), "observe")
    dev.observe(buf)
    chk.after_observe("observe", buf)
    note("observe", obs=buf.host()[:buf.size].reshape(buf.shape).copy())
    t_before = ref.get("t")
    cur = step("last step", cur, False)
    ended = t_before + 1 >= sc.max_step
    assert (ended == ~mask.astype(bool)).all() and (ref.get("t")[ended] == sc.max_step).all(), "the last step ends group B only, unreset"
    return chk.share


# ------------------------------------------------------------------------------------------------ a device in numpy
def round_twice(v32):
    """float32 -> 12 significant bits -> binary16: a double rounding (differs from the direct one just above a tie)."""
    v = np.asarray(v32, F64)
    m, e = np.frexp(v)
    return (np.ldexp(np.rint(m * 4096.0), e - 12)).astype(F16)


class FakeDevice:
    """The oracle with its outputs rounded to float32 / binary16 and I stored rounded.  `mutate`: dict(name=, launch=, lane=, ...), one
    defect at one launch (tests/test_env_cases_cpu.py)."""

    def __init__(self, c, sc, table, mutate=None):
        self.c, self.sc, self.ref = c, sc, make_oracle(c, sc, table)
        self.N, self.D, self.half, self.has_head = sc.window[1], obs_dim(c), c.entry == "mixed16_h", c.num_stack > 0
        self.mode = mode_of(c)
        self.head = np.zeros(self.N, np.int64)
        self.launch = 0
        self.mut = dict(mutate or {})
        self.over = {}            # field -> per-lane offset (a mutation's lasting effect on what field() reports)
        self.held = np.zeros((self.N, self.D), F32)   # the rows observe() repeats
        self.pre_I = {}           # launch -> the float32 I before it was stored (for the tests that look for a site)
        self.icol = (2 if c.env == "ph" else 3) if has_I(c) else None

    def _hit(self, name):
        return self.mut.get("name") == name and self.mut.get("launch") == self.launch

    def new_buf(self, shape, kind):
        return HostBuf(shape, np.uint8 if kind == "done" else (F16 if self.half and kind != "observe" else F32))

    def _poke(self, bufs):
        if self._hit("poke"):
            b = bufs[self.mut["buf"]]
            b.full[self.mut["index"]] = self.mut["value"]
        self.launch += 1

    def _reset_heads(self, lanes):
        keep = self.head.copy()
        self.head[lanes] = 0
        if self._hit("ring_not_reheaded"):
            self.head[self.mut["lane"]] = keep[self.mut["lane"]]

    def _carry_I(self, rows, I_before):
        if self._hit("I_carried"):
            L = self.mut["lane"]
            I = self.ref.get("I")
            I[L] = I_before[L]
            self.ref.set("I", I)
            rows[L, self.icol] = I_before[L]

    def reset(self, mask, out):
        m = None if mask is None else np.array(mask, np.uint8)
        if self._hit("selected_skipped"):
            m[self.mut["lane"]] = 0
        I_before = self.ref.get("I") if has_I(self.c) else None
        rows = self.ref.reset(mask=m)
        sel = np.ones(self.N, bool) if m is None else m.astype(bool)
        self._reset_heads(sel)
        if I_before is not None:
            self._carry_I(rows, I_before)
        if self._hit("episode_stuck"):
            self.over["episode"] = np.zeros(self.N)
            self.over["episode"][self.mut["lane"]] = -1
        out.rows[sel] = rows.astype(out.rows.dtype)[sel]
        self.held[sel] = rows[sel]
        self._poke({"obs": out})

    def step(self, action, residual, auto_reset, out_obs, out_reward, out_done):
        a_env = np.asarray(action, F64) if residual is None else oracle.residual_action(action, np.asarray(residual[0]).astype(F32), residual[1])
        I_before = self.ref.get("I") if has_I(self.c) else None
        obs32, _, rew, done = self.ref.step(a_env, auto_reset=auto_reset)
        fresh = done & bool(auto_reset)
        if self.c.num_stack:
            self.head = (self.head + 1) % self.c.num_stack
            self._reset_heads(fresh)
        if self.icol is not None and self.mode != "f64":
            I32 = self.ref.get("I").astype(F32)
            self.pre_I[self.launch] = I32.copy()
            if self.mode == "mixed16":   # stored as binary16; the row carries the stored word
                Ih = I32.astype(F16)
                if self._hit("I_rounded_twice"):
                    Ih[self.mut["lane"]] = round_twice(I32[self.mut["lane"]])
                I32 = Ih.astype(F32)
            self.ref.set("I", I32.astype(F64))
            obs32[:, self.icol] = I32
        if I_before is not None and fresh.any():
            self._carry_I(obs32, I_before)
        self.held = obs32.copy()
        if self._hit("ring_rotated"):
            obs32[self.mut["lane"]] = np.roll(obs32[self.mut["lane"]], 3)
        d = done.astype(np.uint8)
        if self._hit("done_missing"):
            d[self.mut["lane"]] = 0
        out_obs.rows[:] = obs32.astype(out_obs.rows.dtype)
        out_reward.rows[:] = rew.astype(F32).astype(out_reward.rows.dtype)
        out_done.rows[:] = d
        self._poke({"obs": out_obs, "reward": out_reward, "done": out_done})

    def observe(self, out):
        out.rows[:] = self.held
        self._poke({"obs": out})

    def field(self, name):
        if name == "head":
            return self.head.astype(F64)
        v = self.ref.get(name)
        narrow = dict(ph=("r", "I"), wt=("h1", "h2", "r", "I", "a1", "a2", "Kp"))[self.c.env]
        if self.mode != "f64" and name in narrow:
            v = v.astype(F32).astype(F64)
        return v + self.over[name] if name in self.over else v


class TwinDevice:
    """The product's own lane arithmetic built for the host (oracle.twin.TwinEnv: float64 state, pH and the Integrator tank)."""
    half, has_head = False, False

    def __init__(self, c, sc, table):
        import pime_amd.native as nt
        from oracle.twin import TwinEnv
        assert c.entry == "f64" and has_I(c) and not sc.env_kw
        g0, n = sc.window
        self.c, self.N, self.D = c, n, obs_dim(c)
        self.table = np.ascontiguousarray(table, F64)
        self.env = TwinEnv(c.env, n, table=self.table, seed=sc.seed, env_offset=sc.env_offset + g0, max_steps=sc.max_step,
                           resample_every=sc.resample_every, reward_type=nt.REWARD["square_distance" if c.env == "ph" else "distance"])

    def new_buf(self, shape, kind):
        return HostBuf(shape, np.uint8 if kind == "done" else F32)

    def reset(self, mask, out):
        rows = self.env.reset(mask=mask)
        sel = np.ones(self.N, bool) if mask is None else np.asarray(mask, bool)
        out.rows[sel] = rows[sel]

    def step(self, action, residual, auto_reset, out_obs, out_reward, out_done):
        if residual is None:
            o, r, d = self.env.step(np.asarray(action, F64), auto_reset=auto_reset)
        else:
            o, r, d = self.env.step_residual(action, residual[0], residual[1], auto_reset=auto_reset)
        out_obs.rows[:], out_reward.rows[:], out_done.rows[:] = o, r, d

    def observe(self, out):
        g = self.env.get
        if self.c.env == "ph":
            k = np.rint(g("C") * g("x") * 1e5).astype(np.int64)
            out.rows[:] = np.stack([self.table[k], g("r"), g("I")], axis=1)
        else:
            out.rows[:] = np.stack([g("h1"), g("h2"), g("r"), g("I")], axis=1)

    def field(self, name):
        return self.env.get(name)
