"""Test helper: seeded cases for the fused TD3 step (csrc/td3_fused.hip), their kink margins, oracle mutants and an Adam replay.
Plain module (like tests/oracle_env.py), shared by tests/test_td3_cases_cpu.py and tests/test_gpu_td3_sweep.py so that the CPU
tests see bit for bit what the GPU tests run: every weight, buffer row, index and noise draw is made on the CPU from a seed
(numpy) and loaded into the agent with load_state_dict.

Three numbers rule the inputs.  They are conditions on the INPUTS, checked on the CPU; none of them is a tolerance on a kernel.

  * DELTA = 1e-5, the kink margin.  The TD3 objective is not differentiable where a ReLU pre-activation is 0, where the smoothing
    noise meets its clip, where the smoothed action meets +-1, where the twin target heads are equal and where |q - label| = 1.
    A float32 evaluation that lands on the other side of such a point than the float64 reference changes a weight-gradient row by
    O(1 / B) -- a legitimate rounding difference that looks like an error of many times the 3e-4 bar.  A sample's margin is its
    smallest relative distance to any such point (`reference_step(margins=True)`); samples below DELTA are redrawn.  1e-5 is about 100 x the relative
    rounding error of a 256-term float32 dot product (~ sqrt(256) * 2^-24 = 1e-6 typical), so no float32 evaluation order can
    carry a vetted sample across a kink.
  * MUTATION_MARGIN = 10 (x the 3e-4 bar = 3e-3 of a tensor's largest entry).  A gradient check only says something about a
    branch of the arithmetic if getting that branch wrong would move the gradient by clearly more than the tolerance.  For every
    vetted case every mutant of the oracle (MUTANTS: a twin head instead of the min, no noise clip, no action clamp, mask ignored,
    SmoothL1 all quadratic / all linear, the actor objective through the second head, any ReLU gate left open) must move at least
    one gradient tensor by 10 x the bar: ten, so that "within 3e-4" cannot be met by a kernel that gets the branch wrong even when
    its error is spread over several tensors; the generator's scales below reach far more at most shapes.
  * F32_STABILITY = 1e-4 (a third of the bar): the reference arithmetic evaluated in float32 on the CPU must agree with itself in
    float64 to that much of each tensor's largest entry.  A case on which plain float32 numpy uses up the bar cannot tell a wrong
    kernel from a right one; such a case gets a smaller batch, not a larger number.

Replay bounds (`replay_bounds`) are derived from the float32 operation count of td3_apply_kernel, see there."""
import collections
import functools

import numpy as np

from oracle import td3 as O

DELTA = 1e-5
BAR = 3e-4
MUTATION_MARGIN = 10.0
F32_STABILITY = 1e-4

WIDTHS = (64, 128, 256)
ALL_D = tuple(range(1, 32))
COMPILED_D = (3, 4, 12, 30)


def kernel_class(width, D):
    """The instantiation `launch_td3_grad` (csrc/td3_fused.hip; `grad_dispatch` of csrc/td3_device.hpp) picks for (width, D): the state width compiled in
    (D = 3, 4, 12, 30), else run-time D with two first-layer k-steps while the critic's D + 1 inputs fit 8 columns (td3.hpp:
    td3_first_ksteps), else with eight."""
    if D in COMPILED_D:
        return width, f"D{D}"
    return width, "rt2" if D + 1 <= 8 else "rt8"


ALL_CLASSES = tuple((w, k) for w in WIDTHS for k in ("D3", "D4", "D12", "D30", "rt2", "rt8"))

Hyper = collections.namedtuple("Hyper", "lr betas eps tau policy_noise noise_clip update_freq")
DEFAULT_HYPER = Hyper(1e-4, (0.9, 0.999), 1e-8, 2.0 ** -8, 0.6, 0.5, 2)
# section c of the sweep: nothing at its default
OTHER_HYPER = Hyper(3e-4, (0.8, 0.99), 1e-6, 0.05, 0.4, 0.3, 3)

# width, D, B, table rows, the row that is stepped, whether that step blends the targets, hyper-parameters, whether the samples
# of `row` are vetted (margins >= DELTA); the seed follows from the rest
Spec = collections.namedtuple("Spec", "width D B rows row soft hyper vet")


def spec(width, D, B, rows=1, row=0, soft=None, hyper=DEFAULT_HYPER, vet=True):
    return Spec(width, D, B, rows, row, (row % hyper.update_freq == 0) if soft is None else bool(soft), hyper, vet)


def spec_id(s):
    tag = f"{s.width}-D{s.D}-B{s.B}"
    if s.rows > 1:
        tag += f"-row{s.row}of{s.rows}"
    if s.hyper != DEFAULT_HYPER:
        tag += "-hyper2" + ("-soft" if s.soft else "-nosoft")
    return tag


# ---------------------------------------------------------------------------------------------------------------- sweep lists
def shapes_93():
    """Section a: every supported (width, D) at B = 37 (three 16-sample tiles, the last one ragged)."""
    return [spec(w, D, 37) for w in WIDTHS for D in ALL_D]


_RT2_D, _RT8_D = (1, 2, 7), (8, 15, 16, 17, 29, 31, 16, 8, 31)
REGIME_B = (1, 17, 8193)


def regime_cases():
    """Section b: every instantiation x B in {1, 17, 8193}; D varies inside the run-time classes so that 1, 2, 7 (two k-steps)
    and 8, 15, 16, 17, 29, 31 (eight) all occur."""
    out = []
    for i, w in enumerate(WIDTHS):
        for j, B in enumerate(REGIME_B):
            for D in COMPILED_D + (_RT2_D[(i + j) % 3], _RT8_D[3 * i + j]):
                out.append(spec(w, D, B))
    return out


def third_group_cases():
    """Section b: B = 16 400 = 1 025 tiles > 2 x 512 workgroups (workgroup 0 accumulates a third group) -- one class of every
    (width, k-steps) combination."""
    return [spec(64, 7, 16400), spec(64, 30, 16400), spec(128, 3, 16400), spec(128, 17, 16400), spec(256, 2, 16400),
            spec(256, 12, 16400)]


HYPER_SHAPES = ((64, 12, 100), (128, 7, 100), (256, 31, 100))


def hyper_cases():
    """Section c: (spec, soft_mode) -- a four-row table stepped at row 3 on a fresh agent, update_freq 3 (row 3 is a delayed step),
    every hyper-parameter off its default, soft_mode 0 (never), 1 (always), 2 (row % update_freq == 0)."""
    return [(spec(w, D, B, rows=4, row=3, soft=mode != 0, hyper=OTHER_HYPER), mode) for w, D, B in HYPER_SHAPES for mode in (0, 1, 2)]


def class_cases_37():
    """One B = 37 case of section a per instantiation (sections d and f)."""
    pick = {"D3": 3, "D4": 4, "D12": 12, "D30": 30}
    out = []
    for i, w in enumerate(WIDTHS):
        for k in ("D3", "D4", "D12", "D30", "rt2", "rt8"):
            D = pick.get(k) or (_RT2_D[i] if k == "rt2" else (17, 31, 8)[i])
            out.append(spec(w, D, 37))
    return out


def gradient_specs():
    """Every spec whose gradients a GPU test compares with the oracle (each once)."""
    seen = []
    for s in shapes_93() + regime_cases() + third_group_cases() + [c for c, _ in hyper_cases()]:
        if s not in seen:
            seen.append(s)
    return seen


# ---------------------------------------------------------------------------------------------------------------- generator
N_BUF = 2048   # replay rows of a case; samples draw from [2, N_BUF - 3), positions 0 and B - 1 name row 0 and row N_BUF - 2


def _linear(rng, n_out, n_in):
    k = 1.0 / np.sqrt(n_in)
    return rng.uniform(-k, k, (n_out, n_in)), rng.uniform(-k, k, n_out)


def make_nets(width, D, seed):
    """(act, act_target, cri, cri_target) state dicts, float32.  Trunks as nn.Linear's default; the scales that the mutation
    check (test_td3_cases_cpu.py) needs are set here: policy outputs centred, of order 1.5 before tanh (so that tanh + noise crosses
    +-1), an action column of order 0.5 in both critics (so that the smoothed action reaches the label), twin heads that are
    independent draws with q centred near 0 and of order 0.6 (so that min picks either head and |q - label| straddles 1 with most
    samples in the quadratic branch), targets that are the online nets plus a perturbation of a third of their scale."""
    rng = np.random.RandomState([seed, width, D, 17])
    probe = rng.uniform(-1.5, 1.5, (256, D))

    def actor():
        p = {}
        for name, (o, i) in (("net.0", (width, D)), ("net.2", (width, width)), ("net.4", (width, width)), ("net.6", (1, width))):
            p[name + ".weight"], p[name + ".bias"] = _linear(rng, o, i)
        return p

    def critic():
        p = {}
        for name, (o, i) in (("net_sa.0", (width, D + 1)), ("net_sa.2", (width, width)), ("net_q1", (1, width)), ("net_q2", (1, width))):
            p[name + ".weight"], p[name + ".bias"] = _linear(rng, o, i)
        p["net_sa.0.weight"][:, -1] = rng.uniform(-1.0, 1.0, width)
        return p

    def perturbed(p):
        return {k: v + rng.standard_normal(v.shape) * (0.3 * v.std() if v.size > 1 else 0.1) for k, v in p.items()}

    act, cri = actor(), critic()
    act_t, cri_t = perturbed(act), perturbed(cri)
    for a in (act, act_t):     # pre-tanh output on the probe rows: mean within +-0.2, standard deviation 1.5
        pre = O.actor_hidden(a, probe)[3]
        a["net.6.weight"] *= 1.5 / pre.std()
        a["net.6.bias"][:] = rng.uniform(-0.2, 0.2) - (pre.mean() - a["net.6.bias"]) * 1.5 / pre.std()
    pa = np.tanh(rng.standard_normal((256, 1)))
    for c in (cri, cri_t):     # both heads on the probe rows: mean within +-0.3 (each its own), standard deviation 0.6
        for h in ("net_q1", "net_q2"):
            q = O.critic_hidden(c, probe, pa)[3 if h == "net_q1" else 4]
            c[h + ".weight"] *= 0.6 / q.std()
            c[h + ".bias"][:] = rng.uniform(-0.3, 0.3) - (q.mean() - c[h + ".bias"]) * 0.6 / q.std()
    return tuple({k: v.astype(np.float32) for k, v in p.items()} for p in (act, act_t, cri, cri_t))


Case = collections.namedtuple("Case", "spec nets state other idx nxt noise redraw_rounds redrawn mid")


def _draw_rows(rng, n, D):
    state = rng.uniform(-1.5, 1.5, (n, D)).astype(np.float32)
    other = np.stack([rng.standard_normal(n) * 0.4, np.where(rng.rand(n) < 0.2, 0.0, 0.99), np.tanh(rng.standard_normal(n))],
                     axis=1).astype(np.float32)   # reward of a few tenths, 20 % terminal rows, stored action
    return state, other


@functools.lru_cache(maxsize=None)
def build(s):
    """The case of a spec: nets, replay rows [N_BUF], index tables idx / nxt [rows, B] (nxt = idx + 1), noise table [rows, B].
    With s.vet, the samples of row s.row whose margin is below DELTA get a new replay row and a new noise draw until none is left
    (positions 0 and B - 1, which name replay row 0 and the last row with a successor, keep their index: the CONTENT of their replay
    rows is drawn again instead)."""
    seed = (s.width * 1000003 + s.D * 10007 + s.B * 101 + s.rows * 7 + s.row) % (2 ** 31)
    rng = np.random.RandomState([seed, int(s.soft), int(s.hyper != DEFAULT_HYPER)])
    nets = make_nets(s.width, s.D, seed)
    state, other = _draw_rows(rng, N_BUF, s.D)
    idx = rng.randint(2, N_BUF - 3, size=(s.rows, s.B)).astype(np.int64)
    noise = rng.standard_normal((s.rows, s.B)).astype(np.float32)
    fixed = {}
    if s.B >= 2:
        fixed = {0: 0, s.B - 1: N_BUF - 2}
    elif s.D % 2:
        fixed = {0: N_BUF - 2}
    else:
        fixed = {0: 0}
    for pos, r in fixed.items():
        idx[s.row, pos] = r
    rounds, redrawn, mid = 0, 0, None
    while s.vet:
        case = Case(s, nets, state, other, idx, idx + 1, noise, rounds, redrawn, None)
        mid = reference_step(case, margins=True)
        bad = np.flatnonzero(mid["margin"] < DELTA)
        if bad.size == 0:
            break
        redrawn += bad.size if rounds == 0 else 0
        while bad.size:      # the redrawn samples alone, against the batch's scales, until they are clear; then the whole batch again
            rounds += 1
            assert rounds < 200, "redraw does not converge"
            for pos in bad:
                if pos in fixed:
                    r = fixed[pos]
                    st, ot = _draw_rows(rng, 2, s.D)
                    state[r:r + 2], other[r:r + 2] = st, ot
                else:
                    idx[s.row, pos] = rng.randint(2, N_BUF - 3)
                noise[s.row, pos] = rng.standard_normal()
            case = Case(s, nets, state, other, idx, idx + 1, noise, rounds, redrawn, None)
            m = reference_step(case, margins=True, subset=bad, scales=mid["scales"], cri_t_actor=mid["cri_t_actor"])["margin"]
            bad = bad[m < 2 * DELTA]   # (twice: the whole-batch pass that follows moves the scales and the mid-step target a little)
    for a in (state, other, idx, noise):
        a.setflags(write=False)
    return Case(s, nets, state, other, idx, idx + 1, noise, rounds, redrawn, mid)   # mid: reference_step of the final, vetted inputs


# ---------------------------------------------------------------------------------------------------------------- the step, restated
MUTANTS_CRITIC = ("q1_only", "q2_only", "no_noise_clip", "no_action_clamp", "mask_ignored", "all_quadratic", "all_linear",
                  "open_gate_c1", "open_gate_c2")
MUTANTS_ACTOR = ("second_head", "open_gate_tc1", "open_gate_tc2", "open_gate_h1", "open_gate_h2", "open_gate_h3")
MUTANTS = MUTANTS_CRITIC + MUTANTS_ACTOR


def _actor_fw(p, s):
    z1 = s @ p["net.0.weight"].T + p["net.0.bias"]
    h1 = np.maximum(z1, 0)
    z2 = h1 @ p["net.2.weight"].T + p["net.2.bias"]
    h2 = np.maximum(z2, 0)
    z3 = h2 @ p["net.4.weight"].T + p["net.4.bias"]
    h3 = np.maximum(z3, 0)
    return (z1, z2, z3), (h1, h2, h3), h3 @ p["net.6.weight"].T + p["net.6.bias"]


def _critic_fw(p, s, a):
    x = np.concatenate([s, a], axis=1)
    z1 = x @ p["net_sa.0.weight"].T + p["net_sa.0.bias"]
    c1 = np.maximum(z1, 0)
    z2 = c1 @ p["net_sa.2.weight"].T + p["net_sa.2.bias"]
    c2 = np.maximum(z2, 0)
    return x, (z1, z2), (c1, c2), c2 @ p["net_q1.weight"].T + p["net_q1.bias"], c2 @ p["net_q2.weight"].T + p["net_q2.bias"]


def _cast(p, dt):
    return {k: np.asarray(v, dtype=dt) for k, v in p.items()}


class _Margin:
    """Running minimum per sample of the relative distance to a kink; layer scales are the batch's largest |pre-activation| (or
    the ones handed in, when only a subset of the batch is evaluated)."""

    def __init__(self, n, scales):
        self.m, self.given, self.scales = np.full(n, np.inf), scales, {}

    def layer(self, tag, z):
        sc = self.scales[tag] = float(np.abs(z).max())
        if self.given is not None:
            sc = max(sc, self.given[tag])
        self.m = np.minimum(self.m, np.abs(z).min(axis=1) / sc)

    def point(self, dist):
        self.m = np.minimum(self.m, np.abs(dist).reshape(len(self.m), -1).min(axis=1))


def _memo(cache, key, fn):
    if cache is None:
        return fn()
    if key not in cache:
        cache[key] = fn()
    return cache[key]


def critic_pass(nets, batch, hyper, dt=np.float64, mutant=None, mg=None, cache=None, light=False):
    """(obj_critic, gradients of the online critic) in dtype dt, with one branch of the arithmetic changed when `mutant` names it.
    With mutant None and float64 this is oracle.td3.critic_objective, operation for operation (the CPU test compares them).
    cache: a dict that keeps the forward passes between the mutants of ONE batch and dtype; light: the bias and head gradients
    only (no weight-gradient products of the trunk)."""
    act_t, cri, cri_t = (_cast(p, dt) for p in (nets[1], nets[2], nets[3]))
    s, a, r, m, s2, eps = (np.asarray(v, dtype=dt) for v in batch)
    B = len(s)
    zt, _, pre = _memo(cache, "act_t", lambda: _actor_fw(act_t, s2))
    sn = eps.reshape(B, 1) * dt(hyper.policy_noise)
    noise = sn if mutant == "no_noise_clip" else np.clip(sn, -dt(hyper.noise_clip), dt(hyper.noise_clip))
    raw = np.tanh(pre) + noise
    next_a = raw if mutant == "no_action_clamp" else np.clip(raw, -1.0, 1.0)
    _, ztc, _, tq1, tq2 = _memo(cache, ("cri_t", mutant if mutant in ("no_noise_clip", "no_action_clamp") else None),
                                lambda: _critic_fw(cri_t, s2, next_a))
    tq = tq1 if mutant == "q1_only" else tq2 if mutant == "q2_only" else np.minimum(tq1, tq2)
    mask = np.full((B, 1), dt(0.99)) if mutant == "mask_ignored" else m.reshape(B, 1)
    label = r.reshape(B, 1) + mask * tq
    x, zc, (c1, c2), q1, q2 = _memo(cache, "cri", lambda: _critic_fw(cri, s, a.reshape(B, 1)))
    if mg is not None:
        for i, z in enumerate(zt):
            mg.layer(f"act_t{i}", z)
        for i, z in enumerate(ztc):
            mg.layer(f"cri_t{i}", z)
        for i, z in enumerate(zc):
            mg.layer(f"cri{i}", z)
        mg.point(np.abs(sn) - hyper.noise_clip)
        mg.point(np.abs(raw) - 1.0)
        mg.scales["tq"] = float(max(np.abs(tq1).max(), np.abs(tq2).max()))
        mg.point((tq1 - tq2) / max(mg.scales["tq"], (mg.given or {}).get("tq", 0.0)))
        mg.point(np.abs(q1 - label) - 1.0)
        mg.point(np.abs(q2 - label) - 1.0)

    def smooth(d):
        ad = np.abs(d)
        if mutant == "all_quadratic":
            return 0.5 * d * d, d
        if mutant == "all_linear":
            return ad - 0.5, np.sign(d)
        return np.where(ad < 1.0, 0.5 * d * d, ad - 0.5), np.where(ad < 1.0, d, np.sign(d))
    l1, g1 = smooth(q1 - label)
    l2, g2 = smooth(q2 - label)
    obj = l1.mean() + l2.mean()
    g1, g2 = g1 / B, g2 / B
    g = {"net_q1.weight": g1.T @ c2, "net_q1.bias": g1.sum(0), "net_q2.weight": g2.T @ c2, "net_q2.bias": g2.sum(0)}
    dz2 = g1 @ cri["net_q1.weight"] + g2 @ cri["net_q2.weight"]
    if mutant != "open_gate_c2":
        dz2 = dz2 * (c2 > 0)
    g["net_sa.2.bias"] = dz2.sum(0)
    dz1 = dz2 @ cri["net_sa.2.weight"]
    if mutant != "open_gate_c1":
        dz1 = dz1 * (c1 > 0)
    g["net_sa.0.bias"] = dz1.sum(0)
    if not light:
        g["net_sa.2.weight"], g["net_sa.0.weight"] = dz2.T @ c1, dz1.T @ x
    return obj, g


def actor_pass(act, cri_t, s, dt=np.float64, mutant=None, mg=None, cache=None, light=False):
    """(obj_actor, gradients of the actor) through the target critic's first head; oracle.td3.actor_objective when mutant is None."""
    act, cri_t, s = _cast(act, dt), _cast(cri_t, dt), np.asarray(s, dtype=dt)
    B = len(s)
    za, (h1, h2, h3), pre = _memo(cache, "act", lambda: _actor_fw(act, s))
    action = np.tanh(pre)
    _, zc, (c1, c2), q1, q2 = _memo(cache, "cri_t_actor", lambda: _critic_fw(cri_t, s, action))
    if mg is not None:
        for i, z in enumerate(za):
            mg.layer(f"act{i}", z)
        for i, z in enumerate(zc):
            mg.layer(f"cri_t_actor{i}", z)
    head = "net_q2.weight" if mutant == "second_head" else "net_q1.weight"
    obj = -(q2 if mutant == "second_head" else q1).mean()
    gq = np.full((B, 1), -1.0 / B, dtype=dt)
    gates = {"open_gate_tc2": c2, "open_gate_tc1": c1, "open_gate_h3": h3, "open_gate_h2": h2, "open_gate_h1": h1}

    def gate(d, name):
        return d if mutant == name else d * (gates[name] > 0)
    dz2 = gate(gq @ cri_t[head], "open_gate_tc2")
    dz1 = gate(dz2 @ cri_t["net_sa.2.weight"], "open_gate_tc1")
    da = dz1 @ cri_t["net_sa.0.weight"][:, -1:]
    dpre = da * (1.0 - action * action)
    g = {"net.6.weight": dpre.T @ h3, "net.6.bias": dpre.sum(0)}
    d3 = gate(dpre @ act["net.6.weight"], "open_gate_h3")
    d2 = gate(d3 @ act["net.4.weight"], "open_gate_h2")
    d1 = gate(d2 @ act["net.2.weight"], "open_gate_h1")
    g["net.4.bias"], g["net.2.bias"], g["net.0.bias"] = d3.sum(0), d2.sum(0), d1.sum(0)
    if not light:
        g["net.4.weight"], g["net.2.weight"], g["net.0.weight"] = d3.T @ h2, d2.T @ h1, d1.T @ s
    return obj, g


def batch_of(case, subset=None):
    s = case.spec
    idx, nxt, eps = case.idx[s.row], case.nxt[s.row], case.noise[s.row]
    if subset is not None:
        idx, nxt, eps = idx[subset], nxt[subset], eps[subset]
    o = case.other[idx]
    return case.state[idx], o[:, 2], o[:, 0], o[:, 1], case.state[nxt], eps


def reference_step(case, dt=np.float64, margins=False, subset=None, scales=None, cri_t_actor=None):
    """The stepped row of a case: critic objective and gradients (dtype dt), the critic's Adam step and the soft update replayed in
    float64 from those gradients on zero moments (a fresh agent; the step number is row + 1, as td3_apply_kernel counts), then the
    actor objective through the target critic AS THE STEP LEFT IT.  With margins=True also every sample's kink margin over the five
    forward passes.  subset / scales / cri_t_actor: margins of some samples only, against the batch's scales and mid-step target."""
    s, h = case.spec, case.spec.hyper
    batch = batch_of(case, subset)
    mg = _Margin(len(batch[0]), scales) if margins else None
    obj_c, gc = critic_pass(case.nets, batch, h, dt, None, mg)
    if cri_t_actor is None:
        cri = flatten(case.nets[2], O.CRITIC_KEYS)
        rep = adam_replay(cri, np.zeros_like(cri), np.zeros_like(cri), flatten(gc, O.CRITIC_KEYS), s.row + 1, h.lr, h.betas, h.eps,
                          target=flatten(case.nets[3], O.CRITIC_KEYS) if s.soft else None, tau=h.tau)
        cri_t_actor = unflatten(rep["target"], case.nets[3], O.CRITIC_KEYS) if s.soft else case.nets[3]
    obj_a, ga = actor_pass(case.nets[0], cri_t_actor, batch[0], dt, None, mg)
    out = {"obj_c": obj_c, "obj_a": obj_a, "gc": gc, "ga": ga, "cri_t_actor": cri_t_actor}
    if margins:
        out["margin"], out["scales"] = mg.m, mg.scales if scales is None else {k: max(v, scales[k]) for k, v in mg.scales.items()}
    return out


def flatten(p, keys):
    return np.concatenate([np.asarray(p[k], dtype=np.float64).reshape(-1) for k in keys])


def unflatten(flat, like, keys):
    out, o = {}, 0
    for k in keys:
        n = like[k].size
        out[k] = flat[o:o + n].reshape(like[k].shape)
        o += n
    return out


def mutant_reach(case, mid, mutant, cache=None):
    """Largest |mutant's gradient - oracle's| / max|oracle's| over the gradient tensors of the net the mutant touches: over the
    bias and head gradients if that already exceeds MUTATION_MARGIN x BAR (a lower bound of the reach, cheaper), else over all.
    cache: a dict shared by the mutants of one case (the forward passes that a mutant leaves alone are made once)."""
    for light in (True, False):
        if mutant in MUTANTS_CRITIC:
            want, got = mid["gc"], critic_pass(case.nets, batch_of(case), case.spec.hyper, mutant=mutant, cache=cache, light=light)[1]
        else:
            want, got = mid["ga"], actor_pass(case.nets[0], mid["cri_t_actor"], batch_of(case)[0], mutant=mutant, cache=cache,
                                              light=light)[1]
        reach = max(float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()) for k in got)
        if reach > MUTATION_MARGIN * BAR:
            break
    return reach


# ---------------------------------------------------------------------------------------------------------------- Adam replay
def _f32(x):
    return float(np.float32(x))


def adam_replay(param, exp_avg, exp_avg_sq, grad, step, lr, betas=(0.9, 0.999), eps=1e-8, target=None, tau=None,
                blend_param=None, f32_hyper=True):
    """torch.optim.Adam's step number `step` (no weight decay, no amsgrad) and, with `target`, the soft update
    target = param * tau + target * (1 - tau), in float64 from float32 (or any) inputs.  `grad` is the gradient the step itself
    wrote: the expectation then holds element by element, including the elements whose gradient is rounding noise.
    f32_hyper: lr, betas, eps, tau rounded to float32 first, as the device receives them (1 - float32(0.9) differs from 0.1 by
    2^-22 relative, the size of the moment bound).  blend_param: the parameters to blend into the target instead of the replayed
    ones (the device's own float32 result: the blend's expectation then does not inherit the parameter's rounding)."""
    rnd = _f32 if f32_hyper else float
    lr, b1, b2, eps = rnd(lr), rnd(betas[0]), rnd(betas[1]), rnd(eps)
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (param, exp_avg, exp_avg_sq, grad))
    m2 = m + (g - m) * (1.0 - b1)
    v2 = v * b2 + g * g * (1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p2 = p - (lr / bc1) * (m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps))
    out = {"param": p2, "exp_avg": m2, "exp_avg_sq": v2, "target": None}
    if target is not None:
        tau = rnd(tau)
        w = p2 if blend_param is None else np.asarray(blend_param, dtype=np.float64)
        out["target"] = w * tau + np.asarray(target, dtype=np.float64) * (1.0 - tau)
    return out


def adam_f32(param, exp_avg, exp_avg_sq, grad, step, lr, betas=(0.9, 0.999), eps=1e-8, target=None, tau=None):
    """The same step in float32 numpy, operation for operation as td3_apply_kernel forms it (bias corrections in double, rounded
    once): what the replay bounds have to hold for."""
    f = np.float32
    p, m, v, g = (np.asarray(x, dtype=f) for x in (param, exp_avg, exp_avg_sq, grad))
    lr, b1, b2, eps = f(lr), f(betas[0]), f(betas[1]), f(eps)
    step_size = lr / f(1.0 - float(b1) ** step)
    bc2_sqrt = f(np.sqrt(1.0 - float(b2) ** step))
    m2 = m + (g - m) * (f(1) - b1)
    v2 = v * b2 + g * g * (f(1) - b2)
    p2 = p - step_size * (m2 / (np.sqrt(v2) / bc2_sqrt + eps))
    out = {"param": p2, "exp_avg": m2, "exp_avg_sq": v2, "target": None}
    if target is not None:
        out["target"] = p2 * f(tau) + np.asarray(target, dtype=f) * (f(1) - f(tau))
    assert all(x is None or x.dtype == f for x in out.values())
    return out


def replay_bounds(rep, exp_avg_before, grad, lr, target_before=None):
    """Largest |device - replay| that float32 rounding explains, per element; derived from the operations, not measured.

      param    w' = w - step_size * (m' / (sqrt(v') / sqrt(bc2) + eps)).  The update is at most lr (1 - b1) / sqrt(1 - b2) (3.2 lr at
               the defaults) and is formed by about ten float32 operations (2^-24 relative each: ~2e-6 lr together with the
               absolute error of m' below, which the division by sqrt(v') >= sqrt(1 - b2) |g| amplifies to at most ~1.2e-6 lr);
               the final subtraction rounds to half an ulp of w'.  Bound: 2^-23 |w'| + 1e-5 lr.
      exp_avg  m' = m + (g - m)(1 - b1): three roundings (two with a fused multiply-add), each relative to an operand that is at
               most max(|m|, |g|) -- NOT relative to m', which can cancel (g = -9 m gives m' = 0 with the rounding error of the
               operands).  Bound: 2^-22 max(|m|, |g|).  (The first derivation had 2^-22 |m'|; float32 numpy breaks that on
               cancelling elements from step 2 on, test_td3_cases_cpu.py shows both.)
      exp_avg_sq  v' = v b2 + g g (1 - b2): four roundings of positive terms, no cancellation.  Bound: 2^-22 |v'| + 1e-37 (float32
               subnormals).
      target   t' = w' tau + t (1 - tau) with the device's own w' (adam_replay's blend_param): four roundings, each relative to at most
               max(|w'|, |t|).  Bound: 2^-22 max(|w'|, |t|)."""
    b = {"param": 2.0 ** -23 * np.abs(rep["param"]) + 1e-5 * lr,
         "exp_avg": 2.0 ** -22 * np.maximum(np.abs(np.asarray(exp_avg_before, dtype=np.float64)), np.abs(np.asarray(grad, dtype=np.float64))),
         "exp_avg_sq": 2.0 ** -22 * np.abs(rep["exp_avg_sq"]) + 1e-37}
    if target_before is not None:
        b["target"] = 2.0 ** -22 * np.maximum(np.abs(rep["param"]), np.abs(np.asarray(target_before, dtype=np.float64)))
    return b
