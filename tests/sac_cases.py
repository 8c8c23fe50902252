"""Test helper: seeded cases for the fused SAC step (csrc/sac_fused.hip), their kink margins and oracle mutants, in the mould of
tests/td3_cases.py (whose Adam replay and replay bounds are reused: the apply launch is the same kernel).  Shared by
tests/test_sac_cases_cpu.py and tests/test_gpu_sac_sweep.py so that the CPU tests see bit for bit what the GPU tests run.

The same three numbers rule the inputs (conditions on the INPUTS, checked on the CPU; none is a tolerance on a kernel):

  * DELTA = 1e-5, the kink margin.  The SAC objective is not differentiable where a first-layer ReLU pre-activation (actor, both
    critics) is 0, where a Hardswish pre-activation of the actor's second or third layer is -3 or +3, where the log-std head is
    -20 or 2, where the twin target heads are equal (in the label AND under the actor objective) and where |q - label| = 1.
    Samples whose relative distance to any such point is below DELTA are redrawn; at most MAX_REDRAWN of a case's samples may be
    (a cap, not a measurement: a case that needs more changes its scales).
  * MUTATION_MARGIN = 10 (x the 3e-4 bar).  Every mutant of the oracle (sac_oracle.MUTANTS) must move at least one gradient tensor
    of every vetted case by 10 x the bar.  Two mutants need hyper-parameters away from the agent's defaults to be visible at all:
    "alpha_before" (alpha taken before instead of after the temperature step) moves the actor objective by the relative change of
    alpha in one Adam step, about the temperature's learning rate; "target_before" (the target critic before instead of after the
    soft update) by tau x the distance between the critics.  The cases therefore step the temperature with lr_alpha = 0.3 and
    blend with tau = 0.3 (and keep the nets' own learning rate at 1e-4): conditions on inputs, like TD3's policy_noise = 0.6.
  * F32_STABILITY = 1e-4: the reference arithmetic in float32 numpy must agree with float64 to that much of each gradient tensor's
    largest entry -- in particular 1.000001 - tanh(u)^2 must not eat the bar; the CPU test decides, not a bound on |u|.

The generator's scales make the branches ACTIVE that the reference's own initialisation never reaches: Hardswish pre-activations
of standard deviation 1.5 (2 % of a layer's units beyond each knee, on most samples some unit; at 2.5 the knees add
2 % to the 3.3 % of the samples of a width-128 case that sit within DELTA of a ReLU gate: too close to the cap for the small cases), a log-std head of mean -10 and standard deviation 8 (about 7 % of
the samples above 2 and a tenth below -20).  A clamped sample has std = e^2 = 7.4; with standard normal draws |u| = |avg + std eps|
would pass 6 on most of them, where float32 loses 1 - tanh(u)^2 (it is 2.5e-5 at |u| = 6, next to a rounding error of 1e-7 and the
1e-6 of the reference's 1.000001): the reference arithmetic itself then misses F32_STABILITY by a factor of ten to a hundred.  The
cases' noise tables are therefore normal draws of standard deviation NOISE_SCALE = 0.2 -- to the kernels a table is any float32
array; the in-kernel Philox draws are tested on the reference's own nets (tests/test_gpu_sac_fused.py).
With log-stds around -10 the "logprob" is around -10 too; the cases start from alpha = exp(-3) = 0.05 so that the entropy term of
the label is a few tenths, like the rewards and the q values, and |q - label| straddles 1 with most samples in the quadratic
branch of SmoothL1 (at alpha = 1 nearly every sample sits in the linear branch, whose gradient ignores the label's value)."""
import collections
import functools

import numpy as np

import sac_oracle as S
from oracle.td3 import CRITIC_KEYS
from td3_cases import _Margin, adam_replay, flatten, replay_bounds, unflatten   # noqa: F401  (replay_bounds: for the GPU tests)

DELTA = 1e-5
BAR = 3e-4
MUTATION_MARGIN = 10.0
F32_STABILITY = 1e-4
MAX_REDRAWN = 0.10
NOISE_SCALE = 0.2

WIDTHS = (64, 128)
ALL_D = tuple(range(1, 8))
COMPILED_D = (3, 4)


def served():
    """Every (width, state_dim) that pime_sac_supported claims (action_dim 1)."""
    return [(w, D) for w in WIDTHS for D in ALL_D]


def kernel_class(width, D):
    """The instantiation launch_sac_grad picks: the state width compiled in (3: pH, 4: tank Integrator), else run-time D."""
    return width, f"D{D}" if D in COMPILED_D else "rt2"


ALL_CLASSES = tuple((w, k) for w in WIDTHS for k in ("D3", "D4", "rt2"))

Hyper = collections.namedtuple("Hyper", "lr lr_alpha betas eps tau target_entropy alpha_log0")
DEFAULT_HYPER = Hyper(1e-4, 0.3, (0.9, 0.999), 1e-8, 0.3, 0.0, -3.0)
OTHER_HYPER = Hyper(3e-4, 0.2, (0.8, 0.99), 1e-6, 0.2, -0.7, -2.5)   # nothing at its default

Spec = collections.namedtuple("Spec", "width D B rows row hyper vet")


def spec(width, D, B, rows=1, row=0, hyper=DEFAULT_HYPER, vet=True):
    return Spec(width, D, B, rows, row, hyper, vet)


def spec_id(s):
    tag = f"{s.width}-D{s.D}-B{s.B}"
    if s.rows > 1:
        tag += f"-row{s.row}of{s.rows}"
    if s.hyper != DEFAULT_HYPER:
        tag += "-hyper2"
    return tag


def shape_cases():
    """Every supported (width, D) at B = 37 (three 16-sample tiles, the last one ragged)."""
    return [spec(w, D, 37) for w, D in served()]


REGIME_B = (1, 17, 8193)
_RT_D = (1, 2, 7, 5, 6, 7)


def regime_cases():
    """Every instantiation x B in {1, 17, 8193}; D varies inside the run-time class so that 1, 2, 5, 6, 7 all occur."""
    out = []
    for i, w in enumerate(WIDTHS):
        for j, B in enumerate(REGIME_B):
            for D in COMPILED_D + (_RT_D[3 * i + j],):
                out.append(spec(w, D, B))
    return out


HYPER_SHAPES = ((64, 3, 100), (128, 7, 100))


def hyper_cases():
    """A four-row table stepped at row 3 on a fresh agent (Adam step number 4), every hyper-parameter off its default."""
    return [spec(w, D, B, rows=4, row=3, hyper=OTHER_HYPER) for w, D, B in HYPER_SHAPES]


def gradient_specs():
    seen = []
    for s in shape_cases() + regime_cases() + hyper_cases():
        if s not in seen:
            seen.append(s)
    return seen


# ---------------------------------------------------------------------------------------------------------------- generator
# A sample of a width-128 case has about 2 000 kinks within reach (ReLU gates and Hardswish knees of five forward passes) and
# lands within DELTA of one with probability ~0.05; a B = 17 case, which may redraw ONE sample, then trips the cap with probability
# ~0.2 by chance alone, and the one-element bias gradients of a B = 17 case are sums of 17 terms that can cancel to a tenth of a
# term (float32 then keeps 1e-4 of them).  SALT is the first of 0, 1, 2, ... for which every listed case meets the redraw cap and
# F32_STABILITY (test_sac_cases_cpu.py); it was fixed on the CPU before any kernel existed and is a property of the inputs only.
SALT = 1
N_BUF = 2048   # replay rows of a case; samples draw from [2, N_BUF - 3), positions 0 and B - 1 name row 0 and row N_BUF - 2


def _linear(rng, n_out, n_in):
    k = 1.0 / np.sqrt(n_in)
    return rng.uniform(-k, k, (n_out, n_in)), rng.uniform(-k, k, n_out)


def make_nets(width, D, seed):
    """(act, cri, cri_target) state dicts, float32; the scales of the module docstring are set on 256 probe rows."""
    rng = np.random.RandomState([seed, width, D, 23])
    probe = rng.uniform(-1.5, 1.5, (256, D))
    act = {}
    for name, (o, i) in (("net_state.0", (width, D)), ("net_state.2", (width, width)), ("net_state.4", (width, width)),
                         ("net_a_avg", (1, width)), ("net_a_std", (1, width))):
        act[name + ".weight"], act[name + ".bias"] = _linear(rng, o, i)
    for layer, z in (("net_state.2", "z2"), ("net_state.4", "z3")):   # Hardswish pre-activations: standard deviation 1.5
        k = 1.5 / S.actor_forward(act, probe)[z].std()
        act[layer + ".weight"] *= k
        act[layer + ".bias"] *= k
    for head, key, mean, std in (("net_a_avg", "avg", rng.uniform(-0.2, 0.2), 1.0), ("net_a_std", "raw", -10.0, 8.0)):
        v = S.actor_forward(act, probe)[key]
        act[head + ".weight"] *= std / v.std()
        act[head + ".bias"][:] = mean - (v.mean() - act[head + ".bias"]) * std / v.std()

    cri = {}
    for name, (o, i) in (("net_sa.0", (width, D + 1)), ("net_sa.2", (width, width)), ("net_q1", (1, width)), ("net_q2", (1, width))):
        cri[name + ".weight"], cri[name + ".bias"] = _linear(rng, o, i)
    cri["net_sa.0.weight"][:, -1] = rng.uniform(-1.0, 1.0, width)   # an action column of order 0.5: the action reaches q
    cri_t = {k: v + rng.standard_normal(v.shape) * (0.3 * v.std() if v.size > 1 else 0.1) for k, v in cri.items()}
    pa = np.tanh(rng.standard_normal((256, 1)))
    for c in (cri, cri_t):     # both heads on the probe rows: mean within +-0.3 (each its own), standard deviation 0.6
        for h in ("net_q1", "net_q2"):
            q = S.critic_fw(c, probe, pa)[3 if h == "net_q1" else 4]
            c[h + ".weight"] *= 0.6 / q.std()
            c[h + ".bias"][:] = rng.uniform(-0.3, 0.3) - (q.mean() - c[h + ".bias"]) * 0.6 / q.std()
    return tuple({k: v.astype(np.float32) for k, v in p.items()} for p in (act, cri, cri_t))


Case = collections.namedtuple("Case", "spec nets state other idx nxt noise_next noise_pg redraw_rounds redrawn mid")


def _draw_rows(rng, n, D):
    state = rng.uniform(-1.5, 1.5, (n, D)).astype(np.float32)
    other = np.stack([rng.standard_normal(n) * 0.4, np.where(rng.rand(n) < 0.2, 0.0, 0.99), np.tanh(rng.standard_normal(n))],
                     axis=1).astype(np.float32)   # reward of a few tenths, 20 % terminal rows, stored action
    return state, other


@functools.lru_cache(maxsize=None)
def build(s):
    """The case of a spec: nets, replay rows [N_BUF], index tables idx / nxt [rows, B] (nxt = idx + 1), two noise tables [rows, B].
    With s.vet, the samples of row s.row whose margin is below DELTA get a new replay row and new draws until none is left
    (positions 0 and B - 1, which name replay row 0 and the last row with a successor, keep their index: the CONTENT of their
    replay rows is drawn again instead).  Case.redrawn counts the samples of the first pass that had to go."""
    seed = (s.width * 1000003 + s.D * 10007 + s.B * 101 + s.rows * 7 + s.row) % (2 ** 31)
    rng = np.random.RandomState([seed, SALT, int(s.hyper != DEFAULT_HYPER)])
    nets = make_nets(s.width, s.D, seed)
    state, other = _draw_rows(rng, N_BUF, s.D)
    idx = rng.randint(2, N_BUF - 3, size=(s.rows, s.B)).astype(np.int64)
    n1 = (rng.standard_normal((s.rows, s.B)) * NOISE_SCALE).astype(np.float32)
    n2 = (rng.standard_normal((s.rows, s.B)) * NOISE_SCALE).astype(np.float32)
    if s.B >= 2:
        fixed = {0: 0, s.B - 1: N_BUF - 2}
    else:
        fixed = {0: N_BUF - 2} if s.D % 2 else {0: 0}
    for pos, r in fixed.items():
        idx[s.row, pos] = r
    rounds, redrawn, mid = 0, 0, None
    while s.vet:
        case = Case(s, nets, state, other, idx, idx + 1, n1, n2, rounds, redrawn, None)
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
                n1[s.row, pos], n2[s.row, pos] = rng.standard_normal(2) * NOISE_SCALE
            case = Case(s, nets, state, other, idx, idx + 1, n1, n2, rounds, redrawn, None)
            m = reference_step(case, margins=True, subset=bad, given=mid)["margin"]
            bad = bad[m < 2 * DELTA]   # (twice: the whole-batch pass that follows moves the scales and the mid-step values a little)
    for a in (state, other, idx, n1, n2):
        a.setflags(write=False)
    return Case(s, nets, state, other, idx, idx + 1, n1, n2, rounds, redrawn, mid)   # mid: reference_step of the final inputs


def batch_of(case, subset=None):
    s = case.spec
    idx, nxt, e1, e2 = case.idx[s.row], case.nxt[s.row], case.noise_next[s.row], case.noise_pg[s.row]
    if subset is not None:
        idx, nxt, e1, e2 = idx[subset], nxt[subset], e1[subset], e2[subset]
    o = case.other[idx]
    return (case.state[idx], o[:, 2], o[:, 0], o[:, 1], case.state[nxt], e1), e2


def temperature_replay(h, alpha_log, m, v, g, step):
    """The scalar Adam step of alpha_log (float64 from the values given), as a dict like adam_replay's."""
    return adam_replay(np.array([alpha_log]), np.array([m]), np.array([v]), np.array([g]), step, h.lr_alpha, h.betas, h.eps)


def reference_step(case, dt=np.float64, margins=False, subset=None, given=None):
    """The stepped row of a case on a fresh agent (zero moments; the step number is row + 1, as the apply launch counts): critic
    objective and gradients (dtype dt), the critic's Adam step and the soft update replayed in float64 from those gradients, the
    temperature's gradient mean(lp) - target_entropy and its Adam step, then the actor objective with the new alpha through the
    target critic AS THE STEP LEFT IT.  margins=True: every sample's kink margin over the five forward passes.  subset / given:
    the margins of some samples only, against the whole batch's scales and mid-step values (cri_t_actor, alpha1) of `given`."""
    s, h = case.spec, case.spec.hyper
    act, cri, cri_t = case.nets
    batch, eps_pg = batch_of(case, subset)
    mg = _Margin(len(batch[0]), None if given is None else given["scales"]) if margins else None
    alpha0 = float(np.exp(h.alpha_log0))
    obj_c, gc = S.critic_objective(act, cri, cri_t, batch, alpha0, dt, None, mg)
    if given is None:
        c0 = flatten(cri, CRITIC_KEYS)
        rep = adam_replay(c0, np.zeros_like(c0), np.zeros_like(c0), flatten(gc, CRITIC_KEYS), s.row + 1, h.lr, h.betas, h.eps,
                          target=flatten(cri_t, CRITIC_KEYS), tau=h.tau)
        cri_after = unflatten(rep["param"], cri, CRITIC_KEYS)
        cri_t_actor = unflatten(rep["target"], cri_t, CRITIC_KEYS)
        g_alpha = S.policy_logprob(act, batch[0], eps_pg, dt) - h.target_entropy
        alpha_log1 = float(temperature_replay(h, h.alpha_log0, 0.0, 0.0, g_alpha, s.row + 1)["param"][0])
    else:
        cri_after, cri_t_actor, g_alpha, alpha_log1 = given["cri_after"], given["cri_t_actor"], given["g_alpha"], given["alpha_log1"]
    obj_a, ga = S.actor_objective(act, cri_t_actor, batch[0], eps_pg, float(np.exp(alpha_log1)), dt, None, mg)
    out = {"obj_c": obj_c, "obj_a": obj_a, "obj_alpha": h.alpha_log0 * g_alpha, "gc": gc, "ga": ga, "g_alpha": g_alpha,
           "alpha_log1": alpha_log1, "cri_after": cri_after, "cri_t_actor": cri_t_actor}
    if margins:
        sc = mg.scales if given is None else {k: max(v, given["scales"][k]) for k, v in mg.scales.items()}
        out["margin"], out["scales"] = mg.m, sc
    return out


def mutant_reach(case, mid, mutant):
    """Largest |mutant's gradient - oracle's| / max|oracle's| over the gradient tensors the mutant can touch (the critic's for the
    label mutants, the actor's for the actor-objective mutants, both for the policy mutants); the bias and head gradients first
    (a lower bound of the reach, cheaper), all tensors if that does not already exceed MUTATION_MARGIN x BAR."""
    h = case.spec.hyper
    act, cri, cri_t = case.nets
    batch, eps_pg = batch_of(case)
    alpha0, alpha1 = float(np.exp(h.alpha_log0)), float(np.exp(mid["alpha_log1"]))
    reach = 0.0
    for light in (True, False):
        pairs = []
        if mutant in S.MUTANTS_CRITIC + S.MUTANTS_POLICY:
            pairs.append((mid["gc"], S.critic_objective(act, cri, cri_t, batch, alpha0, mutant=mutant, light=light)[1]))
        if mutant in S.MUTANTS_ACTOR + S.MUTANTS_POLICY:
            crit = {"target_before": cri_t, "online_critic": mid["cri_after"]}.get(mutant, mid["cri_t_actor"])
            alpha = alpha0 if mutant == "alpha_before" else alpha1
            pairs.append((mid["ga"], S.actor_objective(act, crit, batch[0], eps_pg, alpha, mutant=mutant, light=light)[1]))
        reach = max(float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()) for want, got in pairs for k in got)
        if reach > MUTATION_MARGIN * BAR:
            break
    return reach
