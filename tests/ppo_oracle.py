"""Test helper: the PPO minibatch gradient (the loss of the reference's elegantrl/agent.py:637-655) in plain numpy, forward and
backward written out by hand -- no torch, no autograd.  Float64 by default; dt=np.float32 runs the same operations in float32
(tests/test_ppo_cases_cpu.py uses it to show that the bar of the GPU sweep is not eaten by float32 itself).

Nets are dicts of arrays under the torch state_dict names:
  critic  (CriticAdv)                               net.0 / .2 / .4 ReLU, net.6 linear
  "plain" (ActorPPO, ActorResidualPPO)              net.0 / .2 / .4 Tanh, net.6 linear, a_std_log [1, 1]
  "modular" (ActorResidualIntegratorModularPPO)     other_net.0 / .2 Tanh on state[:, :D - Di], integrator_net.0 / .2 Tanh on
                                                    state[:, D - Di:], net.0 Tanh on their concatenation, net.2 linear, a_std_log

The objective of a minibatch (state s, pre-tanh action a, old log-prob, advantage, target r_sum; B samples):
  logp   = -(a_std_log + log sqrt(2 pi) + ((mean(s) - a) / exp(a_std_log))^2 / 2)
  ratio  = exp(logp - logp_old)
  surr   = min(adv * ratio, adv * clamp(ratio, 1 - clip, 1 + clip))          torch's backward: a tie of `min` splits the gradient
                                                                             in halves, `clamp` passes it on the closed interval
  obj_a  = -mean(surr) + lambda_entropy * mean(exp(logp) * logp)             (the reference's entropy proxy)
  obj_c  = mean(SmoothL1(v(s) - r_sum))                                      quadratic below |d| = 1, linear from there on
  united = obj_a + obj_c / (std_unbiased(r_sum) + 1e-5)
`gradients` returns d united / d every parameter, the three loss sums the kernels report, the critic scale and the two target
moments.  MUTANTS names one-line deviations of that arithmetic: a sweep that cannot tell the oracle from one of them is blind to
the branch the mutant changes (tests/test_ppo_cases_cpu.py holds every vetted case to that)."""
import numpy as np

LOG_SQRT_2PI = float(np.log(np.sqrt(2.0 * np.pi)))

CRITIC_LAYERS = ("net.0", "net.2", "net.4", "net.6")
PLAIN_LAYERS = ("net.0", "net.2", "net.4", "net.6")
MODULAR_LAYERS = ("other_net.0", "other_net.2", "integrator_net.0", "integrator_net.2", "net.0", "net.2")

# loss-level mutants change the per-sample loss gradients only; net-level mutants change a forward or backward pass of a net
MUTANTS_ACTOR_LOSS = ("no_clip",            # the clamp's backward mask dropped: the clipped branch passes the gradient on
                      "clip_any_sign",      # the clipped surrogate alone, whatever the advantage's sign (min dropped, surr2 kept)
                      "surr1_only",         # min dropped, surr1 kept
                      "no_entropy",         # lambda_entropy * mean(exp(logp) * logp) dropped
                      "entropy_sign",       # ... subtracted instead of added
                      "std_no_entropy")     # the gradient of a_std_log from the surrogate alone
MUTANTS_CRITIC_LOSS = ("l1_quadratic_only",  # SmoothL1 = d^2 / 2 everywhere
                       "l1_linear_only",     # SmoothL1 = |d| - 1 / 2 everywhere
                       "biased_std",         # std with 1 / B instead of 1 / (B - 1)
                       "no_scale")           # 1 / (std + 1e-5) not applied to the critic's gradients
MUTANTS_CRITIC_NET = ("open_relu_1", "open_relu_2", "open_relu_3")   # the backward pass ignores one layer's ReLU gate
MUTANTS_ACTOR_NET = ("tanh_drop_first",     # the derivative of the first Tanh (plain net.0, modular other_net.0) taken as 1
                     "tanh_drop_last")      # ... of the last Tanh (plain net.4, modular net.0)
MUTANTS_MODULAR = ("towers_swapped",        # concatenation [integrator, plant] instead of [plant, integrator]
                   "integrator_wrong_end")  # the integrator tower reads state[:, :Di], the plant tower the rest
MUTANTS_BOTH = ("drop_last_sample",         # sample B - 1 contributes to no sum (the means still divide by B)
                "drop_col_last")            # column D - 1 of the state reaches no first layer
MUTANTS = (MUTANTS_ACTOR_LOSS + MUTANTS_CRITIC_LOSS + MUTANTS_CRITIC_NET + MUTANTS_ACTOR_NET + MUTANTS_MODULAR + MUTANTS_BOTH)


def mutants_of(kind):
    """The mutants that are defined for an actor kind (the tower mutants need the modular actor)."""
    return tuple(m for m in MUTANTS if kind == "modular" or m not in MUTANTS_MODULAR)


def touches(mutant):
    """Which nets' gradients a mutant can move: "act", "cri" or both."""
    if mutant in MUTANTS_ACTOR_LOSS + MUTANTS_ACTOR_NET + MUTANTS_MODULAR:
        return ("act",)
    if mutant in MUTANTS_CRITIC_LOSS + MUTANTS_CRITIC_NET:
        return ("cri",)
    return ("act", "cri")


class Margin:
    """Running minimum per sample of the relative distance to a kink of the objective.  A layer's scale is the batch's largest
    |pre-activation| (or the larger of that and the one handed in, when a subset of a batch is looked at)."""

    def __init__(self, n, scales=None):
        self.m, self.given, self.scales = np.full(n, np.inf), scales, {}

    def layer(self, tag, z):
        sc = float(np.abs(z).max())
        if self.given is not None:
            sc = max(sc, self.given[tag])
        self.scales[tag] = sc
        self.m = np.minimum(self.m, np.abs(z).min(axis=1) / sc)

    def point(self, dist):
        self.m = np.minimum(self.m, np.abs(dist))


def _cast(p, dt):
    return {k: np.asarray(v, dtype=dt) for k, v in p.items()}


def _lin(p, name, x):
    return x @ p[name + ".weight"].T + p[name + ".bias"]


def _state(s, mutant):
    if mutant == "drop_col_last":
        s = s.copy()
        s[:, -1] = 0
    return s


# ------------------------------------------------------------------------------------------------------------------- critic
def critic_forward(cri, s, dt=np.float64, mg=None):
    """v(s) [B] of CriticAdv and the pre-activations of its three ReLU layers."""
    cri, x = _cast(cri, dt), np.asarray(s, dtype=dt)
    zs, h = [], x
    for i, name in enumerate(CRITIC_LAYERS[:3]):
        z = _lin(cri, name, h)
        if mg is not None:
            mg.layer(f"relu{i + 1}", z)
        zs.append(z)
        h = np.maximum(z, 0)
    return _lin(cri, "net.6", h)[:, 0], zs


def critic_pass(cri, s, r_sum, dt=np.float64, mutant=None, mg=None, light=False):
    """Gradients of obj_c / (std + 1e-5) for the critic's parameters, sum(SmoothL1), the scale and the target moments.
    light: the head's gradients only (what a loss-level mutant moves already)."""
    cri = _cast(cri, dt)
    x, r = _state(np.asarray(s, dtype=dt), mutant), np.asarray(r_sum, dtype=dt)
    B = len(r)
    v, zs = critic_forward(cri, x, dt, mg)
    hs = [x] + [np.maximum(z, 0) for z in zs]
    d = v - r
    if mg is not None:
        mg.point(np.abs(d) - 1)
    quad = np.abs(d) < 1
    if mutant == "l1_quadratic_only":
        quad = np.ones(B, dtype=bool)
    elif mutant == "l1_linear_only":
        quad = np.zeros(B, dtype=bool)
    loss = np.where(quad, d * d * dt(0.5), np.abs(d) - dt(0.5))
    g = np.where(quad, d, np.sign(d))
    std = r.std(ddof=0 if mutant == "biased_std" else 1) if B > 1 else dt(np.nan)
    scale = dt(1) / (std + dt(1e-5))
    gv = g * ((dt(1) if mutant == "no_scale" else scale) / dt(B))
    if mutant == "drop_last_sample":
        gv, loss = gv.copy(), loss.copy()
        gv[-1] = loss[-1] = 0
    r64 = np.asarray(r_sum, dtype=np.float32).astype(np.float64)
    out = {"sum_cri": float(loss.sum(dtype=np.float64)), "scale": float(scale), "moments": (float(r64.sum()), float((r64 * r64).sum()))}
    grads = {"net.6.weight": gv[None, :] @ hs[3], "net.6.bias": gv.sum(keepdims=True)}
    if not light:
        delta = gv[:, None] * cri["net.6.weight"]
        for i in (2, 1, 0):
            if mutant != f"open_relu_{i + 1}":
                delta = delta * (zs[i] > 0)
            name = CRITIC_LAYERS[i]
            grads[name + ".weight"], grads[name + ".bias"] = delta.T @ hs[i], delta.sum(axis=0)
            if i:
                delta = delta @ cri[name + ".weight"]
    out["grads"] = grads
    return out


# -------------------------------------------------------------------------------------------------------------------- actor
def actor_forward(act, kind, Di, s, dt=np.float64, mutant=None):
    """(mean [B], cache for the backward pass) of a plain or modular actor."""
    act, x = _cast(act, dt), _state(np.asarray(s, dtype=dt), mutant)
    if kind == "plain":
        hs = [x]
        for name in PLAIN_LAYERS[:3]:
            hs.append(np.tanh(_lin(act, name, hs[-1])))
        return _lin(act, "net.6", hs[-1])[:, 0], hs
    assert kind == "modular" and 1 <= Di < x.shape[1]
    Do = x.shape[1] - Di
    xo, xi = (x[:, Di:], x[:, :Di]) if mutant == "integrator_wrong_end" else (x[:, :Do], x[:, Do:])
    o1 = np.tanh(_lin(act, "other_net.0", xo))
    o2 = np.tanh(_lin(act, "other_net.2", o1))
    i1 = np.tanh(_lin(act, "integrator_net.0", xi))
    i2 = np.tanh(_lin(act, "integrator_net.2", i1))
    cat = np.concatenate([i2, o2] if mutant == "towers_swapped" else [o2, i2], axis=1)
    n1 = np.tanh(_lin(act, "net.0", cat))
    return _lin(act, "net.2", n1)[:, 0], (xo, o1, o2, xi, i1, i2, cat, n1)


def _dtanh(h, dropped):
    return 1 if dropped else 1 - h * h


def actor_backward(act, kind, cache, gm, dt=np.float64, mutant=None, light=False):
    """Gradients of sum(gm * mean) for the actor's net parameters."""
    act = _cast(act, dt)
    first, last = mutant == "tanh_drop_first", mutant == "tanh_drop_last"
    if kind == "plain":
        hs = cache
        grads = {"net.6.weight": gm[None, :] @ hs[3], "net.6.bias": gm.sum(keepdims=True)}
        if light:
            return grads
        delta = gm[:, None] * act["net.6.weight"]
        for i in (2, 1, 0):
            delta = delta * _dtanh(hs[i + 1], (first and i == 0) or (last and i == 2))
            name = PLAIN_LAYERS[i]
            grads[name + ".weight"], grads[name + ".bias"] = delta.T @ hs[i], delta.sum(axis=0)
            if i:
                delta = delta @ act[name + ".weight"]
        return grads
    xo, o1, o2, xi, i1, i2, cat, n1 = cache
    grads = {"net.2.weight": gm[None, :] @ n1, "net.2.bias": gm.sum(keepdims=True)}
    if light:
        return grads
    dn = gm[:, None] * act["net.2.weight"] * _dtanh(n1, last)
    grads["net.0.weight"], grads["net.0.bias"] = dn.T @ cat, dn.sum(axis=0)
    dcat = dn @ act["net.0.weight"]
    half = o2.shape[1]
    d_o2, d_i2 = (dcat[:, half:], dcat[:, :half]) if mutant == "towers_swapped" else (dcat[:, :half], dcat[:, half:])
    for tower, x, h1, h2, d2, drop in (("other_net", xo, o1, o2, d_o2, first), ("integrator_net", xi, i1, i2, d_i2, False)):
        d2 = d2 * _dtanh(h2, False)
        grads[tower + ".2.weight"], grads[tower + ".2.bias"] = d2.T @ h1, d2.sum(axis=0)
        d1 = (d2 @ act[tower + ".2.weight"]) * _dtanh(h1, drop)
        grads[tower + ".0.weight"], grads[tower + ".0.bias"] = d1.T @ x, d1.sum(axis=0)
    return grads


def logprob(act, kind, Di, s, a, dt=np.float64):
    """log-probability of the pre-tanh actions a [B] under the policy (GaussianHead.compute_logprob)."""
    asl = dt(np.asarray(act["a_std_log"]).reshape(-1)[0])
    mean, _ = actor_forward(act, kind, Di, s, dt)
    z = (mean - np.asarray(a, dtype=dt)) / np.exp(asl)
    return -(asl + dt(LOG_SQRT_2PI) + z * z * dt(0.5))


def actor_pass(act, kind, Di, s, a, logp_old, adv, clip, lam, dt=np.float64, mutant=None, mg=None, light=False):
    """Gradients of obj_a for the actor's parameters (a_std_log included), sum(-surr) and sum(exp(logp) * logp)."""
    a, lp_old, adv = (np.asarray(v, dtype=dt) for v in (a, logp_old, adv))
    B = len(a)
    clip, lam = dt(clip), dt(lam)
    asl = dt(np.asarray(act["a_std_log"]).reshape(-1)[0])
    mean, cache = actor_forward(act, kind, Di, s, dt, mutant)
    inv_std = np.exp(-asl)
    z = (mean - a) * inv_std
    lp = -(asl + dt(LOG_SQRT_2PI) + z * z * dt(0.5))
    ratio = np.exp(lp - lp_old)
    lo, hi = dt(1) - clip, dt(1) + clip
    if mg is not None:   # the clip is live above 1 + clip for a positive advantage, below 1 - clip for a negative one
        mg.point(np.where(adv >= 0, ratio - hi, ratio - lo))
    s1, s2 = adv * ratio, adv * np.clip(ratio, lo, hi)
    inside = ((ratio >= lo) & (ratio <= hi)).astype(dt)
    w1 = (s1 < s2) + dt(0.5) * (s1 == s2)
    w2 = (s2 < s1) + dt(0.5) * (s1 == s2)
    if mutant == "no_clip":
        inside = np.ones(B, dtype=dt)
    elif mutant == "clip_any_sign":
        w1, w2 = np.zeros(B, dtype=dt), np.ones(B, dtype=dt)
    elif mutant == "surr1_only":
        w1, w2 = np.ones(B, dtype=dt), np.zeros(B, dtype=dt)
    surr = s2 if mutant == "clip_any_sign" else s1 if mutant == "surr1_only" else np.minimum(s1, s2)
    p = np.exp(lp)
    ent = p * lp
    lam_g = dt(0) if mutant == "no_entropy" else -lam if mutant == "entropy_sign" else lam
    g_sur = -(adv * (w1 + w2 * inside)) * ratio / dt(B)      # d(-mean surr) / d logp
    g_ent = lam_g * p * (lp + dt(1)) / dt(B)                  # d(lambda * mean(exp(logp) logp)) / d logp
    if mutant == "drop_last_sample":
        g_sur, g_ent, surr, ent = g_sur.copy(), g_ent.copy(), surr.copy(), ent.copy()
        g_sur[-1] = g_ent[-1] = surr[-1] = ent[-1] = 0
    g_lp = g_sur + g_ent
    grads = actor_backward(act, kind, cache, g_lp * (-z * inv_std), dt, mutant, light)
    grads["a_std_log"] = ((g_sur if mutant == "std_no_entropy" else g_lp) * (z * z - dt(1))).sum().reshape(1, 1)
    return {"grads": grads, "sum_sur": float(-surr.sum(dtype=np.float64)), "sum_ent": float(ent.sum(dtype=np.float64)),
            "ratio": ratio, "adv": adv}


def gradients(act, cri, kind, Di, batch, clip, lam, dt=np.float64, mutant=None, margins=False, light=False):
    """batch = (state [B, D], action [B], logprob_old [B], adv [B], r_sum [B]).  Returns {"ga": actor gradients by parameter name
    (with "a_std_log"), "gc": critic gradients, "sums": (sum(-surr), sum(exp(logp) logp), sum(SmoothL1)), "scale", "moments",
    "ratio", "d": v - r_sum, and with margins=True "margin" [B] and "scales"}."""
    s, a, lp_old, adv, r = batch
    mg = Margin(len(r)) if margins else None
    A = actor_pass(act, kind, Di, s, a, lp_old, adv, clip, lam, dt, mutant, mg, light)
    Cr = critic_pass(cri, s, r, dt, mutant, mg, light)
    out = {"ga": A["grads"], "gc": Cr["grads"], "sums": (A["sum_sur"], A["sum_ent"], Cr["sum_cri"]), "scale": Cr["scale"],
           "moments": Cr["moments"], "ratio": A["ratio"]}
    if margins:
        out["margin"], out["scales"] = mg.m, mg.scales
    return out


def sample_margins(act, cri, kind, Di, batch, clip, scales=None):
    """Forward passes only: every sample's kink margin (float64) and the layer scales.  The kinks: ratio at 1 + clip (advantage
    >= 0) or 1 - clip (advantage < 0), |v - r_sum| at 1, every critic ReLU pre-activation at 0 (relative to the layer's scale)."""
    s, a, lp_old, adv, r = (np.asarray(v, dtype=np.float64) for v in batch)
    mg = Margin(len(r), scales)
    ratio = np.exp(logprob(act, kind, Di, s, a) - lp_old)
    mg.point(np.where(adv >= 0, ratio - (1 + clip), ratio - (1 - clip)))
    v, _ = critic_forward(cri, s, np.float64, mg)
    mg.point(np.abs(v - r) - 1)
    return mg.m, mg.scales, ratio, v - r
