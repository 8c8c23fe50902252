"""Test helper: numpy restatement (float64 by default) of one SAC optimizer step -- TEST INFRASTRUCTURE ONLY, beside the tests
because nothing under oracle/ changes.  Follows the reference line by line (paths under /root/reference):
  * elegantrl/net.py:175-239   ActorSAC: D -> md ReLU -> md Hardswish -> md Hardswish, heads net_a_avg / net_a_std;
                               get_action_logprob: ls = clamp(net_a_std, -20, 2), u = avg + exp(ls) * eps, a = tanh(u),
                               "logprob" = ls + log(sqrt(2 pi)) + ((avg - u) / std)^2 / 2 + log(1.000001 - a^2) -- the NEGATIVE
                               log-density, used with that sign throughout.  ((avg - u) / std)^2 / 2 is eps^2 / 2 and carries no
                               gradient: its derivatives with respect to avg and std cancel analytically.)
  * elegantrl/net.py:305-332   CriticTwin (oracle.td3.critic_hidden)
  * elegantrl/agent.py:519-527 get_obj_critic_raw: q_label = r + mask * (min(cri_target(s', a')) + lp' * alpha) with the ONLINE actor
  * elegantrl/agent.py:442-468 the loop body: critic Adam, soft update on every step, temperature objective
                               alpha_log * mean(lp - target_entropy) and its Adam, alpha = exp(alpha_log) after it,
                               obj_actor = -(min(cri_target(s, a_pg)) + lp * alpha).mean() through the target critic as the soft
                               update left it, actor Adam
`mutant` changes ONE branch of the arithmetic (tests/sac_cases.py lists them and checks that the gradient tests can see each);
`mg` collects every sample's distance to the kinks of the objective."""
import numpy as np

from oracle.td3 import CRITIC_KEYS, Adam, critic_hidden, smooth_l1, soft_update   # noqa: F401  (re-exported)

ACTOR_KEYS = ["net_state.0.weight", "net_state.0.bias", "net_state.2.weight", "net_state.2.bias", "net_state.4.weight",
              "net_state.4.bias", "net_a_avg.weight", "net_a_avg.bias", "net_a_std.weight", "net_a_std.bias"]
LOG_SQRT_2PI = float(np.log(np.sqrt(2 * np.pi)))

MUTANTS_CRITIC = ("label_q1_only", "label_q2_only", "mask_ignored", "label_no_entropy", "all_quadratic", "all_linear")
MUTANTS_POLICY = ("no_tanh_correction", "no_clamp", "relu_for_hardswish_2", "relu_for_hardswish_3")   # reach both objectives
MUTANTS_ACTOR = ("actor_q1_only", "actor_q2_only", "actor_no_entropy", "alpha_before", "target_before", "online_critic")
MUTANTS = MUTANTS_CRITIC + MUTANTS_POLICY + MUTANTS_ACTOR


def f64(sd, keys):
    return {k: np.asarray(sd[k], dtype=np.float64).copy() for k in keys}


def cast(p, dt):
    return {k: np.asarray(v, dtype=dt) for k, v in p.items()}


def hardswish(x):
    return x * np.clip(x + 3.0, 0.0, 6.0) / 6.0


def hardswish_grad(x):
    """torch's hardswish_backward: 0 below -3, x / 3 + 0.5 up to and including 3, 1 above."""
    return np.where(x < -3.0, 0.0, np.where(x <= 3.0, x / 3.0 + 0.5, 1.0))


def actor_forward(p, s, eps=None, mutant=None):
    """Every intermediate of ActorSAC on the rows s (dtype of p); with eps also the sample, its tanh and the "logprob"."""
    dt = p["net_state.0.weight"].dtype.type
    f = {}
    f["z1"] = s @ p["net_state.0.weight"].T + p["net_state.0.bias"]
    f["h1"] = np.maximum(f["z1"], 0)
    f["z2"] = f["h1"] @ p["net_state.2.weight"].T + p["net_state.2.bias"]
    f["h2"] = np.maximum(f["z2"], 0) if mutant == "relu_for_hardswish_2" else hardswish(f["z2"])
    f["z3"] = f["h2"] @ p["net_state.4.weight"].T + p["net_state.4.bias"]
    f["h3"] = np.maximum(f["z3"], 0) if mutant == "relu_for_hardswish_3" else hardswish(f["z3"])
    f["avg"] = f["h3"] @ p["net_a_avg.weight"].T + p["net_a_avg.bias"]
    f["raw"] = f["h3"] @ p["net_a_std.weight"].T + p["net_a_std.bias"]
    f["ls"] = f["raw"] if mutant == "no_clamp" else np.clip(f["raw"], -20.0, 2.0)
    f["std"] = np.exp(f["ls"])
    if eps is not None:
        e = np.asarray(eps, dtype=dt).reshape(-1, 1)
        f["eps"] = e
        f["u"] = f["avg"] + f["std"] * e
        f["a"] = np.tanh(f["u"])
        f["corr"] = dt(1.000001) - f["a"] * f["a"]
        f["lp"] = f["ls"] + dt(LOG_SQRT_2PI) + e * e * dt(0.5)
        if mutant != "no_tanh_correction":
            f["lp"] = f["lp"] + np.log(f["corr"])
    return f


def actor_margins(mg, tag, f):
    """Kinks of one ActorSAC forward: the ReLU gates, the Hardswish knees at +-3, the log-std clamp at -20 and 2."""
    mg.layer(f"{tag}0", f["z1"])
    for key, knees in (("z2", (-3.0, 3.0)), ("z3", (-3.0, 3.0)), ("raw", (-20.0, 2.0))):
        z = f[key]
        sc = mg.scales[tag + key] = float(np.abs(z).max())   # distances relative to the layer's largest pre-activation
        sc = max(sc, (mg.given or {}).get(tag + key, 0.0))
        for k in knees:
            mg.point(np.abs(z - k).min(axis=1) / sc)


def actor_backward(p, f, s, g_a, g_lp, mutant=None, light=False):
    """Gradients of ActorSAC's ten tensors from d obj / d a (the squashed action) and d obj / d lp, per sample [B, 1]."""
    a = f["a"]
    g_a = g_a if mutant == "no_tanh_correction" else g_a + g_lp * (-2.0 * a / f["corr"])
    g_u = g_a * (1.0 - a * a)
    g_avg = g_u
    open_clamp = np.ones_like(f["raw"]) if mutant == "no_clamp" else ((f["raw"] >= -20.0) & (f["raw"] <= 2.0))
    g_raw = (g_u * f["std"] * f["eps"] + g_lp) * open_clamp
    g = {"net_a_avg.weight": g_avg.T @ f["h3"], "net_a_avg.bias": g_avg.sum(0),
         "net_a_std.weight": g_raw.T @ f["h3"], "net_a_std.bias": g_raw.sum(0)}
    d3 = g_avg @ p["net_a_avg.weight"] + g_raw @ p["net_a_std.weight"]
    d3 = d3 * ((f["z3"] > 0) if mutant == "relu_for_hardswish_3" else hardswish_grad(f["z3"]))
    d2 = d3 @ p["net_state.4.weight"]
    d2 = d2 * ((f["z2"] > 0) if mutant == "relu_for_hardswish_2" else hardswish_grad(f["z2"]))
    d1 = (d2 @ p["net_state.2.weight"]) * (f["h1"] > 0)
    g["net_state.4.bias"], g["net_state.2.bias"], g["net_state.0.bias"] = d3.sum(0), d2.sum(0), d1.sum(0)
    if not light:
        g["net_state.4.weight"], g["net_state.2.weight"], g["net_state.0.weight"] = d3.T @ f["h2"], d2.T @ f["h1"], d1.T @ s
    return g


def critic_fw(p, s, a):
    """oracle.td3.critic_hidden with the pre-activations (for the margins)."""
    x = np.concatenate([s, a], axis=1)
    z1 = x @ p["net_sa.0.weight"].T + p["net_sa.0.bias"]
    c1 = np.maximum(z1, 0)
    z2 = c1 @ p["net_sa.2.weight"].T + p["net_sa.2.bias"]
    c2 = np.maximum(z2, 0)
    return x, (z1, z2), (c1, c2), c2 @ p["net_q1.weight"].T + p["net_q1.bias"], c2 @ p["net_q2.weight"].T + p["net_q2.bias"]


def critic_objective(act, cri, cri_t, batch, alpha, dt=np.float64, mutant=None, mg=None, light=False):
    """(obj_critic, gradients of the online critic): agent.py:519-527 + backward().  batch = (s, a, r, m, s2, eps_next)."""
    act, cri, cri_t = cast(act, dt), cast(cri, dt), cast(cri_t, dt)
    s, a, r, m, s2, eps = (np.asarray(v, dtype=dt) for v in batch)
    B = len(s)
    fn = actor_forward(act, s2, eps, mutant if mutant in MUTANTS_POLICY else None)
    _, ztc, _, tq1, tq2 = critic_fw(cri_t, s2, fn["a"])
    tq = tq1 if mutant == "label_q1_only" else tq2 if mutant == "label_q2_only" else np.minimum(tq1, tq2)
    mask = np.full((B, 1), dt(0.99)) if mutant == "mask_ignored" else m.reshape(B, 1)
    ent = 0.0 if mutant == "label_no_entropy" else fn["lp"] * dt(alpha)
    label = r.reshape(B, 1) + mask * (tq + ent)
    x, zc, (c1, c2), q1, q2 = critic_fw(cri, s, a.reshape(B, 1))
    if mg is not None:
        actor_margins(mg, "act_next", fn)
        for i, z in enumerate(ztc):
            mg.layer(f"cri_t{i}", z)
        for i, z in enumerate(zc):
            mg.layer(f"cri{i}", z)
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
        return smooth_l1(d)
    l1, g1 = smooth(q1 - label)
    l2, g2 = smooth(q2 - label)
    obj = l1.mean() + l2.mean()
    g1, g2 = g1 / B, g2 / B
    g = {"net_q1.weight": g1.T @ c2, "net_q1.bias": g1.sum(0), "net_q2.weight": g2.T @ c2, "net_q2.bias": g2.sum(0)}
    dz2 = (g1 @ cri["net_q1.weight"] + g2 @ cri["net_q2.weight"]) * (c2 > 0)
    g["net_sa.2.bias"] = dz2.sum(0)
    dz1 = (dz2 @ cri["net_sa.2.weight"]) * (c1 > 0)
    g["net_sa.0.bias"] = dz1.sum(0)
    if not light:
        g["net_sa.2.weight"], g["net_sa.0.weight"] = dz2.T @ c1, dz1.T @ x
    return obj, g


def policy_logprob(act, s, eps, dt=np.float64, mutant=None):
    """mean of the "logprob" of a_pg on the rows s: the temperature's gradient is this minus target_entropy."""
    f = actor_forward(cast(act, dt), np.asarray(s, dtype=dt), eps, mutant if mutant in MUTANTS_POLICY else None)
    return float(f["lp"].mean())


def actor_objective(act, cri_t, s, eps, alpha, dt=np.float64, mutant=None, mg=None, light=False):
    """(obj_actor, gradients of the actor): -(min(cri_target.get_q1_q2(s, a_pg)) + lp * alpha).mean(), agent.py:463-468."""
    act, cri_t, s = cast(act, dt), cast(cri_t, dt), np.asarray(s, dtype=dt)
    B = len(s)
    f = actor_forward(act, s, eps, mutant if mutant in MUTANTS_POLICY else None)
    _, zc, (c1, c2), q1, q2 = critic_fw(cri_t, s, f["a"])
    if mg is not None:
        actor_margins(mg, "act_pg", f)
        for i, z in enumerate(zc):
            mg.layer(f"cri_t_actor{i}", z)
        mg.scales["aq"] = float(max(np.abs(q1).max(), np.abs(q2).max()))
        mg.point((q1 - q2) / max(mg.scales["aq"], (mg.given or {}).get("aq", 0.0)))
    first = np.ones_like(q1, dtype=bool) if mutant == "actor_q1_only" else np.zeros_like(q1, dtype=bool) if mutant == "actor_q2_only" \
        else q1 <= q2
    q = np.where(first, q1, q2)
    a_eff = dt(0.0) if mutant == "actor_no_entropy" else dt(alpha)
    obj = -(q + f["lp"] * a_eff).mean()
    gq = np.full((B, 1), -1.0 / B, dtype=dt)
    head = np.where(first, cri_t["net_q1.weight"], cri_t["net_q2.weight"])   # [B, md]: each sample's selected head
    dz2 = (gq * head) * (c2 > 0)
    dz1 = (dz2 @ cri_t["net_sa.2.weight"]) * (c1 > 0)
    g_a = dz1 @ cri_t["net_sa.0.weight"][:, -1:]
    g_lp = gq * a_eff
    return obj, actor_backward(act, f, s, g_a, g_lp, mutant if mutant in MUTANTS_POLICY else None, light)


class ScalarAdam:
    """torch.optim.Adam on the one-element alpha_log."""

    def __init__(self, lr, betas=(0.9, 0.999), eps=1e-8):
        self.lr, self.b1, self.b2, self.eps, self.t, self.m, self.v = lr, betas[0], betas[1], eps, 0, 0.0, 0.0

    def step(self, x, g):
        self.t += 1
        self.m += (g - self.m) * (1.0 - self.b1)
        self.v = self.v * self.b2 + g * g * (1.0 - self.b2)
        return x - (self.lr / (1.0 - self.b1 ** self.t)) * (self.m / (np.sqrt(self.v) / np.sqrt(1.0 - self.b2 ** self.t) + self.eps))


class Sac:
    """The three nets, the temperature and the three optimizers of AgentSAC (agent.py:405-417), float64."""

    def __init__(self, act, cri, cri_t, alpha_log=0.0, lr=1e-4, tau=2 ** -8, target_entropy=0.0, lr_alpha=None, betas=(0.9, 0.999),
                 eps=1e-8):
        self.act, self.cri, self.cri_t = f64(act, ACTOR_KEYS), f64(cri, CRITIC_KEYS), f64(cri_t, CRITIC_KEYS)
        self.opt_a, self.opt_c = Adam(self.act, lr, betas, eps), Adam(self.cri, lr, betas, eps)
        self.opt_t = ScalarAdam(lr if lr_alpha is None else lr_alpha, betas, eps)
        self.alpha_log, self.tau, self.target_entropy = float(alpha_log), tau, target_entropy

    def step(self, state, other, idx, nxt, eps_next, eps_pg):
        """One iteration of update_net's loop on the sampled rows idx (successors nxt) with the two draws per sample.  Returns the
        objectives, alpha after the temperature step and the three gradients."""
        s, s2 = state[idx].astype(np.float64), state[nxt].astype(np.float64)
        o = other[idx].astype(np.float64)
        obj_c, gc = critic_objective(self.act, self.cri, self.cri_t, (s, o[:, 2], o[:, 0], o[:, 1], s2, eps_next), np.exp(self.alpha_log))
        self.opt_c.step(self.cri, gc)
        soft_update(self.cri_t, self.cri, self.tau)
        g_alpha = policy_logprob(self.act, s, eps_pg) - self.target_entropy
        obj_alpha = self.alpha_log * g_alpha
        self.alpha_log = float(self.opt_t.step(self.alpha_log, g_alpha))
        alpha = np.exp(self.alpha_log)
        obj_a, ga = actor_objective(self.act, self.cri_t, s, eps_pg, alpha)
        self.opt_a.step(self.act, ga)
        return {"obj_a": obj_a, "obj_c": obj_c, "obj_alpha": obj_alpha, "alpha": alpha, "g_alpha": g_alpha, "gc": gc, "ga": ga}


STREAM_NEXT, STREAM_PG = 4, 5   # Philox streams of the two draws (exploration is 2, the TD3 smoothing noise 3)


def philox_noise(seed, epoch, row, B, stream):
    """float32[B]: the draws the fused step makes when no noise table is given -- Philox4x32-10 keyed by `seed`, counter (batch
    position, epoch, table row, stream), Box-Muller cosine branch (float64 here, float32 hardware transcendentals in the kernel:
    they agree to ~1e-6 relative, as oracle.td3.smoothing_noise documents for stream 3)."""
    from oracle.binding import philox_uniform_pair
    out = np.empty(B, dtype=np.float32)
    for p in range(B):
        ua, ub = philox_uniform_pair(seed, p, epoch, row, stream)
        out[p] = np.float32(np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(6.283185307179586476925286766559 * ub))
    return out
