"""Checker of the policy sweep (`pime_policy_sweep`, csrc/policy_sweep.hpp) and a numpy restatement of `protocols.select_policy`.
Shared by tests/test_policy_sweep_cpu.py and tests/test_gpu_policy_sweep.py.  TEST INFRASTRUCTURE.

`check_recording` takes what a call left -- actions, outputs [T, P, N], pairs [S, 8, P, N], summary [P, S, 8, 5] -- and the lane state
it started from, and runs EVERY row p through tests/margin_sweep.py's `check_recording` with the one-row nominal grid (1, 0, 0), that
row's prior gain K[p] and that row's float64 policy term: the float64 oracle replays the row's recorded actions open-loop (the
[trajectory] bar), the action of every step is the float64 controller's on the oracle's observation within ACT_BAR (the [action]
bar: margin_sweep.ACT_BAR, measured there without a kernel; the policy sweep's loop is that sweep's nominal row, so its bar holds),
and `pairs` are held to the traces ([metrics]: seven rows bit for bit, the return at the trajectory bar).  Then the summary is held
to summary_from_pairs(pairs).  A row that fails is re-checked against the ways a policy grid can go wrong, and the assertion is named
for the one that explains it:
  [layout]   the row passes once `pairs` is read with p and i exchanged
  [image]    the row passes with the policy term of ANOTHER row (a stale image in LDS; an image read at the wrong stride)
  [gain]     the row passes with the prior gain of ANOTHER row
  [noise]    the row passes with the tank's process noise keyed on the pair (p * N + i) instead of the plant
  [row]      none of these
  [summary]  the summary is not the fold of the call's own pairs
`numpy_sweep` synthesises a recording with margin_sweep.numpy_loop, one row at a time, and takes one named fault (FAULTS)."""
import numpy as np

import margin_sweep as G
import prior_sweep as P

N, OFFSET, SEED = G.N, G.OFFSET, G.SEED                      # 81 plants at lane offset 1000
N_STEPS, SEG, TAIL, BAND = G.N_STEPS, G.SEG, G.TAIL, G.BAND  # 23 steps in segments of 9 (the last one ragged), tail 4
SETPOINTS, PRIOR_K = G.SETPOINTS, G.PRIOR_K
ROWS = 5                                                      # rows 0 and 4 the same policy and gain, row 2 with K halved
NOMINAL = np.array([[1.0, 0.0, 0.0]])
FAULTS = ("stale_image", "gain_of_row0", "pairs_exchanged", "stride_zero", "summary_wrong_row", "noise_pair")
METRIC_NAMES = ("iae", "ise", "itae", "overshoot", "settling_step", "steady_state_error", "return", "action_variation")
SUM, MAX, ARGMAX, FINITE = P.SUM, P.MAX, P.ARGMAX, P.FINITE


def bits_equal(a, b):
    return P.bits_equal(a, b)


def row_gains(kind):
    """[ROWS, D]: the env's own -K, row 2 halved."""
    K = np.tile(PRIOR_K[kind], (ROWS, 1)).astype(np.float64)
    K[2] *= 0.5
    return K


def numpy_policies(kind):
    """ROWS numpy actors: rows 1 .. 3 of other seeds, row 4 the actor of row 0."""
    D = len(PRIOR_K[kind])
    pols = [G.NumpyPolicy(D, seed=11 + p) for p in range(ROWS - 1)]
    return pols + [pols[0]]


def _shifted(cfg, by):
    c = type(cfg).from_buffer_copy(cfg)
    c.env_offset = cfg.env_offset + by
    return c


def exchange(a):
    """[..., P, N] stored with column i * P + p in place of p * N + i (and back: `unexchange`)."""
    return np.ascontiguousarray(np.swapaxes(a, -1, -2)).reshape(a.shape)


def unexchange(a):
    return np.ascontiguousarray(np.swapaxes(a.reshape(a.shape[:-2] + (a.shape[-1], a.shape[-2])), -1, -2))


def numpy_sweep(kind, cfg, lanes, table, pols, Ks, fault=None, n_steps=N_STEPS, seg_len=SEG, band=BAND, tail=TAIL):
    """The sweep in numpy: row p is margin_sweep.numpy_loop's nominal row under pols[p] and Ks[p].  Returns dict actions, outputs
    [T, P, N], pairs [S, 8, P, N], summary [P, S, 8, 5]."""
    assert fault is None or fault in FAULTS
    n, Pn = len(lanes["r"]), len(pols)
    rows = []
    for p in range(Pn):
        pol, K, c = pols[p], Ks[p], cfg
        if fault == "stale_image" and p == 2:
            pol = pols[1]
        if fault == "stride_zero":
            pol = pols[0]
        if fault == "gain_of_row0":
            K = Ks[0]
        if fault == "noise_pair":
            c = _shifted(cfg, p * n)
        rows.append(G.numpy_loop(kind, c, lanes, table, perturb=NOMINAL, K=K, policy=pol, n_steps=n_steps, seg_len=seg_len, band=band,
                                 tail=tail))
    rec = {k: np.concatenate([r[k] for r in rows], axis=-2) for k in ("actions", "outputs", "pairs")}
    rec["summary"] = P.summary_from_pairs(rec["pairs"])
    if fault == "summary_wrong_row":
        rec["summary"][2] = rec["summary"][1]
    if fault == "pairs_exchanged":
        rec["pairs"] = exchange(rec["pairs"])
    return rec


def _row(rec, p):
    return {k: np.ascontiguousarray(rec[k][..., p:p + 1, :]) for k in ("actions", "outputs", "pairs")}


def check_recording(kind, cfg, lanes, table, rec, Ks, terms, n_steps=N_STEPS, seg_len=SEG, setpoints=None, band=BAND, tail=TAIL, tag=""):
    """rec: dict actions, outputs [T, P, N], pairs [S, 8, P, N], summary [P, S, 8, 5] of one call from the lane state `lanes`; Ks
    [P, D]; terms: P callables obs float64 [N, D] -> the float64 tanh term [N].  Returns the largest share of each bar over the rows."""
    n, Pn = len(lanes["r"]), len(terms)
    S = P.n_segments(n_steps, seg_len)
    assert rec["actions"].shape == rec["outputs"].shape == (n_steps, Pn, n) and rec["pairs"].shape == (S, 8, Pn, n), rec["pairs"].shape
    assert rec["summary"].shape == (Pn, S, 8, 5), rec["summary"].shape

    def run(r, p, K, term, c=cfg):
        return G.check_recording(kind, c, lanes, table, _row(r, p), perturb=NOMINAL, K=K, policy=term, n_steps=n_steps, seg_len=seg_len,
                                 setpoints=setpoints, band=band, tail=tail, tag=f"{tag} policy row {p}")

    def passes(*a, **kw):
        try:
            run(*a, **kw)
            return True
        except AssertionError:
            return False
    use = dict(trajectory=0.0, ret=0.0, action=0.0, gap=0.0)
    for p in range(Pn):
        try:
            u = run(rec, p, Ks[p], terms[p])
        except AssertionError as e:
            if passes(dict(rec, pairs=unexchange(rec["pairs"])), p, Ks[p], terms[p]):
                raise AssertionError(f"[layout] {tag} row {p} passes once pairs is read with p and i exchanged; {e}") from None
            for q in range(Pn):
                if q != p and passes(rec, p, Ks[p], terms[q]):
                    raise AssertionError(f"[image] {tag} row {p} ran the image of row {q}; {e}") from None
            for q in range(Pn):
                if q != p and passes(rec, p, Ks[q], terms[p]):
                    raise AssertionError(f"[gain] {tag} row {p} ran the prior gain of row {q}; {e}") from None
            if kind == "wt" and passes(rec, p, Ks[p], terms[p], c=_shifted(cfg, p * n)):
                raise AssertionError(f"[noise] {tag} row {p}: the process noise is keyed on the pair, not on the plant; {e}") from None
            raise AssertionError(f"[row] {tag} row {p}; {e}") from None
        use = {k: max(use[k], u[k]) for k in use}
    try:
        P.check_summary(rec["summary"], rec["pairs"], tag=tag)
    except AssertionError as e:
        raise AssertionError(f"[summary] {tag} the summary is not the fold of the call's own pairs; {e}") from None
    return use


# ------------------------------------------------------------------------------------------------ select_policy in numpy
def numpy_select(summary, settled, n, cost="itae", robust="worst"):
    """protocols.select_policy restated with loops: (best row, nominal row, order) -- a policy with a plant that is not finite
    somewhere or does not settle ranks behind every policy without one; then the smaller cost (worst: the sum over segments of the
    plants' maximum; mean: of their mean; not finite: +inf); then the lower row."""
    summary = np.asarray(summary, dtype=np.float64)
    Pn, S = summary.shape[:2]
    row = METRIC_NAMES.index(cost)

    def key(p, how):
        fit = int(settled[p]) == n and all(summary[p, s, r, FINITE] == n for s in range(S) for r in range(8))
        c = 0.0
        for s in range(S):
            c += summary[p, s, row, MAX] if how == "worst" else summary[p, s, row, SUM] / summary[p, s, row, FINITE]
        return (0 if fit else 1, c if np.isfinite(c) else np.inf, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        order = sorted(range(Pn), key=lambda p: key(p, robust))
        nominal = sorted(range(Pn), key=lambda p: key(p, "mean"))
    return order[0], nominal[0], order
