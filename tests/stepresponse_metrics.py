"""Independent numpy reference of the eight step-response metrics of `pime_rollout_eval_metrics` (include/pime_hip.h), from
step-by-step records or from the evaluation kernel's own trace.  Pure numpy: no import of the package's `metrics_from_records`.

Every sum is a plain loop over the steps in ascending order (vectorised over lanes only), so a kernel that adds the same terms in
the same order agrees bit for bit; `bars` holds, per row, n * 2^-52 * sum|term| -- the bound for n sequential double additions.

`fault=` plants ONE mistake an implementation could make; tests/test_stepresponse_metrics_cpu.py shows that each of them moves
some row on the golden records, i.e. that a comparison against this reference can see it."""
import numpy as np

ROWS = ("iae", "ise", "itae", "overshoot", "settling_step", "steady_state_error", "return", "action_variation")
IAE, ISE, ITAE, OVERSHOOT, SETTLING, SSE, RETURN, ACTION_VAR = range(8)
EXACT_ROWS = (OVERSHOOT, SETTLING)
FAULTS = ("output_before_step", "settling_off_by_one", "tail_shifted", "overshoot_sign", "variation_across_boundary",
          "no_clear_at_boundary", "itae_from_zero", "squared_for_absolute")
EPS = 2.0 ** -52


def reference_metrics(rec, band, tail, fault=None):
    """rec: dict with y_after [T, N] (the controlled output after each step), r [T, N], action [T, N], reward [T, N],
    y_start [n_segments, N] (the output before each segment's first step), seg_len (0: one segment).
    Returns (metrics [n_segments, 8, N], bars [n_segments, 8, N])."""
    assert fault is None or fault in FAULTS
    y, r, a = (np.asarray(rec[k], dtype=np.float64) for k in ("y_after", "r", "action"))
    rew = np.asarray(rec["reward"]).astype(np.float32).astype(np.float64)     # the rewards are float32 before they are widened
    y_start = np.asarray(rec["y_start"], dtype=np.float64)
    T, N = y.shape
    L0 = rec["seg_len"] if rec["seg_len"] > 0 else T
    n_seg = -(-T // L0)
    assert y_start.shape == (n_seg, N) and r.shape == a.shape == rew.shape == (T, N)
    M = np.zeros((n_seg, 8, N))
    B = np.zeros((n_seg, 8, N))
    iae = ise = itae = ret = av = np.zeros(N)
    b_iae = b_ise = b_itae = b_ret = b_av = np.zeros(N)
    for s in range(n_seg):
        t0 = s * L0
        L = min(L0, T - t0)
        rs = r[t0]
        if not (fault == "no_clear_at_boundary" and s > 0):
            iae = ise = itae = ret = av = np.zeros(N)
            b_iae = b_ise = b_itae = b_ret = b_av = np.zeros(N)
        d = np.where(rs >= y_start[s], 1.0, -1.0)
        if fault == "overshoot_sign":
            d = -d
        peak = np.zeros(N)
        settle = np.zeros(N)
        w = min(tail, L)
        lo = L - w - (1 if fault == "tail_shifted" else 0)
        tail_sum, b_tail = np.zeros(N), np.zeros(N)
        for k in range(L):
            t = t0 + k
            yk = y[t]
            if fault == "output_before_step":
                yk = y_start[s] if k == 0 else y[t - 1]
            e = rs - yk
            ae = np.abs(e)
            if fault == "squared_for_absolute":
                iae = iae + e * e; b_iae = b_iae + e * e
            else:
                iae = iae + ae; b_iae = b_iae + ae
            ise = ise + e * e; b_ise = b_ise + e * e
            wk = float(k if fault == "itae_from_zero" else k + 1)
            itae = itae + wk * ae; b_itae = b_itae + wk * ae
            peak = np.maximum(peak, d * (yk - rs))
            settle = np.where(ae > band, float(k if fault == "settling_off_by_one" else k + 1), settle)
            if lo <= k < lo + w:
                tail_sum = tail_sum + e; b_tail = b_tail + ae
            ret = ret + rew[t]; b_ret = b_ret + np.abs(rew[t])
            if k >= 1 or (fault == "variation_across_boundary" and t >= 1):
                av = av + np.abs(a[t] - a[t - 1]); b_av = b_av + np.abs(a[t] - a[t - 1])
        M[s] = np.stack([iae, ise, itae, peak, settle, tail_sum / w, ret, av])
        B[s] = L * EPS * np.stack([b_iae, b_ise, b_itae, np.zeros(N), np.zeros(N), b_tail / w, b_ret, b_av])
    return M, B


def records_from_trace(tr, is_ph, seg_len, y_last=None, y_first=None):
    """The evaluation kernel's trace [T, 6, N] as records.  pH rows: y, r, I BEFORE the step | action, reward, x after -- the
    output after step k is row k + 1's y (the plant state is carried across a boundary), and the last step's is `y_last` [N]
    (the traced x through the titration table).  Tank rows: h1, h2, r, I after the step | reward, action -- the output before
    the first step is `y_first` [N] (h2 before the launch)."""
    tr = np.asarray(tr, dtype=np.float64)
    T = tr.shape[0]
    L0 = seg_len if seg_len > 0 else T
    if is_ph:
        y_before = tr[:, 0]
        y_after = np.concatenate([y_before[1:], np.asarray(y_last, dtype=np.float64)[None]])
        return dict(y_after=y_after, r=tr[:, 1], action=tr[:, 3], reward=tr[:, 4], y_start=y_before[::L0], seg_len=seg_len)
    y_after = tr[:, 1]
    y_before = np.concatenate([np.asarray(y_first, dtype=np.float64)[None], y_after[:-1]])
    return dict(y_after=y_after, r=tr[:, 2], action=tr[:, 5], reward=tr[:, 4], y_start=y_before[::L0], seg_len=seg_len)


def ph_table_lookup(table, C, x):
    """ph.py:187-189: the titration-table value at state x (first i with MHCl[i] >= around(C x, 5) == rint(C x 1e5), clamped)."""
    k = np.clip(np.rint(np.asarray(C) * np.asarray(x) * 1e5).astype(np.int64), 0, len(table) - 1)
    return np.asarray(table)[k]


def golden_ph_records(g, table, zoh):
    """tests/golden/ph_stepresponse.npz (two plants, r = 10,6,3,8,5 x 50 steps) as records of two lanes.  zoh(qww_V, qc_V) ->
    (A, B, C) of the plant; the interior outputs are the golden's next rows (checked against the table), the last one comes from the table."""
    cols = {k: [] for k in ("y_after", "r", "action", "reward", "y_before")}
    for tag in ("nominal", "corner"):
        C = zoh(*g[tag + "_params"])[2]
        y_tab = ph_table_lookup(table, C, g[tag + "_x"])
        # the golden y of row k + 1 is the table value at row k's x (the reference's own table differs from ours in the last bit)
        np.testing.assert_allclose(y_tab[:-1], g[tag + "_y"][1:], rtol=0, atol=1e-14)
        cols["y_after"].append(np.concatenate([g[tag + "_y"][1:], y_tab[-1:]])); cols["y_before"].append(g[tag + "_y"])
        cols["r"].append(g[tag + "_r"]); cols["action"].append(g[tag + "_act"]); cols["reward"].append(g[tag + "_rew"])
    rec = {k: np.stack(v, axis=1) for k, v in cols.items()}
    rec["y_start"] = rec.pop("y_before")[::50]
    rec["seg_len"] = 50
    return rec


def golden_wt_records(g):
    """tests/golden/wt_stepresponse.npz, plants robust1 / robust3 (r = 3,6,9,4,2 x 500 steps from empty tanks) as two lanes."""
    obs = np.stack([g["robust1_obs"], g["robust3_obs"]], axis=1)          # [T, lane, (h1, h2, r, I)]
    y_after = obs[:, :, 1]
    y_before = np.concatenate([np.zeros((1, 2)), y_after[:-1]])
    return dict(y_after=y_after, r=obs[:, :, 2], action=np.stack([g["robust1_act"], g["robust3_act"]], axis=1),
                reward=np.stack([g["robust1_rew"], g["robust3_rew"]], axis=1), y_start=y_before[::500], seg_len=500)
