"""Independent numpy reference of `pime_rollout_eval_band` (include/pime_hip.h): per step and lane group the sum, sum of squares,
minimum and maximum of the four signals Y, E, A, R, and the histogram of Y -- from the records of a launch's own trace
(`stepresponse_metrics.records_from_trace`).  Pure numpy: no import of the package's `band_from_records`.

The bars are derived, not measured: a sum of n terms taken in ANY order differs from another order of the same terms by at most
n * 2^-52 * sum|term| (each of the n - 1 additions of either order rounds a partial sum no larger than sum|term| by at most
2^-53 of it), the form tests/test_gpu_eval_metrics.py uses; the same holds for SUMSQ with the terms x * x, which both sides round
before they add.  MIN, MAX and every count are exact.  The reference adds in ascending lane order.

`fault=` plants ONE mistake an implementation could make; tests/test_response_band_cpu.py shows that `check_band` sees each."""
import numpy as np

SIGNALS = ("y", "e", "action", "reward")
STATS = ("sum", "sumsq", "min", "max")
Y, E, A, R = range(4)
SUM, SUMSQ, MIN, MAX = range(4)
ROWS = 16
EPS = 2.0 ** -52
FAULTS = ("shadow_lanes_counted", "tile_copies_counted", "group_boundary_one_tile_off", "output_before_step", "error_sign",
          "previous_setpoint", "reward_not_float32", "min_max_from_zero", "stale_tile_partial", "edge_in_lower_bin",
          "above_hi_dropped")

# every class the fused evaluation kernels serve, (policy, width, env, state mode, tiling) -- tests/test_gpu_eval_band.py checks the
# list against pime_rollout_eval_supported: the prior controller (one tiling), the four actors at widths 64 / 128 in either state
# mode and at width 256 (no ActorSAC there) in mixed mode on the pH / Integrator observation, and Stacking 1 / 4 / 10 at width 256
CLASSES = []
for _env in ("PH_V35", "WT_INTEGRATOR"):
    CLASSES += [("prior", 0, _env, _mode, "narrow") for _mode in ("mixed", "f64")]
    for _t in ("quad", "narrow"):
        CLASSES += [(_k, _md, _env, "mixed", _t) for _k in ("modular", "plain", "td3") for _md in (64, 128, 256)]
        CLASSES += [("sac", _md, _env, "mixed", _t) for _md in (64, 128)]
        CLASSES += [(_k, _md, _env, "f64", _t) for _k in ("modular", "plain", "sac", "td3") for _md in (64, 128)]
CLASSES += [(_k, 256, f"WT_STACKING{_s}", "mixed", _t) for _s in (1, 4, 10) for _k in ("plain", "td3") for _t in ("quad", "narrow")]


def group_of(n, group_lanes):
    """(group index of every lane [n], G).  group_lanes: a positive multiple of 16, or >= n (None: one group)."""
    gl = n if group_lanes is None or group_lanes >= n else int(group_lanes)
    assert gl > 0 and (gl >= n or gl % 16 == 0), group_lanes
    return np.arange(n) // gl, -(-n // gl)


def bin_of(y, bins, lo, hi, fault=None):
    """The histogram bin of every y, as the header defines it; -1: not counted (only a fault drops a value)."""
    scale = float(bins) / (hi - lo)
    with np.errstate(invalid="ignore"):
        pos = (np.where(np.isfinite(y), y, lo) - lo) * scale
        inside = np.floor(pos)
        if fault == "edge_in_lower_bin":
            inside = np.ceil(pos) - 1
        inside = np.clip(inside, 0, bins - 1).astype(np.int64)
        b = np.where(~(y >= lo), 0, np.where(y >= hi, -1 if fault == "above_hi_dropped" else bins - 1, inside))
    return b


def signals(rec, fault=None):
    """The four signals [4, T, N] of a launch's records: Y, E, A, R."""
    y, r, a = (np.asarray(rec[k], dtype=np.float64) for k in ("y_after", "r", "action"))
    rew = np.asarray(rec["reward"], dtype=np.float64)
    if fault != "reward_not_float32":
        rew = np.asarray(rec["reward"]).astype(np.float32).astype(np.float64)   # the rewards are float32 before they are widened
    if fault == "output_before_step":            # the plant state is carried across a boundary: before step t = after step t - 1
        y = np.concatenate([np.asarray(rec["y_start"], dtype=np.float64)[:1], y[:-1]])
    if fault == "previous_setpoint" and rec["seg_len"] > 0:
        r = np.concatenate([r[:rec["seg_len"]], r[:-rec["seg_len"]]])
    e = y - r if fault == "error_sign" else r - y
    sig = np.stack([y, e, a, rew])
    if fault == "stale_tile_partial" and sig.shape[2] > 16:   # the second tile's values are those of the step before
        sig[:, 1:, 16:32] = sig[:, :-1, 16:32].copy()
    return sig


def reference_band(rec, group_lanes=None, hist=None, fault=None):
    """rec: the dict of stepresponse_metrics.records_from_trace (y_after, r, action, reward [T, N], y_start [n_segments, N], seg_len).
    hist: None or (bins, lo, hi).  Returns dict: stats [T, 16, G], bars [T, 16, G], count [G], hist [T, G, bins] or None."""
    assert fault is None or fault in FAULTS
    sig = signals(rec, fault)
    _, T, N = sig.shape
    grp, G = group_of(N, group_lanes)
    if fault == "group_boundary_one_tile_off":
        grp = np.minimum((np.arange(N) + 16) // (N if group_lanes is None or group_lanes >= N else group_lanes), G - 1)
    lanes = np.arange(N)
    if fault == "shadow_lanes_counted":          # the idle lanes of the last tile shadow lane N - 1
        lanes = np.concatenate([lanes, np.full((-N) % 16, N - 1, dtype=np.int64)])
    if fault == "tile_copies_counted":           # the four lane groups of a wave hold copies of the tile
        lanes = np.repeat(lanes, 4)
    stats = np.zeros((T, ROWS, G))
    bars = np.zeros((T, ROWS, G))
    count = np.zeros(G, dtype=np.int64)
    counts = None
    if hist is not None:
        bins, lo, hi = int(hist[0]), float(hist[1]), float(hist[2])
        b = bin_of(sig[Y], bins, lo, hi, fault)
        counts = np.zeros((T, G, bins), dtype=np.int64)
    for g in range(G):
        members = lanes[grp[lanes] == g]
        count[g] = len(members)
        n = len(members)
        for s in range(4):
            x = sig[s][:, members]               # [T, n]
            acc, acc2 = np.zeros(T), np.zeros(T)
            for j in range(n):                   # ascending lane order, one addition at a time
                acc = acc + x[:, j]
                acc2 = acc2 + x[:, j] * x[:, j]
            stats[:, 4 * s + SUM, g], stats[:, 4 * s + SUMSQ, g] = acc, acc2
            mn, mx = x.min(axis=1), x.max(axis=1)
            if fault == "min_max_from_zero":
                mn, mx = np.minimum(mn, 0.0), np.maximum(mx, 0.0)
            stats[:, 4 * s + MIN, g], stats[:, 4 * s + MAX, g] = mn, mx
            bars[:, 4 * s + SUM, g] = n * EPS * np.abs(x).sum(axis=1)
            bars[:, 4 * s + SUMSQ, g] = n * EPS * (x * x).sum(axis=1)
        if counts is not None:
            for t in range(T):
                bt = b[t, members]
                counts[t, g] = np.bincount(bt[bt >= 0], minlength=bins)
    return {"stats": stats, "bars": bars, "count": count, "hist": counts}


def check_band(stats, hist, want, tag=""):
    """Assert that a band (stats [T, 16, G], hist [T, G, bins] or None) is the reference's `want`: sums within the bars, MIN / MAX and
    every count exact, every step's counts summing to the group's size.  Returns the largest used share of a bar."""
    stats = np.asarray(stats, dtype=np.float64)
    assert stats.shape == want["stats"].shape, (stats.shape, want["stats"].shape)
    assert np.isfinite(stats).all(), f"non-finite stats ({tag})"
    share = 0.0
    for s, sname in enumerate(SIGNALS):
        for k, kname in enumerate(STATS):
            row = 4 * s + k
            got, ref, bar = stats[:, row], want["stats"][:, row], want["bars"][:, row]
            if k in (MIN, MAX):
                np.testing.assert_array_equal(got, ref, err_msg=f"{kname} of {sname} ({tag})")
                continue
            err = np.abs(got - ref)
            assert (err <= bar).all(), f"{kname} of {sname} ({tag}): {err.max():.3e} over the bar, at most {bar.max():.3e}"
            with np.errstate(divide="ignore", invalid="ignore"):
                share = max(share, float(np.where(err > 0, err / bar, 0.0).max()))
    if want["hist"] is not None:
        assert hist is not None, f"no histogram ({tag})"
        hist = np.asarray(hist).astype(np.int64)
        assert hist.shape == want["hist"].shape, (hist.shape, want["hist"].shape)
        np.testing.assert_array_equal(hist.sum(axis=2), np.broadcast_to(want["count"], hist.shape[:2]),
                                      err_msg=f"every step's counts sum to the group's size ({tag})")
        np.testing.assert_array_equal(hist, want["hist"], err_msg=f"histogram ({tag})")
    return share
