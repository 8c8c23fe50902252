"""The response band without a device: the numpy reference of tests/response_band.py is vetted on recordings synthesised from the
oracle envs -- its bars hold for other summation orders with room to spare, and `check_band` sees every single fault an
implementation could make -- the package's `protocols.band_from_records` / `band_quantiles` agree with it, and the C ABI of
`pime_rollout_eval_band` (exports, row count, argument errors -- as far as a host without a device gets)."""
import ctypes as C

import numpy as np
import pytest

import response_band as RB

N, T, SEG = 81, 24, 7                # the GPU test's shapes: five whole tiles and one lane, three whole segments and three steps
SETPOINTS = {"ph": (10., 6., 3., 8.), "wt": (3., 6., 9., 4.)}
GROUP = 32                           # groups of 32, 32 and 17 lanes
HIST = {"ph": (32, 4.0, 8.0), "wt": (32, 0.5, 4.5)}     # dyadic bin width 1/8: edges are exact doubles


def _synthesise(kind, table):
    """T steps of N oracle lanes under the prior controller along the set-point schedule, as the records of a launch: the
    controlled output after each step, the set-point, the env action and the float64 reward (NOT float32-representable)."""
    from oracle.cpu_stack import OracleVecEnv
    kw = dict(table=table) if kind == "ph" else dict(reward_type="distance")
    env = OracleVecEnv(kind, N, seed=6, env_offset=8192, max_steps=64, **kw)
    obs = env.reset().numpy().astype(np.float64)
    core, K = env.core, -env.K
    r_col, i_col = (1, 2) if kind == "ph" else (2, 3)
    y_col = 0 if kind == "ph" else 1
    y_before = core.get("y") if kind == "ph" else core.get("h2")
    out = {k: [] for k in ("y_after", "r", "action", "reward")}
    y_start = []
    for t in range(T):
        if t % SEG == 0:
            sp = SETPOINTS[kind][t // SEG]
            core.set("r", sp); core.set("I", 0.0)
            obs[:, r_col], obs[:, i_col] = sp, 0.0
            y_start.append(y_before)
        a = obs @ K
        _, obs64, rew, _ = core.step(a)
        obs = obs64.astype(np.float32).astype(np.float64)
        y_before = obs64[:, y_col].copy()
        out["y_after"].append(y_before); out["r"].append(core.get("r")); out["action"].append(a); out["reward"].append(rew.copy())
    rec = {k: np.stack(v) for k, v in out.items()}
    rec["y_start"] = np.stack(y_start)
    rec["seg_len"] = SEG
    return rec


@pytest.fixture(scope="module")
def records(ph_table_oracle):
    rec = {k: _synthesise(k, ph_table_oracle) for k in ("ph", "wt")}
    for k, r in rec.items():         # one output exactly on an inner bin edge, one exactly on hi, some outside on both sides
        bins, lo, hi = HIST[k]
        r["y_after"][3, 5] = lo + 7 * (hi - lo) / bins
        r["y_after"][4, 40] = hi
        r["y_after"][5, 70] = hi + 1.0
        r["y_after"][6, 2] = lo - 1.0
    return rec


@pytest.fixture(scope="module")
def reference(records):
    return {k: RB.reference_band(rec, GROUP, HIST[k]) for k, rec in records.items()}


@pytest.mark.parametrize("which", ["ph", "wt"])
def test_the_recordings_exercise_the_histogram_and_the_rounding(records, reference, which):
    rec, (bins, lo, hi) = records[which], HIST[which]
    y = rec["y_after"]
    assert (y < lo).any() and (y >= hi).any() and ((y >= lo) & (y < hi)).any()
    assert (rec["reward"] != rec["reward"].astype(np.float32)).any(), "rewards that float32 rounds"
    assert list(reference[which]["count"]) == [32, 32, 17]
    assert reference[which]["hist"].sum() == T * N


@pytest.mark.parametrize("which", ["ph", "wt"])
def test_other_summation_orders_stay_below_half_of_every_bar(records, reference, which):
    """The kernel's order (a butterfly per tile, then the tiles) is neither of these and not the reference's: the bar is for any order."""
    sig = RB.signals(records[which])
    grp, G = RB.group_of(N, GROUP)
    want = reference[which]
    share = 0.0
    for g in range(G):
        for s in range(4):
            x = sig[s][:, grp == g]
            for terms, row in ((x, 4 * s + RB.SUM), (x * x, 4 * s + RB.SUMSQ)):
                rev = np.zeros(T)
                for j in range(terms.shape[1] - 1, -1, -1):
                    rev = rev + terms[:, j]
                pair = [terms[:, j] for j in range(terms.shape[1])]
                while len(pair) > 1:
                    pair = [pair[j] + pair[j + 1] if j + 1 < len(pair) else pair[j] for j in range(0, len(pair), 2)]
                for other in (rev, pair[0]):
                    err, bar = np.abs(other - want["stats"][:, row, g]), want["bars"][:, row, g]
                    assert (bar > 0).all()
                    assert (err < 0.5 * bar).all(), f"row {row} group {g}: {(err / bar).max():.3f} of the bar"
                    share = max(share, float((err / bar).max()))
    print(f"\n{which}: reversed / pairwise sums use at most {share:.4f} of a bar")


@pytest.mark.parametrize("fault", RB.FAULTS)
def test_every_single_fault_trips_the_check(records, reference, fault):
    tripped = []
    for which, rec in records.items():
        faulty = RB.reference_band(rec, GROUP, HIST[which], fault=fault)
        try:
            RB.check_band(faulty["stats"], faulty["hist"], reference[which], tag=fault)
        except AssertionError as e:
            tripped.append(f"{which}: {str(e).strip().splitlines()[0]}")
    print(f"\n{fault}: " + " | ".join(tripped))
    assert len(tripped) == len(records), f"the check does not see the fault {fault} on every recording"


def test_the_check_passes_the_reference_itself(records, reference):
    for which in records:
        assert RB.check_band(reference[which]["stats"], reference[which]["hist"], reference[which]) == 0.0


@pytest.mark.parametrize("which", ["ph", "wt"])
@pytest.mark.parametrize("group_lanes", [None, 16, 32, 48, 2 * N])
def test_band_from_records_agrees_with_the_reference(records, which, group_lanes):
    from pime_amd import protocols
    rec = records[which]
    want = RB.reference_band(rec, group_lanes, HIST[which])
    got = protocols.band_from_records(rec["y_after"], rec["r"], rec["action"], rec["reward"], group_lanes=group_lanes, hist=HIST[which])
    assert tuple(protocols.BAND_SIGNALS) == RB.SIGNALS and tuple(protocols.BAND_STATS) == RB.STATS
    np.testing.assert_array_equal(got["count"], want["count"])
    RB.check_band(got["stats"], got["hist"], want, tag=f"band_from_records {which} {group_lanes}")
    no_hist = protocols.band_from_records(rec["y_after"], rec["r"][:, :1], rec["action"], rec["reward"], group_lanes=group_lanes)
    assert no_hist["hist"] is None
    np.testing.assert_array_equal(no_hist["stats"], got["stats"])       # (all lanes share the set-point: r may be [T, 1])


def test_band_from_records_refuses_bad_groups_and_bounds(records):
    from pime_amd import protocols
    rec = records["wt"]
    args = (rec["y_after"], rec["r"], rec["action"], rec["reward"])
    for gl in (0, -16, 8, 24):
        with pytest.raises(ValueError, match="group_lanes"):
            protocols.band_from_records(*args, group_lanes=gl)
    for h in ((0, 0., 1.), (257, 0., 1.), (8, 1., 1.), (8, 2., 1.), (8, float("nan"), 1.), (8, 0., float("inf"))):
        with pytest.raises(ValueError, match="hist"):
            protocols.band_from_records(*args, hist=h)


def test_band_quantiles_interpolate_inside_the_bin():
    from pime_amd import protocols
    edges = np.array([0., 1., 2., 4.])
    hist = np.array([[2, 6, 2], [0, 0, 4], [0, 0, 0]])
    q = protocols.band_quantiles(hist, edges, [0.0, 0.1, 0.5, 0.9, 1.0])
    np.testing.assert_allclose(q[0], [0.0, 0.5, 1.5, 3.0, 4.0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(q[1], [2.0, 2.2, 3.0, 3.8, 4.0], rtol=0, atol=1e-12)
    assert np.isnan(q[2]).all()
    rng = np.random.default_rng(3)        # against numpy on a sample: within one bin width
    x = rng.normal(5.0, 1.0, 20000)
    edges = np.linspace(0.0, 10.0, 129)
    got = protocols.band_quantiles(np.histogram(x, edges)[0], edges, [0.05, 0.5, 0.95])
    np.testing.assert_allclose(got, np.quantile(x, [0.05, 0.5, 0.95]), rtol=0, atol=10.0 / 128)
    assert protocols.band_quantiles(hist, np.array([0., 1., 2., 4.]), 0.5).shape == (3, 1)


# ---- the C ABI, as far as a host without a device gets ----------------------------------------------------------------------
def test_band_symbols_are_exported_and_bound():
    import pime_amd.native as nt
    raw = C.CDLL(nt.LIB_PATH)
    for name in ("pime_rollout_eval_band_rows", "pime_rollout_eval_band_workspace_bytes", "pime_rollout_eval_band"):
        assert hasattr(raw, name) and name in nt.EXPORTS
    assert nt.lib().pime_rollout_eval_band_rows() == 16 == nt.BAND_ROWS == RB.ROWS
    assert tuple(nt.BAND_SIGNALS) == RB.SIGNALS and tuple(nt.BAND_STATS) == RB.STATS


def _call(metrics=True, stats=True, workspace=True, hist=False, bins=32, lo=0.0, hi=1.0):
    import pime_amd.native as nt
    m, s, w, h, k = np.zeros(8), np.zeros(16 * 5), np.zeros(16 * 5), np.zeros(5 * 256, dtype=np.uint32), np.zeros(4)
    return nt.lib().pime_rollout_eval_band(None, -1, 0, None, nt.ptr(k), 5, 0, None, 0, 0.05, 10, None, None, nt.ptr(m) if metrics else None,
                                           16, nt.ptr(s) if stats else None, nt.ptr(h) if hist else None, bins, lo, hi,
                                           nt.ptr(w) if workspace else None, None)


@pytest.mark.parametrize("kw,word", [(dict(metrics=False), "metrics"), (dict(stats=False), "stats"), (dict(workspace=False), "workspace"),
                                     (dict(hist=True, bins=0), "bins"), (dict(hist=True, bins=257), "bins"),
                                     (dict(hist=True, lo=1.0, hi=1.0), "lo"), (dict(hist=True, lo=2.0, hi=1.0), "lo"),
                                     (dict(hist=True, lo=float("nan")), "lo"), (dict(hist=True, hi=float("nan")), "hi"),
                                     (dict(hist=True, hi=float("inf")), "hi")])
def test_each_argument_error_names_its_argument(kw, word):
    """The checks that need no handle come before anything touches it: they answer on a host without a device."""
    import pime_amd.native as nt
    assert _call(**kw) == -1     # PIME_ERR_ARG
    assert word in nt.last_error() and "pime_rollout_eval_band" in nt.last_error(), nt.last_error()


def test_a_null_handle_is_an_argument_error():
    import pime_amd.native as nt
    assert _call() == -1 and "handle" in nt.last_error()
    assert _call(hist=True) == -1 and "handle" in nt.last_error()
    assert nt.lib().pime_rollout_eval_band_workspace_bytes(None, -1, 0, 5, 16) == -1
