"""The loop-perturbation sweep without a GPU: the HOST build of the pair function the kernel runs (csrc/margin_sweep.hpp compiled into
libpime_margin_host.so, the prior controller alone, float64 and float32 state) against the numpy restatement and the checker of
tests/margin_sweep.py, and that checker against itself.  Shapes: 81 plants at lane offset 1000, five perturbation rows with the
nominal one first and last (delays 0, 1, 3, 8; gains 0.5, 2; sigma 0, 0.05), 23 steps in segments of 9, tail 4, the tank's process
noise on.
  1. symbols: header, binding and libraries agree; ABI 26; pime_margin_sweep_supported(NULL, -1, 0) == 0; the package never names
     the host library;
  2. the float64 host build: sigma = 0 rows bit-equal to the numpy restatement, every row inside the checker's bars, the nominal
     rows bit-equal to libpime_sweep_host.so's pairs with the same gain, summary bit-equal to summary_from_pairs(pairs) (also at
     N = 130: three blocks), NULL pairs / actions / outputs change no bit of summary; the float32 host build inside the bars;
  3. the measured bar of the applied action (profiles/margin_sweep_bars.txt);
  4. the checker: honest synthetic recordings (with a numpy policy) use less than 0.1 of every bar, each of the twelve single faults
     trips the assertion named for it;
  5. every argument error of the host build carries its message;
  6. protocols.perturbation_grid's order, protocols.loop_margins on hand-made summaries, the wrapper's ValueErrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import margin_sweep as G
import prior_sweep as P
from conftest import ROOT

CLASSES = [(kind, sm) for kind in ("ph", "wt") for sm in ("f64", "mixed")]


@pytest.fixture(scope="module")
def cases(ph_table_oracle):
    """(cfg, keep, lanes, host recording) per class, computed once and left unchanged."""
    out = {}
    for kind, sm in CLASSES:
        cfg, keep, lanes = G.twin_case(kind, G.N, ph_table_oracle, sm)
        out[kind, sm] = (cfg, keep, lanes, G.host_margin(kind, cfg, lanes))
    return out


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pime_margin_sweep_supported", "pime_margin_sweep_workspace_bytes", "pime_margin_sweep")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(pime_[a-z0-9_]+)\s*\(", src))


def test_header_binding_and_libraries_agree_on_the_new_symbols():
    import pime_amd.native as nt
    declared = _declared("pime_hip.h")
    lib = C.CDLL(nt.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in nt.EXPORTS and hasattr(lib, name), name
    assert nt.ABI_VERSION == 26 == nt.lib().pime_abi_version()
    assert nt.lib().pime_margin_sweep_supported(None, -1, 0) == 0
    assert nt.lib().pime_margin_sweep_workspace_bytes(None, 1, 1, 0) == -1
    assert (nt.PERTURB_COLS, nt.MARGIN_MAX_DELAY, nt.PERTURB_NAMES) == (3, 8, ("gain", "delay", "sigma"))
    header = open(os.path.join(ROOT, "include", "pime_hip.h")).read()
    assert "PIME_PERTURB_GAIN = 0, PIME_PERTURB_DELAY = 1, PIME_PERTURB_SIGMA = 2, PIME_PERTURB_COLS = 3" in header
    assert "PIME_MARGIN_MAX_DELAY = 8" in header
    host = C.CDLL(G.HOST_LIB_PATH)
    assert _declared("pime_margin_host.h") == set(G.HOST_EXPORTS)
    for name in G.HOST_EXPORTS:
        assert hasattr(host, name), name
    for name in NEW_SYMBOLS:     # the host library is no second door to the product's entry points
        assert not hasattr(host, name), name


def test_the_package_never_names_the_host_library():
    for d, _, files in os.walk(P.PKG):
        for f in files:
            if f.endswith(".py"):
                assert "margin_host" not in open(os.path.join(d, f)).read(), os.path.join(d, f)


# ---- 2. the host build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_host_equals_numpy_on_the_noise_free_rows(cases, ph_table_oracle, kind):
    cfg, _, lanes, rec = cases[kind, "f64"]
    assert not any((rec[k] == -777.0).any() for k in rec), "every word is written"
    ref = G.numpy_loop(kind, cfg, lanes, ph_table_oracle)
    quiet = [p for p in range(len(G.PERTURB)) if G.PERTURB[p, 2] == 0.0]
    assert quiet == [0, 1, 4]
    for k in ("actions", "outputs", "pairs"):
        assert G.bits_equal(rec[k][..., quiet, :], ref[k][..., quiet, :]), k
    assert G.bits_equal(rec["pairs"][:, :, 0], rec["pairs"][:, :, 4]) and G.bits_equal(rec["actions"][:, 0], rec["actions"][:, 4])
    assert not G.bits_equal(rec["actions"][:, 0], rec["actions"][:, 1])
    assert (rec["actions"][:1, 1] == 0.0).all() and (rec["actions"][:3, 2] == 0.0).all() and (rec["actions"][:8, 3] == 0.0).all()
    assert (rec["actions"][8, 3] != 0.0).all(), "the first controller output arrives after eight steps, across a segment boundary"


@pytest.mark.parametrize("kind,sm", CLASSES, ids=lambda v: str(v))
def test_host_build_passes_the_checker(cases, ph_table_oracle, kind, sm):
    cfg, _, lanes, rec = cases[kind, sm]
    use = G.check_recording(kind, cfg, lanes, ph_table_oracle, rec, tag=f"{kind}-{sm}")
    print(f"\nMARGIN host id={kind}-{sm} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action "
          f"{use['action']:.3g} (gap {use['gap']:.4g})")
    P.check_summary(rec["summary"], rec["pairs"], tag=f"{kind}-{sm}")
    if sm == "f64":
        assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_nominal_rows_are_the_prior_sweeps_pairs(cases, ph_table_oracle, kind):
    cfg, _, lanes, rec = cases[kind, "f64"]
    over = {} if kind == "ph" else {"wt_noise_scale": 0.01}
    _, want = P.host_sweep(kind, lanes, G.PRIOR_K[kind][None], G.N_STEPS, G.SEG, G.SETPOINTS[kind], G.BAND, G.TAIL, table=ph_table_oracle,
                           seed=G.SEED, env_offset=G.OFFSET, cfg_over=over)
    for p in (0, 4):
        assert G.bits_equal(rec["pairs"][:, :, p], want[:, :, 0]), p
    half = G.host_margin(kind, cfg, lanes, perturb=np.array([[0.5, 0.0, 0.0]]))
    _, want = P.host_sweep(kind, lanes, 0.5 * G.PRIOR_K[kind][None], G.N_STEPS, G.SEG, G.SETPOINTS[kind], G.BAND, G.TAIL,
                           table=ph_table_oracle, seed=G.SEED, env_offset=G.OFFSET, cfg_over=over)
    # (0.5 * (sum_j o_j K_j) == sum_j o_j (0.5 K_j): a power of two scales every product and sum exactly)
    assert G.bits_equal(half["pairs"][:, :, 0], want[:, :, 0]), "the gain of the loop on the prior alone is a gain of the prior"


def test_three_summary_blocks_and_null_outputs(ph_table_oracle):
    cfg, keep, lanes = G.twin_case("wt", 130, ph_table_oracle)
    rec = G.host_margin("wt", cfg, lanes)
    P.check_summary(rec["summary"], rec["pairs"], tag="N = 130")
    assert (rec["summary"][..., P.FINITE] == 130).all()
    quiet = G.host_margin("wt", cfg, lanes, trace=False, want_pairs=False)
    assert quiet["pairs"] is None and G.bits_equal(quiet["summary"], rec["summary"]), "NULL pairs / actions / outputs must not change a bit"
    one = G.host_margin("wt", cfg, lanes, perturb=G.PERTURB[2:3])
    assert G.bits_equal(one["pairs"][:, :, 0], rec["pairs"][:, :, 2]) and G.bits_equal(one["summary"][0], rec["summary"][2]), \
        "a row's result does not depend on the other rows"


def test_the_delay_is_rounded_and_clamped(cases):
    cfg, _, lanes, rec = cases["ph", "f64"]
    odd = np.array([[2.0, 3.4, 0.05], [1.0, 11.0, 0.05], [1.0, float("nan"), 0.0], [1.0, -2.0, 0.0]])
    got = G.host_margin("ph", cfg, lanes, perturb=odd)
    for p, q in ((0, 2), (1, 3), (2, 0), (3, 0)):
        assert G.bits_equal(got["pairs"][:, :, p], rec["pairs"][:, :, q]), (p, q)


# ---- 3. the bar ------------------------------------------------------------------------------------------------------------------
def test_the_measured_bar(ph_table_oracle):
    """ACT_BAR = 10 x the largest gap of the float32 numpy restatement against the float64 check on these shapes (no kernel)."""
    worst = 0.0
    for kind in ("ph", "wt"):
        cfg, keep, lanes = G.twin_case(kind, G.N, ph_table_oracle, "mixed", noise=0.0)
        for name, pol in (("prior", None), ("policy", G.NumpyPolicy(len(G.PRIOR_K[kind])))):
            rec = G.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol, dtype=np.float32)
            gap = G.check_recording(kind, cfg, lanes, ph_table_oracle, rec, policy=None if pol is None else pol.term, act_bar=1.0)["gap"]
            print(f"\nMARGIN bar id={kind}-{name} largest |applied32 - wanted64| / (1 + |wanted64|) {gap:.6g}")
            worst = max(worst, gap)
    assert 0.0 < worst <= G.ACT_MEASURED and G.ACT_BAR == 10 * G.ACT_MEASURED, (worst, G.ACT_MEASURED)
    text = open(os.path.join(ROOT, "profiles", "margin_sweep_bars.txt")).read()
    assert f"{G.ACT_MEASURED:.4e}" in text and f"{G.ACT_BAR:.4e}" in text


# ---- 4. the checker --------------------------------------------------------------------------------------------------------------
# fault -> (kind, the assertion it trips)
FAULT_CASES = {
    "delay_off_by_one": ("ph", "action"), "line_cleared": ("wt", "action"), "first_held": ("ph", "zero"), "gain_residual_only": ("wt", "action"),
    "noise_pair": ("ph", "action"), "noise_on_setpoint": ("wt", "action"), "sigma_ignored_delayed": ("ph", "action"),
    "sincos_swapped": ("ph", "action"), "noise_into_plant": ("wt", "trajectory"), "commanded_in_variation": ("wt", "metrics"),
    "setpoint_stale": ("ph", "action"), "transposed": ("wt", "action"),
}


def test_every_fault_is_listed():
    assert sorted(FAULT_CASES) == sorted(G.FAULTS) and len(G.FAULTS) == 12


@pytest.fixture(scope="module")
def honest(cases, ph_table_oracle):
    out = {}
    for kind in ("ph", "wt"):
        cfg, _, lanes, _ = cases[kind, "f64"]
        pol = G.NumpyPolicy(len(G.PRIOR_K[kind]))
        out[kind] = (pol, G.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol))
    return out


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_honest_recordings_pass_far_inside(cases, honest, ph_table_oracle, kind):
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, rec = honest[kind]
    use = G.check_recording(kind, cfg, lanes, ph_table_oracle, rec, policy=pol.term)
    assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use
    assert G.bits_equal(rec["pairs"][:, :, 0], rec["pairs"][:, :, 4])


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_each_fault_trips_the_assertion_named_for_it(cases, honest, ph_table_oracle, fault):
    kind, name = FAULT_CASES[fault]
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, _ = honest[kind]
    forged = G.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol, fault=fault)
    with pytest.raises(AssertionError) as caught:
        G.check_recording(kind, cfg, lanes, ph_table_oracle, forged, policy=pol.term)
    assert f"[{name}]" in str(caught.value), str(caught.value)


def test_a_forged_metric_row_trips_the_metrics_assertion(cases, ph_table_oracle):
    cfg, _, lanes, rec = cases["wt", "f64"]
    for row in (2, 6):                                                      # ITAE (bit-equal), return (the oracle's rewards)
        forged = dict(rec, pairs=rec["pairs"].copy())
        forged["pairs"][1, row, 3, 5] *= 1.001
        with pytest.raises(AssertionError) as caught:
            G.check_recording("wt", cfg, lanes, ph_table_oracle, forged)
        assert "[metrics]" in str(caught.value)


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------
def test_host_argument_errors(ph_table_oracle):
    import pime_amd.native as nt
    bad = []
    for kind in ("wt", "ph"):
        cfg, keep, lanes = G.twin_case(kind, 8, ph_table_oracle)
        sp = np.ascontiguousarray(G.SETPOINTS[kind], dtype=np.float64)
        K = np.ascontiguousarray(G.PRIOR_K[kind])
        pt = np.ascontiguousarray(G.PERTURB)
        base = dict(lanes=lanes, N=8, K=K, pt=pt, P=5, n_steps=G.N_STEPS, seg_len=G.SEG, sp=sp, n_sp=3, band=G.BAND, tail=4, summary=True,
                    sm=nt.STATE_F64, stack=0)
        todo = [("P = 0", dict(P=0)), ("perturb is NULL", dict(pt=None)), ("summary is NULL", dict(summary=False)), ("priorK is NULL", dict(K=None)),
                ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)),
                ("n_setpoints 17", dict(n_sp=17)), ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)),
                ("set-point schedule", dict(seg_len=-1)), ("NULL lanes", dict(lanes=None)), ("N = 0", dict(N=0)),
                ("lane array", dict(lanes={k: v for k, v in lanes.items() if k != "r"})), ("state_mode", dict(sm=nt.STATE_MIXED16))]
        if kind == "wt":
            todo.append(("Stacking", dict(stack=1)))
        for word, over in todo:
            kw = dict(base, **over)
            cfg.state_mode, cfg.num_stack = kw["sm"], kw["stack"]
            summary = np.full((5, 3, 8, 5), -777.0)
            rc, msg = G.host_raw(kind, cfg, kw["lanes"], kw["N"], kw["K"], kw["pt"], kw["P"], G.NOISE_SEED, G.NOISE_EPOCH, kw["n_steps"],
                                 kw["seg_len"], kw["sp"], kw["n_sp"], kw["band"], kw["tail"], None, summary if kw["summary"] else None, None, None)
            if rc != -1 or word not in msg or not (summary == -777.0).all():
                bad.append((kind, word, rc, msg))
        cfg.state_mode, cfg.num_stack = nt.STATE_F64, 0
    assert not bad, bad


# ---- 6. protocols and the wrapper --------------------------------------------------------------------------------------------------
def test_perturbation_grid_order():
    from pime_amd import protocols
    grid = protocols.perturbation_grid(gains=(1.0, 2.0), delays=(0, 1, 3), sigmas=(0.0, 0.1))
    assert grid.shape == (12, 3) and grid.dtype == np.float64 and grid.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(grid[:4], [[1, 0, 0], [1, 0, 0.1], [1, 1, 0], [1, 1, 0.1]])
    np.testing.assert_array_equal(grid[6], [2, 0, 0])
    np.testing.assert_array_equal(protocols.perturbation_grid(), [[1.0, 0.0, 0.0]])
    with pytest.raises(ValueError):
        protocols.perturbation_grid(delays=())


def _summary(rows, itae, settle, av, n=4, steps=20):
    """A hand-made one-segment summary [P, 1, 8, 5]: the worst plant's ITAE and settling step and the plants' action variation sum."""
    from pime_amd import protocols
    s = np.zeros((len(rows), 1, 8, 5))
    s[..., P.FINITE] = n
    s[:, 0, protocols.METRIC_NAMES.index("itae"), P.MAX] = itae
    s[:, 0, protocols.METRIC_NAMES.index("settling_step"), P.MAX] = settle
    s[:, 0, protocols.METRIC_NAMES.index("action_variation"), P.SUM] = np.asarray(av) * n
    return dict(perturb=np.asarray(rows, dtype=np.float64), summary=s, pairs=None, steps=steps, n=n)


def test_loop_margins_on_hand_made_summaries():
    from pime_amd import protocols
    rows = [[1, 0, 0], [1, 1, 0], [1, 2, 0], [1, 3, 0], [1, 4, 0], [2, 0, 0], [4, 0, 0], [0.5, 0, 0], [0.25, 0, 0], [1, 0, 0.1], [1, 0, 0.2],
            [2, 1, 0.1]]
    itae = [10, 12, 19, 21, 11, 15, 100, 12, 30, 11, 12, 1]
    settle = [5, 6, 8, 9, 9, 7, 20, 6, 9, 5, 20, 1]
    av = [1.0, 1, 1, 1, 1, 1, 1, 1, 1, 1.5, 2.0, 9]
    m = protocols.loop_margins(_summary(rows, itae, settle, av))
    assert m["nominal"] == 0
    # delay: 3 costs 21 > 2 x 10, so the margin is 2 although 4 would pass again; gain up: 4 never settles; down: 0.25 costs 30
    assert (m["delay_margin"], m["gain_margin"], m["gain_margin_low"]) == (2.0, 2.0, 0.5)
    assert m["sigma_margin"] == 0.1 and m["sigma_slope"] == pytest.approx(5.0)
    assert m["acceptable"].tolist() == [True, True, True, False, True, True, False, True, False, True, False, True]
    assert protocols.loop_margins(_summary(rows, itae, settle, av), factor=3.0)["delay_margin"] == 4.0
    lost = _summary(rows, itae, settle, av)
    lost["summary"][1, 0, 3, P.FINITE] = 3                                  # a plant of the one-step delay row went non-finite
    assert protocols.loop_margins(lost)["delay_margin"] == 0.0
    unsettled = _summary(rows, itae, [20] + settle[1:], av)
    assert np.isnan(protocols.loop_margins(unsettled)["delay_margin"]), "the nominal loop itself does not settle"
    with pytest.raises(ValueError):
        protocols.loop_margins(_summary(rows[1:], itae[1:], settle[1:], av[1:]))
    with pytest.raises(ValueError):
        protocols.loop_margins(_summary(rows, itae, settle, av), cost="nope")
    # per plant, from pairs [S, 8, P, N]: plant 0 tolerates two steps of delay, plant 1 none
    rows = [[1, 0, 0], [1, 1, 0], [1, 2, 0]]
    res = _summary(rows, [10, 30, 30], [5, 6, 7], [1, 1, 1], n=2)
    pairs = np.zeros((1, 8, 3, 2))
    pairs[0, protocols.METRIC_NAMES.index("itae")] = [[10, 10], [12, 30], [13, 30]]
    pairs[0, protocols.METRIC_NAMES.index("settling_step")] = [[5, 5], [6, 6], [7, 7]]
    res["pairs"] = pairs
    m = protocols.loop_margins(res)
    assert m["delay_margin"] == 0.0 and m["plant_delay_margin"].tolist() == [2.0, 0.0] and m["plant_gain_margin"].tolist() == [1.0, 1.0]


def test_the_wrappers_value_errors():
    from pime_amd.vec_env import check_perturb
    good = check_perturb([[1.0, 8, 0.0], [-0.5, 0, 0.3]])
    assert good.shape == (2, 3) and good.dtype == np.float64
    for rows, word in (([[float("nan"), 0, 0]], "gain"), ([[float("inf"), 0, 0]], "gain"), ([[1, 0.5, 0]], "delay"), ([[1, 9, 0]], "delay"),
                       ([[1, -1, 0]], "delay"), ([[1, float("nan"), 0]], "delay"), ([[1, 0, -0.1]], "sigma"), ([[1, 0, float("inf")]], "sigma"),
                       ([[1, 0, float("nan")]], "sigma"), ([[1, 0]], "perturb"), ([1, 0, 0], "perturb"), (np.zeros((0, 3)), "perturb")):
        with pytest.raises(ValueError, match=word):
            check_perturb(rows)
