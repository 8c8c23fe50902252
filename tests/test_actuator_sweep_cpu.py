"""The actuator-limits sweep without a GPU: the HOST build of the pair function the kernel runs (csrc/actuator_sweep.hpp compiled into
libpime_actuator_host.so, the prior controller alone, float64 and float32 state) against the numpy restatement and the checker of
tests/actuator_sweep.py, and that checker against itself.  Shapes: 81 plants at lane offset 1000, the ten rows of
tests/actuator_sweep.py (all-off, each stage alone, clamp + quantise, dead-band + slew, everything on, all-off again), 23 steps in
segments of 9, tail 4, the tank's process noise on.
  1. symbols: header, binding and libraries agree; ABI 26; pime_actuator_sweep_supported(NULL, -1, 0) == 0; the package never names
     the host library;
  2. the float64 host build: bit-equal to the numpy restatement on both envs, the all-off rows bit-equal to libpime_sweep_host.so's
     pairs with the same gain and to the (1, 0, 0) row of libpime_margin_host.so, every stage changes at least one step of at least one
     plant, summary bit-equal to summary_from_pairs(pairs) (also at N = 130: three blocks), NULL pairs / actions / commands / outputs
     change no bit of summary; the float32 host build inside the bars;
  3. how a row is decoded: every "off" spelling;
  4. the checker: honest synthetic recordings (with a numpy policy) use less than 0.1 of every bar, each single fault trips the
     assertion named for it;
  5. every argument error of the host build carries its message;
  6. protocols.actuator_grid's order, protocols.actuator_summary on hand-made results, protocols.rig_row against its derivation, the
     wrapper's ValueErrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import actuator_sweep as A
import margin_sweep as G
import prior_sweep as P
from conftest import ROOT

CLASSES = [(kind, sm) for kind in ("ph", "wt") for sm in ("f64", "mixed")]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def cases(ph_table_oracle):
    """(cfg, keep, lanes, host recording) per class, computed once and left unchanged."""
    out = {}
    for kind, sm in CLASSES:
        cfg, keep, lanes = A.twin_case(kind, A.N, ph_table_oracle, sm)
        out[kind, sm] = (cfg, keep, lanes, A.host_actuator(kind, cfg, lanes))
    return out


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pime_actuator_sweep_supported", "pime_actuator_sweep_workspace_bytes", "pime_actuator_sweep")


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
    assert nt.lib().pime_actuator_sweep_supported(None, -1, 0) == 0
    assert nt.lib().pime_actuator_sweep_workspace_bytes(None, 1, 1, 0) == -1
    assert (nt.ACT_COLS, nt.ACT_ROWS) == (6, 8) == (A.COLS, A.AROWS)
    assert nt.ACT_COL_NAMES == ("lo", "hi", "rate", "deadband", "qu", "qy")
    assert nt.ACT_ROW_NAMES == ("sat_steps", "rate_steps", "hold_steps", "gap_peak", "gap_iae", "reversals", "tail_y_p2p", "tail_u_p2p")
    header = open(os.path.join(ROOT, "include", "pime_hip.h")).read()
    for j, name in enumerate(nt.ACT_COL_NAMES):
        assert f"PIME_ACT_{name.upper()} = {j}" in header, name
    for j, name in enumerate(nt.ACT_ROW_NAMES):
        assert f"PIME_ACT_{name.upper()} = {j}" in header, name
    assert "PIME_ACT_COLS = 6" in header and "PIME_ACT_ROWS = 8" in header
    host = C.CDLL(A.HOST_LIB_PATH)
    assert _declared("pime_actuator_host.h") == set(A.HOST_EXPORTS)
    for name in A.HOST_EXPORTS:
        assert hasattr(host, name), name
    for name in NEW_SYMBOLS:     # the host library is no second door to the product's entry points
        assert not hasattr(host, name), name


def test_the_package_never_names_the_host_library():
    for d, _, files in os.walk(P.PKG):
        for f in files:
            if f.endswith(".py"):
                assert "actuator_host" not in open(os.path.join(d, f)).read(), os.path.join(d, f)


# ---- 2. the host build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_host_equals_numpy(cases, ph_table_oracle, kind):
    cfg, _, lanes, rec = cases[kind, "f64"]
    assert not any((rec[k] == -777.0).any() for k in rec), "every word is written"
    ref = A.numpy_loop(kind, cfg, lanes, ph_table_oracle)
    for k in ("commands", "actions", "outputs", "pairs"):
        assert A.bits_equal(rec[k], ref[k]), k


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_every_stage_changes_a_step(cases, kind):
    """What the rows are about: each stage acts on at least one step of at least one plant, alone and in company."""
    _, _, _, rec = cases[kind, "f64"]
    pairs, act, cmd, out = rec["pairs"], rec["actions"], rec["commands"], rec["outputs"]
    count = lambda row, p: pairs[:, row, p].sum()
    assert count(A.SAT_STEPS, 1) > 0 and count(A.RATE_STEPS, 2) > 0 and count(A.HOLD_STEPS, 3) > 0
    assert (act[:, 4] != cmd[:, 4]).any() and (cmd[:, 5] != cmd[:, 0]).any(), "the actuator's and the sensor's quantum"
    assert count(A.SAT_STEPS, 6) > 0 and count(A.RATE_STEPS, 7) > 0 and count(A.HOLD_STEPS, 7) > 0
    assert all(count(r, 8) > 0 for r in (A.SAT_STEPS, A.RATE_STEPS, A.HOLD_STEPS))
    # the tank's clamp sits inside the range the prior's first-step command reaches, on both sides
    if kind == "wt":
        assert (cmd[0, 1] < A.ACT[kind][1, A.LO]).any() and (cmd[0, 1] > A.ACT[kind][1, A.HI]).any()
    # clamp last: a saturated step sits ON the limit, which is no multiple of QU; quantised steps inside the limits are multiples
    lo, hi, qu = A.ACT[kind][6, A.LO], A.ACT[kind][6, A.HI], A.ACT[kind][6, A.QU]
    u = act[:, 6]
    assert ((u == lo) | (u == hi)).any() and (u >= lo).all() and (u <= hi).all()
    assert np.rint(lo / qu) * qu != lo and np.rint(hi / qu) * qu != hi
    inside = (u > lo) & (u < hi)
    assert inside.any() and (u[inside] == qu * np.rint(u[inside] / qu)).all()
    # slew alone: no move exceeds the rate (to an ulp of the sum's rounding), and the gap rows see it
    rate = A.ACT[kind][2, A.RATE]
    moves = np.diff(np.concatenate([np.zeros_like(act[:1, 2]), act[:, 2]]), axis=0)
    assert (np.abs(moves) <= rate * (1 + 1e-12)).all() and (pairs[:, A.GAP_PEAK, 2] > 0).any()
    # dead-band alone: a held step repeats the previous applied action
    held = np.abs(cmd[1:, 3] - act[:-1, 3]) <= A.ACT[kind][3, A.DEADBAND]
    assert held.any() and (act[1:, 3][held] == act[:-1, 3][held]).all() and (act[1:, 3][~held] == cmd[1:, 3][~held]).all()
    # the sensor's quantum moves the trajectory; the all-off rows are the ideal loop and agree with each other
    assert (out[:, 5] != out[:, 0]).any()
    assert A.bits_equal(pairs[:, :, 0], pairs[:, :, 9]) and A.bits_equal(act[:, 0], cmd[:, 0]) and A.bits_equal(act[:, 9], act[:, 0])
    assert (pairs[:, 8:13, 0] == 0).all(), "no stage, no gap"
    assert np.isfinite(pairs).all() and (pairs[:, [A.SAT_STEPS, A.RATE_STEPS, A.HOLD_STEPS, A.REVERSALS]] % 1 == 0).all()
    assert (pairs[:, A.REVERSALS] <= np.array([9, 9, 5])[:, None, None] - 1).all()


@pytest.mark.parametrize("kind,sm", CLASSES, ids=lambda v: str(v))
def test_host_build_passes_the_checker(cases, ph_table_oracle, kind, sm):
    cfg, _, lanes, rec = cases[kind, sm]
    use = A.check_recording(kind, cfg, lanes, ph_table_oracle, rec, tag=f"{kind}-{sm}")
    print(f"\nACTUATOR host id={kind}-{sm} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action "
          f"{use['action']:.3g} (gap {use['gap']:.4g})")
    P.check_summary(rec["summary"], rec["pairs"], tag=f"{kind}-{sm}")
    assert (rec["summary"][..., P.FINITE] == A.N).all(), "every row of every segment is finite"
    if sm == "f64":
        assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_all_off_rows_are_the_prior_sweeps_and_the_margin_sweeps_pairs(cases, ph_table_oracle, kind):
    cfg, _, lanes, rec = cases[kind, "f64"]
    over = {} if kind == "ph" else {"wt_noise_scale": 0.01}
    _, want = P.host_sweep(kind, lanes, A.PRIOR_K[kind][None], A.N_STEPS, A.SEG, A.SETPOINTS[kind], A.BAND, A.TAIL, table=ph_table_oracle,
                           seed=A.SEED, env_offset=A.OFFSET, cfg_over=over)
    margin = G.host_margin(kind, cfg, lanes, perturb=np.array([[1.0, 0.0, 0.0]]), n_steps=A.N_STEPS, seg_len=A.SEG, band=A.BAND, tail=A.TAIL)
    for p in A.ALL_OFF:
        assert A.bits_equal(rec["pairs"][:, :8, p], want[:, :, 0]), p
        assert A.bits_equal(rec["pairs"][:, :8, p], margin["pairs"][:, :, 0]), p
        assert A.bits_equal(rec["actions"][:, p], margin["actions"][:, 0]) and A.bits_equal(rec["outputs"][:, p], margin["outputs"][:, 0])
        assert A.bits_equal(rec["commands"][:, p], rec["actions"][:, p])


def test_three_summary_blocks_and_null_outputs(ph_table_oracle):
    cfg, keep, lanes = A.twin_case("wt", 130, ph_table_oracle)
    rec = A.host_actuator("wt", cfg, lanes)
    P.check_summary(rec["summary"], rec["pairs"], tag="N = 130")
    assert (rec["summary"][..., P.FINITE] == 130).all() and rec["summary"].shape == (10, 3, 16, 5)
    quiet = A.host_actuator("wt", cfg, lanes, trace=False, want_pairs=False)
    assert quiet["pairs"] is None and A.bits_equal(quiet["summary"], rec["summary"]), "NULL pairs / traces must not change a bit"
    one = A.host_actuator("wt", cfg, lanes, rows=A.ACT["wt"][8:9])
    assert A.bits_equal(one["pairs"][:, :, 0], rec["pairs"][:, :, 8]) and A.bits_equal(one["summary"][0], rec["summary"][8]), \
        "a row's result does not depend on the other rows"


# ---- 3. how a row is decoded ---------------------------------------------------------------------------------------------------------
def test_every_off_spelling_is_the_all_off_row(cases):
    cfg, _, lanes, rec = cases["wt", "f64"]
    odd = np.array([[NAN, NAN, NAN, NAN, NAN, NAN], [-INF, NAN, 0.0, -1.0, -0.5, -2.0], [NAN, INF, -3.0, 0.0, 0.0, 0.0],
                    [-INF, INF, INF, -0.0, -0.0, -0.0],
                    [NAN, 0.5, INF, 0, 0, 0], [-0.35, NAN, INF, 0, 0, 0]])
    got = A.host_actuator("wt", cfg, lanes, rows=odd)
    for p in range(4):
        for k in ("pairs", "actions", "commands", "outputs"):
            assert A.bits_equal(got[k][..., p, :], rec[k][..., 0, :]), (p, k)
    # a NaN limit beside a real one never binds: a one-sided clamp
    u, c = got["actions"], got["commands"]
    assert A.bits_equal(u[:, 4], np.minimum(c[:, 4], 0.5)) and (c[:, 4] > 0.5).any() and (u[:, 4] < -0.35).any()
    assert A.bits_equal(u[:, 5], np.maximum(c[:, 5], -0.35)) and (u[:, 5] > 0.5).any()


def test_the_chain_keeps_a_negative_zero_and_rounds_ties_to_even():
    z = np.array([-0.0, 0.0])
    u, _ = A.chain(A.OFF, z, np.zeros(2))
    assert A.bits_equal(u, z)
    u, _ = A.chain(A.OFF, z, np.zeros(2), fault="off_stage_rewrites")
    assert not A.bits_equal(u, z) and (u == z).all()
    q = 2.0 ** -5
    u, _ = A.chain((-INF, INF, INF, 0, q, 0), np.array([0.5, 1.5, 2.5, -0.5, -2.5]) * q, np.zeros(5))
    np.testing.assert_array_equal(u, np.array([0.0, 2.0, 2.0, -0.0, -2.0]) * q)
    # dead-band: the boundary holds; slew: measured from the applied action; clamp after quantise
    u, (held, _, _) = A.chain((-INF, INF, INF, 0.25, 0, 0), np.array([0.25, 0.2500001]), np.zeros(2))
    assert held.tolist() == [True, False] and u.tolist() == [0.0, 0.2500001]
    u, (_, slewed, _) = A.chain((-INF, INF, 0.5, 0, 0, 0), np.array([2.0, 0.25, -3.0]), np.array([1.0, 0.0, 0.0]))
    assert slewed.tolist() == [True, False, True] and u.tolist() == [1.5, 0.25, -0.5]
    u, (_, _, clamped) = A.chain((-0.35, 0.5, INF, 0, 0.12, 0), np.array([0.47, 0.55, -0.4, 0.1]), np.zeros(4))
    assert clamped.tolist() == [False, True, True, False] and u.tolist() == [0.12 * 4, 0.5, -0.35, 0.12]


# ---- 4. the checker --------------------------------------------------------------------------------------------------------------
_Q = 2.0 ** -4
# fault -> (kind, the assertion it trips, how the loop is run: its own rows / const: zero prior gains and a constant policy term / negzero)
FAULT_CASES = {
    "clamp_before_quantise": ("wt", "chain", {}),
    "slew_from_command": ("ph", "chain", {}),
    "uprev_cleared": ("wt", "chain", {}),
    "deadband_strict": ("wt", "chain", dict(rows=[A.OFF, (-INF, INF, INF, 0.375, 0, 0)], const=0.375)),      # |a_c - 0| == DEADBAND at step 0
    "round_half_up": ("ph", "chain", dict(rows=[A.OFF, (-INF, INF, INF, 0, _Q, 0)], const=2.5 * _Q)),         # a tie: to even, 2 Q
    "qy_on_setpoint": ("wt", "action", dict(rows=[A.OFF, (-INF, INF, INF, 0, 0, 0.35)])),                     # (no set-point is a multiple of 0.35)
    "qy_truncates": ("ph", "action", {}),
    "metrics_fed_command": ("wt", "metrics", {}),
    "reversals_count_zero": ("ph", "actuator", {}),
    "tail_off_by_one": ("wt", "actuator", {}),
    "sat_counts_unchanged": ("ph", "actuator", {}),
    "gap_iae_descending": ("wt", "actuator", {}),
    "off_stage_rewrites": ("wt", "chain", dict(rows=[A.OFF, A.OFF], const=0.0, negzero=True)),
}


def test_every_fault_is_listed():
    assert sorted(FAULT_CASES) == sorted(A.FAULTS) and len(A.FAULTS) >= 12


@pytest.fixture(scope="module")
def honest(cases, ph_table_oracle):
    out = {}
    for kind in ("ph", "wt"):
        cfg, _, lanes, _ = cases[kind, "f64"]
        pol = G.NumpyPolicy(len(A.PRIOR_K[kind]))
        out[kind] = (pol, A.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol))
    return out


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_honest_recordings_pass_far_inside(cases, honest, ph_table_oracle, kind):
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, rec = honest[kind]
    use = A.check_recording(kind, cfg, lanes, ph_table_oracle, rec, policy=pol.term)
    assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use
    assert A.bits_equal(rec["pairs"][:, :, 0], rec["pairs"][:, :, 9])
    assert all(rec["pairs"][:, r, 8].sum() > 0 for r in (A.SAT_STEPS, A.RATE_STEPS, A.HOLD_STEPS)), "under the policy too, every stage acts"


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_each_fault_trips_the_assertion_named_for_it(cases, honest, ph_table_oracle, fault):
    kind, name, how = FAULT_CASES[fault]
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, _ = honest[kind]
    kw = {}
    if how:
        kw = dict(rows=np.array(how["rows"], dtype=np.float64))
        if "const" in how:
            pol, kw["K"] = A.ConstPolicy(how["const"]), np.zeros(len(A.PRIOR_K[kind]))
        run = dict(kw, negzero=how.get("negzero", False))
        # the honest recording of this set-up passes: the fault alone trips
        A.check_recording(kind, cfg, lanes, ph_table_oracle, A.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol, **run), policy=pol.term, **kw)
    else:
        run = {}
    forged = A.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol, fault=fault, **run)
    with pytest.raises(AssertionError) as caught:
        A.check_recording(kind, cfg, lanes, ph_table_oracle, forged, policy=pol.term, **kw)
    assert f"[{name}]" in str(caught.value), str(caught.value)


def test_a_forged_row_trips_its_assertion(cases, ph_table_oracle):
    cfg, _, lanes, rec = cases["wt", "f64"]
    for row, name in ((2, "metrics"), (7, "metrics"), (A.GAP_IAE, "actuator"), (A.TAIL_U_P2P, "actuator"), (A.SAT_STEPS, "actuator")):
        forged = dict(rec, pairs=rec["pairs"].copy())
        forged["pairs"][1, row, 8, 5] = forged["pairs"][1, row, 8, 5] * 1.001 + 1.0
        with pytest.raises(AssertionError) as caught:
            A.check_recording("wt", cfg, lanes, ph_table_oracle, forged)
        assert f"[{name}]" in str(caught.value)


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------
def test_host_argument_errors(ph_table_oracle):
    import pime_amd.native as nt
    bad = []
    for kind in ("wt", "ph"):
        cfg, keep, lanes = A.twin_case(kind, 8, ph_table_oracle)
        sp = np.ascontiguousarray(A.SETPOINTS[kind], dtype=np.float64)
        K = np.ascontiguousarray(A.PRIOR_K[kind])
        at = np.ascontiguousarray(A.ACT[kind])
        base = dict(lanes=lanes, N=8, K=K, at=at, P=10, n_steps=A.N_STEPS, seg_len=A.SEG, sp=sp, n_sp=3, band=A.BAND, tail=4, summary=True,
                    sm=nt.STATE_F64, stack=0)
        todo = [("P = 0", dict(P=0)), ("actuator is NULL", dict(at=None)), ("summary is NULL", dict(summary=False)), ("priorK is NULL", dict(K=None)),
                ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)),
                ("n_setpoints 17", dict(n_sp=17)), ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)),
                ("set-point schedule", dict(seg_len=-1)), ("NULL lanes", dict(lanes=None)), ("N = 0", dict(N=0)),
                ("lane array", dict(lanes={k: v for k, v in lanes.items() if k != "r"})), ("state_mode", dict(sm=nt.STATE_MIXED16))]
        if kind == "wt":
            todo.append(("Stacking", dict(stack=1)))
        for word, over in todo:
            kw = dict(base, **over)
            cfg.state_mode, cfg.num_stack = kw["sm"], kw["stack"]
            summary = np.full((10, 3, 16, 5), -777.0)
            rc, msg = A.host_raw(kind, cfg, kw["lanes"], kw["N"], kw["K"], kw["at"], kw["P"], kw["n_steps"], kw["seg_len"], kw["sp"], kw["n_sp"],
                                 kw["band"], kw["tail"], None, summary if kw["summary"] else None, None, None, None)
            if rc != -1 or word not in msg or not (summary == -777.0).all():
                bad.append((kind, word, rc, msg))
        cfg.state_mode, cfg.num_stack = nt.STATE_F64, 0
    assert not bad, bad


# ---- 6. protocols and the wrapper --------------------------------------------------------------------------------------------------
def test_actuator_grid_is_a_product_led_by_the_all_off_row():
    from pime_amd import protocols
    grid = protocols.actuator_grid(limits=[(-0.5, 0.5)], rates=(0.1,), qu=(0.01, 0.02))
    assert grid.shape == (2 * 2 * 1 * 3 * 1, 6) and grid.dtype == np.float64 and grid.flags["C_CONTIGUOUS"]
    off = list(protocols.ACT_OFF)
    np.testing.assert_array_equal(grid[0], off)
    assert not any(A.stages(grid[0]).values())
    want = [[-INF, INF, INF, 0, 0, 0], [-INF, INF, INF, 0, 0.01, 0], [-INF, INF, INF, 0, 0.02, 0],
            [-INF, INF, 0.1, 0, 0, 0], [-INF, INF, 0.1, 0, 0.01, 0], [-INF, INF, 0.1, 0, 0.02, 0],
            [-0.5, 0.5, INF, 0, 0, 0], [-0.5, 0.5, INF, 0, 0.01, 0], [-0.5, 0.5, INF, 0, 0.02, 0],
            [-0.5, 0.5, 0.1, 0, 0, 0], [-0.5, 0.5, 0.1, 0, 0.01, 0], [-0.5, 0.5, 0.1, 0, 0.02, 0]]
    np.testing.assert_array_equal(grid, want)
    np.testing.assert_array_equal(protocols.actuator_grid(), [off])
    full = protocols.actuator_grid(limits=[(-1, 1), (0, 1)], rates=(1, 2), deadbands=(0.1,), qu=(0.5,), qy=(0.25, 0.125, 0.5))
    assert full.shape == (3 * 3 * 2 * 2 * 4, 6) and len({tuple(r) for r in full}) == len(full)
    np.testing.assert_array_equal(full[1], [-INF, INF, INF, 0, 0, 0.25])


def test_rig_row_follows_its_derivation():
    from pime_amd import protocols
    row = protocols.rig_row(10.0)
    volts = lambda a, p: a * p / 2 + p / 2                       # the rig's map from the command to the pump voltage
    assert volts(row[A.LO], 10.0) == 0.0 and volts(row[A.HI], 10.0) == 10.0
    assert volts(row[A.QU], 10.0) - volts(0.0, 10.0) == 10.0 / 256       # one DAC level, in volts
    assert row[A.QY] == 10.0 / 504 and row[A.RATE] == INF and row[A.DEADBAND] == 0.0
    assert A.stages(row) == dict(clamp=True, slew=False, hold=False, quant=True, sense=True)
    np.testing.assert_array_equal(row, [-1.0, 1.0, INF, 0.0, 2.0 / 256, 10.0 / 504])
    big = protocols.rig_row(20.0)                                 # a 20 V command range clipped at 10 V: the upper half is lost
    assert volts(big[A.LO], 20.0) == 0.0 and volts(big[A.HI], 20.0) == 10.0 and big[A.HI] == 0.0 and big[A.QU] == 1.0 / 256
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            protocols.rig_row(bad)


def test_actuator_summary_on_hand_made_results():
    from pime_amd import protocols
    rows = np.concatenate([protocols.actuator_grid(qu=(0.01, 0.02, 0.04))[:, :], protocols.actuator_grid(limits=[(-1, 1), (-0.5, 0.5)])[1:],
                           [[-1, 1, INF, 0, 0.01, 0]]])
    Pn, S, n, band = len(rows), 2, 3, 0.05
    assert Pn == 7
    from pime_amd.native import METRIC_NAMES
    itae, y_p2p, rev = METRIC_NAMES.index("itae"), A.TAIL_Y_P2P, A.REVERSALS
    pairs = np.zeros((S, 16, Pn, n))
    pairs[:, itae] = 1.0
    pairs[1, itae, 0, 2] = 4.0                                     # the ideal row's worst plant
    pairs[0, itae, 2, 1] = 6.0
    pairs[:, y_p2p, 2] = [[0.0, 0.06, 0.0], [0.0, 0.0, 0.0]]       # qu 0.02: one of six pairs cycles
    pairs[:, y_p2p, 3] = 0.2                                        # qu 0.04: all
    pairs[:, y_p2p, 1] = 0.05                                       # qu 0.01: AT the band is not beyond it
    pairs[:, y_p2p, 5] = [[0.1, 0.0, 0.0], [0.1, 0.0, 0.0]]        # the tighter clamp
    pairs[:, rev, 3] = [[1, 2, 3], [4, 5, 60]]
    summary = P.summary_from_pairs(pairs)
    res = dict(rows=rows, summary=summary, pairs=pairs, steps=9, band=band, n=n)
    r = protocols.actuator_summary(res)
    np.testing.assert_array_equal(r["itae_ratio"], [1.0, 0.25, 1.5, 0.25, 0.25, 0.25, 0.25])
    np.testing.assert_array_equal(r["limit_cycle"], [0, 0, 1 / 6, 1.0, 0, 1 / 3, 0])
    np.testing.assert_array_equal(r["reversals"], [0, 0, 0, 3.5, 0, 0, 0])
    assert r["qu_tolerated"] == 0.01 and r["limits_tolerated"] == 2.0
    assert np.isnan(r["rate_tolerated"]) and np.isnan(r["deadband_tolerated"]) and np.isnan(r["qy_tolerated"])
    quiet = protocols.actuator_summary(dict(res, pairs=None))
    np.testing.assert_array_equal(quiet["itae_ratio"], r["itae_ratio"])
    np.testing.assert_array_equal(quiet["limit_cycle"], [0, 0, 0.5, 1.0, 0, 1.0, 0])
    assert np.isnan(quiet["reversals"]).all() and quiet["qu_tolerated"] == 0.01
    with pytest.raises(ValueError, match="row 0"):
        protocols.actuator_summary(dict(res, rows=rows[1:], summary=summary[1:], pairs=pairs[:, :, 1:]))


def test_the_wrappers_value_errors():
    from pime_amd.vec_env import check_actuator
    good = check_actuator([[-1, 1, INF, 0, 1 / 128, 10 / 504], list(A.OFF), [-INF, 0.5, 0.0, INF, 0, 0]])
    assert good.shape == (3, 6) and good.dtype == np.float64
    for rows, word in (([[NAN, 1, INF, 0, 0, 0]], "limit"), ([[-1, NAN, INF, 0, 0, 0]], "limit"), ([[1, -1, INF, 0, 0, 0]], "limit"),
                       ([[-1, 1, NAN, 0, 0, 0]], "rate"), ([[-1, 1, -0.1, 0, 0, 0]], "rate"), ([[-1, 1, INF, NAN, 0, 0]], "deadband"),
                       ([[-1, 1, INF, -1, 0, 0]], "deadband"), ([[-1, 1, INF, 0, -1, 0]], "qu"), ([[-1, 1, INF, 0, INF, 0]], "qu"),
                       ([[-1, 1, INF, 0, 0, NAN]], "qy"), ([[-1, 1, INF, 0, 0, INF]], "qy"), ([[-1, 1, INF, 0, 0]], "rows"),
                       ([-1, 1, INF, 0, 0, 0], "rows"), (np.zeros((0, 6)), "rows")):
        with pytest.raises(ValueError, match=word):
            check_actuator(rows)
