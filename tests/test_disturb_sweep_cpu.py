"""The disturbance-rejection sweep without a GPU: the HOST build of the pair function the kernel runs (csrc/disturb_sweep.hpp compiled
into libpime_disturb_host.so, the prior controller alone, float64 and float32 state) against the numpy restatement and the checker of
tests/disturb_sweep.py, and that checker against itself.  Shapes: 81 plants at lane offset 1000, the seven rows of
tests/disturb_sweep.py (nominal, load step, pulse from the first step, plant step, a late onset with load and plant step, a pulse the
boundary cuts, nominal with a finite window), 23 steps in segments of 9, tail 4, the tank's process noise on.
  1. symbols: header, binding and libraries agree; ABI 26; pime_disturb_sweep_supported(NULL, -1, 0) == 0; the package never names
     the host library;
  2. the float64 host build: bit-equal to the numpy restatement on the tank rows and the pH rows with M0 == 1 (the others through the
     checker: libm and numpy may differ in the last bit of exp), the eight rows of rows 1 and 7 bit-equal to libpime_sweep_host.so's
     pairs with the same gain and to the (1, 0, 0) row of libpime_margin_host.so, summary bit-equal to summary_from_pairs(pairs) (also at
     N = 130: three blocks), NULL pairs / actions / outputs change no bit of summary; the float32 host build inside the bars;
  3. how a row is read: rounding, clamping, NaN;
  4. the checker: honest synthetic recordings (with a numpy policy) use less than 0.1 of every bar, each single fault trips the
     assertion named for it;
  5. every argument error of the host build carries its message;
  6. protocols.disturbance_grid's order, protocols.rejection_summary on hand-made summaries, the wrapper's ValueErrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import disturb_sweep as D
import margin_sweep as G
import prior_sweep as P
from conftest import ROOT

CLASSES = [(kind, sm) for kind in ("ph", "wt") for sm in ("f64", "mixed")]


@pytest.fixture(scope="module")
def cases(ph_table_oracle):
    """(cfg, keep, lanes, host recording) per class, computed once and left unchanged."""
    out = {}
    for kind, sm in CLASSES:
        cfg, keep, lanes = D.twin_case(kind, D.N, ph_table_oracle, sm)
        out[kind, sm] = (cfg, keep, lanes, D.host_disturb(kind, cfg, lanes))
    return out


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pime_disturb_sweep_supported", "pime_disturb_sweep_workspace_bytes", "pime_disturb_sweep")


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
    assert nt.lib().pime_disturb_sweep_supported(None, -1, 0) == 0
    assert nt.lib().pime_disturb_sweep_workspace_bytes(None, 1, 1, 0) == -1
    assert (nt.DISTURB_COLS, nt.DISTURB_ROWS) == (6, 7) == (D.COLS, D.DROWS)
    assert nt.DISTURB_COL_NAMES == ("onset", "length", "load", "m0", "m1", "m2")
    assert nt.DISTURB_ROW_NAMES == ("e0", "peak", "peak_step", "recovery", "iae", "itae", "action_peak")
    header = open(os.path.join(ROOT, "include", "pime_hip.h")).read()
    for j, name in enumerate(nt.DISTURB_COL_NAMES):
        assert f"PIME_DISTURB_{name.upper()} = {j}" in header, name
    for j, name in enumerate(nt.DISTURB_ROW_NAMES):
        assert f"PIME_DISTURB_{name.upper()} = {j}" in header, name
    assert "PIME_DISTURB_COLS = 6" in header and "PIME_DISTURB_ROWS = 7" in header
    host = C.CDLL(D.HOST_LIB_PATH)
    assert _declared("pime_disturb_host.h") == set(D.HOST_EXPORTS)
    for name in D.HOST_EXPORTS:
        assert hasattr(host, name), name
    for name in NEW_SYMBOLS:     # the host library is no second door to the product's entry points
        assert not hasattr(host, name), name


def test_the_package_never_names_the_host_library():
    for d, _, files in os.walk(P.PKG):
        for f in files:
            if f.endswith(".py"):
                assert "disturb_host" not in open(os.path.join(d, f)).read(), os.path.join(d, f)


# ---- 2. the host build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_host_equals_numpy(cases, ph_table_oracle, kind):
    cfg, _, lanes, rec = cases[kind, "f64"]
    assert not any((rec[k] == -777.0).any() for k in rec), "every word is written"
    ref = D.numpy_loop(kind, cfg, lanes, ph_table_oracle)
    exact = [p for p in range(len(D.DISTURB[kind])) if kind == "wt" or D.DISTURB[kind][p, 3] == 1.0]
    assert exact == ([0, 1, 2, 3, 4, 5, 6] if kind == "wt" else [0, 1, 2, 4, 5, 6])
    for k in ("actions", "outputs", "pairs"):
        assert D.bits_equal(rec[k][..., exact, :], ref[k][..., exact, :]), k
    # what the rows are about
    pairs, act, out = rec["pairs"], rec["actions"], rec["outputs"]
    assert D.bits_equal(pairs[:, :8, 0], pairs[:, :8, 6]) and D.bits_equal(act[:, 0], act[:, 6]), "zero load, unit multipliers: any onset"
    assert np.isnan(pairs[2, 8:, 4]).all() and np.isnan(pairs[2, 8:, 5]).all(), "onset beyond the ragged segment (5 steps)"
    assert np.isfinite(pairs[:2, 8:, 4]).all() and np.isfinite(pairs[:, 8:, [0, 1, 2, 3, 6]]).all()
    assert D.bits_equal(out[:3, 1], out[:3, 0]) and (out[3, 1] != out[3, 0]).any(), "the load arrives with step 3"
    assert (out[0, 2] != out[0, 0]).any() and (pairs[0, D.E0, 2] == pairs[0, D.E0, 0]).all(), "a pulse from the first step starts where the segment starts"
    assert D.bits_equal(out[:8, 5], out[:8, 0]) and (out[8, 5] != out[8, 0]).any() and not D.bits_equal(act[9, 5], act[9, 0])
    assert (pairs[:, D.PEAK_STEP, 0] >= 1).all() and (pairs[:2, D.RECOVERY, 0] <= 9).all() and (pairs[2, D.RECOVERY, 0] <= 5).all()


@pytest.mark.parametrize("kind,sm", CLASSES, ids=lambda v: str(v))
def test_host_build_passes_the_checker(cases, ph_table_oracle, kind, sm):
    cfg, _, lanes, rec = cases[kind, sm]
    use = D.check_recording(kind, cfg, lanes, ph_table_oracle, rec, tag=f"{kind}-{sm}")
    print(f"\nDISTURB host id={kind}-{sm} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action "
          f"{use['action']:.3g} (gap {use['gap']:.4g})")
    P.check_summary(rec["summary"], rec["pairs"], tag=f"{kind}-{sm}")
    assert (rec["summary"][4, 2, 8:, P.FINITE] == 0).all() and (rec["summary"][4, 2, :8, P.FINITE] == D.N).all(), "NaN rows are not counted"
    if sm == "f64":
        assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_undisturbed_rows_are_the_prior_sweeps_and_the_margin_sweeps_pairs(cases, ph_table_oracle, kind):
    cfg, _, lanes, rec = cases[kind, "f64"]
    over = {} if kind == "ph" else {"wt_noise_scale": 0.01}
    _, want = P.host_sweep(kind, lanes, D.PRIOR_K[kind][None], D.N_STEPS, D.SEG, D.SETPOINTS[kind], D.BAND, D.TAIL, table=ph_table_oracle,
                           seed=D.SEED, env_offset=D.OFFSET, cfg_over=over)
    margin = G.host_margin(kind, cfg, lanes, perturb=np.array([[1.0, 0.0, 0.0]]), n_steps=D.N_STEPS, seg_len=D.SEG, band=D.BAND, tail=D.TAIL)
    for p in (0, 6):
        assert D.bits_equal(rec["pairs"][:, :8, p], want[:, :, 0]), p
        assert D.bits_equal(rec["pairs"][:, :8, p], margin["pairs"][:, :, 0]), p
        assert D.bits_equal(rec["actions"][:, p], margin["actions"][:, 0]) and D.bits_equal(rec["outputs"][:, p], margin["outputs"][:, 0])


def test_three_summary_blocks_and_null_outputs(ph_table_oracle):
    cfg, keep, lanes = D.twin_case("wt", 130, ph_table_oracle)
    rec = D.host_disturb("wt", cfg, lanes)
    P.check_summary(rec["summary"], rec["pairs"], tag="N = 130")
    counted = rec["summary"][..., P.FINITE]
    assert ((counted == 130) | (counted == 0)).all() and (counted[:, :, :8] == 130).all() and rec["summary"].shape == (7, 3, 15, 5)
    quiet = D.host_disturb("wt", cfg, lanes, trace=False, want_pairs=False)
    assert quiet["pairs"] is None and D.bits_equal(quiet["summary"], rec["summary"]), "NULL pairs / actions / outputs must not change a bit"
    one = D.host_disturb("wt", cfg, lanes, rows=D.DISTURB["wt"][3:4])
    assert D.bits_equal(one["pairs"][:, :, 0], rec["pairs"][:, :, 3]) and D.bits_equal(one["summary"][0], rec["summary"][3]), \
        "a row's result does not depend on the other rows"


# ---- 3. how a row is read -----------------------------------------------------------------------------------------------------------
def test_onset_and_length_are_rounded_and_clamped(cases):
    cfg, _, lanes, rec = cases["wt", "f64"]
    nan = float("nan")
    odd = np.array([[3.4, 0.2, 0.3, 1, 1, 1], [-2.0, 2.0, -0.5, 1, 1, 1], [8.0, 1e12, 0.1, 1, 1, 1], [nan, 0, 0.3, 1.5, 0.7, 1], [3.0, nan, 0.3, 1, 1, 1],
                    [1e12, 0, 0.3, 1, 1, 1]])
    got = D.host_disturb("wt", cfg, lanes, rows=odd)
    for p, q in ((0, 1), (1, 2), (2, 5), (4, 1)):
        assert D.bits_equal(got["pairs"][:, :, p], rec["pairs"][:, :, q]), (p, q)
    for p in (3, 5):                                                      # never: the nominal response and no window anywhere
        assert D.bits_equal(got["pairs"][:, :8, p], rec["pairs"][:, :8, 0]) and np.isnan(got["pairs"][:, 8:, p]).all(), p


def test_a_negative_zero_action_keeps_its_sign():
    """Inactive steps add nothing: with zero gains the controller's output is obs * 0.0 summed from 0.0, and a row whose load is -0.0
    or whose window never opens leaves the same bits as the nominal row."""
    import oracle
    cfg, keep, lanes = D.twin_case("wt", 8, oracle.ph_table())
    K = np.array([0.0, -0.0, 0.0, 0.0])
    rows = np.array([[0, 0, 0.0, 1, 1, 1], [50, 0, 0.5, 2, 2, 2], [0, 0, -0.0, 1, 1, 1]], dtype=np.float64)
    got = D.host_disturb("wt", cfg, lanes, rows=rows, K=K)
    assert D.bits_equal(got["outputs"][:, 1], got["outputs"][:, 0]) and D.bits_equal(got["actions"][:, 1], got["actions"][:, 0])
    assert D.bits_equal(got["outputs"][:, 2], got["outputs"][:, 0])


# ---- 4. the checker --------------------------------------------------------------------------------------------------------------
# fault -> (kind, the assertion it trips, the prior gain's scale)
FAULT_CASES = {
    "onset_off_by_one": ("wt", "trajectory", 1.0), "pulse_long": ("ph", "trajectory", 1.0), "pulse_short": ("wt", "trajectory", 1.0),
    "kept_over_boundary": ("ph", "trajectory", 1.0), "load_behind_clip": ("ph", "trajectory", 40.0), "load_recorded": ("wt", "action", 1.0),
    "multiplier_wrong_parameter": ("wt", "trajectory", 1.0), "A_rebuilt_B_kept": ("ph", "trajectory", 1.0),
    "C_scaled_by_M0": ("ph", "trajectory", 1.0), "e0_after_step": ("wt", "rejection", 1.0), "peak_step_from_segment": ("ph", "rejection", 1.0),
    "recovery_from_segment": ("wt", "rejection", 1.0), "window_from_segment": ("ph", "rejection", 1.0), "finite_for_nan": ("wt", "nan", 1.0),
}


def test_every_fault_is_listed():
    assert sorted(FAULT_CASES) == sorted(D.FAULTS) and len(D.FAULTS) == 14


@pytest.fixture(scope="module")
def honest(cases, ph_table_oracle):
    out = {}
    for kind in ("ph", "wt"):
        cfg, _, lanes, _ = cases[kind, "f64"]
        pol = G.NumpyPolicy(len(D.PRIOR_K[kind]))
        out[kind] = (pol, D.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol))
    return out


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_honest_recordings_pass_far_inside(cases, honest, ph_table_oracle, kind):
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, rec = honest[kind]
    use = D.check_recording(kind, cfg, lanes, ph_table_oracle, rec, policy=pol.term)
    assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use
    assert D.bits_equal(rec["pairs"][:, :8, 0], rec["pairs"][:, :8, 6])


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_each_fault_trips_the_assertion_named_for_it(cases, honest, ph_table_oracle, fault):
    kind, name, scale = FAULT_CASES[fault]
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, _ = honest[kind]
    K = scale * D.PRIOR_K[kind]
    if scale != 1.0:     # the honest recording at this gain passes: the fault alone trips
        D.check_recording(kind, cfg, lanes, ph_table_oracle, D.numpy_loop(kind, cfg, lanes, ph_table_oracle, K=K, policy=pol), K=K, policy=pol.term)
    forged = D.numpy_loop(kind, cfg, lanes, ph_table_oracle, K=K, policy=pol, fault=fault)
    with pytest.raises(AssertionError) as caught:
        D.check_recording(kind, cfg, lanes, ph_table_oracle, forged, K=K, policy=pol.term)
    assert f"[{name}]" in str(caught.value), str(caught.value)


def test_a_late_row_that_differs_early_trips_the_nominal_assertion(cases, ph_table_oracle):
    cfg, _, lanes, rec = cases["wt", "f64"]
    forged = dict(rec, outputs=rec["outputs"].copy(), actions=rec["actions"].copy())
    forged["outputs"][:, 1], forged["actions"][:, 1] = rec["outputs"][:, 6], rec["actions"][:, 6]     # (keeps [trajectory] quiet: no load at all)
    with pytest.raises(AssertionError):
        D.check_recording("wt", cfg, lanes, ph_table_oracle, forged, only=[1])
    swapped = dict(rec, outputs=rec["outputs"].copy())
    swapped["outputs"][1, 0, 7] = np.nextafter(rec["outputs"][1, 0, 7], 1.0)                            # the nominal row moved by an ulp
    with pytest.raises(AssertionError) as caught:
        D.check_recording("wt", cfg, lanes, ph_table_oracle, swapped, only=[1])
    assert "[nominal]" in str(caught.value), str(caught.value)


def test_a_forged_row_trips_its_assertion(cases, ph_table_oracle):
    cfg, _, lanes, rec = cases["wt", "f64"]
    for row, name in ((2, "metrics"), (6, "metrics"), (D.ITAE, "rejection"), (D.ACTION_PEAK, "rejection")):
        forged = dict(rec, pairs=rec["pairs"].copy())
        forged["pairs"][1, row, 3, 5] *= 1.001
        with pytest.raises(AssertionError) as caught:
            D.check_recording("wt", cfg, lanes, ph_table_oracle, forged)
        assert f"[{name}]" in str(caught.value)


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------
def test_host_argument_errors(ph_table_oracle):
    import pime_amd.native as nt
    bad = []
    for kind in ("wt", "ph"):
        cfg, keep, lanes = D.twin_case(kind, 8, ph_table_oracle)
        sp = np.ascontiguousarray(D.SETPOINTS[kind], dtype=np.float64)
        K = np.ascontiguousarray(D.PRIOR_K[kind])
        dt = np.ascontiguousarray(D.DISTURB[kind])
        qww, qc = (None, None) if kind == "wt" else (np.ascontiguousarray(lanes["qww_V"]), np.ascontiguousarray(lanes["qc_V"]))
        base = dict(lanes=lanes, N=8, K=K, dt=dt, P=7, n_steps=D.N_STEPS, seg_len=D.SEG, sp=sp, n_sp=3, band=D.BAND, tail=4, summary=True,
                    sm=nt.STATE_F64, stack=0, qww=qww, qc=qc)
        todo = [("P = 0", dict(P=0)), ("disturb is NULL", dict(dt=None)), ("summary is NULL", dict(summary=False)), ("priorK is NULL", dict(K=None)),
                ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)),
                ("n_setpoints 17", dict(n_sp=17)), ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)),
                ("set-point schedule", dict(seg_len=-1)), ("NULL lanes", dict(lanes=None)), ("N = 0", dict(N=0)),
                ("lane array", dict(lanes={k: v for k, v in lanes.items() if k != "r"})), ("state_mode", dict(sm=nt.STATE_MIXED16))]
        if kind == "wt":
            todo.append(("Stacking", dict(stack=1)))
        else:
            todo += [("ph_qww or ph_qc is NULL", dict(qww=None)), ("ph_qww or ph_qc is NULL", dict(qc=None))]
        for word, over in todo:
            kw = dict(base, **over)
            cfg.state_mode, cfg.num_stack = kw["sm"], kw["stack"]
            summary = np.full((7, 3, 15, 5), -777.0)
            rc, msg = D.host_raw(kind, cfg, kw["lanes"], kw["N"], kw["qww"], kw["qc"], kw["K"], kw["dt"], kw["P"], kw["n_steps"], kw["seg_len"],
                                 kw["sp"], kw["n_sp"], kw["band"], kw["tail"], None, summary if kw["summary"] else None, None, None)
            if rc != -1 or word not in msg or not (summary == -777.0).all():
                bad.append((kind, word, rc, msg))
        cfg.state_mode, cfg.num_stack = nt.STATE_F64, 0
    assert not bad, bad


# ---- 6. protocols and the wrapper --------------------------------------------------------------------------------------------------
def test_disturbance_grid_order():
    from pime_amd import protocols
    grid = protocols.disturbance_grid(5, loads=(-0.1, 0.2), m0=(0.5,), m1=(1.5, 2.0), m2=(0.8,), length=3)
    assert grid.shape == (7, 6) and grid.dtype == np.float64 and grid.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(grid, [[5, 3, 0, 1, 1, 1], [5, 3, -0.1, 1, 1, 1], [5, 3, 0.2, 1, 1, 1], [5, 3, 0, 0.5, 1, 1],
                                         [5, 3, 0, 1, 1.5, 1], [5, 3, 0, 1, 2.0, 1], [5, 3, 0, 1, 1, 0.8]])
    np.testing.assert_array_equal(protocols.disturbance_grid(0), [[0, 0, 0, 1, 1, 1]])


def test_rejection_summary_on_hand_made_summaries():
    from pime_amd import protocols
    rows = np.array([[4, 0, 0, 1, 1, 1], [4, 0, 0.2, 1, 1, 1], [30, 0, 0.2, 1, 1, 1]], dtype=np.float64)
    steps, n = 10, 2                                                    # a window of 6 steps; row 2 never starts
    s = np.zeros((3, 2, 15, 5))
    s[..., P.FINITE] = n
    s[2, :, 8:, P.FINITE] = 0
    s[2, :, 8:, P.MAX], s[2, :, 8:, P.MIN] = -np.inf, np.inf
    s[:2, :, D.PEAK, P.MAX] = [[0.1, 0.3], [0.9, 0.4]]
    s[:2, :, D.RECOVERY, P.MAX] = [[0, 2], [6, 3]]
    s[:2, :, D.IAE, P.MAX] = [[0.5, 0.7], [3.0, 1.0]]
    s[:2, :, D.E0, P.MIN], s[:2, :, D.E0, P.MAX] = [[-0.02, -0.01], [-0.2, 0.0]], [[0.01, 0.03], [0.1, 0.0]]
    res = dict(rows=rows, summary=s, pairs=None, steps=steps, n=n)
    r = protocols.rejection_summary(res)
    np.testing.assert_array_equal(r["worst_peak"], [0.3, 0.9, np.nan])
    np.testing.assert_array_equal(r["worst_recovery"], [2, 6, np.nan])
    np.testing.assert_array_equal(r["worst_iae"], [0.7, 3.0, np.nan])
    np.testing.assert_array_equal(r["worst_e0"], [0.03, 0.2, np.nan])
    np.testing.assert_array_equal(r["recovered"], [1.0, 0.5, np.nan])   # (without pairs: segments whose worst plant recovered)
    pairs = np.zeros((2, 15, 3, n))
    pairs[:, 8:, 2] = np.nan
    pairs[:, D.RECOVERY, 0] = [[0, 0], [2, 1]]
    pairs[:, D.RECOVERY, 1] = [[6, 1], [3, 3]]
    r = protocols.rejection_summary(dict(res, pairs=pairs))
    np.testing.assert_array_equal(r["recovered"], [1.0, 0.75, np.nan])


def test_the_wrappers_value_errors():
    from pime_amd.vec_env import check_disturb
    good = check_disturb([[3, 0, -0.5, 1.5, 0.7, 1.0], [0, 2, 0.0, 1, 1, 0.8]], False)
    assert good.shape == (2, 6) and good.dtype == np.float64
    nan, inf = float("nan"), float("inf")
    for rows, word in (([[0.5, 0, 0, 1, 1, 1]], "onset"), ([[-1, 0, 0, 1, 1, 1]], "onset"), ([[nan, 0, 0, 1, 1, 1]], "onset"),
                       ([[0, 1.5, 0, 1, 1, 1]], "length"), ([[0, -2, 0, 1, 1, 1]], "length"), ([[0, inf, 0, 1, 1, 1]], "length"),
                       ([[0, 0, nan, 1, 1, 1]], "load"), ([[0, 0, inf, 1, 1, 1]], "load"), ([[0, 0, 0, 0, 1, 1]], "multiplier"),
                       ([[0, 0, 0, 1, -1, 1]], "multiplier"), ([[0, 0, 0, 1, 1, nan]], "multiplier"), ([[0, 0, 0, inf, 1, 1]], "multiplier"),
                       ([[0, 0, 0, 1, 1]], "rows"), ([0, 0, 0, 1, 1, 1], "rows"), (np.zeros((0, 6)), "rows")):
        with pytest.raises(ValueError, match=word):
            check_disturb(rows, False)
    with pytest.raises(ValueError, match="m2"):
        check_disturb([[0, 0, 0, 1, 1, 0.8]], True)
    assert check_disturb([[0, 0, 0, 1.2, 0.8, 1]], True).shape == (1, 6)
