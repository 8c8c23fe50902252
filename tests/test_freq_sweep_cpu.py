"""The frequency-response sweep without a GPU: the HOST build of the pair function the kernel runs (csrc/freq_sweep.hpp compiled into
libpime_freq_host.so, the prior controller alone, float64 and float32 state) against the numpy restatement and the checker of
tests/freq_sweep.py, and that checker against itself.  Shapes: 81 plants at lane offset 1000, the seven rows of tests/freq_sweep.py
(nominal, set-point, load, measurement, a load whose onset lies beyond the ragged segment, zero amplitude on a measurement row, a
set-point row from the first step), 23 steps in segments of 9, tail 4, the tank's process noise on.
  1. symbols: header, binding and libraries agree; ABI 26; pime_freq_sweep_supported(NULL, -1, 0) == 0; the package never names the
     host library;
  2. the float64 host build: bit-equal to the numpy restatement on the rows that add nothing in float32 (the measurement row through
     the checker), A = 0 rows bit-equal to libpime_disturb_host.so's nominal row for any POINT and ONSET, summary bit-equal to
     summary_from_pairs(pairs) (also at N = 130: three blocks), NULL pairs / actions / outputs change no bit of summary, a pair's rows
     do not depend on P, N or its place in the grid; the float32 host build inside the bars;
  3. how a row is read: rounding, clamping, NaN;
  4. the checker: honest synthetic recordings (with a numpy policy) use less than 0.1 of every bar, each single fault trips the
     assertion named for it;
  5. every argument error of the host build carries its message;
  6. protocols.excitation_grid, frequency_response and stability_margins on a linear loop with a closed form; the wrapper's
     ValueErrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import disturb_sweep as D
import freq_sweep as F
import margin_sweep as G
import prior_sweep as P
from conftest import ROOT

CLASSES = [(kind, sm) for kind in ("ph", "wt") for sm in ("f64", "mixed")]


@pytest.fixture(scope="module")
def cases(ph_table_oracle):
    """(cfg, keep, lanes, host recording) per class, computed once and left unchanged."""
    out = {}
    for kind, sm in CLASSES:
        cfg, keep, lanes = F.twin_case(kind, F.N, ph_table_oracle, sm)
        out[kind, sm] = (cfg, keep, lanes, F.host_freq(kind, cfg, lanes))
    return out


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pime_freq_sweep_supported", "pime_freq_sweep_workspace_bytes", "pime_freq_sweep")


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
    assert nt.lib().pime_freq_sweep_supported(None, -1, 0) == 0
    assert nt.lib().pime_freq_sweep_workspace_bytes(None, 1, 1, 0) == -1
    assert (nt.FREQ_COLS, nt.FREQ_ROWS) == (3, 8) == (F.COLS, F.FROWS)
    assert nt.FREQ_COL_NAMES == ("point", "amplitude", "onset")
    assert nt.FREQ_ROW_NAMES == ("yc", "ys", "uc", "us", "y0", "u0", "y2", "u2")
    assert nt.FREQ_POINTS == {"setpoint": F.SETPOINT, "load": F.LOAD, "measurement": F.MEASUREMENT}
    header = open(os.path.join(ROOT, "include", "pime_hip.h")).read()
    for names in (nt.FREQ_COL_NAMES, nt.FREQ_ROW_NAMES):
        for j, name in enumerate(names):
            assert f"PIME_FREQ_{name.upper()} = {j}" in header, name
    for name, j in nt.FREQ_POINTS.items():
        assert f"PIME_FREQ_{name.upper()} = {j}" in header, name
    assert "PIME_FREQ_COLS = 3" in header and "PIME_FREQ_ROWS = 8" in header
    host = C.CDLL(F.HOST_LIB_PATH)
    assert _declared("pime_freq_host.h") == set(F.HOST_EXPORTS)
    for name in F.HOST_EXPORTS:
        assert hasattr(host, name), name
    for name in NEW_SYMBOLS:     # the host library is no second door to the product's entry points
        assert not hasattr(host, name), name


def test_the_package_never_names_the_host_library():
    for d, _, files in os.walk(P.PKG):
        for f in files:
            if f.endswith(".py"):
                assert "freq_host" not in open(os.path.join(d, f)).read(), os.path.join(d, f)


# ---- 2. the host build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_host_equals_numpy(cases, ph_table_oracle, kind):
    cfg, _, lanes, rec = cases[kind, "f64"]
    assert not any((rec[k] == -777.0).any() for k in rec), "every word is written"
    ref = F.numpy_loop(kind, cfg, lanes, ph_table_oracle)
    exact = [p for p in range(len(F.EXCITE)) if not (F.EXCITE[p, 0] == F.MEASUREMENT and F.EXCITE[p, 1] != 0.0)]
    assert exact == [0, 1, 2, 4, 5, 6]
    for k in ("actions", "outputs", "pairs"):
        assert F.bits_equal(rec[k][..., exact, :], ref[k][..., exact, :]), k
    # what the rows are about
    pairs, act, out = rec["pairs"], rec["actions"], rec["outputs"]
    assert F.bits_equal(pairs[:, :8, 0], pairs[:, :8, 5]) and F.bits_equal(act[:, 0], act[:, 5]), "zero amplitude: any point, any onset"
    assert np.isnan(pairs[2, 8:, 4]).all() and np.isnan(pairs[2, 8:, 5]).all(), "onset beyond the ragged segment (5 steps)"
    assert np.isfinite(pairs[:2, 8:]).all() and np.isfinite(pairs[:, 8:, [0, 1, 2, 3, 6]]).all()
    assert (out[1, 2] != out[1, 0]).any(), "the excitation runs from the segment's first step, not from the onset"
    assert not F.bits_equal(act[1, 1], act[1, 0]) and not F.bits_equal(act[1, 3], act[1, 0])
    assert F.bits_equal(act[0, 6], act[0, 0]), "s_0 = 0 with the onset at 0"
    # a constant table turns Y0 and U0 into YC and UC
    ones = np.ones_like(F.WAVE)
    flat = F.host_freq(kind, cfg, lanes, wave=ones)
    assert F.bits_equal(flat["pairs"][:, F.YC, 0], flat["pairs"][:, F.Y0, 0]) and F.bits_equal(flat["pairs"][:, F.US, 0], flat["pairs"][:, F.U0, 0])


@pytest.mark.parametrize("kind,sm", CLASSES, ids=lambda v: str(v))
def test_host_build_passes_the_checker(cases, ph_table_oracle, kind, sm):
    cfg, _, lanes, rec = cases[kind, sm]
    use = F.check_recording(kind, cfg, lanes, ph_table_oracle, rec, tag=f"{kind}-{sm}")
    print(f"\nFREQ host id={kind}-{sm} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} action "
          f"{use['action']:.3g} (gap {use['gap']:.4g})")
    P.check_summary(rec["summary"], rec["pairs"], tag=f"{kind}-{sm}")
    assert (rec["summary"][4, 2, 8:, P.FINITE] == 0).all() and (rec["summary"][4, 2, :8, P.FINITE] == F.N).all(), "NaN rows are not counted"
    if sm == "f64":
        assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use


@pytest.mark.parametrize("kind,sm", CLASSES, ids=lambda v: str(v))
def test_zero_amplitude_rows_are_the_disturbance_sweeps_nominal_row(cases, ph_table_oracle, kind, sm):
    cfg, _, lanes, rec = cases[kind, sm]
    dcfg, dkeep, dlanes = D.twin_case(kind, F.N, ph_table_oracle, sm)
    want = D.host_disturb(kind, dcfg, dlanes, rows=np.array([[0, 0, 0, 1, 1, 1]], dtype=np.float64))
    rows = np.array([(0, 0.0, 3), (1, 0.0, 0), (2, 0.0, 7), (2, -0.0, 50), (1, 0.0, float("nan"))])
    got = F.host_freq(kind, cfg, lanes, rows=rows, wave=F.sinusoids((1, 2, 1, 3, 1), (3, 0, 7, 3, 0), F.SEG))
    for p in range(len(rows)):
        assert F.bits_equal(got["pairs"][:, :8, p], want["pairs"][:, :8, 0]), p
        assert F.bits_equal(got["actions"][:, p], want["actions"][:, 0]) and F.bits_equal(got["outputs"][:, p], want["outputs"][:, 0]), p
    assert F.bits_equal(rec["pairs"][:, :8, 0], want["pairs"][:, :8, 0])


def test_three_summary_blocks_null_outputs_and_independence(cases, ph_table_oracle):
    cfg, keep, lanes = F.twin_case("wt", 130, ph_table_oracle)
    rec = F.host_freq("wt", cfg, lanes)
    P.check_summary(rec["summary"], rec["pairs"], tag="N = 130")
    counted = rec["summary"][..., P.FINITE]
    assert ((counted == 130) | (counted == 0)).all() and (counted[:, :, :8] == 130).all() and rec["summary"].shape == (7, 3, 16, 5)
    quiet = F.host_freq("wt", cfg, lanes, trace=False, want_pairs=False)
    assert quiet["pairs"] is None and F.bits_equal(quiet["summary"], rec["summary"]), "NULL pairs / actions / outputs must not change a bit"
    # a pair's rows do not depend on P or its place in the grid ...
    one = F.host_freq("wt", cfg, lanes, rows=F.EXCITE[3:4], wave=F.WAVE[3:4])
    assert F.bits_equal(one["pairs"][:, :, 0], rec["pairs"][:, :, 3]) and F.bits_equal(one["summary"][0], rec["summary"][3])
    back = F.host_freq("wt", cfg, lanes, rows=F.EXCITE[::-1], wave=F.WAVE[::-1])
    assert F.bits_equal(back["pairs"][:, :, ::-1], rec["pairs"]) and F.bits_equal(back["outputs"][:, ::-1], rec["outputs"])
    # ... nor on N: the first 40 of the 130 plants alone (the same lane state, the same global lanes)
    few = F.host_freq("wt", cfg, {k: np.ascontiguousarray(v[:40]) for k, v in lanes.items()})
    assert F.bits_equal(rec["pairs"][..., :40], few["pairs"]) and F.bits_equal(rec["actions"][..., :40], few["actions"])


# ---- 3. how a row is read -----------------------------------------------------------------------------------------------------------
def test_point_and_onset_are_rounded_and_clamped(cases):
    cfg, _, lanes, rec = cases["wt", "f64"]
    nan = float("nan")
    odd = np.array([[0.4, 0.5, 4.4], [nan, 0.5, 3.6], [-3.0, 0.5, 4.0], [1.4, 0.3, 3.0], [7.0, 0.2, 3.0], [1.0, -0.25, nan], [1.0, -0.25, 1e12]])
    wave = F.WAVE[[1, 1, 1, 2, 3, 4, 4]]
    got = F.host_freq("wt", cfg, lanes, rows=odd, wave=wave)
    for p, q in ((0, 1), (1, 1), (2, 1), (3, 2), (4, 3)):
        assert F.bits_equal(got["pairs"][:, :, p], rec["pairs"][:, :, q]), (p, q)
    for p in (5, 6):                                                      # never: the excitation runs, no window anywhere
        assert F.bits_equal(got["actions"][:, p], rec["actions"][:, 4]) and np.isnan(got["pairs"][:, 8:, p]).all(), p


# ---- 4. the checker --------------------------------------------------------------------------------------------------------------
# fault -> (kind, the assertion it trips, the prior gain's scale)
FAULT_CASES = {
    "window_early": ("wt", "lockin", 1.0), "window_late": ("ph", "lockin", 1.0), "table_by_launch_step": ("wt", "lockin", 1.0),
    "neighbour_table": ("wt", "lockin", 1.0), "cs_swapped": ("ph", "lockin", 1.0), "amplitude_on_reference": ("wt", "metrics", 1.0),
    "load_behind_clip": ("ph", "trajectory", 40.0), "setpoint_not_integrated": ("ph", "action", 1.0), "measure_h1": ("wt", "action", 1.0),
    "measure_into_integrator": ("ph", "action", 1.0), "a_env_recorded": ("wt", "action", 1.0), "finite_for_nan": ("wt", "nan", 1.0),
}
# the same faults seen on one excited row alone: where the excitation itself went wrong the replay says so
FAULT_ROWS = {"table_by_launch_step": (2, "trajectory"), "cs_swapped": (2, "trajectory"), "neighbour_table": (2, "trajectory")}


def test_every_fault_is_listed():
    assert sorted(FAULT_CASES) == sorted(F.FAULTS) and len(F.FAULTS) == 12


@pytest.fixture(scope="module")
def honest(cases, ph_table_oracle):
    out = {}
    for kind in ("ph", "wt"):
        cfg, _, lanes, _ = cases[kind, "f64"]
        pol = G.NumpyPolicy(len(F.PRIOR_K[kind]))
        out[kind] = (pol, F.numpy_loop(kind, cfg, lanes, ph_table_oracle, policy=pol))
    return out


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_honest_recordings_pass_far_inside(cases, honest, ph_table_oracle, kind):
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, rec = honest[kind]
    use = F.check_recording(kind, cfg, lanes, ph_table_oracle, rec, policy=pol.term)
    assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use
    assert F.bits_equal(rec["pairs"][:, :8, 0], rec["pairs"][:, :8, 5])


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_each_fault_trips_the_assertion_named_for_it(cases, honest, ph_table_oracle, fault):
    kind, name, scale = FAULT_CASES[fault]
    cfg, _, lanes, _ = cases[kind, "f64"]
    pol, _ = honest[kind]
    K = scale * F.PRIOR_K[kind]
    if scale != 1.0:     # the honest recording at this gain passes: the fault alone trips
        F.check_recording(kind, cfg, lanes, ph_table_oracle, F.numpy_loop(kind, cfg, lanes, ph_table_oracle, K=K, policy=pol), K=K, policy=pol.term)
    forged = F.numpy_loop(kind, cfg, lanes, ph_table_oracle, K=K, policy=pol, fault=fault)
    with pytest.raises(AssertionError) as caught:
        F.check_recording(kind, cfg, lanes, ph_table_oracle, forged, K=K, policy=pol.term)
    assert f"[{name}]" in str(caught.value), str(caught.value)
    if fault in FAULT_ROWS:
        row, name = FAULT_ROWS[fault]
        with pytest.raises(AssertionError) as caught:
            F.check_recording(kind, cfg, lanes, ph_table_oracle, forged, K=K, policy=pol.term, only=[row])
        assert f"[{name}]" in str(caught.value), str(caught.value)


def test_a_zero_amplitude_row_that_differs_trips_the_nominal_assertion(cases, ph_table_oracle):
    cfg, _, lanes, rec = cases["wt", "f64"]
    moved = dict(rec, outputs=rec["outputs"].copy())
    moved["outputs"][1, 0, 7] = np.nextafter(rec["outputs"][1, 0, 7], 1.0)                            # the nominal row moved by an ulp
    with pytest.raises(AssertionError) as caught:
        F.check_recording("wt", cfg, lanes, ph_table_oracle, moved, only=[5])
    assert "[nominal]" in str(caught.value), str(caught.value)


def test_a_forged_row_trips_its_assertion(cases, ph_table_oracle):
    cfg, _, lanes, rec = cases["wt", "f64"]
    for row, name in ((2, "metrics"), (6, "metrics"), (F.YS, "lockin"), (F.U2, "lockin")):
        forged = dict(rec, pairs=rec["pairs"].copy())
        forged["pairs"][1, row, 3, 5] *= 1.001
        with pytest.raises(AssertionError) as caught:
            F.check_recording("wt", cfg, lanes, ph_table_oracle, forged)
        assert f"[{name}]" in str(caught.value)


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------
def test_host_argument_errors(ph_table_oracle):
    import pime_amd.native as nt
    bad = []
    for kind in ("wt", "ph"):
        cfg, keep, lanes = F.twin_case(kind, 8, ph_table_oracle)
        sp = np.ascontiguousarray(F.SETPOINTS[kind], dtype=np.float64)
        K = np.ascontiguousarray(F.PRIOR_K[kind])
        ex, wave = np.ascontiguousarray(F.EXCITE), np.ascontiguousarray(F.WAVE)
        base = dict(lanes=lanes, N=8, K=K, ex=ex, wave=wave, wl=F.SEG, P=7, n_steps=F.N_STEPS, seg_len=F.SEG, sp=sp, n_sp=3, band=F.BAND,
                    tail=4, summary=True, sm=nt.STATE_F64, stack=0)
        todo = [("P = 0", dict(P=0)), ("excite is NULL", dict(ex=None)), ("summary is NULL", dict(summary=False)), ("priorK is NULL", dict(K=None)),
                ("wave is NULL", dict(wave=None)), ("wave_len 8", dict(wl=8)), ("wave_len 23", dict(wl=F.N_STEPS)), ("wave_len 9", dict(seg_len=0, sp=None, n_sp=0)),
                ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)),
                ("n_setpoints 17", dict(n_sp=17)), ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)),
                ("set-point schedule", dict(seg_len=-1)), ("NULL lanes", dict(lanes=None)), ("N = 0", dict(N=0)),
                ("lane array", dict(lanes={k: v for k, v in lanes.items() if k != "r"})), ("state_mode", dict(sm=nt.STATE_MIXED16))]
        if kind == "wt":
            todo.append(("Stacking", dict(stack=1)))
        for word, over in todo:
            kw = dict(base, **over)
            cfg.state_mode, cfg.num_stack = kw["sm"], kw["stack"]
            summary = np.full((7, 3, 16, 5), -777.0)
            rc, msg = F.host_raw(kind, cfg, kw["lanes"], kw["N"], kw["K"], kw["ex"], kw["wave"], kw["wl"], kw["P"], kw["n_steps"], kw["seg_len"],
                                 kw["sp"], kw["n_sp"], kw["band"], kw["tail"], None, summary if kw["summary"] else None, None, None)
            if rc != -1 or word not in msg or not (summary == -777.0).all():
                bad.append((kind, word, rc, msg))
        cfg.state_mode, cfg.num_stack = nt.STATE_F64, 0
    assert not bad, bad


# ---- 6. protocols and the wrapper --------------------------------------------------------------------------------------------------
def test_excitation_grid():
    from pime_amd import protocols
    rows, wave = protocols.excitation_grid([1, 4, 8], [0.5, 0.25, 0.1], ["setpoint", 1, "measurement"], 24, 8)
    assert rows.shape == (3, 3) and wave.shape == (3, 24, 2) and rows.dtype == wave.dtype == np.float64
    assert rows.flags["C_CONTIGUOUS"] and wave.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(rows, [[0, 0.5, 8], [1, 0.25, 8], [2, 0.1, 8]])
    assert F.bits_equal(wave, F.sinusoids((1, 4, 8), (8, 8, 8), 24))
    w = wave[:, 8:]
    for p in range(3):      # an integer number of cycles: c and s are orthogonal over the window and to a constant
        assert abs((w[p, :, 0] * w[p, :, 1]).sum()) < 1e-12 and abs(w[p, :, 0].sum()) < 1e-12 and abs(w[p, :, 1].sum()) < 1e-12
    assert np.abs(w[2, :, 1]).max() < 1e-14, "the Nyquist rate: s vanishes"
    rows, wave = protocols.excitation_grid(2, 0.0, "load", 10, [0, 2, 4])     # scalars serve every row
    np.testing.assert_array_equal(rows, [[1, 0, 0], [1, 0, 2], [1, 0, 4]])
    assert F.bits_equal(wave, F.sinusoids((2, 2, 2), (0, 2, 4), 10))
    nan, inf = float("nan"), float("inf")
    for args, word in ((([1], 0.1, 3, 24, 8), "point"), (([1], 0.1, "output", 24, 8), "point"), (([1], nan, 0, 24, 8), "finite"),
                       (([1], 0.1, 0, 24, 24), "onset"), (([1], 0.1, 0, 24, -1), "onset"), (([1], 0.1, 0, 24, 1.5), "onset"),
                       (([9], 0.1, 0, 24, 8), "cycles"), (([1.5], 0.1, 0, 24, 8), "cycles"), (([-1], 0.1, 0, 24, 8), "cycles"),
                       (([inf], 0.1, 0, 24, 8), "finite")):
        with pytest.raises(ValueError, match=word):
            protocols.excitation_grid(*args)


# A linear loop with a closed form: y_k = a y_{k-1} + b u_k under u_k = Kp (r_k - y_{k-1}).  With z = e^{j omega}:
#   G = b / (1 - a / z) from u to y, the loop transfer function L = Kp G / z (the controller reads the output of the step before),
#   T = Kp G / (1 + L), S = 1 / (1 + L), and y = -T n for n added to what the controller reads.
# The closed-loop pole is p = a - Kp b = 0.2; the loop starts |r - y| = 1 away from its fixed point and the window opens at k0 = 32:
# |p|^32 = 4.3e-23 < 1e-12, so the window holds the periodic state to rounding.
LIN_A, LIN_B, LIN_KP = 0.8, 0.5, 1.2
LIN_L, LIN_K0 = 96, 32
LIN_W = LIN_L - LIN_K0
LIN_M = np.arange(1, LIN_W // 2)                    # 1 .. 31 cycles: omega = 2 pi m / 64
assert abs(LIN_A - LIN_KP * LIN_B) ** LIN_K0 * 1.0 < 1e-12


def _lin_curves(omega, delay=1):
    z = np.exp(1j * np.asarray(omega, dtype=np.float64))
    Gz = LIN_B / (1.0 - LIN_A / z)
    L = LIN_KP * Gz / z ** delay
    return L, LIN_KP * Gz / (1.0 + L), 1.0 / (1.0 + L)


def _lin_simulate(point, A, wave):
    y, r0 = 0.0, 1.0
    ys, us = np.zeros((LIN_L, 1)), np.zeros((LIN_L, 1))
    for k in range(LIN_L):
        e = A * wave[k, 1]
        r = r0 + e if point == F.SETPOINT else r0
        u = LIN_KP * (r - (y + e if point == F.MEASUREMENT else y))
        y = LIN_A * y + LIN_B * (u + e if point == F.LOAD else u)
        ys[k], us[k] = y, u
    return us, ys


@pytest.fixture(scope="module")
def linear_response():
    from pime_amd import protocols
    m = np.concatenate([LIN_M, LIN_M, LIN_M])
    point = np.repeat([F.SETPOINT, F.LOAD, F.MEASUREMENT], len(LIN_M))
    rows, wave = protocols.excitation_grid(m, 0.1, point, LIN_L, LIN_K0)
    pairs = np.zeros((1, F.ROWS, len(rows), 1))
    for p in range(len(rows)):
        us, ys = _lin_simulate(int(point[p]), 0.1, wave[p])
        pairs[:, 8:, p] = F.lockin_rows(us, ys, wave[p], LIN_K0)
    return protocols.frequency_response(dict(rows=rows, wave=wave, pairs=pairs, n_steps=LIN_L)), point


def test_frequency_response_matches_the_closed_form(linear_response):
    fr, point = linear_response
    omega = 2.0 * np.pi * LIN_M / LIN_W
    np.testing.assert_allclose(fr["omega"], np.tile(omega, 3), rtol=1e-12)
    L, T, S = _lin_curves(omega)
    sp, ld, ms = (np.flatnonzero(point == v) for v in (F.SETPOINT, F.LOAD, F.MEASUREMENT))
    for name, idx, want in (("T", sp, T), ("L", ld, L), ("S", ld, S), ("N", ms, -T)):
        got = fr[name][idx, 0, 0]
        assert np.abs(got - want).max() <= 1e-9, (name, np.abs(got - want).max())
        other = np.setdiff1d(np.arange(len(point)), idx)
        assert np.isnan(fr[name][other]).all(), name
    np.testing.assert_allclose(fr["E"][:, 0], 0.1, atol=1e-12)
    np.testing.assert_allclose(fr["Y"][sp, 0, 0], 0.1 * T, atol=1e-10)
    np.testing.assert_allclose(fr["share"][:, 0, 0], 1.0, atol=1e-9)     # a linear loop answers at the fundamental alone


def test_the_share_falls_with_a_harmonic_and_quiet_rows_hold_nan():
    from pime_amd import protocols
    rows, wave = protocols.excitation_grid([2, 32, 2], [0.1, 0.1, 0.0], 1, LIN_L, LIN_K0)
    th = 2.0 * np.pi * 2 * (np.arange(LIN_L) - LIN_K0) / LIN_W
    y = (3.0 + np.sin(th) + 0.5 * np.sin(3 * th))[:, None]               # a third harmonic of half the amplitude: 1 / 1.25 of the variance
    pairs = np.zeros((1, F.ROWS, 3, 1))
    for p in range(3):
        pairs[:, 8:, p] = F.lockin_rows(np.zeros_like(y), y, wave[p], LIN_K0)
    fr = protocols.frequency_response(dict(rows=rows, wave=wave, pairs=pairs))
    assert abs(fr["share"][0, 0, 0] - 0.8) < 1e-12 and abs(fr["Y"][0, 0, 0] - 1.0) < 1e-12
    assert np.isnan(fr["L"][1:]).all() and np.isnan(fr["S"][1:]).all(), "the Nyquist rate and a zero amplitude excite nothing"
    assert abs(fr["omega"][1] - np.pi) < 1e-12
    pairs[:, 8:, 0] = np.nan                                             # a segment that never reaches the onset
    assert np.isnan(protocols.frequency_response(dict(rows=rows, wave=wave, pairs=pairs))["L"][0]).all()


def _crossing(w, f, level, v):
    """The test's own interpolation: f first falls through `level` between two grid points, linearly in log w: (w there, v there)."""
    for i in range(len(w) - 1):
        if f[i] > level >= f[i + 1]:
            x = (level - f[i]) / (f[i + 1] - f[i])
            return np.exp(np.log(w[i]) + x * np.log(w[i + 1] / w[i])), v[i] + x * (v[i + 1] - v[i])
    return np.nan, np.nan


def _bisect(f, lo, hi):
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if (f(lo) > 0) == (f(mid) > 0) else (lo, mid)
    return 0.5 * (lo + hi)


def test_stability_margins_match_the_analytic_crossings(linear_response):
    from pime_amd import protocols
    fr, _ = linear_response
    got = {k: v[0, 0] for k, v in protocols.stability_margins(fr).items()}
    omega = 2.0 * np.pi * LIN_M / LIN_W
    L, T, S = _lin_curves(omega)
    # phase margin: the true gain crossover, and what linear interpolation in log omega makes of the ANALYTIC curve on this grid
    w_gc = _bisect(lambda w: abs(_lin_curves(w)[0]) - 1.0, omega[0], omega[-1])
    pm_true = 180.0 + np.degrees(np.angle(_lin_curves(w_gc)[0]))
    pm_grid = 180.0 + np.degrees(_crossing(omega, np.log(np.abs(L)), 0.0, np.unwrap(np.angle(L)))[1])
    assert abs(got["phase_margin"] - pm_grid) <= 1e-6 and abs(got["phase_margin"] - pm_true) <= abs(pm_grid - pm_true) + 1e-6
    assert 60.0 < pm_true < 120.0 and abs(pm_grid - pm_true) < 0.5
    # bandwidth of |T|
    w_bw = _bisect(lambda w: abs(_lin_curves(w)[1]) - np.sqrt(0.5), omega[0], omega[-1])
    bw_grid = _crossing(omega, np.abs(T), np.sqrt(0.5), np.abs(T))[0]
    assert abs(got["bandwidth"] - bw_grid) <= 1e-9 and abs(got["bandwidth"] - w_bw) <= abs(bw_grid - w_bw) + 1e-9
    assert abs(bw_grid - w_bw) < 0.01 * w_bw
    # |S| rises to 1.5 at the Nyquist rate, where nothing can be excited: the grid's last row is its maximum
    assert abs(got["peak_S"] - np.abs(S[-1])) <= 1e-9 and abs(got["peak_S"] - 1.5) <= abs(np.abs(S[-1]) - 1.5) + 1e-9
    # the phase of this loop reaches -180 degrees only AT the Nyquist rate: no row brackets a crossing
    assert np.isnan(got["gain_margin"])


def test_gain_margin_and_interior_peak_on_an_analytic_curve():
    """The same loop with one more sample of dead time has a phase crossover and a sensitivity peak inside the grid; stability_margins is
    fed the analytic L itself."""
    from pime_amd import protocols
    omega = 2.0 * np.pi * LIN_M / LIN_W
    L = _lin_curves(omega, delay=2)[0]
    fr = dict(omega=omega, point=np.full(len(omega), F.LOAD), L=L[:, None, None], T=np.full((len(omega), 1, 1), np.nan + 0j))
    got = {k: v[0, 0] for k, v in protocols.stability_margins(fr).items()}
    w_pc = _bisect(lambda w: np.angle(_lin_curves(w, 2)[0] * np.exp(1j * np.pi)), 0.5, 2.5)     # arg L = -180 degrees
    gm_true = 1.0 / abs(_lin_curves(w_pc, 2)[0])
    ph = np.unwrap(np.angle(L))
    gm_grid = np.exp(-_crossing(omega, ph, -np.pi, np.log(np.abs(L)))[1])
    assert abs(got["gain_margin"] - gm_grid) <= 1e-9 and abs(got["gain_margin"] - gm_true) <= abs(gm_grid - gm_true) + 1e-9
    assert 1.0 < gm_true < 10.0 and abs(gm_grid - gm_true) < 0.01 * gm_true
    dense = np.linspace(omega[0], omega[-1], 200001)
    peak_true = np.abs(1.0 / (1.0 + _lin_curves(dense, 2)[0])).max()
    grid_max = np.abs(1.0 / (1.0 + L)).max()
    assert grid_max <= got["peak_S"] + 1e-12 and abs(got["peak_S"] - peak_true) <= abs(grid_max - peak_true) + 1e-9
    assert np.isnan(got["bandwidth"])


def test_the_wrappers_value_errors():
    from pime_amd.vec_env import check_excite
    rows, wave = check_excite(F.EXCITE, F.WAVE, F.SEG)
    assert rows.shape == (7, 3) and wave.shape == (7, 9, 2) and rows.dtype == wave.dtype == np.float64
    nan, inf = float("nan"), float("inf")
    w1 = F.WAVE[:1]
    for r, w, word in (([[3, 0.1, 0]], w1, "point"), ([[0.5, 0.1, 0]], w1, "point"), ([[nan, 0.1, 0]], w1, "point"), ([[0, nan, 0]], w1, "amplitude"),
                       ([[0, inf, 0]], w1, "amplitude"), ([[0, 0.1, 0.5]], w1, "onset"), ([[0, 0.1, -1]], w1, "onset"), ([[0, 0.1, nan]], w1, "onset"),
                       ([[0, 0.1]], w1, "rows"), ([0, 0.1, 0], w1, "rows"), (np.zeros((0, 3)), w1, "rows"), ([[0, 0.1, 0]], F.WAVE[:2], "wave"),
                       ([[0, 0.1, 0]], w1[:, :8], "wave"), ([[0, 0.1, 0]], np.full_like(w1, nan), "wave entry")):
        with pytest.raises(ValueError, match=word):
            check_excite(r, w, F.SEG)
