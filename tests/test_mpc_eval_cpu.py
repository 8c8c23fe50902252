"""The receding-horizon benchmark controller without a GPU: the HOST build of the closed loop the kernel runs (csrc/mpc_eval.hpp
compiled into libpime_mpc_host.so, float64 and float32 state) against the checker of tests/mpc_eval.py, and that checker against
itself.  Shapes: 70 plants at a lane offset, 24 steps in segments of 10 (the last one ragged), horizon 5, 2 passes, the tank's
n_discrete as registered and its process noise on.
  1. the four classes (pH / tank x float64 / float32 state) pass the checker and use at most 0.1 of every bar; the largest relative
     optimality gap of the float32 build is the measured value OPT_BAR is ten times of (profiles/mpc_eval_bars.txt);
  2. the float64 host build equals the numpy restatement's choice at every step of every plant (the applied actions, the winners'
     costs of every pass and the metrics bit for bit), on inputs whose runner-up costs differ by more than 1e-9 relative -- verified;
  3. the chosen cost never rises from pass to pass; a third pass and a penalty rho change the actions;
  4. model_plants equal to the plants' own gives the bits of NULL, a mismatched model changes the actions, NULL actions / outputs
     leave metrics bit-identical;
  5. every argument error carries its message and leaves metrics untouched;
  6. the checker: each of the ten single faults trips a named assertion;
  7. symbols: header, binding and libraries agree; ABI 26; the package never names the host library; protocols.regret."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mpc_eval as M
import prior_sweep as P
from conftest import ROOT

CLASSES = [(kind, sm) for kind in ("ph", "wt") for sm in ("f64", "mixed")]


@pytest.fixture(scope="module")
def cases(ph_table_oracle):
    """(cfg, keep, lanes, host recording) per class, computed once and left unchanged."""
    out = {}
    for kind, sm in CLASSES:
        cfg, keep, lanes = M.twin_case(kind, M.N, ph_table_oracle, sm)
        out[kind, sm] = (cfg, keep, lanes, M.host_mpc(kind, cfg, lanes))
    return out


# ---- 1. the four classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sm", CLASSES, ids=lambda v: str(v))
def test_host_build_passes_the_checker(cases, ph_table_oracle, kind, sm):
    cfg, _, lanes, rec = cases[kind, sm]
    assert not any((rec[k] == -777.0).any() for k in rec), "every word is written"
    use = M.check_recording(kind, cfg, lanes, ph_table_oracle, rec, tag=f"{kind}-{sm}")
    print(f"\nMPC host id={kind}-{sm} share of the bars: trajectory {use['trajectory']:.3g} return {use['ret']:.3g} optimal {use['optimal']:.3g} "
          f"(gap {use['gap']:.4g})")
    assert max(use["trajectory"], use["ret"], use["optimal"]) <= 0.1, use
    if sm == "f64":
        assert use["gap"] == 0.0 and use["trajectory"] == 0.0


def test_the_measured_bar(cases, ph_table_oracle):
    """OPT_BAR = 10 x the largest gap of the float32 host build against the float64 restatement on these shapes."""
    worst = 0.0
    for kind in ("ph", "wt"):
        cfg, _, lanes, rec = cases[kind, "mixed"]
        gap = M.optimality_gaps(kind, cfg, lanes, ph_table_oracle, rec["actions"], M.HORIZON, M.PASSES, 0.0, M.N_STEPS, M.SEG, None)[4]
        print(f"\nMPC bar id={kind}-mixed largest relative gap {gap.max():.6g}")
        worst = max(worst, float(gap.max()))
    assert 0.0 < worst <= M.OPT_MEASURED and M.OPT_BAR == 10 * M.OPT_MEASURED, (worst, M.OPT_MEASURED)
    text = open(os.path.join(ROOT, "profiles", "mpc_eval_bars.txt")).read()
    assert f"{M.OPT_MEASURED:.4e}" in text and f"{M.OPT_BAR:.4e}" in text


# ---- 2. the numpy restatement's choice -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_float64_host_equals_the_numpy_choice_at_every_step(cases, ph_table_oracle, kind, rho):
    cfg, _, lanes, rec = cases[kind, "f64"]
    if rho:
        rec = M.host_mpc(kind, cfg, lanes, rho=rho)
    ref = M.numpy_mpc(kind, cfg, lanes, ph_table_oracle, rho=rho)
    assert ref["margin"].min() > 1e-9, f"a runner-up is within 1e-9 relative: pick other inputs ({ref['margin'].min():.3g})"
    assert M.bits_equal(rec["actions"], ref["actions"]), np.argwhere(rec["actions"] != ref["actions"])[:4]
    assert M.bits_equal(rec["pass_costs"], ref["pass_costs"])
    # (the same action from the same grid is the same index: a clipped duplicate of the winner never has the smaller index at -1,
    #  and at +1 both sides take the smaller one)
    assert M.bits_equal(rec["metrics"], ref["metrics"]) and M.bits_equal(rec["outputs"], ref["outputs"])


# ---- 3. passes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sm", CLASSES, ids=lambda v: str(v))
def test_the_chosen_cost_never_rises_from_pass_to_pass(cases, kind, sm):
    cfg, _, lanes, rec2 = cases[kind, sm]
    rec = M.host_mpc(kind, cfg, lanes, passes=3)
    pc = rec["pass_costs"]
    assert pc.shape == (M.N_STEPS, 3, M.N) and (pc[:, 1] <= pc[:, 0]).all() and (pc[:, 2] <= pc[:, 1]).all()
    assert (pc[:, 1] < pc[:, 0]).any()
    assert M.bits_equal(rec["pass_costs"][0, :2], rec2["pass_costs"][0]), "the first step's first two passes are those of a two-pass run"
    assert not M.bits_equal(M.host_mpc(kind, cfg, lanes, rho=0.5)["actions"], rec2["actions"]), "rho changes the actions"
    one = M.host_mpc(kind, cfg, lanes, passes=1)
    assert np.isin(one["actions"], M.grid0()).all() and not np.isin(rec2["actions"], M.grid0()).all()


# ---- 4. the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", ["f64", "mixed"])
def test_model_plants(cases, ph_table_oracle, sm):
    cfg, _, lanes, rec = cases["wt", sm]
    own = np.column_stack([lanes["a1"], lanes["a2"], lanes["Kp"]])
    same = M.host_mpc("wt", cfg, lanes, model=own)
    assert all(M.bits_equal(same[k], rec[k]) for k in rec), "the plants' own rows as the model give the bits of model_plants = NULL"
    one = np.broadcast_to(own[0], own.shape).copy()
    other = M.host_mpc("wt", cfg, lanes, model=one)
    assert not M.bits_equal(other["actions"], rec["actions"]) and M.bits_equal(other["actions"][:, 0], rec["actions"][:, 0])
    M.check_recording("wt", cfg, lanes, ph_table_oracle, other, model=one, tag=f"wt-{sm} broadcast model")
    quiet = M.host_mpc("wt", cfg, lanes, trace=False)
    assert quiet["actions"] is None and M.bits_equal(quiet["metrics"], rec["metrics"]), "NULL actions / outputs must not change a bit"


def test_null_traces_ph(cases):
    cfg, _, lanes, rec = cases["ph", "mixed"]
    assert M.bits_equal(M.host_mpc("ph", cfg, lanes, trace=False)["metrics"], rec["metrics"])


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------
def test_host_argument_errors(ph_table_oracle):
    import pime_amd.native as nt
    bad = []
    for kind in ("wt", "ph"):
        cfg, keep, lanes = M.twin_case(kind, 8, ph_table_oracle)
        sp = np.ascontiguousarray(M.SETPOINTS[kind], dtype=np.float64)
        model = np.zeros((8, 3))
        base = dict(lanes=lanes, N=8, model=None, H=5, passes=2, rho=0.0, n_steps=M.N_STEPS, seg_len=10, sp=sp, n_sp=3, band=M.BAND, tail=4,
                    metrics=True, sm=nt.STATE_F64, stack=0)
        cases = [("horizon 0", dict(H=0)), ("horizon 65", dict(H=65)), ("passes 0", dict(passes=0)), ("passes 4", dict(passes=4)),
                 ("rho", dict(rho=-1.0)), ("rho", dict(rho=float("nan"))), ("rho", dict(rho=float("inf"))), ("metrics is NULL", dict(metrics=False)),
                 ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)),
                 ("n_setpoints 17", dict(n_sp=17)), ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)),
                 ("set-point schedule", dict(seg_len=-1)), ("NULL lanes", dict(lanes=None)), ("N = 0", dict(N=0)),
                 ("lane array", dict(lanes={k: v for k, v in lanes.items() if k != "r"})), ("state_mode", dict(sm=nt.STATE_MIXED16))]
        cases.append(("model_plants on a pH handle", dict(model=model)) if kind == "ph" else ("Stacking", dict(stack=1)))
        for word, over in cases:
            kw = dict(base, **over)
            cfg.state_mode, cfg.num_stack = kw["sm"], kw["stack"]
            metrics = np.full((3, 8, 8), -777.0)
            rc, msg = M.host_raw(kind, cfg, kw["lanes"], kw["N"], kw["model"], kw["H"], kw["passes"], kw["rho"], kw["n_steps"], kw["seg_len"],
                                 kw["sp"], kw["n_sp"], kw["band"], kw["tail"], metrics if kw["metrics"] else None, None, None)
            if rc != -1 or word not in msg or not (metrics == -777.0).all():
                bad.append((kind, word, rc, msg))
        cfg.state_mode, cfg.num_stack = nt.STATE_F64, 0
        metrics = np.full((3, 8, 8), -777.0)
        rc, msg = M.host_raw(kind, cfg, lanes, 8, None, 64, 3, 0.0, M.N_STEPS, 10, sp, 3, M.BAND, 4, metrics, None, None)
        assert rc == 0 and not (metrics == -777.0).any(), msg      # and the good call at the limits goes through
    assert not bad, bad


# ---- 6. the checker --------------------------------------------------------------------------------------------------------------
# fault -> (kind, keyword arguments of the run, the assertion it trips)
FAULT_CASES = {
    "horizon_short": ("wt", {}, "optimal"), "rho_ignored": ("wt", dict(rho=0.5), "optimal"), "u_prev_stale": ("ph", dict(rho=0.5), "optimal"),
    "model_noise": ("wt", {}, "optimal"), "prior_added": ("wt", {}, "trajectory"), "setpoint_stale": ("ph", {}, "optimal"),
    "refine_from_zero": ("wt", {}, "optimal"), "tie_larger": ("ph", dict(passes=3), "tie"), "unclipped": ("wt", {}, "grid"),
    "model_neighbour": ("wt", dict(model=True), "optimal"),
}


def test_every_fault_is_listed():
    assert sorted(FAULT_CASES) == sorted(M.FAULTS) and len(M.FAULTS) == 10


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_each_fault_trips_a_named_assertion(cases, ph_table_oracle, fault):
    kind, kw, name = FAULT_CASES[fault]
    cfg, _, lanes, _ = cases[kind, "f64"]
    kw = dict(kw)
    if kw.get("model"):
        kw["model"] = np.column_stack([lanes["a1"], lanes["a2"], lanes["Kp"]])
    honest = M.numpy_mpc(kind, cfg, lanes, ph_table_oracle, **kw)
    use = M.check_recording(kind, cfg, lanes, ph_table_oracle, honest, **kw)                      # honest: passes, far inside
    assert max(use["trajectory"], use["ret"], use["optimal"]) <= 0.1
    with pytest.raises(AssertionError) as caught:
        M.check_recording(kind, cfg, lanes, ph_table_oracle, M.numpy_mpc(kind, cfg, lanes, ph_table_oracle, fault=fault, **kw), **kw)
    assert f"[{name}]" in str(caught.value), str(caught.value)


def test_a_forged_metric_row_trips_the_metrics_assertion(cases, ph_table_oracle):
    cfg, _, lanes, rec = cases["wt", "f64"]
    for row in (2, 6):                                                      # ITAE (bit-equal), return (the oracle's rewards)
        forged = dict(rec, metrics=rec["metrics"].copy())
        forged["metrics"][1, row, 5] *= 1.001
        with pytest.raises(AssertionError) as caught:
            M.check_recording("wt", cfg, lanes, ph_table_oracle, forged)
        assert "[metrics]" in str(caught.value)


# ---- 7. symbols ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pime_mpc_eval_supported", "pime_mpc_eval")


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
    assert nt.lib().pime_mpc_eval_supported(None) == 0
    host = C.CDLL(M.HOST_LIB_PATH)
    assert _declared("pime_mpc_host.h") == set(M.HOST_EXPORTS)
    for name in M.HOST_EXPORTS:
        assert hasattr(host, name), name
    for name in NEW_SYMBOLS:     # the host library is no second door to the product's entry points
        assert not hasattr(host, name), name


def test_the_package_never_names_the_host_library():
    for d, _, files in os.walk(P.PKG):
        for f in files:
            if f.endswith(".py"):
                assert "mpc_host" not in open(os.path.join(d, f)).read(), os.path.join(d, f)


def test_regret():
    from pime_amd import protocols
    pol = {"itae": np.array([[4.0, 3.0], [1.0, 0.0]]), "iae": np.array([[1.0, 1.0], [1.0, 1.0]])}
    base = {"itae": np.array([[2.0, 3.0], [0.0, 0.0]]), "iae": np.array([[0.5, 2.0], [1.0, 4.0]])}
    diff, ratio = protocols.regret(pol, base)
    np.testing.assert_array_equal(diff, [[2.0, 0.0], [1.0, 0.0]])
    np.testing.assert_array_equal(ratio, [[2.0, 1.0], [np.nan, np.nan]])
    diff, ratio = protocols.regret(pol, base, name="iae")
    np.testing.assert_array_equal(ratio, [[2.0, 0.5], [1.0, 0.25]])
