"""The case rule of the fused SAC step's gradient tests (tests/sac_cases.py), checked on the CPU: every case that a GPU test
compares with the oracle is vetted (kink margins), redraws at most a tenth of its samples, exposes every oracle mutant by ten times
the tolerance, is stable in float32, and exercises the branches the reference's initialisation never reaches."""
import numpy as np
import pytest

import sac_cases as SC
import sac_oracle as S

SPECS = SC.gradient_specs()


def test_the_lists_cover_every_served_shape_and_instantiation():
    assert {(s.width, s.D) for s in SC.shape_cases()} == set(SC.served())
    for B in SC.REGIME_B:
        assert {SC.kernel_class(s.width, s.D) for s in SC.regime_cases() if s.B == B} == set(SC.ALL_CLASSES)
    assert {s.D for s in SC.regime_cases() if s.D not in SC.COMPILED_D} == {1, 2, 5, 6, 7}
    assert {SC.kernel_class(s.width, s.D) for s in SPECS if s.B >= 32} == set(SC.ALL_CLASSES)   # none exempt from the mutants
    assert all(a != b for a, b in zip(SC.OTHER_HYPER, SC.DEFAULT_HYPER))
    assert (SC.DELTA, SC.MUTATION_MARGIN, SC.F32_STABILITY, SC.BAR) == (1e-5, 10.0, 1e-4, 3e-4)


@pytest.mark.parametrize("s", SPECS, ids=SC.spec_id)
def test_case_is_vetted_and_cheaply_so(s):
    case = SC.build(s)
    assert case.mid["margin"].min() >= SC.DELTA
    assert case.redrawn <= SC.MAX_REDRAWN * s.B, f"{case.redrawn} of {s.B} samples redrawn"
    assert case.idx.min() >= 0 and case.nxt.max() < SC.N_BUF
    if s.B >= 2:
        assert case.idx[s.row, 0] == 0 and case.nxt[s.row, -1] == SC.N_BUF - 1   # both ends of the ring are gathered


@pytest.mark.parametrize("s", [s for s in SPECS if s.B >= 32], ids=SC.spec_id)
def test_every_mutant_is_exposed(s):
    """(Cases of fewer than 32 samples are exempt, as in tests/test_td3_cases_cpu.py: with a handful of samples the min may pick
    the same head, or the mask be the same, on all of them.  Every instantiation has a larger case: first test above.)"""
    case = SC.build(s)
    for mutant in S.MUTANTS:
        reach = SC.mutant_reach(case, case.mid, mutant)
        assert reach > SC.MUTATION_MARGIN * SC.BAR, f"{mutant}: reach {reach:.2e}"


@pytest.mark.parametrize("s", SPECS, ids=SC.spec_id)
def test_float32_reference_arithmetic_is_stable(s):
    case = SC.build(s)
    lo = SC.reference_step(case, dt=np.float32, given=case.mid)
    for tag in ("gc", "ga"):
        for k, want in case.mid[tag].items():
            err = np.abs(lo[tag][k].astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30)   # (B = 1: a closed clamp zeroes a head)
            assert err <= SC.F32_STABILITY, f"{tag}.{k}: {err:.2e}"


@pytest.mark.parametrize("s", [s for s in SPECS if s.B >= 100], ids=SC.spec_id)
def test_clamp_and_knees_are_active(s):
    """A visible share (2 %) of the stepped samples beyond each Hardswish knee (some unit of the layer) and on each side of the
    log-std clamp, in the policy-gradient forward."""
    case = SC.build(s)
    (st, *_), eps = SC.batch_of(case)
    f = S.actor_forward(S.cast(case.nets[0], np.float64), st.astype(np.float64), eps)
    for z in ("z2", "z3"):
        assert (f[z] > 3).any(axis=1).mean() > 0.02 and (f[z] < -3).any(axis=1).mean() > 0.02
    assert (f["raw"] > 2).mean() > 0.02 and (f["raw"] < -20).mean() > 0.02


def test_oracle_class_agrees_with_the_case_step():
    """sac_oracle.Sac.step (what the golden and GPU tests drive) and sac_cases.reference_step are the same arithmetic."""
    s = SC.spec(64, 4, 37)
    case = SC.build(s)
    h = s.hyper
    o = S.Sac(*case.nets, alpha_log=h.alpha_log0, lr=h.lr, tau=h.tau, target_entropy=h.target_entropy, lr_alpha=h.lr_alpha)
    r = o.step(case.state, case.other, case.idx[0], case.nxt[0], case.noise_next[0], case.noise_pg[0])
    for tag in ("gc", "ga"):
        for k, want in case.mid[tag].items():
            np.testing.assert_allclose(r[tag][k], want, rtol=1e-6, atol=1e-7 * np.abs(want).max())
    np.testing.assert_allclose([r["obj_a"], r["obj_c"], o.alpha_log], [case.mid["obj_a"], case.mid["obj_c"], case.mid["alpha_log1"]], rtol=1e-6)
