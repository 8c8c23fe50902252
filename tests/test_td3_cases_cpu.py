"""What the fused-TD3 sweep (tests/test_gpu_td3_sweep.py) rests on, checked without a GPU: the sweep lists are complete, every
vetted case exercises every branch of the arithmetic (by mutation of the oracle), the reference arithmetic is stable on every case
(kink margins, float32 against float64), and the Adam replay and its bounds hold against the reference's recorded step and
against float32 numpy.  The numbers are conditions on the test inputs (tests/td3_cases.py); no kernel runs here."""
import numpy as np
import pytest

import td3_cases as T
from conftest import load_golden
from oracle import td3 as O

GRADIENT_SPECS = T.gradient_specs()


def _launch_class(md, D):
    # csrc/td3_device.hpp grad_dispatch_d<K, MD>: D == 3 | 4 | 12 | 30 compiled in; else run-time D, td3_first_ksteps(D) = (D + 1 <= 8 ? 2 : 8)
    if D in (3, 4, 12, 30):
        return md, f"D{D}"
    return md, "rt2" if D + 1 <= 8 else "rt8"


def test_the_sweep_lists_cover_every_instantiation_and_every_shape():
    classes = {_launch_class(w, k) for w in (64, 128, 256) for k in range(1, 32)}
    assert len(classes) == 18 and classes == set(T.ALL_CLASSES)
    assert all(T.kernel_class(w, D) == _launch_class(w, D) for w in (64, 128, 256) for D in range(1, 32))
    a = T.shapes_93()
    assert len(a) == 93 and {(s.width, s.D) for s in a} == {(w, D) for w in (64, 128, 256) for D in range(1, 32)}
    assert all(s.B == 37 and s.vet for s in a)
    b = T.regime_cases()
    assert len(b) == 54
    for B in (1, 17, 8193):
        assert {_launch_class(s.width, s.D) for s in b if s.B == B} == classes
    assert {1, 2, 7, 8, 15, 16, 17, 29, 31} <= {s.D for s in b}
    c = T.third_group_cases()
    assert {(s.width, 2 if s.D + 1 <= 8 else 8) for s in c} == {(w, k) for w in (64, 128, 256) for k in (2, 8)}   # (width, k-steps)
    assert all(s.B == 16400 and (s.B + 15) // 16 > 2 * 512 for s in c)
    assert {_launch_class(s.width, s.D) for s in T.class_cases_37()} == classes and set(T.class_cases_37()) <= set(a)
    h = T.hyper_cases()
    assert {s.width for s, _ in h} == {64, 128, 256} and (128, 7) in {(s.width, s.D) for s, _ in h}
    assert {mode for _, mode in h} == {0, 1, 2} and all(s.row == 3 and s.rows == 4 and s.row % s.hyper.update_freq == 0 for s, _ in h)
    # a class whose only case is exempt from the mutation check (B < 32) would be untested
    assert {_launch_class(s.width, s.D) for s in GRADIENT_SPECS if s.B >= 32} == classes


def test_the_library_serves_all_93_shapes():
    from pime_amd import native
    for w in (64, 128, 256):
        for D in range(1, 32):
            assert native.lib().pime_td3_supported(D, 1, w) == 1, (w, D)


def test_the_restated_step_is_the_oracle():
    """tests/td3_cases.py restates the two objectives (to mutate them and to evaluate them in float32); unmutated and in float64 they
    are oracle/td3.py bit for bit, and its Adam replay is oracle.td3.Adam."""
    case = T.build(T.spec(128, 7, 37))
    h = case.spec.hyper
    s, a, r, m, s2, eps = (np.asarray(v, dtype=np.float64) for v in T.batch_of(case))
    act, act_t, cri, cri_t = (O.f64(p, keys) for p, keys in zip(case.nets, (O.ACTOR_KEYS, O.ACTOR_KEYS, O.CRITIC_KEYS, O.CRITIC_KEYS)))
    obj, g = O.critic_objective(cri, cri_t, act_t, s, a, r, m, s2, eps, h.policy_noise, h.noise_clip)
    obj2, g2 = T.critic_pass(case.nets, T.batch_of(case), h)
    assert obj == obj2 and all(np.array_equal(g[k], g2[k]) for k in g)
    obj, g = O.actor_objective(act, cri_t, s)
    obj2, g2 = T.actor_pass(case.nets[0], case.nets[3], s)
    assert obj == obj2 and all(np.array_equal(g[k], g2[k]) for k in g)
    opt = O.Adam(cri, 3e-4, (0.8, 0.99), 1e-6)
    p, mo, v = T.flatten(cri, O.CRITIC_KEYS), 0.0, 0.0
    rng = np.random.RandomState(0)
    for t in (1, 2, 3):
        grads = {k: rng.standard_normal(x.shape) for k, x in cri.items()}
        opt.step(cri, grads)
        rep = T.adam_replay(p, mo, v, T.flatten(grads, O.CRITIC_KEYS), t, 3e-4, (0.8, 0.99), 1e-6, f32_hyper=False)
        p, mo, v = rep["param"], rep["exp_avg"], rep["exp_avg_sq"]
        np.testing.assert_allclose(p, T.flatten(cri, O.CRITIC_KEYS), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("s", GRADIENT_SPECS, ids=T.spec_id)
def test_case_is_stable_and_exercises_every_branch(s):
    """Sections b and c of the input rule, per case: after the redraw no sample is within DELTA of a kink and float32 numpy agrees
    with float64 to F32_STABILITY of each tensor's largest entry; and (B >= 32) every mutant of the oracle moves a gradient tensor
    by more than MUTATION_MARGIN x the 3e-4 bar."""
    case = T.build(s)
    mid = case.mid     # reference_step(case, margins=True) of the inputs as build() left them
    assert mid["margin"].shape == (s.B,) and mid["margin"].min() >= T.DELTA
    f32 = T.reference_step(case, dt=np.float32)
    dev = max(float(np.abs(f32[g][k] - mid[g][k]).max() / np.abs(mid[g][k]).max()) for g in ("gc", "ga") for k in mid[g])
    line = f"td3 case {T.spec_id(s)}: redrawn {case.redrawn}/{s.B} in {case.redraw_rounds} rounds, min margin {mid['margin'].min():.2e}, " \
           f"float32 vs float64 {dev:.1e}"
    if s.B >= 32:
        cache = {}
        reach = {m: T.mutant_reach(case, mid, m, cache) for m in T.MUTANTS}
        weakest = min(reach, key=reach.get)
        line += f", weakest mutant {weakest} {reach[weakest] / T.BAR:.0f} x bar"
    print(line)
    assert dev <= T.F32_STABILITY
    if s.B >= 32:
        assert reach[weakest] > T.MUTATION_MARGIN * T.BAR, reach


@pytest.mark.parametrize("fixture", ["multi", "256"])
def test_adam_replay_reproduces_the_references_first_step(fixture):
    """Weights before + the reference's own first-step .grad -> adam_replay -> the recorded weights after step 1, within the
    replay bound plus one float32 ulp of the recorded value (torch rounds its own way); the soft-updated targets likewise."""
    if fixture == "multi":
        g = load_golden("td3_update_multi.npz")
        hyper = g["td3m:hyper"]
        lr, tau = float(hyper[4]), float(hyper[5])
        sets = [("td3m:act0", "td3m:grad1:act", "td3m:act_step1", "td3m:act_target0", "td3m:act_target_step1", O.ACTOR_KEYS),
                ("td3m:cri0", "td3m:grad1:cri", "td3m:cri_step1", "td3m:cri_target0", "td3m:cri_target_step1", O.CRITIC_KEYS)]
        get = lambda key: g[key]
    else:
        parts = [load_golden(f"td3_update_256{k}.npz") for k in ("", "_nets0", "_grad1", "_step1")]
        hyper = parts[0]["td3w:hyper"]
        lr, tau = float(hyper[3]), float(hyper[4])
        sets = [("td3w:act0", "td3w:grad1:act", "td3w:act_step1", None, None, O.ACTOR_KEYS),
                ("td3w:cri0", "td3w:grad1:cri", "td3w:cri_step1", None, None, O.CRITIC_KEYS)]

        def get(key):
            return next(p[key] for p in parts if key in p.files)
    for w0, gr, w1, t0, t1, keys in sets:
        before = np.concatenate([get(f"{w0}.{k}").reshape(-1) for k in keys])
        grad = np.concatenate([get(f"{gr}.{k}").reshape(-1) for k in keys])
        after = np.concatenate([get(f"{w1}.{k}").reshape(-1) for k in keys])
        assert before.dtype == grad.dtype == after.dtype == np.float32
        tb = np.concatenate([get(f"{t0}.{k}").reshape(-1) for k in keys]) if t0 else None
        rep = T.adam_replay(before, np.zeros_like(before), np.zeros_like(before), grad, 1, lr, target=tb, tau=tau, blend_param=after if t0 else None)
        bound = T.replay_bounds(rep, np.zeros_like(before), grad, lr, tb)
        assert np.all(np.abs(after - rep["param"]) <= bound["param"] + np.spacing(np.abs(after))), w1
        assert np.abs(after - before).max() > 0.5 * lr
        if t0:
            ta = np.concatenate([get(f"{t1}.{k}").reshape(-1) for k in keys])
            assert np.all(np.abs(ta - rep["target"]) <= bound["target"] + np.spacing(np.abs(ta))), t1


@pytest.mark.parametrize("hyper", [T.DEFAULT_HYPER, T.OTHER_HYPER], ids=["default", "hyper2"])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_replay_bounds_hold_for_float32_numpy(step, hyper):
    """The derived bounds against a float32 evaluation of td3_apply_kernel's formulas: bias corrections near 1 - beta (step 1, 2)
    and near 1 (step 1 000); gradients over twelve decades, zeros, moments independent of the gradient (so that exp_avg cancels on
    some elements: the case that the first derivation of its bound, 2^-22 |m'|, does not survive -- shown here)."""
    rng = np.random.RandomState(step)
    n = 200000
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 0, n)).astype(np.float32)
    g[::97] = 0.0
    p = rng.uniform(-1, 1, n).astype(np.float32) * (10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    t = (p + rng.standard_normal(n).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        scale = np.abs(g) + np.float32(1e-20)
        m = (rng.standard_normal(n) * scale).astype(np.float32)
        m[::5] = (-g[::5] * np.float32((1 - hyper.betas[0]) / hyper.betas[0]) * (1 + rng.standard_normal(len(g[::5])) * 1e-3)).astype(np.float32)
        v = (rng.uniform(0.5, 2.0, n) * scale * scale).astype(np.float32)
    got = T.adam_f32(p, m, v, g, step, hyper.lr, hyper.betas, hyper.eps, t, hyper.tau)
    rep = T.adam_replay(p, m, v, g, step, hyper.lr, hyper.betas, hyper.eps, t, hyper.tau, blend_param=got["param"])
    bound = T.replay_bounds(rep, m, g, hyper.lr, t)
    for k in ("param", "exp_avg", "exp_avg_sq", "target"):
        err = np.abs(got[k].astype(np.float64) - rep[k])
        assert np.all(err <= bound[k]), (k, float((err / np.maximum(bound[k], 1e-300)).max()))
    if step > 1:   # the first derivation's moment bound fails on cancelling elements; the operand-relative one holds (above)
        naive = 2.0 ** -22 * np.abs(rep["exp_avg"])
        assert np.any(np.abs(got["exp_avg"].astype(np.float64) - rep["exp_avg"]) > naive)
