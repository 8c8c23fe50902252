"""The case rule of the PPO gradient sweep (tests/ppo_cases.py, tests/ppo_oracle.py), checked on the CPU: every case that
tests/test_gpu_ppo_sweep.py compares with the oracle is vetted (kink margins), redraws at most a tenth of its samples, exposes
every oracle mutant by ten times the bar, is stable in float32 and populates every branch of the loss; the route model the specs
are named from is the library's; the lists cover every route and kernel class the library can answer over the swept shapes; and
the oracle reproduces the reference's own first-step gradients (tests/golden/ppo_update_multi.npz)."""
import ctypes as C

import numpy as np
import pytest

import ppo_cases as PC
import ppo_oracle as P
from conftest import load_golden

SPECS = PC.gradient_specs()
LARGE = [s for s in SPECS if s.B >= 32]
SCALE_RTOL = 3e-6   # the bar of critic_scale in the GPU tests (tests/test_gpu_ppo_fused.py)
library_route = PC.library_route


def _all_shapes():
    for aw in PC.WIDTHS:
        for cw in PC.WIDTHS:
            for D in range(1, PC.MAX_D + 1):
                yield "plain", D, 0, aw, cw
                for Di in range(1, min(D, 4)):
                    yield "modular", D, Di, aw, cw


def test_the_route_model_is_the_librarys():
    """expected_route (what every spec names, and every GPU case asserts again on the GPU machine) against pime_ppo_route -- the
    function pime_ppo_minibatch_grad dispatches on -- for every actor kind, D 1..32, Di 1..3 and every pair of widths.  The
    query is host-only.  (Without PIME_MLP16 in the environment: the forced routes are asserted by the child process of the GPU
    sweep.)"""
    import os
    if os.environ.get("PIME_MLP16") is not None:
        pytest.fail("PIME_MLP16 is set: the route model of the default process cannot be checked")
    import pime_amd.native as nt
    L = nt.lib()
    n = 0
    for kind, D, Di, aw, cw in _all_shapes():
        assert library_route(kind, D, Di, aw, cw) == PC.expected_route(kind, D, Di, aw, cw), (kind, D, Di, aw, cw)
        k = nt.MLP_MODULAR_ACTOR if kind == "modular" else nt.MLP_PLAIN_ACTOR
        if aw == cw:   # pime_ppo_pair_fits is the same answer
            assert L.pime_ppo_pair_fits(k, D, Di, aw) == int(PC.expected_route(kind, D, Di, aw, cw)[2] == "pair")
        n += 1
    assert n == 9 * (32 + 31 + 30 + 29)
    assert L.pime_ppo_route(nt.MLP_CRITIC, 3, 0, 128, 128, (C.c_int32 * 3)()) != 0   # not an actor
    assert L.pime_ppo_route(nt.MLP_PLAIN_ACTOR, 33, 0, 128, 128, (C.c_int32 * 3)()) != 0
    # the grid caps the regime list is built on
    assert L.pime_ppo_fused_grid(1 << 30) == PC.FUSED_CAP
    for s in PC.shape_cases():
        fa, fc, _ = s.route
        if fa == "16tile":
            ka = nt.MLP_MODULAR_ACTOR if s.kind == "modular" else nt.MLP_PLAIN_ACTOR
            assert L.pime_ppo_grid16(ka, 1 << 30, s.aw, s.D, s.Di) == PC.GRID16_CAP
        if fc == "16tile":
            assert L.pime_ppo_grid16(nt.MLP_CRITIC, 1 << 30, s.cw, s.D, 0) == PC.GRID16_CAP
    assert L.pime_ppo_grid16(nt.MLP_CRITIC, 65, 256, 3, 0) == 2 and L.pime_ppo_grid16(nt.MLP_CRITIC, 64, 256, 3, 0) == 1


def test_the_lists_cover_every_route_and_class():
    """Over the swept shapes (equal widths, plain D 1..32, modular D 2..32 x Di 1..3) the library answers a set of routes and the
    model a set of kernel classes: the shape list holds every one, the regime list every class at every batch size of its
    families, the cap batch once per (route, width), and every class has a case of 32 samples or more (none exempt from the
    mutants).  The mixed list holds the three single-net launches of the LDS-resident kernel."""
    shapes = [(k, D, Di, w) for k, D, Di, w, cw in _all_shapes() if w == cw]
    routes = {library_route(k, D, Di, w, w) for k, D, Di, w in shapes}
    assert routes == {s.route for s in PC.shape_cases()}
    assert routes == {("lds", "lds", "pair"), ("lds", "lds", "dual"), ("16tile", "16tile", "single"), ("split", "16tile", "single")}
    classes = {PC.kernel_class(PC.spec(k, D, Di, w, 37)) for k, D, Di, w in shapes}
    assert classes == {PC.kernel_class(s) for s in PC.shape_cases()}
    regimes = PC.regime_cases()
    for cls in classes:
        members = [s for s in regimes if PC.kernel_class(s) == cls]
        want = {b for fam in cls[0][:2] for b in PC.REGIME_B[fam]}
        assert want <= {s.B for s in members}, cls
    for route, w in {(c[0], c[1]) for c in classes}:
        big = [s.B for s in regimes if s.route == route and s.aw == w and s.B > 10000]
        assert len(big) == 1, (route, w)
        assert big[0] == max(PC.FUSED_CAP * 256 + 1 if "lds" in route else 0, PC.GRID16_CAP * 64 + 1 if "lds" not in route else 0)
    assert classes <= {PC.kernel_class(s) for s in LARGE}
    # the !early_w branch of the pair kernel (fan-in above first_grad_valu's 7) exists at width 128 only at D = 8, at width 64 from 8 on
    assert {s.D for s in PC.shape_cases() if s.aw == 128 and s.route[2] == "pair" and s.D > 7} == {8}
    assert {s.D for s in regimes if s.aw == 128 and s.route[2] == "pair" and s.D > 7} == {8}
    assert {(s.kind, s.aw, s.cw) for s in PC.mixed_cases()} == {("plain", 64, 128), ("modular", 128, 64), ("plain", 256, 128)}
    assert all(s.route[2] == "single" and "lds" in s.route for s in PC.mixed_cases())
    assert {s.Di for s in SPECS} == {0, 1, 2, 3} and any(s.kind == "ppo" for s in SPECS)
    assert {s.D for s in PC.shape_cases() if s.kind == "plain"} == set(range(1, 33))
    assert min(s.B for s in SPECS) == 2   # B = 1: no reference (module docstring of ppo_cases)
    assert (PC.DELTA, PC.MUTATION_MARGIN, PC.F32_STABILITY, PC.BAR, PC.MAX_REDRAWN) == (1e-5, 10.0, 1e-4, 3e-4, 0.10)
    forced = {PC.kernel_class(s, forced16=True)[0] for s in PC.forced16_cases()}
    assert forced == {("16tile", "16tile", "single"), ("lds", "16tile", "single")}


@pytest.mark.parametrize("s", SPECS, ids=PC.spec_id)
def test_case_is_vetted_and_cheaply_so(s):
    case = PC.build(s)
    assert case.mid["margin"].min() >= PC.DELTA
    assert case.redrawn <= PC.MAX_REDRAWN * PC.N_ROWS, f"{case.redrawn} of the table's {PC.N_ROWS} rows redrawn"
    assert case.idx.min() == 0 and case.idx.max() == PC.N_ROWS - 1 and case.idx[0] == 0 and case.idx[-1] == PC.N_ROWS - 1
    assert s.B < 4 or len(set(case.idx.tolist())) < s.B   # repeats
    assert s.route == PC.expected_route(s.kind, s.D, s.Di, s.aw, s.cw)
    assert case.salt <= PC.MAX_SALT
    assert all(np.isfinite(g).all() for net in ("ga", "gc") for g in case.mid[net].values())


@pytest.mark.parametrize("s", LARGE, ids=PC.spec_id)
def test_every_branch_of_the_loss_is_populated(s):
    """Each (advantage sign x clip side) category and the unclipped one holds at least 10 % of the samples, each SmoothL1 branch at
    least 20 % -- read from the oracle's own ratio and v - r_sum."""
    case = PC.build(s)
    cat, branch = PC.categories(case)
    share = np.bincount(cat, minlength=5) / s.B
    assert share.min() >= 0.10, dict(zip(PC.RATIO_CATEGORIES, share))
    assert (np.bincount(branch, minlength=2) / s.B).min() >= 0.20
    adv = case.table[3][case.idx]
    assert (np.sign(adv[cat == 1]) == 1).all() and (np.sign(adv[cat == 3]) == -1).all()


@pytest.mark.parametrize("s", LARGE, ids=PC.spec_id)
def test_every_mutant_is_exposed(s):
    """Every mutant moves a gradient tensor by more than 10 x the bar.  (Cases of fewer than 32 samples are exempt, as in the TD3
    and SAC case tests; every class has a larger case.)  One mutant cannot be held to that through the gradients: the biased
    standard deviation multiplies the critic scale, hence the critic's gradients, by 1 / sqrt(1 - 1 / B) = 1 + 1 / (2 B) whatever
    the inputs -- under 10 x 3e-4 from B = 167 on.  It is held to what it is: its reach on the scale must BE 1 / (2 B) (to
    1 % + 1 / B of it: the next term of the series is 3 / (8 B^2), and there is the 1e-5 under the fraction), and that must exceed the bar of the check that
    sees it, critic_scale at rtol 3e-6 -- which it does up to B = 166 666, beyond every batch of the lists."""
    case = PC.build(s)
    for mutant in P.mutants_of(PC.okind(s.kind)):
        if mutant == "biased_std":
            reach = PC.reference(case, mutant=mutant, light=True)["scale"] / case.mid["scale"] - 1
            assert abs(reach * 2 * s.B - 1) <= 0.01 + 1.0 / s.B, f"{mutant}: reach {reach:.3e} is not 1 / (2 B)"
            assert 1 / (2 * s.B) > SCALE_RTOL
            continue
        reach = PC.mutant_reach(case, mutant)
        assert reach > PC.MUTATION_MARGIN * PC.BAR, f"{mutant}: reach {reach:.2e}"


@pytest.mark.parametrize("s", SPECS, ids=PC.spec_id)
def test_float32_oracle_is_stable(s):
    case = PC.build(s)
    lo = PC.reference(case, dt=np.float32)
    for net in ("ga", "gc"):
        for k, want in case.mid[net].items():
            assert lo[net][k].dtype == np.float32
            err = np.abs(lo[net][k].astype(np.float64) - want).max() / np.abs(want).max()
            assert err <= PC.F32_STABILITY, f"{net}.{k}: {err:.2e}"
    assert abs(lo["scale"] / case.mid["scale"] - 1) <= PC.F32_STABILITY
    assert lo["moments"] == case.mid["moments"]   # float64 sums of the float32 targets in either mode


def test_mutants_are_one_line_deviations():
    """Every mutant differs from the oracle, no two tower or net mutants coincide, and each one moves only the nets it names."""
    case = PC.build(PC.spec("modular", 5, 2, 128, 37))
    assert len(set(P.MUTANTS)) == len(P.MUTANTS) == 19 and set(P.mutants_of("plain")) == set(P.MUTANTS) - set(P.MUTANTS_MODULAR)
    for mutant in P.MUTANTS:
        got = PC.reference(case, mutant=mutant)
        moved = {net for net, tag in (("act", "ga"), ("cri", "gc"))
                 if any(not np.array_equal(got[tag][k], case.mid[tag][k]) for k in got[tag])}
        assert moved == set(P.touches(mutant)), (mutant, moved)


def test_oracle_against_finite_differences():
    """The hand-written backward passes against central differences of the hand-written objective (float64; the scale is a
    constant of the batch): both actor kinds, Di 2, every parameter tensor's largest-gradient element and a_std_log."""
    for kind, Di in (("plain", 0), ("modular", 2)):
        case = PC.build(PC.spec(kind, 5, Di, 64, 37))
        act, cri = ({k: v.astype(np.float64) for k, v in p.items()} for p in case.nets)
        s, a, lp_old, adv, r = (np.asarray(t, dtype=np.float64) for t in PC.batch_of(case))

        def united(act_, cri_):
            lp = P.logprob(act_, kind, Di, s, a)
            ratio = np.exp(lp - lp_old)
            surr = np.minimum(adv * ratio, adv * np.clip(ratio, 1 - PC.RATIO_CLIP, 1 + PC.RATIO_CLIP))
            d = P.critic_forward(cri_, s)[0] - r
            l1 = np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
            return -surr.mean() + PC.LAMBDA_ENTROPY * (np.exp(lp) * lp).mean() + l1.mean() / (r.std(ddof=1) + 1e-5)
        for net, tag in ((act, "ga"), (cri, "gc")):
            for k, g in case.mid[tag].items():
                g = g.reshape(net[k].shape)
                at = np.unravel_index(np.argmax(np.abs(g)), g.shape)
                h = 1e-6
                keep = net[k][at]
                net[k][at] = keep + h
                up = united(act, cri)
                net[k][at] = keep - h
                down = united(act, cri)
                net[k][at] = keep
                assert abs((up - down) / (2 * h) - g[at]) <= 1e-6 * abs(g[at]) + 1e-9, (kind, tag, k)


def test_oracle_reproduces_the_references_first_step_gradients():
    """tests/golden/ppo_update_multi.npz, case `mw` (pH, modular actor, width 128, batch 4 096): the minibatch of the first
    optimizer step rebuilt from the fixture's buffer, indices and initial weights -- values by oracle.critic_forward, reward sums
    and advantages by oracle.gae, the normalisation and the old log-probs as the agent forms them, in float32 -- and the float64
    oracle's gradients against the reference's own .grad tensors (torch fp32 on the CPU), at the bar the GPU test holds the
    kernels to for the same tensors (tests/test_gpu_update_golden.py: 3e-4 of the largest entry)."""
    import oracle
    g = load_golden("ppo_update_multi.npz")
    tag, case = "ph128", "mw"
    hyper = g[f"{tag}:{case}:hyper"]
    batch, lam = int(hyper[2]), float(hyper[4])
    state, other = g[f"{tag}:buf_state"], g[f"{tag}:buf_other"]
    act = {k[len(tag) + 6:]: g[k] for k in g.files if k.startswith(f"{tag}:act0.")}
    cri = {k[len(tag) + 6:]: g[k] for k in g.files if k.startswith(f"{tag}:cri0.")}
    reward, mask, action, noise = other[:, 0], other[:, 1], other[:, 2], other[:, 3]
    T = len(state)
    value = oracle.critic_forward(state, cri)
    r_sum, adv = oracle.gae(reward.reshape(T, 1), mask.reshape(T, 1), value.reshape(T, 1), lam, True)
    r_sum, adv = r_sum.reshape(-1), adv.reshape(-1)
    adv = ((adv - adv.mean(dtype=np.float32)) / (adv.std(ddof=1, dtype=np.float32) + np.float32(1e-5))).astype(np.float32)
    logp_old = -(noise * noise * np.float32(0.5) + act["a_std_log"].reshape(()) + np.float32(P.LOG_SQRT_2PI)).astype(np.float32)
    idx = g[f"{tag}:{case}:indices"][0].astype(np.int64)
    assert idx.shape == (batch,)
    out = P.gradients(act, cri, "modular", 1, (state[idx], action[idx], logp_old[idx], adv[idx], r_sum[idx]), 0.2, 0.02)
    worst, n = 0.0, 0
    for net, grads in (("act", out["ga"]), ("cri", out["gc"])):
        for k, got in grads.items():
            want = g[f"{tag}:{case}:grad1:{net}.{k}"]
            share = np.abs(got.reshape(want.shape) - want).max() / np.abs(want).max()
            worst = max(worst, share)
            n += want.size
            assert share <= 3e-4, f"{net}.{k}: {share:.2e} of the largest entry"
    assert n == 67459   # every trainable parameter of both nets
    print(f"ppo oracle against the reference's first-step gradients (mw): worst share of a tensor's largest entry {worst:.2e}")
