"""The case rule of the PPO gradient sweep (tests/ppo_cases.py, tests/ppo_oracle.py), checked on the CPU: every case that
tests/test_gpu_ppo_sweep.py compares with the oracle is vetted (kink margins), redraws at most a tenth of its samples, exposes
every oracle mutant by ten times the bar, is stable in float32 and populates every branch of the loss; the route model the specs
are named from is the library's; the lists cover every route and kernel class the library can answer over the swept shapes; and
the oracle reproduces the reference's own first-step gradients (tests/golden/ppo_update_multi.npz)."""
import ctypes as C
import functools

import numpy as np
import pytest

import ppo_cases as PC
import ppo_oracle as P
from conftest import load_golden

B3_FORCED16 = dict(PC.b3_gradient_specs())   # the bf16x3 variant's own specs -> run under PIME_MLP16=1 as well?
SPECS = PC.gradient_specs() + list(B3_FORCED16)
LARGE = [s for s in SPECS if s.B >= 32]
SCALE_RTOL = 3e-6   # the bar of critic_scale in the GPU tests (tests/test_gpu_ppo_fused.py)
library_route = PC.library_route


def _id(s):
    return PC.spec_id(s) + (("-b3-mlp16" if B3_FORCED16[s] else "-b3") if s in B3_FORCED16 else "")


def _model_route(s):
    """The route a spec must name: the default process's model, or for the variant's own specs the model of their process."""
    if s in B3_FORCED16:
        return PC.expected_route(s.kind, s.D, s.Di, s.aw, s.cw, forced16=B3_FORCED16[s], b3=True)
    return PC.expected_route(s.kind, s.D, s.Di, s.aw, s.cw)


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
    assert {s.Di for s in PC.gradient_specs()} == {0, 1, 2, 3} and any(s.kind == "ppo" for s in PC.gradient_specs())
    assert {s.D for s in PC.shape_cases() if s.kind == "plain"} == set(range(1, 33))
    assert min(s.B for s in PC.gradient_specs()) == 2   # B = 1: no reference (module docstring of ppo_cases)
    assert (PC.DELTA, PC.MUTATION_MARGIN, PC.F32_STABILITY, PC.BAR, PC.MAX_REDRAWN) == (1e-5, 10.0, 1e-4, 3e-4, 0.10)
    forced = {PC.kernel_class(s, forced16=True)[0] for s in PC.forced16_cases()}
    assert forced == {("16tile", "16tile", "single"), ("lds", "16tile", "single")}


@pytest.mark.parametrize("s", SPECS, ids=_id)
def test_case_is_vetted_and_cheaply_so(s):
    case = PC.build(s)
    assert case.mid["margin"].min() >= PC.DELTA
    assert case.redrawn <= PC.MAX_REDRAWN * PC.N_ROWS, f"{case.redrawn} of the table's {PC.N_ROWS} rows redrawn"
    assert case.idx.min() == 0 and case.idx.max() == PC.N_ROWS - 1 and case.idx[0] == 0 and case.idx[-1] == PC.N_ROWS - 1
    assert s.B < 4 or len(set(case.idx.tolist())) < s.B   # repeats
    assert s.route == _model_route(s)
    assert case.salt <= PC.MAX_SALT
    assert all(np.isfinite(g).all() for net in ("ga", "gc") for g in case.mid[net].values())


@pytest.mark.parametrize("s", LARGE, ids=_id)
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


@pytest.mark.parametrize("s", LARGE, ids=_id)
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


@pytest.mark.parametrize("s", SPECS, ids=_id)
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


# ------------------------------------------------------------------------------------------------ the bf16x3 variant
_B3_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import ppo_cases as PC
import pime_amd.native as nt
L = nt.lib()
forced16 = PC.forced16_process()
assert PC.b3_process()
none, n = [], 0
for aw in PC.WIDTHS:
    for cw in PC.WIDTHS:
        for D in range(1, PC.MAX_D + 1):
            for kind, Di in [("plain", 0)] + [("modular", Di) for Di in range(1, min(D, 4))]:
                want = PC.expected_route(kind, D, Di, aw, cw, forced16, b3=True)
                got = PC.library_route(kind, D, Di, aw, cw)
                assert got == want, (kind, D, Di, aw, cw, got, want)
                if "none" in got:
                    assert "LDS map does not fit" in nt.last_error()
                    none.append((kind, D, Di, aw, cw))
                ka = nt.MLP_MODULAR_ACTOR if kind == "modular" else nt.MLP_PLAIN_ACTOR
                for k, okind, w, di in ((ka, kind, aw, Di), (nt.MLP_CRITIC, "critic", cw, 0)):
                    planes = L.pime_ppo_bwd_image_floats(k, D, di, w) > L.pime_ppo_bwd_image_f32_floats(k, D, di, w)
                    assert L.pime_ppo_bwd_image_f32_floats(k, D, di, w) > 0
                    assert planes == PC.b3_net(okind, w, D, di, forced16), (okind, w, D, di)
                n += 1
caps = {}
for s in (PC.b3_forced16_cases() if forced16 else PC.b3_regime_cases()):
    if s.B == PC.CAP_B:
        r, grids = PC.resolve_cap(s, forced16)
        caps[PC.spec_id(s)] = [r.B, grids]
print("B3_MODEL " + json.dumps({"n": n, "none": none, "caps": caps}))
"""


@functools.lru_cache(maxsize=None)
def _b3_child(forced16):
    """The variant's model against the library in a child process (both variables are read once per process; every query is
    host-only)."""
    import json
    import os
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("PIME_MLP16", "PIME_GRAD_BF16X3")}
    env.update(PIME_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PIME_GRAD_BF16X3="1")
    if forced16:
        env["PIME_MLP16"] = "1"
    r = subprocess.run([sys.executable, "-c", _B3_CHILD], env=env, capture_output=True, text=True, timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("B3_MODEL ")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(line[0].split(" ", 1)[1])


@pytest.mark.parametrize("forced16", (False, True), ids=("b3", "b3-mlp16"))
def test_the_variants_route_model_is_the_librarys(forced16):
    """Under PIME_GRAD_BF16X3=1, alone and with PIME_MLP16=1: expected_route(..., b3=True) against pime_ppo_route for every actor
    kind, D 1..32, Di 1..3 and every pair of widths; the transposed image carries planes (pime_ppo_bwd_image_floats above
    pime_ppo_bwd_image_f32_floats) exactly where b3_net says so; the shapes without a kernel are the modular actors of width 256
    with a plant tower of 29 floats or more, and the query's error names the LDS map."""
    rec = _b3_child(forced16)
    assert rec["n"] == 9 * (32 + 31 + 30 + 29)
    none = {tuple(x) for x in rec["none"]}
    assert none == {("modular", D, Di, 256, cw) for cw in PC.WIDTHS for D in range(2, 33) for Di in range(1, min(D, 4)) if D - Di >= 29}
    assert len({x[1:3] for x in none}) == 6
    # the default process's model knows no such family
    assert all("none" not in PC.expected_route(k, D, Di, aw, cw, f16) for k, D, Di, aw, cw in _all_shapes() for f16 in (False, True))


def _instantiations(s, forced16):
    """The B3 = true kernel instantiations a case runs, each with its partner's family: (kernel, T, role, partner)."""
    out = set()
    on = PC.b3_nets(s, forced16)
    if on[0] and s.route[0] == "16tile":
        out.add(("ppo16m" if s.kind == "modular" else "ppo16", s.aw // 16, "actor", "b3" if on[1] else s.route[1]))
    if on[1] and s.route[1] == "16tile":
        out.add(("ppo16", s.cw // 16, "critic", "b3" if on[0] else s.route[0]))
    return out


def test_the_variants_lists_cover_every_b3_kernel_and_class():
    """Every case of the variant's lists runs at least one B3 kernel; the shape list holds every B3 kernel class of the square shapes
    the variant serves, the regime list every class at every 16-tile batch regime and the cap batch once per (route, width); every
    instantiation -- ppo16_kernel<8 | 16, actor | critic, true>, ppo16m_kernel<8 | 16, true> -- appears next to a B3 partner and
    next to an f32 partner of another family (the LDS-resident kernels or the split pipeline)."""
    lists = {name: (f16, fn()) for name, (f16, fn) in PC.B3_LISTS.items()}
    for name, (f16, cases) in lists.items():
        for s in cases:
            assert any(PC.b3_nets(s, f16)) and "none" not in s.route, (name, PC.spec_id(s))
            assert s.route == PC.expected_route(s.kind, s.D, s.Di, s.aw, s.cw, f16, b3=True) and s.vet
    served = [PC.b3_spec(k, D, Di, w, 37) for k, D, Di, w, cw in _all_shapes() if w == cw]
    served = [s for s in served if "none" not in s.route and any(PC.b3_nets(s))]
    classes = {PC.b3_kernel_class(s) for s in served}
    assert classes == {PC.b3_kernel_class(s) for s in PC.b3_shape_cases()} and len(classes) == 8
    regimes = PC.b3_regime_cases()
    for cls in classes:
        members = {s.B for s in regimes if PC.b3_kernel_class(s) == cls}
        assert set(PC.REGIME_B["16tile"]) <= members, cls
    for route, w in {(c[0], c[1]) for c in classes}:
        assert len([s for s in regimes if s.route == route and s.aw == w and s.B == PC.CAP_B]) == 1, (route, w)
    assert len([s for s in PC.b3_forced16_cases() if s.B == PC.CAP_B and s.kind == "modular"]) == 1
    assert {s.aw for s in PC.b3_forced16_cases()} == {128} and {s.cw for s in PC.b3_forced16_cases()} == {128, 64}
    assert {(s.kind, s.D, s.Di) for s in PC.b3_shape_cases(256)} >= {("modular", 31, 3), ("modular", 4, 2), ("modular", 7, 3), ("modular", 29, 1)}
    assert not any(s.kind == "modular" and s.D - s.Di > 28 for s in PC.b3_shape_cases(256))
    inst = set()
    for f16, cases in lists.values():
        for s in cases:
            inst |= _instantiations(s, f16)
    kernels = {("ppo16", 8, "actor"), ("ppo16", 16, "actor"), ("ppo16", 8, "critic"), ("ppo16", 16, "critic"), ("ppo16m", 8, "actor"),
               ("ppo16m", 16, "actor")}
    assert {i[:3] for i in inst} == kernels
    assert {i[:3] for i in inst if i[3] == "b3"} == kernels
    # next to an f32 partner of another family (LDS-resident, split pipeline).  ppo16m_kernel<16, true>: a critic of width 64 / 128
    # on the actor's observation would do; the lists hold it next to B3 critics only (the issue's lists).  ppo16m_kernel<8, true>
    # exists under PIME_MLP16=1 alone, which leaves no net outside the 16-tile family: its f32 partner is that family's f32 kernel.
    assert {i[:3] for i in inst if i[3] in ("lds", "split")} == kernels - {("ppo16m", 8, "actor"), ("ppo16m", 16, "actor")}
    assert ("ppo16m", 8, "actor", "16tile") in inst
    # the property and chain shapes: one per (route, widths, actor kind, which nets are B3)
    keys = {(s.route, s.aw, s.cw, PC.okind(s.kind), PC.b3_nets(s)) for s in PC.b3_shape_cases() + PC.b3_mixed_cases()}
    assert keys == {(s.route, s.aw, s.cw, PC.okind(s.kind), PC.b3_nets(s)) for s in PC.b3_per_route_shapes()} and len(keys) == 8
    assert {(s.kind, s.cw, s.B) for s in PC.b3_property_cases(True)} == {(k, cw, B) for k, cw in (("plain", 128), ("modular", 128), ("modular", 64))
                                                                         for B in (293, 100)}


@pytest.mark.parametrize("forced16", (False, True), ids=("b3", "b3-mlp16"))
def test_the_variants_cap_batches_are_vetted(forced16):
    """The "grid x 64 + 1" batches, sized from pime_ppo_grid16 under the variable (child process), held to the same conditions as
    every other case: kink margin, redrawn rows, salt, float32 stability, category shares, every mutant."""
    caps = _b3_child(forced16)["caps"]
    placeholders = [s for s in (PC.b3_forced16_cases() if forced16 else PC.b3_regime_cases()) if s.B == PC.CAP_B]
    assert {PC.spec_id(s) for s in placeholders} == set(caps) and len(caps) == (1 if forced16 else 3)
    for s in placeholders:
        B, grids = caps[PC.spec_id(s)]
        assert B == max(grids.values()) * 64 + 1 and all((B + 63) // 64 > g for g in grids.values())
        s = s._replace(B=B)
        case = PC.build(s)
        assert case.mid["margin"].min() >= PC.DELTA and case.redrawn <= PC.MAX_REDRAWN * PC.N_ROWS and case.salt <= PC.MAX_SALT
        assert case.idx[0] == 0 and case.idx[-1] == PC.N_ROWS - 1
        assert PC.f32_distance(case) <= PC.F32_STABILITY
        cat, branch = PC.categories(case)
        assert (np.bincount(cat, minlength=5) / s.B).min() >= 0.10 and (np.bincount(branch, minlength=2) / s.B).min() >= 0.20
        for mutant in P.mutants_of(PC.okind(s.kind)):
            if mutant == "biased_std":
                reach = PC.reference(case, mutant=mutant, light=True)["scale"] / case.mid["scale"] - 1
                assert abs(reach * 2 * s.B - 1) <= 0.01 + 1.0 / s.B and 1 / (2 * s.B) > SCALE_RTOL
                continue
            reach = PC.mutant_reach(case, mutant)
            assert reach > PC.MUTATION_MARGIN * PC.BAR, f"{PC.spec_id(s)} {mutant}: reach {reach:.2e}"
