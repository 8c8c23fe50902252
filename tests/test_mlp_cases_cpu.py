"""The case table of the fused MLP forward / pack sweep (tests/mlp_cases.py), checked on the CPU: the float64 reference agrees with the
project's C oracle and with this package's own torch modules in float64; the table's served set is the library's; the table names 15
forward and 3 pack kernels; every case is well-conditioned for float32 (a numpy float32 forward uses at most a tenth of the bar) and
exposes every mutant of the reference by ten times the bar."""
import os

import numpy as np
import pytest
import torch

import mlp_cases as MC

SPECS = MC.forward_specs()
FORCED = MC.forced16_specs()
ids = MC.spec_id


def test_the_table_accounts_for_every_instantiation():
    t = MC.table()
    assert len(t) == len(SPECS) + len(FORCED) == 3 * 32 + 3 * 32 + 3 * len(MC.MODULAR_SHAPES) + 2 * 32 + 4 * len(MC.FORCED_D)
    default = {MC.forward_kernel(s) for s in SPECS}
    forced = {MC.forward_kernel(s, True) for s in FORCED}
    assert default == ({f"mlp_forward_kernel<{T}, {k}>" for T in (2, 4) for k in MC.KINDS}
                       | {"mlp16_forward_kernel<16, 0>", "mlp16_forward_kernel<16, 1>", "mlp16m_forward_kernel<16>"})
    assert forced == {f"mlp16_forward_kernel<{T}, {a}>" for T in (4, 8) for a in (0, 1)}
    assert len(default) == 11 and len(forced) == 4 and not default & forced
    assert len({fwd for fwd, _ in t.values()}) == 15
    assert {pk for _, pk in t.values()} == {"mlp_pack_kernel", "pack16_kernel", "pack16m_kernel"}
    assert {pk for i, (_, pk) in t.items() if i.startswith("forced16-")} == {"pack16_kernel"}
    # the shapes: every D of the plain kinds, the modular list, and what it is there for
    for kind in ("critic", "plain_actor", "sac_actor"):
        for md in MC.WIDTHS:
            assert {s.D for s in SPECS if s.kind == kind and s.md == md} == (set() if (kind, md) == ("sac_actor", 256) else set(range(1, 33)))
    shapes = set(MC.MODULAR_SHAPES)
    assert all({(s.D, s.Di) for s in SPECS if s.kind == "modular_actor" and s.md == md} == shapes for md in MC.WIDTHS)
    assert {(D - Di) % 4 for D, Di in shapes} == {Di % 4 for D, Di in shapes} == {0, 1, 2, 3}
    assert any(D - Di == 1 for D, Di in shapes) and any(Di == 1 for D, Di in shapes) and any(Di > 1 and D - Di > 1 for D, Di in shapes)
    # the largest first-layer images of the 16-tile modular kernel: nine k-steps of 4 columns over the two towers
    assert max((D - Di + 3) // 4 + (Di + 3) // 4 for D in range(2, 33) for Di in range(1, D)) == 9
    assert {(D, Di) for D, Di in shapes if (D - Di + 3) // 4 + (Di + 3) // 4 == 9} == {(32, 1), (32, 31)}
    assert all(MC.served(*(s.kind, s.md, s.D, s.Di)) for s in SPECS + FORCED)
    assert (MC.BAR, MC.F32_SHARE, MC.MUTATION_MARGIN, MC.M) == (3e-5, 0.1, 10.0, 97)


def test_the_table_matches_the_library():
    """pime_mlp_packed_floats (host-only) over kind x width {32, 64, 128, 256, 512} x D 0..33 x Di 0..D answers a size exactly on the
    table's served set: ActorSAC is refused at width 256, the modular actor needs 1 <= Di < D.  (Without PIME_MLP16 in the environment:
    the forced family changes the image sizes this test also pins.)"""
    if os.environ.get("PIME_MLP16") is not None:
        pytest.fail("PIME_MLP16 is set: the served set of the default process cannot be checked")
    import pime_amd.native as nt
    from pime_amd import ops
    L = nt.lib()
    n = 0
    for kind in MC.KINDS:
        for md in MC.QUERY_WIDTHS:
            for D in range(0, 34):
                for Di in range(0, D + 1):
                    floats = L.pime_mlp_packed_floats(ops._KINDS[kind], D, Di, md)
                    assert (floats > 0) == MC.served(kind, md, D, Di), (kind, md, D, Di, floats)
                    assert floats > 0 or nt.last_error()
                    n += floats > 0
    # critic, plain actor: 3 widths x (D, any Di <= D); ActorSAC: 2 widths; modular actor: 3 widths x (D, 1 <= Di < D)
    assert n == 2 * 3 * 560 + 2 * 560 + 3 * 496
    assert not MC.served("sac_actor", 256, 3, 0) and MC.served("critic", 256, 3, 0)
    assert not MC.served("modular_actor", 128, 3, 0) and not MC.served("modular_actor", 128, 3, 3) and MC.served("modular_actor", 128, 3, 2)
    assert L.pime_mlp_packed_floats(4, 3, 0, 128) == 0 and L.pime_mlp_packed_floats(-1, 3, 0, 128) == 0
    # every case's image holds its parameters and the padding the layouts are known to have
    for s in SPECS:
        params = sum(o * i + o for _, o, i in MC.layer_shapes(s))
        zeros, unwritten = MC.image_padding(s)
        assert L.pime_mlp_packed_floats(ops._KINDS[s.kind], s.D, s.Di, s.md) == params + zeros + unwritten, ids(s)


@pytest.mark.parametrize("kind,Di", [("critic", 0), ("plain_actor", 0), ("modular_actor", 1), ("modular_actor", 2), ("modular_actor", 5)])
def test_reference_agrees_with_the_c_oracle(kind, Di):
    """oracle.critic_forward / plain_actor_mean / modular_actor_mean (double-accumulated dot products, activations rounded to float32
    per layer) to 1e-6 in the form of the bar, |got - want| <= 1e-6 |want| + 1e-6 max(1, max |want|), on the table's own draws, extreme
    rows included.  The distance is the C oracle's: it rounds every activation and its result to float32 (6e-8 each), which the
    critic's draws with one or two input columns amplify most (all hidden units are multiples of one another: the head cancels)."""
    import oracle
    fn = {"critic": oracle.critic_forward, "plain_actor": oracle.plain_actor_mean, "modular_actor": oracle.modular_actor_mean}[kind]
    worst = 0.0
    for md in MC.WIDTHS:
        for D in ((6, 9, 32) if Di else (1, 2, 5, 31, 32)):
            s = MC.Spec(kind, md, D, Di)
            p, x = MC.draw(s)
            want = MC.reference(s, p, x)
            got = (fn(x, p, Di) if Di else fn(x, p))[:, 0].astype(np.float64)
            err = float((np.abs(got - want) / (np.abs(want) + max(1.0, np.abs(want).max()))).max())
            worst = max(worst, err)
            assert err <= 1e-6, (ids(s), err)
    print(f"\nreference against the C oracle, {kind} Di={Di}: worst {worst:.2e}")


def test_the_16_tile_forwards_fit_the_lds_over_the_whole_served_range():
    """launch_fwd16 and the modular branch of launch_forward16 refuse a request above the 160 KB of LDS (PIME_REQUIRE, as launch_fwd
    does); by the kernels' LDS map no served shape gets there.  The largest requests -- (32, 1) and (32, 31) for the modular actor, D
    from 29 on for the plain nets -- are shapes of the GPU sweep, which launches them."""
    plain = {md: max(MC.lds16_forward_bytes(MC.Spec("critic", md, D, 0)) for D in range(1, 33)) for md in MC.WIDTHS}
    assert plain == {64: 4 * (8 * 256 + 260 + 48 + 4096), 128: 4 * (8 * 512 + 516 + 48 + 12288), 256: 4 * (8 * 1024 + 1028 + 48 + 24576)}
    modular = {(D, Di): MC.lds16_forward_bytes(MC.Spec("modular_actor", 256, D, Di)) for D in range(2, 33) for Di in range(1, D)}
    assert max(modular.values()) == 4 * (9 * 1024 + 1284 + 48 + 24576) == 140496
    assert {k for k, v in modular.items() if v == 140496} == {(D, Di) for D in range(30, 33) for Di in range(1, D) if (D - Di + 3) // 4 + (Di + 3) // 4 == 9}
    assert {(32, 1), (32, 31)} <= {k for k, v in modular.items() if v == 140496} and {(32, 1), (32, 31)} <= set(MC.MODULAR_SHAPES)
    assert max(plain.values()) == 135376 and max(plain.values()) <= MC.LDS_LIMIT and max(modular.values()) <= MC.LDS_LIMIT
    assert {s.D for s in SPECS if s.kind == "critic" and s.md == 256} >= {29, 30, 31, 32}


def _module(s):
    from pime_amd.elegantrl.net import ActorSAC, CriticAdv
    from pime_amd.elegantrl.net_residual import ActorResidualIntegratorModularPPO, ActorResidualPPO
    if s.kind == "critic":
        return CriticAdv(s.D, s.md), lambda net, x: net(x)
    if s.kind == "plain_actor":
        return ActorResidualPPO(s.md, s.D, 1), lambda net, x: net.mean(x)
    if s.kind == "modular_actor":
        return ActorResidualIntegratorModularPPO(s.md, s.D, 1, s.Di), lambda net, x: net.mean(x)
    return ActorSAC(s.md, s.D, 1), lambda net, x: net.net_a_avg(net.net_state(x))


@pytest.mark.parametrize("s", [MC.Spec("critic", 64, 5, 0), MC.Spec("plain_actor", 128, 1, 0), MC.Spec("plain_actor", 256, 31, 0),
                               MC.Spec("sac_actor", 64, 1, 0), MC.Spec("sac_actor", 128, 32, 0), MC.Spec("modular_actor", 64, 3, 2),
                               MC.Spec("modular_actor", 128, 9, 5), MC.Spec("modular_actor", 256, 32, 31), MC.Spec("modular_actor", 64, 2, 1),
                               MC.Spec("modular_actor", 256, 30, 15)], ids=ids)
def test_reference_agrees_with_the_packages_modules(s):
    """This package's own torch modules in float64 on the CPU, loaded with the case's parameters: the only other reference ActorSAC
    and integrator_dim > 1 have.  Two float64 evaluations in different summation orders: 1e-12 of the output scale."""
    case = MC.build(s)
    net, fwd = _module(s)
    net = net.double()
    assert s.kind != "modular_actor" or (net.other_dim, net.integrator_dim) == (s.D - s.Di, s.Di)
    with torch.no_grad():
        own = dict(net.named_parameters())
        assert {k for k in own if k not in ("a_std_log", "priorK")} == set(case.params)
        for k, v in case.params.items():
            assert tuple(own[k].shape) == v.shape, k
            own[k].copy_(torch.as_tensor(v.astype(np.float64)))
        got = fwd(net, torch.as_tensor(case.x.astype(np.float64)))[:, 0].numpy()
    assert np.abs(got - case.want).max() <= 1e-12 * max(1.0, np.abs(case.want).max())
    if s.kind == "sac_actor":   # the second head row is there and is not the first
        assert not np.array_equal(case.params["net_a_std.weight"], case.params["net_a_avg.weight"])


@pytest.mark.parametrize("s", SPECS, ids=ids)
def test_case_is_float32_stable_and_exposes_every_mutant(s):
    case = MC.build(s)
    assert case.salt <= MC.MAX_SALT and case.f32_share <= MC.F32_SHARE, f"float32 share {case.f32_share:.3f} after {case.salt} redraws"
    assert case.x.shape == (MC.M, s.D) and case.x.dtype == np.float32 and all(v.dtype == np.float32 for v in case.params.values())
    assert not case.x[0].any() and np.abs(case.x[1]).max() < 0.05
    if s.kind in MC.TANH_KINDS:
        assert set(np.abs(case.x[2])) == {np.float32(1e4)} and set(case.x[3]) == {np.float32(-3e30)} and np.abs(case.x[4:]).max() < 60
    else:
        assert np.abs(case.x[2:]).max() < 60
    assert np.isfinite(case.want).all() and 0.5 < np.abs(case.want).max() < 1e3
    for mutant in MC.mutants_of(s):
        reach = MC.mutant_reach(case, mutant)
        assert reach >= MC.MUTATION_MARGIN, f"{mutant}: reach {reach:.2f} bars"


def test_mutants_apply_where_the_shape_allows():
    assert set(MC.mutants_of(MC.Spec("modular_actor", 64, 3, 1))) == set(MC.MUTANTS_INPUT + MC.MUTANTS_MODULAR + MC.MUTANTS_NET)
    assert "boundary_moved" not in MC.mutants_of(MC.Spec("modular_actor", 64, 2, 1))
    assert MC.mutants_of(MC.Spec("critic", 64, 1, 0)) == ["last_column_dropped", "weight_transposed", "bias_swapped", "relu_tanh"]
    assert set(MC.mutants_of(MC.Spec("sac_actor", 64, 2, 0))) == set(MC.MUTANTS_INPUT + MC.MUTANTS_NET[:2] + MC.MUTANTS_SAC)
    assert set(m for s in SPECS for m in MC.mutants_of(s)) == set(MC.MUTANTS)
    # the forced cases are draws of the table: the same specs, vetted above
    assert set(FORCED) <= set(SPECS)
