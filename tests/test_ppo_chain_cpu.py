"""The checker of the PPO chain test (tests/ppo_chain.py), on numpy alone: what tests/test_gpu_ppo_chain.py may conclude from a
passing check_chain rests on these conditions.

  1. A clean synthetic recording (float32 oracle gradients, float32 numpy Adam, float32 loss accumulators) passes, and uses at
     most HALF of every derived bound -- every replay_bounds bound and every loss_sums bar.  A condition on the checker: if float32
     numpy itself took more than half of a derived bound, the derivation would be wrong, not the cap.
  2. Every fault of ppo_chain.FAULTS trips the assertion named for it, on every deterministic-route spec; on the split pipeline
     every fault that does not rest on the bit-equality of two gradients.
  3. The index tables hold what they promise, and the specs' routes are the library model's."""
import functools

import numpy as np
import pytest

import ppo_cases as PC
import ppo_chain as CH

B3_SPECS = [s for f16 in (False, True) for s in CH.b3_chain_specs(f16)]   # the bf16x3 variant's chains: the same checker
SPECS = CH.chain_specs() + [s for s in B3_SPECS if s not in CH.chain_specs()]
MAX_SHARE = 0.5


def _id(s):
    """(a spec of the variant under PIME_MLP16=1 differs from the default process's in its route alone)"""
    return PC.spec_id(s) + ("-mlp16" if s not in CH.chain_specs() and s in CH.b3_chain_specs(True) else "")


@functools.lru_cache(maxsize=None)
def _case(s):
    case = PC.build(s)
    return case, CH.index_table(case)


def test_the_spec_list():
    ids = [_id(s) for s in SPECS]
    assert len(set(ids)) == len(ids) and all(s.B == CH.B == 293 and s.vet for s in SPECS)
    assert {(s.route, s.aw, s.cw) for s in PC.per_route_shapes()} <= {(s.route, s.aw, s.cw) for s in SPECS}
    for want in (("modular", 3, 1, 128), ("modular", 4, 1, 64), ("modular", 4, 1, 256), ("plain", 30, 0, 256)):
        assert any((s.kind, s.D, s.Di, s.aw) == want and s.cw == s.aw for s in SPECS), want
    assert any(not CH.deterministic(s) for s in SPECS) and sum(CH.deterministic(s) for s in SPECS) >= 10
    for s in CH.chain_specs():
        assert s.route == PC.expected_route(s.kind, s.D, s.Di, s.aw, s.cw)
    for f16 in (False, True):
        for s in CH.b3_chain_specs(f16):
            assert s.route == PC.expected_route(s.kind, s.D, s.Di, s.aw, s.cw, f16, b3=True) and any(PC.b3_nets(s, f16))
            assert s.B == CH.B and s.vet
    assert len(CH.b3_chain_specs()) == 8 and len(CH.b3_chain_specs(True)) == 3
    assert [CH.deterministic(s) for s in CH.b3_chain_specs()].count(False) == 1   # the split-pipeline actor next to a B3 critic
    assert PC.spec("modular", 3, 1, 128, CH.B).route == ("lds", "lds", "pair")   # the bench's nets: the pair kernel


@pytest.mark.parametrize("s", SPECS, ids=_id)
def test_index_tables(s):
    case, table = _case(s)
    assert table.shape == (CH.K, s.B) and table.dtype == np.int64 and CH.K == 4
    assert np.array_equal(table[0], case.idx)
    assert table.min() >= 0 and table.max() < PC.N_ROWS
    for k in range(1, CH.K):
        assert (table[k] == table[k - 1]).any(), f"row {k} repeats no index of the row before"
        assert np.array_equal(table[k] % 10, np.arange(s.B) % 10), "a position left its combination of ratio category and branch"
        assert len(np.unique(table[k])) > s.B // 2
    assert not np.array_equal(table[1], table[2])


@pytest.mark.parametrize("s", SPECS, ids=_id)
def test_a_clean_recording_passes_with_half_of_every_bound_to_spare(s):
    case, table = _case(s)
    used = CH.check_chain(CH.synthesise(case, table), case, table)
    capped = {k: v for k, v in used.items() if k.startswith(("adam ", "loss_sums"))}
    assert len(capped) == 3 + 5, sorted(capped)
    for k, v in sorted(used.items()):
        print(f"ppo chain cpu {PC.spec_id(s)} {k}: {v:.3f}")
    for k, v in capped.items():
        assert v <= MAX_SHARE, f"{PC.spec_id(s)}: float32 numpy uses {v:.3f} of the bound '{k}'"


@pytest.mark.parametrize("s", SPECS, ids=_id)
def test_every_fault_trips_its_assertion(s):
    case, table = _case(s)
    for fault, name in CH.FAULTS.items():
        if not CH.deterministic(s) and fault in CH.BIT_EQUALITY_FAULTS:
            continue
        with pytest.raises(CH.ChainError) as exc:
            CH.check_chain(CH.synthesise(case, table, fault), case, table)
        assert name in exc.value.failed, f"{fault}: tripped {list(exc.value.failed)}, not '{name}'"
        if fault in CH.ALSO_TRIPS:
            assert CH.ALSO_TRIPS[fault] in exc.value.failed, fault
        assert "gradient_oracle" not in exc.value.failed, f"{fault}: step 0 is before every fault"


def test_subtle_faults_trip_nothing_but_their_own_assertion():
    """The faults that the loose whole-update bar lets through are seen by exactly the assertion that is about them: a gradient
    read at stale images leaves Adam's replay (of the gradient the step really used) and every counter in order
    (at lr 1e-3 the loss sums at weights one step old leave their 2e-4 bar as well)."""
    case, table = _case(PC.spec("modular", 3, 1, 128, CH.B))
    for fault, only in (("stale_images_gradient", {"gradient_fresh", "loss_sums"}), ("forward_image_stale", {"images"}),
                        ("critic_scaled_with_previous_rows_scale", {"gradient_fresh"})):
        with pytest.raises(CH.ChainError) as exc:
            CH.check_chain(CH.synthesise(case, table, fault), case, table)
        assert set(exc.value.failed) <= only, (fault, list(exc.value.failed))


def test_dp_replay_bounds_only_widen():
    rng = np.random.RandomState(3)
    g, m = rng.standard_normal(64), rng.standard_normal(64)
    rep = {"param": rng.standard_normal(64), "exp_avg_sq": g * g}
    plain, dp = CH.replay_bounds(rep, m, g, 1e-3), CH.dp_replay_bounds(rep, m, g, 1e-3)
    for key in ("param", "exp_avg", "exp_avg_sq"):
        assert (dp[key] >= plain[key]).all() and (dp[key] <= 2.0 * plain[key]).all(), key
