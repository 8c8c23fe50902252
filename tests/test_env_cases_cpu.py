"""The case table, scenario and checker of the env kernel sweep (tests/env_cases.py), vetted without a GPU: the table is the kernels'
instantiation list, the scenario produces what it claims, the checker passes a correct device (the oracle rounded as a device rounds, and
the product's host build) and fails each of a list of defects planted in one lane at one launch."""
import numpy as np
import pytest

import env_cases as EC

CASES = EC.cases()
F16 = np.float16
# launches of the scenario: 0 reset, 1..5 free steps, 6 masked reset, 7..28 auto steps (group B ends on 8, 15, 22; A on 13, 20, 27),
# 29 observe, 30 the last step
MASKED, A_ENDS, B_ENDS, LAST = 6, (13, 20, 27), (8, 15, 22), 30


def _case(env, ns, entry, action):
    c = EC.Case(env, ns, entry, action)
    assert c in CASES
    return c


def _clean(c, table, sc=None):
    sc = sc or EC.scenario()
    dev, record = EC.FakeDevice(c, sc, table), []
    share = EC.run_scenario(dev, c, sc, table, record=record)
    return dev, record, share


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_is_the_instantiation_list():
    assert len(CASES) == 55 == len(set(CASES))
    assert EC.instantiations() == [("double", "double", "float"), ("float", "float", "float"), ("float", "half_t", "float"),
                                   ("float", "half_t", "half_t")]
    assert EC.step_forms() == [("double", "false"), ("float", "false"), ("float", "true")] and not EC.half_takes_float64_action()
    for env, ns in EC.HANDLES:
        mine = [(c.entry, c.action) for c in CASES if (c.env, c.num_stack) == (env, ns)]
        assert sorted(mine) == sorted([(e, a) for e in ("f64", "mixed", "mixed16") for a in ("a64", "a32", "residual")]
                                      + [("mixed16_h", "a32"), ("mixed16_h", "residual")])
    assert {ns for env, ns in EC.HANDLES if env == "wt"} == {0, 1, 4, 10}


# ------------------------------------------------------------------------------------------------ the scenario
@pytest.mark.parametrize("c", [_case("ph", 0, "f64", "a64"), _case("wt", 0, "f64", "a32"), _case("wt", 4, "f64", "a64"),
                               _case("wt", 10, "f64", "residual")], ids=EC.case_id)
def test_the_scenario_produces_what_it_claims(c, ph_table_oracle):
    sc = EC.scenario()
    assert (sc.N, sc.max_step, sc.resample_every) == (193, 7, 2) and sc.env_offset != 0 and sc.max_step % 4 and sc.max_step % 10
    mask = EC.lane_mask(sc).astype(bool)
    assert mask[0] and not mask[-1] and 0.35 < mask.mean() < 0.65
    _, rec, _ = _clean(c, ph_table_oracle)
    assert [r["kind"] for r in rec] == ["reset"] + ["step"] * 5 + ["reset"] + ["step"] * 22 + ["observe", "step"]
    assert rec[MASKED]["selected"].tolist() == mask.tolist()
    ends = {r["launch"]: r["done"] for r in rec if r["kind"] == "step" and r["done"].any()}
    assert sorted(ends) == sorted(A_ENDS + B_ENDS + (LAST,))            # the two groups end on different launches, three times each
    assert all((ends[k] == mask).all() for k in A_ENDS) and all((ends[k] == ~mask).all() for k in B_ENDS + (LAST,))
    assert not rec[LAST]["auto"] and (rec[LAST]["episode"] == rec[LAST]["episode_before"]).all()      # ... and B's last end is not reset
    kept = resampled = odd_head = 0
    for prev, r in zip(rec, rec[1:]):
        if r["kind"] == "observe":
            continue
        fresh = r["episode"] != r["episode_before"]
        if not fresh.any():
            continue
        new_plant = r["episode"][fresh] % sc.resample_every == 0
        assert ((r["plant"][fresh] != prev["plant"][fresh]) == new_plant).all()
        resampled += int(new_plant.sum())
        kept += int((~new_plant).sum())
        if c.num_stack:   # the ring head a reset meets: one slot per step since the last reset
            odd_head += int((r["t_before"][fresh] % c.num_stack != 0).sum())
    assert kept and resampled
    if c.num_stack in (4, 10):
        assert odd_head >= mask.sum()


# ------------------------------------------------------------------------------------------------ a correct device passes
@pytest.mark.parametrize("c", CASES, ids=EC.case_id)
def test_the_checker_passes_the_fake_device(c, ph_table_oracle):
    _, rec, share = _clean(c, ph_table_oracle)
    assert len(rec) == 31 and all(np.isfinite(v) and v <= 1.0 for v in share.values())
    print("\n" + EC.share_line(c, EC.scenario(), share) + " fake")


@pytest.mark.parametrize("c", [c for c in CASES if c.entry == "f64" and EC.has_I(c)], ids=EC.case_id)
def test_the_checker_passes_the_host_build_of_the_lanes(c, ph_table_oracle):
    sc = EC.scenario()
    share = EC.run_scenario(EC.TwinDevice(c, sc, ph_table_oracle), c, sc, ph_table_oracle)
    print("\n" + EC.share_line(c, sc, share) + " twin")


def test_windows_of_the_scenario_are_its_lanes(ph_table_oracle):
    """A device that holds lanes g0 .. g0 + n - 1 gets their actions and their part of the mask (the GPU test compares handles with it)."""
    c = _case("wt", 4, "mixed16_h", "residual")
    _, full, _ = _clean(c, ph_table_oracle)
    for win in ((100, 1), (130, 63)):
        _, part, _ = _clean(c, ph_table_oracle, EC.scenario(window=win))
        for a, b in zip(full, part):
            assert np.array_equal(EC.bits(a["obs"][win[0]:win[0] + win[1]]), EC.bits(b["obs"]))


# ------------------------------------------------------------------------------------------------ a defective one does not
S4 = _case("wt", 4, "mixed", "a64")
PH_H = _case("ph", 0, "mixed16_h", "a32")
LANE_A, LANE_B = 0, 192          # a selected and an unselected lane of the masked reset


def _fails(c, table, match, **mutate):
    sc = EC.scenario()
    with pytest.raises(AssertionError, match=match):
        EC.run_scenario(EC.FakeDevice(c, sc, table, mutate=mutate), c, sc, table)


def test_ring_not_reheaded_on_reset(ph_table_oracle):
    _fails(S4, ph_table_oracle, "masked reset: ring head", name="ring_not_reheaded", launch=MASKED, lane=LANE_A)       # head 5 % 4
    _fails(S4, ph_table_oracle, "auto step 7: ring head", name="ring_not_reheaded", launch=A_ENDS[0], lane=LANE_A)     # head 6 % 4
    _fails(_case("wt", 10, "mixed16_h", "a32"), ph_table_oracle, "ring head", name="ring_not_reheaded", launch=B_ENDS[0], lane=LANE_B)


def test_ring_read_out_rotated_by_one_slot(ph_table_oracle):
    _fails(S4, ph_table_oracle, "free step 2: ", name="ring_rotated", launch=3, lane=77)
    _fails(_case("wt", 10, "f64", "residual"), ph_table_oracle, "auto step 3: ", name="ring_rotated", launch=MASKED + 3, lane=LANE_B)


@pytest.mark.parametrize("c", [S4, PH_H, _case("wt", 0, "mixed16", "a64")], ids=EC.case_id)
def test_masked_reset_writes_an_unselected_row_or_skips_a_selected_lane(c, ph_table_oracle):
    D = EC.obs_dim(c)
    _fails(c, ph_table_oracle, "masked reset: obs: a row that must stay untouched", name="poke", launch=MASKED, buf="obs", index=LANE_B * D + D - 1,
           value=0.0)
    _fails(c, ph_table_oracle, "masked reset: obs: unwritten words in written rows", name="selected_skipped", launch=MASKED, lane=LANE_A)


@pytest.mark.parametrize("c", [_case("ph", 0, "mixed", "a32"), _case("wt", 0, "mixed16_h", "residual"), _case("ph", 0, "f64", "a64")],
                         ids=EC.case_id)
def test_integrator_carried_across_a_reset(c, ph_table_oracle):
    _fails(c, ph_table_oracle, "masked reset: the reset rows", name="I_carried", launch=MASKED, lane=LANE_A)
    _fails(c, ph_table_oracle, "auto step 2: the rows of an auto-reset", name="I_carried", launch=B_ENDS[0], lane=LANE_B)


def test_episode_not_advanced(ph_table_oracle):
    _fails(PH_H, ph_table_oracle, "masked reset: episode", name="episode_stuck", launch=MASKED, lane=LANE_A)


def test_done_missing_on_an_auto_reset_step(ph_table_oracle):
    _fails(S4, ph_table_oracle, "auto step 7: done", name="done_missing", launch=A_ENDS[0], lane=LANE_A)


@pytest.mark.parametrize("c", [PH_H, _case("wt", 10, "mixed16_h", "a32")], ids=EC.case_id)
def test_binary16_word_one_ulp_outside_its_interval(c, ph_table_oracle):
    """Every word of a row, at its interval's two ends: the end itself passes, its neighbour outside does not."""
    D, lane, k = EC.obs_dim(c), 77, 3
    _, rec, _ = _clean(c, ph_table_oracle)
    bar = 3e-5 if c.env == "ph" else 2e-4
    for col in range(0, D, 3 if c.num_stack else 1):
        lo, hi = EC.half_interval(rec[k]["want64"][lane, col], bar, bar)
        assert lo <= rec[k]["obs"][lane, col] <= hi
        for end, away in ((lo, -np.inf), (hi, np.inf)):
            out = np.nextafter(F16(end), F16(away))
            _fails(c, ph_table_oracle, "free step 2: .*binary16 interval", name="poke", launch=k, buf="obs", index=lane * D + col, value=out)
    lo, hi = EC.half_interval(rec[k]["want_reward"][lane], bar, bar)
    assert lo <= rec[k]["reward"][lane] <= hi
    _fails(c, ph_table_oracle, "free step 2: reward", name="poke", launch=k, buf="reward", index=lane, value=np.nextafter(hi, F16(np.inf)))


@pytest.mark.parametrize("c", [_case("ph", 0, "mixed16", "a64"), _case("ph", 0, "mixed16_h", "residual")], ids=EC.case_id)
def test_integrator_rounded_to_binary16_twice(c, ph_table_oracle):
    """float32 -> 12 bits -> binary16 instead of float32 -> binary16, at the first (launch, lane) sites where that gives another
    word than the direct rounding and the float32 value is farther from the tie than the bar (nearer, a float32 error could do the same).  pH only: the tank's bar, 2e-4
    relative, is wider than the quarter of a binary16 step (1.2e-4 .. 2.4e-4 relative) such a value can lie above its tie, so there the
    bar itself admits the second rounding."""
    dev, _, _ = _clean(c, ph_table_oracle)
    bar = 3e-5 if c.env == "ph" else 2e-4
    sites = []
    for k in sorted(dev.pre_I):
        v = dev.pre_I[k]
        twice, lo, hi = EC.round_twice(v), *EC.half_interval(v, 1.1 * bar, 1.1 * bar)
        sites += [(k, int(i)) for i in np.nonzero((twice != v.astype(F16)) & ((twice < lo) | (twice > hi)))[0]]
    assert len(sites) >= 3, sites
    for k, lane in sites[:3]:
        _fails(c, ph_table_oracle, "step .*binary16 interval", name="I_rounded_twice", launch=k, lane=lane)


@pytest.mark.parametrize("buf", ["obs", "reward", "done"])
def test_word_written_past_the_last_lane(buf, ph_table_oracle):
    c = S4
    size = 193 * (EC.obs_dim(c) if buf == "obs" else 1)
    _fails(c, ph_table_oracle, f"auto step 4: {buf}: a word behind the buffer", name="poke", launch=MASKED + 4, buf=buf, index=size, value=0)
    _fails(c, ph_table_oracle, f"last step: {buf}: a word behind the buffer", name="poke", launch=LAST, buf=buf, index=size + EC.GUARD - 1, value=0)
    if buf == "obs":
        _fails(c, ph_table_oracle, "observe: observe: a word behind the buffer", name="poke", launch=29, buf="obs", index=size, value=0)
        _fails(c, ph_table_oracle, "reset: obs: a word behind the buffer", name="poke", launch=0, buf="obs", index=size + 1, value=0)


def test_observe_that_differs_from_the_last_row(ph_table_oracle):
    _fails(PH_H, ph_table_oracle, "observe: observe\\(\\) repeats", name="poke", launch=29, buf="obs", index=3 * 50 + 2, value=0.125)
