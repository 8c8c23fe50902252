"""The policy sweep without a GPU: the checker of tests/policy_sweep.py against recordings synthesised in numpy, protocols.select_policy
against its numpy restatement, and the evaluator's snapshot ring.  Shapes: 81 plants at lane offset 1000, five policy rows (rows 0 and
4 the same actor and gain, row 2 with K halved), 23 steps in segments of 9, tail 4, the tank's process noise on.
  1. symbols: header, binding and library agree on the three entry points; the queries refuse a NULL handle;
  2. the checker: honest recordings of five float64 numpy policies pass far inside the bars, each of the six planted faults trips the
     assertion named for it;
  3. select_policy on synthetic summaries: worst / mean, an unsettled plant, NaN, a tie, a case where the nominal and the robust
     choices differ;
  4. the evaluator's snapshot ring with a stub agent: M = 0 records nothing, M = 3 keeps the last three and the nominal best."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import margin_sweep as G
import policy_sweep as S
from conftest import ROOT

NEW_SYMBOLS = ("pime_policy_sweep_supported", "pime_policy_sweep_workspace_bytes", "pime_policy_sweep")


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbols():
    import pime_amd.native as nt
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pime_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pime_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(nt.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in nt.EXPORTS and hasattr(lib, name), name
    for code in (-1, 0, 1, 2, 3):
        assert nt.lib().pime_policy_sweep_supported(None, code, 64) == 0
    assert nt.lib().pime_policy_sweep_workspace_bytes(None, 1, 1, 0) == -1


# ---- 2. the checker --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(ph_table_oracle):
    """(cfg, keep, lanes, policies, gains, honest recording) per env, computed once and left unchanged."""
    out = {}
    for kind in ("ph", "wt"):
        cfg, keep, lanes = G.twin_case(kind, S.N, ph_table_oracle, "f64")
        pols, Ks = S.numpy_policies(kind), S.row_gains(kind)
        out[kind] = (cfg, keep, lanes, pols, Ks, S.numpy_sweep(kind, cfg, lanes, ph_table_oracle, pols, Ks))
    return out


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_honest_recordings_pass_far_inside(cases, ph_table_oracle, kind):
    cfg, _, lanes, pols, Ks, rec = cases[kind]
    use = S.check_recording(kind, cfg, lanes, ph_table_oracle, rec, Ks, [p.term for p in pols], tag=kind)
    assert max(use["trajectory"], use["ret"], use["action"]) <= 0.1, use
    for k in ("pairs", "actions", "outputs"):
        assert S.bits_equal(rec[k][..., 0, :], rec[k][..., 4, :]), "rows 0 and 4 are the same policy"
        assert not S.bits_equal(rec[k][..., 0, :], rec[k][..., 1, :]) and not S.bits_equal(rec[k][..., 1, :], rec[k][..., 2, :])
    assert S.bits_equal(rec["summary"][0], rec["summary"][4])


# fault -> (env, the assertion it trips, what its message names)
FAULT_CASES = {
    "stale_image": ("ph", "image", "row 2 ran the image of row 1"),
    "gain_of_row0": ("wt", "gain", "row 2 ran the prior gain of row 0"),
    "pairs_exchanged": ("ph", "layout", "p and i exchanged"),
    "stride_zero": ("wt", "image", "row 1 ran the image of row 0"),
    "summary_wrong_row": ("ph", "summary", "fold of the call's own pairs"),
    "noise_pair": ("wt", "noise", "keyed on the pair"),
}


def test_every_fault_is_listed():
    assert sorted(FAULT_CASES) == sorted(S.FAULTS) and len(S.FAULTS) == 6


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_each_fault_trips_the_assertion_named_for_it(cases, ph_table_oracle, fault):
    kind, name, words = FAULT_CASES[fault]
    cfg, _, lanes, pols, Ks, _ = cases[kind]
    forged = S.numpy_sweep(kind, cfg, lanes, ph_table_oracle, pols, Ks, fault=fault)
    with pytest.raises(AssertionError) as caught:
        S.check_recording(kind, cfg, lanes, ph_table_oracle, forged, Ks, [p.term for p in pols], tag=kind)
    assert f"[{name}]" in str(caught.value) and words in str(caught.value), str(caught.value)


# ---- 3. select_policy ------------------------------------------------------------------------------------------------------------
def _result(itae_max, itae_mean, settle_max, n=4, steps=20, settled=None, segments=1):
    """A hand-made summary [P, S, 8, 5]: per policy the worst plant's and the mean ITAE and the worst settling step, every segment alike."""
    Pn = len(itae_max)
    s = np.zeros((Pn, segments, 8, 5))
    s[..., S.FINITE] = n
    s[:, :, S.METRIC_NAMES.index("itae"), S.MAX] = np.asarray(itae_max, dtype=np.float64)[:, None]
    s[:, :, S.METRIC_NAMES.index("itae"), S.SUM] = np.asarray(itae_mean, dtype=np.float64)[:, None] * n
    s[:, :, S.METRIC_NAMES.index("itae"), S.ARGMAX] = np.arange(Pn)[:, None] % n
    s[:, :, S.METRIC_NAMES.index("settling_step"), S.MAX] = np.asarray(settle_max, dtype=np.float64)[:, None]
    if settled is None:
        settled = [n if v < steps else n - 1 for v in settle_max]
    return dict(summary=s, settled=np.asarray(settled, dtype=np.int64), pairs=None, steps=steps, n=n)


def _agree(res, **kw):
    from pime_amd import protocols
    got = protocols.select_policy(res, **kw)
    best, nominal, order = S.numpy_select(res["summary"], res["settled"], res["n"], **kw)
    assert (got["best_index"], got["nominal_index"], got["order"].tolist()) == (best, nominal, order), (got, best, nominal, order)
    return got


def test_select_policy_on_synthetic_summaries():
    from pime_amd import protocols
    # the nominal and the robust choices differ: row 1 has the best mean, row 2 the best worst plant
    res = _result(itae_max=[30, 50, 20, 25], itae_mean=[10, 5, 12, 11], settle_max=[5, 5, 5, 5], segments=2)
    got = _agree(res)
    assert (got["best_index"], got["nominal_index"]) == (2, 1) and got["order"].tolist() == [2, 3, 0, 1]
    assert got["worst_cost"].tolist() == [60, 100, 40, 50] and got["mean_cost"].tolist() == [20, 10, 24, 22]
    assert got["worst_plant"].shape == (4, 2) and got["worst_plant"][:, 0].tolist() == [0, 1, 2, 3] and got["fit"].all()
    mean = _agree(res, robust="mean")
    assert mean["best_index"] == 1 == mean["nominal_index"] and mean["cost"].tolist() == [20, 10, 24, 22]
    # an unsettled plant: the cheapest row ranks behind every settled one
    got = _agree(_result([30, 50, 20, 25], [10, 5, 12, 11], settle_max=[5, 5, 20, 5]))
    assert got["best_index"] == 3 and got["order"].tolist() == [3, 0, 1, 2] and got["fit"].tolist() == [True, True, False, True]
    assert got["settled"].tolist() == [4, 4, 3, 4]
    # NaN: a non-finite plant leaves the count short and the row unfit; a NaN cost counts as +inf
    res = _result([30, float("nan"), 20, 25], [10, 5, 12, 11], [5, 5, 5, 5])
    res["summary"][1, 0, S.METRIC_NAMES.index("itae"), S.FINITE] = 3
    res["summary"][2, 0, S.METRIC_NAMES.index("overshoot"), S.FINITE] = 3
    got = _agree(res)
    assert got["best_index"] == 3 and got["order"].tolist() == [3, 0, 2, 1] and got["fit"].tolist() == [True, False, False, True]
    # nobody is fit: the cost alone, then the row
    got = _agree(_result([30, 50, 20, 20], [10, 5, 12, 11], settle_max=[20, 20, 20, 20]))
    assert got["best_index"] == 2 and not got["fit"].any()
    # a tie goes to the lowest row, in both rankings
    got = _agree(_result([20, 50, 20, 20], [7, 5, 12, 5], [5, 5, 5, 5]))
    assert (got["best_index"], got["nominal_index"]) == (0, 1) and got["order"].tolist() == [0, 2, 3, 1]
    for bad in (dict(cost="nope"), dict(robust="median")):
        with pytest.raises(ValueError):
            protocols.select_policy(res, **bad)


# ---- 4. the evaluator's snapshot ring --------------------------------------------------------------------------------------------
class _StubPacked:
    kind, D, Di, md = "modular_actor", 4, 1, 64

    def __init__(self):
        self.packed = torch.zeros(12)


class _StubEnv:
    num_envs, max_step, target_return = 4, 3, 1e9

    def __init__(self, returns):
        self.returns, self.calls = list(returns), 0

    def reset(self):
        return None

    def rollout_eval(self, pk, K, n_steps):
        r = self.returns[min(self.calls, len(self.returns) - 1)]
        self.calls += 1
        return torch.full((self.num_envs,), float(r), dtype=torch.float64), None


class _StubAgent:
    def __init__(self):
        self.act = torch.nn.Linear(2, 1)
        self.pk, self.saved = _StubPacked(), []

    def train_once(self, value):
        with torch.no_grad():
            self.act.weight.fill_(value)
        self.pk.packed.fill_(value)

    def fused_eval_policy(self, env):
        return self.pk, np.array([0.0, -0.4 * float(self.pk.packed[0]), 0.4, 0.0])

    def save_load_model(self, cwd, if_save):
        self.saved.append(float(self.act.weight.detach()[0, 0]))


def _evaluate(checkpoints, returns, tmp_path):
    from pime_amd.elegantrl.run import Evaluator
    env, agent = _StubEnv(returns), _StubAgent()
    ev = Evaluator(cwd=str(tmp_path), agent_id="0", eval_times1=4, eval_times2=4, eval_gap=1, env=env, device="cpu", is_main=True,
                   checkpoints=checkpoints)
    agent.train_once(0.0)
    ev.evaluate_act(agent)
    for j in range(1, len(returns)):
        agent.train_once(float(j))
        ev.evaluate_save(agent, 10, 0.0, 0.0)
    return ev, agent


def test_the_snapshot_ring(tmp_path):
    returns = [-9.0, -5.0, -1.0, -3.0, -4.0, -2.0]          # the nominal best is the third evaluation (step 20)
    ev, agent = _evaluate(0, returns, tmp_path / "a")
    assert ev.snapshots == [] and ev.best_snapshot is None and ev.snapshot_list() == []
    assert agent.saved.count(2.0) == 1, "the nominal-best actor is saved as before"
    ev3, agent3 = _evaluate(3, returns, tmp_path / "b")
    assert [a for a in agent3.saved] == [a for a in agent.saved], "the ring changes nothing the evaluator saves"
    assert [s["step"] for s in ev3.snapshots] == [30, 40, 50] and ev3.best_snapshot["step"] == 20
    snaps = ev3.snapshot_list()
    assert [s["step"] for s in snaps] == [20, 30, 40, 50] and [s["r_avg"] for s in snaps] == [-1.0, -3.0, -4.0, -2.0]
    for s, value in zip(snaps, (2.0, 3.0, 4.0, 5.0)):        # copies of the actor, its image and its gain AS THEY WERE
        assert float(s["state_dict"]["weight"][0, 0]) == value and (s["image"] == value).all() and s["K"][1] == -0.4 * value
        assert s["cls"] == ("modular_actor", 4, 1, 64)
    ev1, _ = _evaluate(1, returns[:3], tmp_path / "c")       # the best one is still in the ring: listed once
    assert [s["step"] for s in ev1.snapshot_list()] == [20]
