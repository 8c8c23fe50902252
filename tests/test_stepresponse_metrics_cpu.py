"""Step-response metrics without a device: the golden protocol records meet the conditions the GPU comparison relies on, the
numpy reference of tests/stepresponse_metrics.py sees every single fault an implementation could make, the package's
`protocols.metrics_from_records` agrees with it, and the C ABI of `pime_rollout_eval_metrics` (exports, row count, argument
errors -- as far as a host without a device gets)."""
import ctypes as C

import numpy as np
import pytest

import stepresponse_metrics as SM
from conftest import load_golden

BANDS = {"ph": 0.05, "wt": 2.0}
TAIL = 10


@pytest.fixture(scope="module")
def records(ph_table_oracle):
    import oracle
    return {"ph": SM.golden_ph_records(load_golden("ph_stepresponse.npz"), ph_table_oracle, oracle.ph_zoh),
            "wt": SM.golden_wt_records(load_golden("wt_stepresponse.npz"))}


@pytest.fixture(scope="module")
def reference(records):
    return {k: SM.reference_metrics(rec, BANDS[k], TAIL)[0] for k, rec in records.items()}


@pytest.mark.parametrize("which", ["ph", "wt"])
def test_no_golden_error_lies_on_the_band(records, which):
    rec, band = records[which], BANDS[which]
    dist = np.abs(np.abs(rec["r"] - rec["y_after"]) - band).min()
    print(f"\n{which}: smallest distance of |e_k| to the band {band}: {dist:.3e}")     # 6.4e-5 (pH), 2.1e-4 (tank)
    assert dist > 1e-6, "an |e_k| on the band would make the settling step depend on the last bits of the trajectory"


def test_golden_records_cover_the_cases_of_the_settling_and_overshoot_rows(records, reference):
    """Over the two files together (the tank, band 2.0, settles in every segment; pH, band 0.05, has the ones that never do)."""
    settled = np.concatenate([(reference[k][:, SM.SETTLING] / records[k]["seg_len"]).ravel() for k in ("ph", "wt")])
    over = np.concatenate([reference[k][:, SM.OVERSHOOT].ravel() for k in ("ph", "wt")])
    assert ((settled > 0) & (settled < 1)).any(), "some segment settles strictly inside"
    assert (settled == 1).any(), "some segment never settles"
    assert (over == 0).any() and (over > 0).any(), "segments without and with overshoot"
    for k in ("ph", "wt"):   # and each file on its own has a segment that settles inside and one with overshoot
        s = reference[k][:, SM.SETTLING]
        assert ((s > 0) & (s < records[k]["seg_len"])).any() and (reference[k][:, SM.OVERSHOOT] > 0).any()


def test_a_tank_band_of_1_6_would_sit_on_a_recorded_error(records):
    rec = records["wt"]
    assert np.abs(np.abs(rec["r"] - rec["y_after"]) - 1.6).min() < 1e-9


@pytest.mark.parametrize("fault", SM.FAULTS)
def test_every_single_fault_moves_a_row_on_the_golden_records(records, reference, fault):
    moved = 0.0
    for which, rec in records.items():
        M = reference[which]
        F = SM.reference_metrics(rec, BANDS[which], TAIL, fault=fault)[0]
        moved = max(moved, float((np.abs(F - M) / np.maximum(np.abs(M), 1e-12))[M != F].max(initial=0.0)))
    print(f"\n{fault}: largest relative move {moved:.3e}")
    assert moved > 1e-6


@pytest.mark.parametrize("which", ["ph", "wt"])
def test_metrics_from_records_agrees_with_the_reference(records, reference, which):
    from pime_amd import protocols
    rec = records[which]
    got = protocols.metrics_from_records(rec["y_after"], rec["r"], rec["action"], rec["reward"], rec["y_start"], seg_len=rec["seg_len"],
                                         band=BANDS[which], tail=TAIL)
    assert tuple(got) == SM.ROWS == tuple(protocols.METRIC_NAMES)
    for j, name in enumerate(SM.ROWS):
        want = reference[which][:, j]
        if j in SM.EXACT_ROWS:
            np.testing.assert_array_equal(got[name], want, err_msg=name)
        else:
            np.testing.assert_allclose(got[name], want, rtol=1e-12, atol=0, err_msg=name)


def test_metrics_from_records_on_a_cut_last_segment_and_without_a_schedule():
    """24 steps in segments of 7 (three whole ones and three steps), and seg_len 0 = one segment: shapes the goldens do not have."""
    from pime_amd import protocols
    rng = np.random.default_rng(5)
    T, N = 24, 6
    for seg_len in (7, 0):
        n_seg = 4 if seg_len else 1
        rec = dict(y_after=rng.normal(5, 2, (T, N)), r=np.repeat(rng.uniform(2, 9, (n_seg, N)), seg_len or T, axis=0)[:T],
                   action=rng.normal(0, 1, (T, N)), reward=rng.normal(-3, 1, (T, N)), y_start=rng.normal(5, 2, (n_seg, N)), seg_len=seg_len)
        want = SM.reference_metrics(rec, 1.0, 5)[0]
        got = protocols.metrics_from_records(rec["y_after"], rec["r"], rec["action"], rec["reward"], rec["y_start"], seg_len=seg_len,
                                             band=1.0, tail=5)
        for j, name in enumerate(SM.ROWS):
            np.testing.assert_allclose(got[name], want[:, j], rtol=0 if j in SM.EXACT_ROWS else 1e-12, atol=0, err_msg=f"{name} seg_len {seg_len}")


# ---- the C ABI, as far as a host without a device gets ----------------------------------------------------------------------
def test_metrics_symbols_are_exported_and_bound():
    import pime_amd.native as nt
    raw = C.CDLL(nt.LIB_PATH)
    for name in ("pime_rollout_eval_metrics_rows", "pime_rollout_eval_metrics"):
        assert hasattr(raw, name) and name in nt.EXPORTS
    assert nt.lib().pime_rollout_eval_metrics_rows() == 8 == nt.METRIC_ROWS == len(SM.ROWS)
    assert tuple(nt.METRIC_NAMES) == SM.ROWS


@pytest.mark.parametrize("band,tail,metrics,word", [(-0.1, 10, True, "band"), (float("nan"), 10, True, "band"), (float("inf"), 10, True, "band"),
                                                    (0.05, 0, True, "tail"), (0.05, -3, True, "tail"), (0.05, 10, False, "metrics")])
def test_each_argument_error_names_its_argument(band, tail, metrics, word):
    """The checks on the new arguments come before anything touches the handle: they answer on a host without a device."""
    import pime_amd.native as nt
    out = np.zeros(8)
    k = np.zeros(4)
    rc = nt.lib().pime_rollout_eval_metrics(None, -1, 0, None, nt.ptr(k), 5, 0, None, 0, band, tail, None, None,
                                            nt.ptr(out) if metrics else None, None)
    assert rc == -1, rc     # PIME_ERR_ARG
    assert word in nt.last_error() and "pime_rollout_eval_metrics" in nt.last_error(), nt.last_error()


def test_a_null_handle_is_an_argument_error():
    import pime_amd.native as nt
    out, k = np.zeros(8), np.zeros(4)
    assert nt.lib().pime_rollout_eval_metrics(None, -1, 0, None, nt.ptr(k), 5, 0, None, 0, 0.05, 10, None, None, nt.ptr(out), None) == -1
    assert "handle" in nt.last_error()
