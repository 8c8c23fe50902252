"""The prior-gain sweep without a GPU: the HOST build of the pair function the kernel runs (csrc/prior_sweep.hpp compiled into
libpime_sweep_host.so) against the reference loop and the numpy summary of tests/prior_sweep.py, and that checker against itself.
  1. the host library, pH and tank (tank with process noise), N in {1, 63, 64, 65, 130} at env_offset 1000, G = 3 gain rows (the
     env's own -K, 1.7 x it, the error gain's sign flipped), n_steps 23 with seg_len 10 (the last segment cut short) under tail 4
     and tail 50 (larger than any segment) and with seg_len 0: pairs bit-equal to the reference loop over the CPU twin, summary
     bit-equal to the numpy restatement of the call's own pairs, summary without pairs bit-equal to summary with them;
  2. two identical gain rows give identical columns; a NaN gain row: every row it leaves without a finite value has FINITE 0, SUM 0,
     MIN +inf, MAX -inf, ARGMAX -1, and the other gains keep every bit.  (The lane steps clip NaN away -- np.clip semantics: a NaN
     action is -1 for pH, a NaN level is -0 for the tank -- so only the action-variation row of a NaN gain is NaN on every plant;
     the all-NaN case of every row is covered on synthetic pairs in 4.);
  3. every argument error carries its message and leaves summary untouched;
  4. the checker: each of the five single faults trips the assertion named for it;
  5. symbols: header, binding and libraries agree; ABI 26; the package never names the host library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prior_sweep as P
from conftest import ROOT

N_STEPS, OFFSET, SEED, BAND = 23, 1000, 3, 0.05
SCHEDULES = [(10, 4), (10, 50), (0, 4)]   # (seg_len, tail)
NOISE = {"ph": {}, "wt": {"wt_noise_scale": 0.01}}


def _case(kind, N, table, gains=None):
    gains = P.gain_rows(kind) if gains is None else gains
    draws = P.case_draws(kind, N, P.SETPOINTS[kind][0])
    twin = P.make_twin(kind, N, table, SEED, OFFSET, NOISE[kind], draws)
    lanes = P.twin_lanes(twin)
    twin.close()
    return gains, draws, lanes


def _host(kind, lanes, gains, seg_len, tail, table, want_pairs=True):
    return P.host_sweep(kind, lanes, gains, N_STEPS, seg_len, P.SETPOINTS[kind], BAND, tail, want_pairs=want_pairs, table=table, seed=SEED,
                        env_offset=OFFSET, cfg_over=NOISE[kind])


# ---- 1. the host library ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_len,tail", SCHEDULES, ids=lambda v: str(v))
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_host_library_against_the_reference_loop(ph_table_oracle, kind, N, seg_len, tail):
    gains, draws, lanes = _case(kind, N, ph_table_oracle)
    summary, pairs = _host(kind, lanes, gains, seg_len, tail, ph_table_oracle)
    assert not (pairs == -777.0).any() and not (summary == -777.0).any(), "every word is written"
    want = P.twin_pairs(kind, N, gains, N_STEPS, seg_len, P.SETPOINTS[kind], BAND, tail, table=ph_table_oracle, seed=SEED,
                        env_offset=OFFSET, cfg_over=NOISE[kind], draws=draws)
    P.check_pairs(pairs, want, f"{kind} N={N} seg_len={seg_len} tail={tail}")
    P.check_summary(summary, pairs)
    nopairs, none = _host(kind, lanes, gains, seg_len, tail, ph_table_oracle, want_pairs=False)
    assert none is None and P.bits_equal(nopairs, summary), "pairs = NULL must not change a bit of summary"
    assert (summary[..., P.FINITE] == N).all() and np.isfinite(pairs).all()
    if kind == "wt":   # the noise is on: the same plant state without it gives other levels
        quiet = P.host_sweep(kind, lanes, gains, N_STEPS, seg_len, P.SETPOINTS[kind], BAND, tail, table=ph_table_oracle, seed=SEED,
                             env_offset=OFFSET, cfg_over={"wt_noise_scale": 0.0})[1]
        assert not P.bits_equal(quiet, pairs)


# ---- 2. gain rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_identical_gain_rows_give_identical_columns(ph_table_oracle, kind):
    rows = P.gain_rows(kind)
    gains, _, lanes = _case(kind, 65, ph_table_oracle, gains=np.ascontiguousarray(rows[[0, 1, 0, 2, 1]]))
    summary, pairs = _host(kind, lanes, gains, 10, 4, ph_table_oracle)
    assert P.bits_equal(pairs[:, :, 0], pairs[:, :, 2]) and P.bits_equal(pairs[:, :, 1], pairs[:, :, 4])
    assert P.bits_equal(summary[0], summary[2]) and P.bits_equal(summary[1], summary[4])
    assert not P.bits_equal(summary[0], summary[1])


@pytest.mark.parametrize("kind", ["ph", "wt"])
def test_a_nan_gain_row_counts_nothing_and_leaves_the_others_alone(ph_table_oracle, kind):
    rows = P.gain_rows(kind)
    gains, _, lanes = _case(kind, 130, ph_table_oracle, gains=np.ascontiguousarray(np.stack([rows[0], np.full(rows.shape[1], np.nan), rows[1]])))
    summary, pairs = _host(kind, lanes, gains, 10, 4, ph_table_oracle)
    P.check_summary(summary, pairs)
    dead = np.isnan(pairs[:, :, 1]).all(axis=-1)                  # [S, 8]: the rows the NaN gain leaves without a value
    assert dead[:, 7].all(), "the action variation of a NaN action is NaN in every segment of two steps or more"
    got = summary[1][dead]
    assert (got[:, P.FINITE] == 0).all() and P.bits_equal(got[:, P.SUM], np.zeros(len(got))) and (got[:, P.MIN] == np.inf).all()
    assert (got[:, P.MAX] == -np.inf).all() and (got[:, P.ARGMAX] == -1).all()
    clean, _ = _host(kind, lanes, np.ascontiguousarray(gains[[0, 2]]), 10, 4, ph_table_oracle)
    assert P.bits_equal(summary[[0, 2]], clean), "the NaN row must not change a bit of the other gains"


# ---- 3. argument errors ----------------------------------------------------------------------------------------------------------
def test_host_argument_errors(ph_table_oracle):
    bad = []
    for kind in ("wt", "ph"):
        gains, _, lanes = _case(kind, 8, ph_table_oracle)
        sp = np.ascontiguousarray(P.SETPOINTS[kind], dtype=np.float64)
        base = dict(lanes=lanes, N=8, gains=gains, G=3, n_steps=N_STEPS, seg_len=10, sp=sp, n_sp=3, band=BAND, tail=4, summary=True)
        cases = [("G = 0", dict(G=0)), ("2^31 - 1", dict(N=2 ** 20, G=2 ** 12)), ("gains is NULL", dict(gains=None)),
                 ("summary is NULL", dict(summary=False)), ("band", dict(band=-1.0)), ("band", dict(band=float("nan"))),
                 ("band", dict(band=float("inf"))), ("tail 0", dict(tail=0)), ("n_steps 0", dict(n_steps=0)), ("n_setpoints 17", dict(n_sp=17)),
                 ("set-point schedule", dict(n_sp=2)), ("set-point schedule", dict(sp=None)), ("set-point schedule", dict(seg_len=-1)),
                 ("NULL lanes", dict(lanes=None)), ("N = 0", dict(N=0)), ("lane array", dict(lanes={k: v for k, v in lanes.items() if k != "r"})),
                 ("lane array", dict(lanes={k: v for k, v in lanes.items() if k != ("x" if kind == "ph" else "h2")}))]
        for word, over in cases:
            kw = dict(base, **over)
            cfg, keep = P.host_cfg(kind, 8, ph_table_oracle, SEED, OFFSET)
            summary = np.full((3, 3, P.ROWS, P.STATS), -777.0)
            rc, msg = P.host_sweep_raw(kind, cfg, kw["lanes"], kw["N"], kw["gains"], kw["G"], kw["n_steps"], kw["seg_len"], kw["sp"], kw["n_sp"],
                                       kw["band"], kw["tail"], None, summary if kw["summary"] else None)
            if rc != -1 or word not in msg or not (summary == -777.0).all():
                bad.append((kind, word, rc, msg))
    cfg, keep = P.host_cfg("wt", 8, None, SEED, OFFSET, num_stack=1)
    rc, msg = P.host_sweep_raw("wt", cfg, lanes, 8, gains, 3, N_STEPS, 0, None, 0, BAND, 4, None, np.zeros((3, 1, P.ROWS, P.STATS)))
    assert rc == -1 and "Stacking" in msg
    assert not bad, bad


# ---- 4. the checker --------------------------------------------------------------------------------------------------------------
def _synthetic_pairs():
    """[2, 8, 3, 130] values spanning 12 decades in both signs, with a tied maximum, NaN / inf gaps and one all-NaN gain."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, P.ROWS, 3, 130)) * 10.0 ** rng.uniform(-6, 6, (2, P.ROWS, 3, 130))
    x[:, :, 0, 17] = x[:, :, 0, 101] = 1e9          # the maximum, twice: ARGMAX is 17
    x[:, :, 0, 40] = np.nan
    x[:, :, 0, 77] = np.inf
    x[:, :, 2] = np.nan
    return x


FAULT_NAMES = {"plain_sum": "sum", "blocks32": "sum", "argmax_last": "argmax", "nan_counted": "finite"}


def test_every_fault_is_listed():
    assert sorted(list(FAULT_NAMES) + ["noise_pair"]) == sorted(P.FAULTS)   # (noise_pair: the reference loop's fault, below)


def test_the_numpy_summary_on_synthetic_pairs():
    x = _synthetic_pairs()
    s = P.summary_from_pairs(x)
    P.check_summary(s, x)
    assert (s[0, :, :, P.ARGMAX] == 17).all() and (s[0, :, :, P.MAX] == 1e9).all() and (s[0, :, :, P.FINITE] == 128).all()
    dead = s[2]
    assert (dead[..., P.FINITE] == 0).all() and P.bits_equal(dead[..., P.SUM], np.zeros(dead.shape[:-1]))
    assert (dead[..., P.MIN] == np.inf).all() and (dead[..., P.MAX] == -np.inf).all() and (dead[..., P.ARGMAX] == -1).all()
    # the tree by hand on one row: blocks [0, 64), [64, 128), [128, 130)
    v = np.where(np.isfinite(x[1, 3, 1]), x[1, 3, 1], 0.0)
    def tree(w):
        w = list(w) + [0.0] * (64 - len(w))
        while len(w) > 1:
            w = [w[2 * j] + w[2 * j + 1] for j in range(len(w) // 2)]
        return w[0]
    assert s[1, 1, 3, P.SUM] == (tree(v[:64]) + tree(v[64:128])) + tree(v[128:])


@pytest.mark.parametrize("fault", sorted(FAULT_NAMES))
def test_each_summary_fault_trips_the_assertion_named_for_it(fault):
    x = _synthetic_pairs()
    with pytest.raises(AssertionError) as caught:
        P.check_summary(P.summary_from_pairs(x, fault=fault), x)
    assert f"[{FAULT_NAMES[fault]}]" in str(caught.value), str(caught.value)


def test_noise_keyed_on_the_pair_index_trips_the_pairs_assertion(ph_table_oracle):
    gains, draws, lanes = _case("wt", 65, ph_table_oracle)
    _, pairs = _host("wt", lanes, gains, 10, 4, ph_table_oracle)
    args = ("wt", 65, gains, N_STEPS, 10, P.SETPOINTS["wt"], BAND, 4)
    kw = dict(seed=SEED, env_offset=OFFSET, cfg_over=NOISE["wt"], draws=draws)
    P.check_pairs(pairs, P.twin_pairs(*args, **kw))               # honest: passes
    wrong = P.twin_pairs(*args, fault="noise_pair", **kw)
    assert P.bits_equal(wrong[:, :, 0], pairs[:, :, 0]), "gain row 0's pair index IS the plant index"
    with pytest.raises(AssertionError) as caught:
        P.check_pairs(pairs, wrong)
    assert "[pairs]" in str(caught.value)


# ---- 5. symbols ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pime_prior_sweep_supported", "pime_prior_sweep_workspace_bytes", "pime_prior_sweep_stats", "pime_prior_sweep")


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
    assert nt.lib().pime_prior_sweep_stats() == len(nt.SWEEP_STATS) == P.STATS and nt.SWEEP_STATS == P.STAT_NAMES
    assert nt.lib().pime_prior_sweep_supported(None) == 0
    assert nt.lib().pime_prior_sweep_workspace_bytes(None, 1, 1, 0) == -1 and "pime_prior_sweep_workspace_bytes" in nt.last_error()
    host = C.CDLL(P.HOST_LIB_PATH)
    assert _declared("pime_sweep_host.h") == set(P.HOST_EXPORTS)
    for name in P.HOST_EXPORTS:
        assert hasattr(host, name), name
    for name in NEW_SYMBOLS:     # the host library is no second door to the product's entry points
        assert not hasattr(host, name), name


def test_sweep_lanes_layout_matches_the_header(tmp_path):
    import subprocess
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pime_sweep_host.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(pime_sweep_lanes));']
    lines += [f'  printf("{f} %zu\\n", offsetof(pime_sweep_lanes, {f}));' for f, _ in P.SweepLanes._fields_]
    lines += ['  printf("stats %d %d %d %d %d %d\\n", PIME_SWEEP_SUM, PIME_SWEEP_MIN, PIME_SWEEP_MAX, PIME_SWEEP_ARGMAX, PIME_SWEEP_FINITE, '
              'PIME_SWEEP_STATS);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(P.SweepLanes)
    for f, _ in P.SweepLanes._fields_:
        assert int(got[f]) == getattr(P.SweepLanes, f).offset, f
    assert got["stats"].split() == [str(v) for v in (P.SUM, P.MIN, P.MAX, P.ARGMAX, P.FINITE, P.STATS)]


def test_the_package_never_names_the_host_library():
    for d, _, files in os.walk(P.PKG):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(d, f)).read()
                assert "sweep_host" not in text, os.path.join(d, f)


def test_gain_box():
    from pime_amd import protocols
    box = protocols.gain_box([0.0, -0.4, 0.4, 0.0], [0.5, 1.0, 2.0])
    assert box.shape == (9, 4) and (box[:, [0, 3]] == 0).all()
    np.testing.assert_array_equal(box[:4], [[0, -0.2, 0.2, 0], [0, -0.2, 0.4, 0], [0, -0.2, 0.8, 0], [0, -0.4, 0.2, 0]])
    np.testing.assert_array_equal(box[4], [0.0, -0.4, 0.4, 0.0])
    per = protocols.gain_box([0.02, -0.02, -0.035], [[1.0], [1.0, 2.0], [0.5, 1.0, 4.0]])
    assert per.shape == (6, 3) and (per[:, 0] == 0.02).all() and list(per[:, 2]) == [-0.0175, -0.035, -0.14] * 2
    with pytest.raises(ValueError):
        protocols.gain_box([1.0, 2.0], [[1.0]])
