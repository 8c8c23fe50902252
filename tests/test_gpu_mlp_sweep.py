"""Every instantiation of the fused MLP forward and pack kernels (`pime_mlp_pack` / `pime_mlp_forward`: mlp_pack_kernel and
mlp_forward_kernel of csrc/mlp_mfma.hip, pack16_kernel / pack16m_kernel / mlp16_forward_kernel / mlp16m_forward_kernel of
csrc/mlp16.hip) against the float64 reference of tests/mlp_cases.py (vetted on the CPU by tests/test_mlp_cases_cpu.py: which kernels
the test ids name, the bar, and which faults of a forward the cases see), and the trajectory scan (gae_scan_kernel of csrc/gae_scan.hip)
bitwise against the oracle on the shapes its launcher and its chunked loop branch on.

  test_forward_matches_the_reference[id]      the 11 instantiations of a default process, every shape of the table, 97 rows
  test_forced_16_tile_widths_64_and_128       mlp16_forward_kernel<{4,8}, {0,1}> in ONE child process with PIME_MLP16=1 (the switch is
                                              read once per process), ids forced16-*
  test_the_image_is_the_parameters            what the three pack kernels write, and what a second repack() changes
  test_row_counts_at_the_launch_edges         the grid rules of launch_fwd / launch_fwd16: rows that repeat a verified 97-row base are
                                              bit-equal to it whatever tile, wave or workgroup computes them
  test_a_nan_row_stays_alone                  a NaN observation gives a NaN output in its row and changes no other row
  test_the_served_set_on_the_device           refused shapes return PIME_ERR_ARG with a message and touch neither image nor out
  test_gae_scan_at_the_launch_and_chunk_edges
Instruments: the image buffer is NaN-filled before repack() (a forward that reads a float no pack kernel wrote cannot stay finite),
`out` carries 64 extra floats preset to a sentinel, and the scan's outputs are allocated NaN-filled.

Every forward case prints one "SHARE" line: the largest used share of the bar over its rows.  Largest per family on an MI355X (all
292 + 24 cases; the numpy float32 forward of the same case beside it):
    32x32x2, mlp_forward_kernel          0.069  critic-64-D1 (float32: 0.072); per kind: critic 0.069, plain 0.019, modular 0.019,
                                                ActorSAC 0.033
    16-tile, mlp16_forward_kernel        0.061  forced16-critic-64-D1 (0.072); width 256: 0.037 plain_actor-256-D1 (0.027)
    16-tile, mlp16m_forward_kernel<16>   0.020  modular_actor-256-D4-Di1
The kernels use what float32 itself uses of the bar; the bar is left where it stands.  The row-count and NaN-row tests hold bit for
bit on the hardware: no row depends on where it is computed.

What the sweep found: the ReLU kinds returned a finite value for a NaN row (`v > 0 ? v : 0` is v_max_f32, which drops a NaN);
pime_mlp_forward now keeps it (csrc/mlp_device.hpp: kActReluNan).  Nothing else: every shape, padding, row count and image float held.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL, SENTINEL = 64, -7777.25
ERR_ARG = -1   # PIME_ERR_ARG (include/pime_hip.h)
SPECS = MC.forward_specs()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the cases' arrays are read-only)


def _device_params(params):
    return {k: _dev(v) for k, v in params.items()}


def _pack(s, params, forced16=False):
    """PackedMLP of the spec, re-packed into a NaN-filled image; the image's size tells which family serves."""
    from pime_amd import ops
    pk = ops.PackedMLP.from_state_dict(s.kind, _device_params(params), state_dim=s.D, integrator_dim=s.Di)
    assert pk.md == s.md
    zeros, unwritten = MC.image_padding(s, forced16)
    assert pk.packed.numel() == sum(v.size for v in params.values()) + zeros + unwritten, "the image is not this family's"
    pk.packed.fill_(float("nan"))
    pk.repack()
    return pk


def _forward(pk, x):
    """out[:M] and the sentinel tail behind it, as numpy."""
    x = x if torch.is_tensor(x) else _dev(x)
    out = torch.full((x.shape[0] + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    pk(x, out=out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[x.shape[0]:] == np.float32(SENTINEL)).all(), "out was written beyond M"
    return out[:x.shape[0]]


def check_case(s, forced16=False):
    case = MC.build(s)
    got = _forward(_pack(s, case.params, forced16), case.x)
    used = MC.share(got, case.want)
    print(f"\nSHARE kernel={MC.forward_kernel(s, forced16)} id={MC.spec_id(s, forced16)} share={used:.4f} "
          f"float32={case.f32_share:.4f} salt={case.salt} scale={np.abs(case.want).max():.3g}")
    assert np.isfinite(got).all(), f"rows {np.flatnonzero(~np.isfinite(got))[:8]} are not finite"
    assert used <= 1.0, f"row {int(np.argmax(np.abs(got - case.want) / MC.bar(case.want)))} uses {used:.2f} of the bar"
    return used


@pytest.mark.parametrize("s", SPECS, ids=MC.spec_id)
def test_forward_matches_the_reference(s):
    assert os.environ.get("PIME_MLP16") is None, "PIME_MLP16 is set: this process does not run the default instantiations"
    check_case(s)


_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["PIME_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PIME_ROOT"], "tests"))
import mlp_cases as MC
import test_gpu_mlp_sweep as t
for s in MC.forced16_specs():
    t.check_case(s, forced16=True)
for s in t.FORCED_ROWS:
    t.check_rows(s, forced16=True)
print("MLP_SWEEP_FORCED_OK")
'''


def test_forced_16_tile_widths_64_and_128():
    """mlp16_forward_kernel<4, 0>, <4, 1>, <8, 0>, <8, 1> and pack16_kernel at those widths, at D in {1, 2, 3, 5, 29, 32}: the image
    size asserted by check_case is the 16-tile layout's, so a child that did not take the forced route fails.  The child also runs the
    row counts of test_row_counts_at_the_launch_edges on two of those instantiations."""
    env = dict(os.environ, PIME_ROOT=ROOT, PIME_MLP16="1")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "MLP_SWEEP_FORCED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    for s in MC.forced16_specs():
        assert f"id={MC.spec_id(s, True)} " in r.stdout


# ---- the image ------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


@pytest.mark.parametrize("s,touched", [(MC.Spec("critic", 64, 5, 0), "net.2.bias"), (MC.Spec("plain_actor", 128, 3, 0), "net.0.weight"),
                                       (MC.Spec("modular_actor", 64, 5, 2), "integrator_net.0.weight"),
                                       (MC.Spec("sac_actor", 128, 7, 0), "net_a_std.weight"), (MC.Spec("critic", 256, 5, 0), "net.0.weight"),
                                       (MC.Spec("plain_actor", 256, 30, 0), "net.6.bias"),
                                       (MC.Spec("modular_actor", 256, 5, 2), "other_net.2.weight")], ids=lambda v: MC.spec_id(v) if isinstance(v, MC.Spec) else v)
def test_the_image_is_the_parameters(s, touched):
    """Index-coded parameters (1, 2, 3, ... over the tensors in pack order: all distinct, none zero) into a NaN-filled image: every value
    occurs exactly once, every other float is 0.0 or still NaN, as many of each as the layout's padding (tests/mlp_cases.py:
    image_padding).  ActorSAC's second head row, which no forward reads, is in the image.  After one tensor changed, a second repack()
    changes exactly the floats that held it."""
    from pime_amd import ops
    params, n = {}, 0
    for name, o, i in MC.layer_shapes(s):
        for key, shape in ((name + ".weight", (o, i)), (name + ".bias", (o,))):
            size = int(np.prod(shape))
            params[key] = (1 + n + np.arange(size)).astype(np.float32).reshape(shape)
            n += size
    assert n < 2 ** 23
    sd = _device_params(params)
    pk = ops.PackedMLP.from_state_dict(s.kind, sd, state_dim=s.D, integrator_dim=s.Di)
    pk.packed.fill_(float("nan"))
    pk.repack()
    torch.cuda.synchronize()
    img = pk.packed.cpu().numpy()
    zeros, unwritten = MC.image_padding(s)
    assert img.size == n + zeros + unwritten
    held = img[~np.isnan(img)]
    assert np.array_equal(np.sort(held[held != 0]), np.arange(1, n + 1, dtype=np.float32)), "a parameter is missing or repeated"
    assert int(np.isnan(img).sum()) <= unwritten and int((held == 0).sum()) + int(np.isnan(img).sum()) == zeros + unwritten
    before = _bits(pk.packed)
    sd[touched].add_(0.5)   # k + 0.5: exact in float32, equal to no other parameter
    pk.repack()
    torch.cuda.synchronize()
    changed = _bits(pk.packed) != before
    assert np.array_equal(changed, np.isin(img, params[touched].reshape(-1)))
    assert np.array_equal(np.sort(pk.packed.cpu().numpy()[changed]), np.sort(params[touched].reshape(-1) + np.float32(0.5)))


# ---- row counts -------------------------------------------------------------------------------------------------------------------
# launch_fwd (csrc/mlp_mfma.hip): tiles of 32 rows; one tile per workgroup below 256 tiles, 256 workgroups up to 512 tiles, then 8 tiles per
# workgroup, and the persistent loop from 256 x 8 tiles on.  launch_fwd16 / launch_forward16 (csrc/mlp16.hip): groups of 64 rows on at most
# 256 workgroups at width 256 (one per CU), 512 at widths 64 / 128.
ROWS_32 = (1, 31, 32, 33, 8160, 8192, 8193, 16384, 16385, 65536, 65537, 65536 + 8 * 32 + 1)
ROWS_16 = (1, 15, 16, 17, 63, 64, 65, 16384, 16385, 32768, 32769)


FORCED_ROWS = (MC.Spec("critic", 128, 5, 0), MC.Spec("plain_actor", 64, 3, 0))   # the 512-workgroup cap exists at widths 64 / 128 only


def check_rows(s, forced16=False):
    case = MC.build(s)
    pk = _pack(s, case.params, forced16)
    base = _forward(pk, case.x)
    assert MC.share(base, case.want) <= 1.0
    x97 = _dev(case.x)
    for rows in (ROWS_16 if MC.family16(s, forced16) else ROWS_32):
        src = np.arange(rows) % MC.M
        got = _forward(pk, x97[_dev(src)])
        differ = np.flatnonzero(got.view(np.int32) != base[src].view(np.int32))
        assert differ.size == 0, f"M = {rows}: rows {differ[:8]} differ from the 97-row call ({differ.size} in all)"


@pytest.mark.parametrize("s", [MC.Spec("critic", 128, 5, 0), MC.Spec("plain_actor", 64, 3, 0), MC.Spec("modular_actor", 128, 6, 3),
                               MC.Spec("sac_actor", 64, 9, 0), MC.Spec("critic", 256, 5, 0), MC.Spec("plain_actor", 256, 30, 0),
                               MC.Spec("modular_actor", 256, 9, 5)], ids=MC.spec_id)
def test_row_counts_at_the_launch_edges(s):
    """Row i of an M-row call is bit-equal to row i % 97 of the verified 97-row call: a row's arithmetic does not depend on the tile,
    wave or workgroup that computes it, and nothing is written beyond M.  (The 16-tile family at widths 64 / 128, whose cap of 512
    workgroups is the 32768-row edge: FORCED_ROWS in the child process of test_forced_16_tile_widths_64_and_128.)"""
    check_rows(s)


@pytest.mark.parametrize("s", [MC.Spec("plain_actor", 128, 5, 0), MC.Spec("critic", 64, 5, 0), MC.Spec("modular_actor", 64, 6, 3),
                               MC.Spec("sac_actor", 128, 5, 0), MC.Spec("plain_actor", 256, 5, 0), MC.Spec("critic", 256, 5, 0),
                               MC.Spec("modular_actor", 256, 6, 3)], ids=MC.spec_id)
def test_a_nan_row_stays_alone(s):
    """Row 40 of x set to NaN, and the last column alone of row 41 (inside a full tile of either family: their neighbours sit on the
    same wave): their outputs are NaN, as the torch modules give (ReLU and Hardswish hand a NaN on as Tanh does), and every other row
    is bit-equal to the run without them."""
    case = MC.build(s)
    pk = _pack(s, case.params)
    base = _forward(pk, case.x)
    x = case.x.copy()
    x[40] = np.nan
    x[41, -1] = np.nan
    got = _forward(pk, x)
    assert np.isnan(got[40]) and np.isnan(got[41]), f"the NaN rows came out as {got[40]}, {got[41]}"
    keep = ~np.isin(np.arange(MC.M), (40, 41))
    assert np.array_equal(got[keep].view(np.int32), base[keep].view(np.int32))


# ---- the served set -----------------------------------------------------------------------------------------------------------------
def test_the_served_set_on_the_device():
    """What tests/test_mlp_cases_cpu.py holds pime_mlp_packed_floats to, asked of the two launching entry points with live device
    buffers: a refused (kind, D, Di, width) and M = 0 return PIME_ERR_ARG with a message, and neither the image nor out is written."""
    from pime_amd import native, ops
    lib = native.lib()
    refused = [(k, md, D, Di) for k in MC.KINDS for md in MC.QUERY_WIDTHS for D in (0, 1, 3, 32, 33) for Di in (0, 1, D - 1, D)
               if 0 <= Di <= D and not MC.served(k, md, D, Di)]
    assert {(k, md) for k, md, _, _ in refused} >= {("sac_actor", 256), ("critic", 32), ("modular_actor", 512)}
    assert ("modular_actor", 128, 3, 0) in refused and ("modular_actor", 128, 3, 3) in refused and ("plain_actor", 64, 33, 0) in refused
    weights = torch.ones(512 * 512, dtype=torch.float32, device=DEV)
    params = (C.c_void_p * 12)(*[weights.data_ptr()] * 12)
    image = torch.full((512 * 1024,), SENTINEL, dtype=torch.float32, device=DEV)
    x = torch.ones(64 * 40, dtype=torch.float32, device=DEV)
    out = torch.full((64 + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    stream = native.current_stream()
    calls = [(ops._KINDS[k], md, D, Di, 64) for k, md, D, Di in refused] + [(4, 128, 3, 0, 64), (-1, 128, 3, 0, 64)]
    calls += [(ops._KINDS[k], md, 3, 1, m) for k in MC.KINDS for md in (64, 256) if MC.served(k, md, 3, 1) for m in (0, -1)]
    for kind, md, D, Di, rows in calls:
        if rows > 0:
            assert lib.pime_mlp_pack(kind, D, Di, md, params, native.ptr(image), stream) == ERR_ARG, (kind, md, D, Di)
            assert native.last_error()
        assert lib.pime_mlp_forward(kind, native.ptr(x), rows, D, Di, md, native.ptr(image), native.ptr(out), stream) == ERR_ARG, \
            (kind, md, D, Di, rows)
        assert native.last_error()
    torch.cuda.synchronize()
    assert bool((image == SENTINEL).all()) and bool((out == SENTINEL).all())


# ---- the trajectory scan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", [(1, 1), (9, 63), (10, 64), (11, 65), (19, 257), (21, 64), (3, 65537)])
@pytest.mark.parametrize("use_gae", [True, False])
def test_gae_scan_at_the_launch_and_chunk_edges(T, N, use_gae):
    """T around the scan's chunk of 10 steps (a ragged chunk alone, a full one, a ragged one after one and after two full ones), N around
    the 64-thread block and beyond 65536, where the launcher takes 256-thread blocks; lambda at both ends; masks drawn per element
    (about a fifth zeros, the last row zero); outputs allocated NaN-filled.  Same float32 operations in the same order: bitwise."""
    import oracle
    from pime_amd import ops
    rng = np.random.RandomState(T * 100003 + N)
    rew = (rng.standard_normal((T, N)) * 3 - 2).astype(np.float32)
    val = rng.standard_normal((T, N)).astype(np.float32)
    mask = np.where(rng.uniform(size=(T, N)) < 0.2, 0.0, 0.99).astype(np.float32)
    mask[-1] = 0
    dev = [_dev(a) for a in (rew, mask, val)]
    for lam in (0.0, 0.97, 1.0):
        r_sum = torch.full((T, N), float("nan"), dtype=torch.float32, device=DEV)
        adv = torch.full((T, N), float("nan"), dtype=torch.float32, device=DEV)
        ops.gae_scan(*dev, lam, use_gae, out_r_sum=r_sum, out_adv=adv)
        w_r, w_a = oracle.gae(rew, mask, val, lam, use_gae)
        np.testing.assert_array_equal(r_sum.cpu().numpy(), w_r)
        np.testing.assert_array_equal(adv.cpu().numpy(), w_a)
