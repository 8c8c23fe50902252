"""Every instantiation of the env step / reset / observe kernels (csrc/env_kernels.hip) on the device against the float64 oracle: the case
table, scenario and checker of tests/env_cases.py (vetted on the CPU by tests/test_env_cases_cpu.py).  Every test prints "SHARE env" lines:
the largest used share of each bar, for the record of a GPU run."""
import numpy as np
import pytest
import torch

import env_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_TORCH = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8}


class TorchBuf:
    """env_cases.HostBuf on the device: 0xFF-filled, GUARD words behind the rows."""

    def __init__(self, shape, dtype):
        self.shape, self.size = tuple(shape), int(np.prod(shape))
        self.full = torch.empty(self.size + EC.GUARD, dtype=_TORCH[np.dtype(dtype)], device=DEV)
        self.full.view(torch.uint8).fill_(0xFF)
        self.rows = self.full[:self.size].view(self.shape)

    def host(self):
        return self.full.cpu().numpy()


def poisoned_draws(inj):
    """vec_env.CallbackDraws on `inj`'s rows whose reset rows are NaN for every lane that was not asked for: a lane that consumes a row it
    has no business with shows it.  `asked` lists the lanes of every call."""
    from pime_amd.vec_env import CallbackDraws

    class PoisonedDraws(CallbackDraws):
        def reset_draws(self, env, lanes):
            lanes = [int(i) for i in lanes]
            self.asked.append(lanes)
            out = np.full((env.num_envs, env.draw_width), np.nan)
            out[lanes] = super().reset_draws(env, lanes)[lanes]
            return out

    src = PoisonedDraws(inj.episode_fn, inj.noise_fn)
    src.asked = []
    return src


class GpuDevice:
    def __init__(self, c, sc, draws=None):
        over = {} if draws is None else dict(draws=draws)
        self.env = EC.make_vec_env(c, sc, DEV, **over)
        self.c, self.N, self.D, self.half, self.has_head = c, self.env.num_envs, self.env.obs_dim, c.entry == "mixed16_h", c.num_stack > 0
        np.testing.assert_array_equal(-self.env.K, EC.prior_gain(c))

    def new_buf(self, shape, kind):
        return TorchBuf(shape, np.uint8 if kind == "done" else (np.float16 if self.half and kind != "observe" else np.float32))

    def reset(self, mask, out):
        (self.env.reset_h if self.half else self.env.reset)(mask=mask, out=out.rows)

    def step(self, action, residual, auto_reset, out_obs, out_reward, out_done):
        a = torch.as_tensor(action).to(DEV)
        assert a.dtype == (torch.float64 if self.c.action == "a64" else torch.float32)
        kw = dict(auto_reset=auto_reset, out_obs=out_obs.rows, out_reward=out_reward.rows, out_done=out_done.rows)
        if residual is not None:
            obs_in = torch.as_tensor(np.ascontiguousarray(residual[0])).to(DEV)
            (self.env.step_residual_h if self.half else self.env.step_residual)(a, obs_in, priorK=residual[1], **kw)
        else:
            (self.env.step_h if self.half else self.env.step)(a, **kw)

    def observe(self, out):
        self.env.observe(out=out.rows)

    def field(self, name):
        return self.env.get_field(name)

    def close(self):
        self.env.close()


def _run(c, sc, table, record=None, injected=False):
    inj = EC.InjectedDraws(c, sc) if injected else None
    src = poisoned_draws(inj) if injected else None
    dev = GpuDevice(c, sc, draws=src)
    try:
        share = EC.run_scenario(dev, c, sc, table, record=record, draws=inj)
    finally:
        dev.close()
    print("\n" + EC.share_line(c, sc, share) + (" injected" if injected else ""))
    return src


# ------------------------------------------------------------------------------------------------ 1: the 55 instantiations
@pytest.mark.parametrize("c", EC.cases(), ids=EC.case_id)
def test_instantiation_against_the_oracle(c, ph_table_oracle):
    _run(c, EC.scenario(), ph_table_oracle)


# ------------------------------------------------------------------------------------------------ 2: rewards, bounds, punishments
VARIANTS = [("ph", 0, dict(reward_type=r)) for r in ("distance", "square_distance", "sparse")] + [
    ("ph", 0, dict(integral_bound=False)),
    ("ph", 0, dict(action_punishment=0.1, action_change_punishment=0.2, integral_punish=0.05)),
] + [("wt", 0, dict(reward_type=r)) for r in ("distance", "square_distance", "sparse")] + [("wt", 0, dict(integral_punish=0.05))]


@pytest.mark.parametrize("entry", ["mixed", "mixed16_h"])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v[0] + "-" + "-".join(f"{k}={x}" for k, x in v[2].items()))
def test_reward_and_bound_variants(variant, entry, ph_table_oracle):
    env, ns, kw = variant
    _run(EC.Case(env, ns, entry, "residual" if "punish" in "".join(kw) else "a32"), EC.scenario(N=65, **kw), ph_table_oracle)


# ------------------------------------------------------------------------------------------------ 3: injected draws, out of lock-step
@pytest.mark.parametrize("c", [EC.Case("ph", 0, "mixed", "a32"), EC.Case("wt", 4, "mixed", "a64"), EC.Case("wt", 0, "mixed16_h", "a32")],
                         ids=EC.case_id)
def test_injected_draws_on_lanes_out_of_lock_step(c, ph_table_oracle):
    """Host-made reset rows (and the tank's process noise): only the lanes that end on a launch consume theirs -- every other row of
    reset_draws is NaN here -- and the others continue bit for bit as the oracle says."""
    sc = EC.scenario(N=65, n_auto=8)
    record = []
    src = _run(c, sc, ph_table_oracle, record=record, injected=True)
    mask = EC.lane_mask(sc).astype(bool)
    steps = [r for r in record if r["kind"] == "step" and r["auto"] and r["done"].any()]
    ends = [np.nonzero(r["done"])[0].tolist() for r in steps]
    assert ends == [np.nonzero(~mask)[0].tolist(), np.nonzero(mask)[0].tolist()]          # B on step 2, A on step 7
    assert src.asked == [list(range(65)), np.nonzero(mask)[0].tolist()] + ends             # the two resets, then the lanes that ended


# ------------------------------------------------------------------------------------------------ 4: the 256-lane block
@pytest.mark.parametrize("c", [EC.Case("ph", 0, "mixed", "residual"), EC.Case("wt", 0, "mixed16_h", "a32"), EC.Case("wt", 10, "mixed", "a64")],
                         ids=EC.case_id)
def test_256_lane_blocks(c, ph_table_oracle):
    """N = 65 793 > 65 536: 257 blocks of 256 lanes and one lane (lane_grid), the Stacking writer at blockDim 256 x 30 words."""
    _run(c, EC.scenario(N=65793, n_auto=8), ph_table_oracle)


# ------------------------------------------------------------------------------------------------ 5: lanes see neither each other nor the grid
@pytest.mark.parametrize("c", [EC.Case("ph", 0, "mixed16_h", "residual"), EC.Case("wt", 0, "f64", "a64"), EC.Case("wt", 1, "mixed", "a32"),
                               EC.Case("wt", 4, "mixed16", "residual"), EC.Case("wt", 10, "mixed16_h", "a32")], ids=EC.case_id)
def test_a_lane_is_the_same_in_any_handle(c, ph_table_oracle):
    """Lanes 0, 100 and 192 of the N = 193 run, bit for bit, in an N = 1 handle and (with their 62 neighbours) in an N = 63 handle at the
    matching env_offset."""
    def recording(sc):
        dev, rec = GpuDevice(c, sc), []
        try:
            EC.run_scenario(dev, c, sc, ph_table_oracle, record=rec)
        finally:
            dev.close()
        return rec

    full = recording(EC.scenario())
    for g0, n in ((0, 1), (100, 1), (192, 1), (0, 63), (65, 63), (130, 63)):
        part = recording(EC.scenario(window=(g0, n)))
        assert len(part) == len(full)
        for a, b in zip(full, part):
            for k in ("obs", "reward"):   # (the rows every lane holds after the launch; the rewards of a step)
                if k in a:
                    assert np.array_equal(EC.bits(a[k][g0:g0 + n]), EC.bits(b[k])), \
                        f"launch {a['launch']} ({a['kind']}): {k} of lanes {g0}..{g0 + n - 1} depends on the handle"


# ------------------------------------------------------------------------------------------------ the defect this sweep found
@pytest.mark.parametrize("env", ["ph", "wt"])
def test_mixed16_float_row_carries_the_stored_integrator(env, ph_table_oracle):
    """PIME_STATE_MIXED16 through the float entry points: the step's float32 row used to carry the integrated error before its rounding to
    the stored binary16 word, so the policy saw an I the next step did not continue from and pime_env_observe did not repeat the row."""
    c = EC.Case(env, 0, "mixed16", "a32")
    dev = GpuDevice(c, EC.scenario(N=65))
    obs = dev.env.reset().clone()
    for t in range(3):
        a = torch.full((65,), 0.3 - 0.2 * t, device=DEV)
        obs = dev.env.step(a, auto_reset=False)[0].clone()
        I = dev.field("I")
        assert np.abs(I).max() > 0 and np.array_equal(I, I.astype(np.float16).astype(np.float64))
        np.testing.assert_array_equal(obs[:, -1].cpu().numpy(), I.astype(np.float32))
        assert torch.equal(dev.env.observe(out=torch.empty_like(obs)), obs)
    dev.close()
