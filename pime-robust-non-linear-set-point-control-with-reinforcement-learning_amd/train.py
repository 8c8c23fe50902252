"""Command-line driver with the reference's flags (/root/reference/train.py:23-78) plus the vectorisation ones.

    python -m pime_amd.train --algo ResidualIntegratorModularPPO --fix_K \\
        --env PH1DChangingParamUniformGoalIntegrator-SqaureDistance-v35 --net_dim 128 \\
        --num_envs 16384 --target_step 819200 --batch_size 65536 --repeat_times 8

With --num_envs 1 (default) it builds the one-instance gym-style env exactly as the reference's train.py does
(gym.make + env.seed + np.random.seed + PreprocessEnv); with --num_envs N > 1 it builds the vectorised env and, when
launched under torchrun, shards N lanes per rank with one RCCL gradient all-reduce per optimizer step.

Reference quirks kept by default: --gamma and --learning_rate are parsed but NOT forwarded
(effective 0.99 / 1e-4); water-tank envs are made with reward_type=args.reward_type and r=args.goal.
`--no_reference_quirks` forwards gamma / learning_rate."""
import argparse
import os
import time
import warnings

import numpy as np
import torch

from . import dist as pdist
from . import gym_compat as gym
from . import gym_control
from .elegantrl.env import PreprocessEnv
from .elegantrl.run import Arguments, train_and_evaluate
from .elegantrl.utils import configure_logger
from .utils import IF_ONPOLICY, MODELS


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--algo", default="PPO", type=str)
    p.add_argument("--env", default=gym_control.WT_INTEGRATOR, type=str)
    p.add_argument("--reward_type", default="distance", type=str, choices=["distance", "sparse"])
    p.add_argument("--fix_K", action="store_true")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--target_return", default=1e6, type=float)
    p.add_argument("--target_step", default=2 ** 3, type=int)
    p.add_argument("--reward_scale", default=1., type=float)
    p.add_argument("--break_step", default=2 ** 20, type=int)
    p.add_argument("--learning_start", default=0, type=int)
    p.add_argument("--gamma", default=0.995, type=float)
    p.add_argument("--batch_size", default=2 ** 6, type=int)
    p.add_argument("--learning_rate", default=3e-4, type=float)
    p.add_argument("--buffer_size", default=2 ** 20, type=int)
    p.add_argument("--net_dim", default=2 ** 4, type=int)
    p.add_argument("--verbose", default=0, type=int)
    p.add_argument("--tensorboard_log", default="tensorboard", type=str)
    p.add_argument("--env_zero_noise", action="store_true")
    p.add_argument("--eval_times1", default=2 ** 3, type=int)
    p.add_argument("--eval_times2", default=2 ** 4, type=int)
    p.add_argument("--eval_gap", default=5, type=int)
    p.add_argument("--robust_test", action="store_true")
    p.add_argument("--goal", default=4.0, type=float)
    p.add_argument("--repeat_times", default=2 ** 4, type=int)
    p.add_argument("--lambda_gae_adv", default=0.97, type=float)
    p.add_argument("--lambda_entropy", default=0.02, type=float)
    p.add_argument("--ratio_clip", default=0.2, type=float)
    p.add_argument("--test_render_times", default=10000, type=int)
    p.add_argument("--load", default="None", type=str)
    p.add_argument("--frozen_modular_integrator", action="store_true")
    p.add_argument("--frozen_transfer", action="store_true")
    # --- this build's additions ---
    p.add_argument("--num_envs", default=1, type=int, help="env lanes per GPU (1 = the reference's single instance)")
    p.add_argument("--resample_every", default=1, type=int, help="redraw ensemble params every n episodes (0 = never)")
    p.add_argument("--device", default="cuda", type=str)
    p.add_argument("--state_dtype", default="mixed", choices=["mixed", "f64"])
    p.add_argument("--draws", default="philox", choices=["philox", "mt19937"],
                   help="vectorised envs: in-kernel Philox or per-env MT19937 streams replayed seed-for-seed")
    p.add_argument("--no_reference_quirks", action="store_true")
    p.add_argument("--log_root", default=None, type=str)
    p.add_argument("--identify", default=None, type=str, metavar="RECORDS.npz",
                   help="recorded runs (action [E, T], output [E, T + 1, C], pH: optionally state0 [E]; optionally mode, skip): score a "
                        "plant grid over the env's ensemble ranges against them and write identified.npz into the run directory")
    p.add_argument("--identify_points", default=9, type=int, help="--identify: grid points per plant parameter")
    p.add_argument("--tune_prior", default=0, type=int, metavar="N",
                   help="sweep N geometric factors in [0.25, 4] per non-zero component of the env's prior gain K over the plants of "
                        "--robust_test in one launch and write tuned_prior.npz into the run directory")
    p.add_argument("--tune_prior_points", default=0, type=int,
                   help="--tune_prior: instead of the --robust_test plants, a grid of this many points per plant parameter over the "
                        "env's ensemble ranges")
    p.add_argument("--mpc_baseline", default=0, type=int, metavar="H",
                   help="after training: the receding-horizon benchmark controller with horizon H on the plants and protocol of "
                        "--robust_test in one launch; writes mpc_baseline.npz (and the policy's ITAE regret against it when "
                        "--robust_test ran) into the run directory (0 = off)")
    p.add_argument("--margins", action="store_true",
                   help="after training: sweep dead time, loop gain and sensor noise of the closed loop (trained agent AND prior alone) "
                        "on the plants of --robust_test, one launch each; writes margins.npz into the run directory")
    p.add_argument("--margins_points", default=0, type=int,
                   help="--margins: instead of the --robust_test plants, a grid of this many points per plant parameter over the "
                        "env's ensemble ranges")
    p.add_argument("--checkpoints", default=0, type=int, metavar="M",
                   help="keep the last M evaluated actors (and the nominal-best one) in memory for --select_policy (0 = off)")
    p.add_argument("--select_policy", action="store_true",
                   help="after training: every kept actor of --checkpoints on the plants of --robust_test in ONE launch; writes "
                        "policy_sweep.npz and actor_robust.pth (the actor with the best worst-plant ITAE) into the run directory; "
                        "actor.pth stays the nominal best")
    p.add_argument("--select_points", default=0, type=int,
                   help="--select_policy: instead of the --robust_test plants, a grid of this many points per plant parameter over the "
                        "env's ensemble ranges")
    p.add_argument("--disturbances", action="store_true",
                   help="after training: load steps at the plant input and steps of the plant's parameters (trained agent AND prior "
                        "alone) on the plants of --robust_test, one launch each; writes disturbances.npz into the run directory")
    p.add_argument("--disturbance_onset", default=-1, type=int, metavar="K",
                   help="--disturbances: the step within every set-point segment at which the disturbance starts (default: half a segment)")
    p.add_argument("--actuator", action="store_true",
                   help="after training: saturation, slew-rate, dead-band, DAC- and ADC-quantum limits of the closed loop (trained agent AND "
                        "prior alone) on the plants of --robust_test, one launch each, with the reference rig's row; writes "
                        "actuator_sweep.npz into the run directory")
    p.add_argument("--actuator_points", default=4, type=int, metavar="Q",
                   help="--actuator: values per axis (limits, rate, dead-band, actuator quantum, sensor quantum), one axis at a time")
    p.add_argument("--bode", action="store_true",
                   help="after training: the loop's frequency response (trained agent AND prior alone) on the plants of --robust_test, one "
                        "launch each -- sinusoids at the set-point and in front of the actuator, lock-in rows, gain and phase margin, peak "
                        "sensitivity, bandwidth; writes frequency_response.npz into the run directory")
    p.add_argument("--bode_points", default=12, type=int, metavar="F",
                   help="--bode: frequencies, spread logarithmically over the whole numbers of cycles the window holds")
    p.add_argument("--bode_amplitude", default=0.05, type=float, metavar="A",
                   help="--bode: amplitude of the excitation (set-point units on set-point rows, normalised action units on load rows)")
    p.add_argument("--mpc_model", default=None, type=str, metavar="FILE.npz",
                   help="--mpc_baseline (tank only): control every plant on FILE's `best` plant (an identified.npz of --identify)")
    p.add_argument("--prior_K", default=None, type=str, metavar="FILE.npz",
                   help="train with FILE's best_gain (a tuned_prior.npz of --tune_prior) as the env's prior gain K")
    return p


def make_env(args, dp=None):
    wt = "NonLinearWaterTank" in args.env
    overrides = {}
    if wt:
        overrides.update(reward_type=args.reward_type, r=args.goal)   # train.py:98-101
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    if args.num_envs > 1:
        overrides.pop("r", None)
        offset = dp.lane_offset(args.num_envs) if dp is not None else 0
        env = gym_control.make_vec(args.env, args.num_envs, device=args.device, state_mode=args.state_dtype,
                                   seed=args.seed, env_offset=offset, draws=args.draws,
                                   resample_every=args.resample_every, **overrides)
        env.env_name = args.env
        env.target_return = args.target_return
        return env
    env = gym.make(args.env, device=args.device, **overrides)
    env.seed(args.seed)
    np.random.seed(args.seed)
    env.target_return = args.target_return
    return env


def prepare_train(args, env):
    algo = args.algo.lower()
    kargs = Arguments(if_on_policy=IF_ONPOLICY[algo])
    kargs.repeat_times = args.repeat_times if IF_ONPOLICY[algo] else 1
    kargs.gpu_id = 0
    kargs.if_remove = False
    kargs.random_seed = args.seed
    kargs.env = PreprocessEnv(env=env)
    kargs.env_eval = PreprocessEnv(env=env)   # the SAME env object, as in the reference (train.py:227-228)
    for k in ("reward_scale", "net_dim", "batch_size", "break_step", "learning_start", "eval_times1", "eval_times2",
              "eval_gap", "fix_K", "frozen_modular_integrator", "frozen_transfer", "test_render_times", "target_step",
              "load"):
        setattr(kargs, k, getattr(args, k))
    kargs.checkpoints = int(getattr(args, "checkpoints", 0))
    if IF_ONPOLICY[algo]:
        kargs.max_memo = args.target_step
    kargs.agent = MODELS[algo](device=args.device)
    if "ppo" in algo:
        kargs.agent.lambda_entropy = args.lambda_entropy
        kargs.agent.ratio_clip = args.ratio_clip
        kargs.agent.lambda_gae_adv = args.lambda_gae_adv
    if args.no_reference_quirks:
        kargs.gamma = args.gamma
        kargs.agent.learning_rate = args.learning_rate
    root = args.log_root or f"log_{args.break_step}"
    tag = f"{args.algo}{'-sparse' if args.reward_type == 'sparse' else ''}-{args.net_dim}{'-fixK' if args.fix_K else ''}"
    zero = "-zero" if args.env_zero_noise else ""
    tb = os.path.join(root, f"{args.tensorboard_log}_{args.env}{zero}/")
    configure_logger(args.verbose, tb, tag, True)
    # data-parallel ranks must agree on the run directory (they all watch its `stop` file): rank 0's clock names it
    stamp = time.strftime("%Y-%m-%d-%H_%M_%S", time.localtime(pdist.broadcast_scalar(time.time())))
    kargs.cwd = os.path.join(root, f"{args.env}{zero}/{tag}/seed{args.seed}/{stamp}")
    return kargs, tb


def robust_test(args, agent, cwd):
    """--robust_test (reference train.py:198-200 -> utils/robust_test.py:4-46, without its plots): the environment's step-response
    protocol under the final deterministic policy on the reference's plant set, one env lane per plant -- the tank's three robust
    plants at max_step 500, the pH plant grid of utils/test.py:1225-1236 -- reduced to the per-segment control indices of
    protocols.step_response_metrics (one launch where the fused evaluation kernel serves the agent).  Writes
    <cwd>/robust_metrics.npz: metrics [n_plants, n_segments, 8] in the row order `metric_names`, plants, setpoints, band, tail."""
    from . import protocols
    if "Stacking" in args.env:
        print("robust test skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
    policy = None
    if protocols._fused_policy(env, None, agent) is None:   # e.g. a width the fused kernel has no instantiation for
        act = getattr(agent, "eval_policy", None) or agent.act

        def policy(obs):
            with torch.no_grad():
                return act(obs)
    m = protocols.step_response_metrics(env, agent=agent, policy=policy, setpoints=setpoints, steps=steps, plants=plants, band=band,
                                        tail=tail)
    env.close()
    metrics = np.stack([m[name] for name in protocols.METRIC_NAMES], axis=-1).transpose(1, 0, 2)   # [plant, segment, row]
    path = os.path.join(cwd, "robust_metrics.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, metrics=metrics, metric_names=np.asarray(protocols.METRIC_NAMES), plants=plants,
             setpoints=np.asarray(setpoints, dtype=np.float64), band=band, tail=tail, steps=steps)
    print(f"robust test: {len(plants)} plants x {len(setpoints)} set-points -> {path}")
    response_band(args, agent, cwd, policy, setpoints, steps, overrides)
    return path


def identify(args, cwd):
    """--identify RECORDS.npz: the recorded runs of the file replayed over a grid of --identify_points values per plant parameter,
    spanning the env's registered ensemble ranges, in one launch (protocols.identify_plants).  Writes <cwd>/identified.npz -- the
    axes, cost / rmse / count / max_error over the grid, the best plant, and the plausible ensemble box at twice the best rmse --
    and prints the last two.  Training does not read the result: the ranges are passed on by the user as before."""
    from collections import OrderedDict
    from . import protocols
    if "Stacking" in args.env:
        print("identification skipped: the plant is the Integrator env's; identify there")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    z = np.load(args.identify, allow_pickle=False)
    records = {k: np.asarray(z[k], dtype=np.float64) for k in ("action", "output", "state0") if k in z.files}
    mode = str(z["mode"]) if "mode" in z.files else "simulate"
    skip = int(z["skip"]) if "skip" in z.files else 0
    n = int(args.identify_points)
    env = gym_control.make_vec(args.env, n ** (2 if is_ph else 3), device=args.device, state_mode=args.state_dtype, seed=args.seed)
    ranges = (("qww_V", env.qww_Vrange), ("qc_V", env.qc_Vrange)) if is_ph else \
        (("a1", env.a1_range), ("a2", env.a2_range), ("Kp", env.Kp_range))
    axes = OrderedDict((k, np.linspace(lo, hi, n)) for k, (lo, hi) in ranges)
    res = protocols.identify_plants(env, records, axes, mode=mode, skip=skip)
    env.close()
    box = protocols.ensemble_ranges(res, 2.0)
    path = os.path.join(cwd, "identified.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, axis_names=np.asarray(list(axes)), **{f"axis_{k}": v for k, v in axes.items()}, cost=res["cost"], rmse=res["rmse"],
             count=res["count"], max_error=res["max_error"], best_index=res["best_index"],
             best=np.asarray(list(res["best"].values())), ensemble_low=np.asarray([lo for lo, _ in box.values()]),
             ensemble_high=np.asarray([hi for _, hi in box.values()]), mode=mode, skip=skip)
    print(f"identified plant: {dict(res['best'])}  rmse {float(np.nanmin(res['rmse'])):.4g}")
    print(f"plausible ensemble (rmse <= 2 x best): {dict(box)} -> {path}")
    return path


def tune_prior(args, cwd):
    """--tune_prior N: the prior controller alone under every gain of the box K[j] x N geometric factors in [0.25, 4] (per non-zero
    component of the env's built-in K) on every plant of --robust_test's plant set (or, with --tune_prior_points P, of a P-per-
    parameter grid over the env's ensemble ranges), the step-response protocol of --robust_test, in one launch
    (protocols.tune_prior: worst-plant ITAE).  Writes <cwd>/tuned_prior.npz -- gains, cost, worst_plant, settled_all, summary in the
    kernels' sign (priorK = -K), and best_gain / builtin_K in the ENV's sign (what --prior_K reads) -- and prints the best gain
    and the cost of the built-in K.  Training does not read the result unless it is passed back with --prior_K."""
    from . import protocols
    if "Stacking" in args.env:
        print("prior tuning skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    n = int(args.tune_prior_points)
    if n > 0:
        probe = gym_control.make_vec(args.env, 1, device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
        ranges = (probe.qww_Vrange, probe.qc_Vrange) if is_ph else (probe.a1_range, probe.a2_range, probe.Kp_range)
        probe.close()
        mesh = np.meshgrid(*[np.linspace(lo, hi, n) for lo, hi in ranges], indexing="ij")
        plants = np.stack([m.reshape(-1) for m in mesh], axis=1)
    env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
    K = np.asarray(env.K, dtype=np.float64).reshape(-1)
    factors = np.geomspace(0.25, 4.0, int(args.tune_prior))
    gains = np.concatenate([protocols.gain_box(-K, list(factors)), -K[None]])   # the last row: the built-in gain itself
    res = protocols.tune_prior(env, gains, plants=plants, setpoints=setpoints, steps=steps, band=band, tail=tail)
    env.close()
    path = os.path.join(cwd, "tuned_prior.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, gains_priorK=res["gains"], cost=res["cost"], worst_plant=res["worst_plant"], settled_all=res["settled_all"],
             summary=res["summary"], best_index=res["best_index"], best_priorK=res["best_gain"], best_gain=-res["best_gain"],
             builtin_K=K, builtin_cost=res["cost"][-1], factors=factors, plants=plants,
             setpoints=np.asarray(setpoints, dtype=np.float64), steps=steps, band=band, tail=tail, cost_name="itae", robust="worst")
    print(f"tuned prior: {len(gains)} gains x {len(plants)} plants -> {path}")
    print(f"best prior gain K = {(-res['best_gain']).tolist()}  worst-plant ITAE {res['cost'][res['best_index']]:.6g}  "
          f"(built-in K = {K.tolist()}: {res['cost'][-1]:.6g})")
    return path


def mpc_baseline(args, cwd, robust_path=None):
    """--mpc_baseline H: the non-linear receding-horizon controller (protocols.mpc_baseline: horizon H, 2 passes, rho 0) on the plant
    set and protocol of --robust_test, every plant on its own model -- or, with --mpc_model FILE.npz (tank), on FILE's `best` plant
    -- in one launch.  Writes <cwd>/mpc_baseline.npz: metrics [n_plants, n_segments, 8] in the row order `metric_names` (the layout
    of robust_metrics.npz), plants, setpoints, horizon, passes, rho, band, tail, steps, and, when robust_metrics.npz was written in
    the same run, itae_regret / itae_ratio [n_plants, n_segments] of the policy against it."""
    from . import protocols
    if "Stacking" in args.env:
        print("mpc baseline skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    horizon, passes, rho = int(args.mpc_baseline), 2, 0.0
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    model = None
    if args.mpc_model:
        if is_ph:
            raise ValueError("--mpc_model: the pH env's state is not measured; a model plant is served for the tank only")
        model = np.asarray(np.load(args.mpc_model, allow_pickle=False)["best"], dtype=np.float64).reshape(3)
    env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
    m = protocols.mpc_baseline(env, plants=plants, setpoints=setpoints, steps=steps, horizon=horizon, passes=passes, rho=rho, model=model,
                               band=band, tail=tail)
    env.close()
    metrics = np.stack([m[name] for name in protocols.METRIC_NAMES], axis=-1).transpose(1, 0, 2)   # [plant, segment, row]
    extra = {}
    if robust_path is not None:
        pol = np.load(robust_path, allow_pickle=False)["metrics"]
        j = protocols.METRIC_NAMES.index("itae")
        diff, ratio = protocols.regret({"itae": pol[:, :, j]}, {"itae": metrics[:, :, j]})
        extra = dict(itae_regret=diff, itae_ratio=ratio)
        print(f"policy ITAE / MPC ITAE per plant (mean over segments): {np.nanmean(ratio, axis=1).round(3).tolist()}")
    if model is not None:
        extra["model"] = model
    path = os.path.join(cwd, "mpc_baseline.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, metrics=metrics, metric_names=np.asarray(protocols.METRIC_NAMES), plants=plants,
             setpoints=np.asarray(setpoints, dtype=np.float64), horizon=horizon, passes=passes, rho=rho, band=band, tail=tail, steps=steps,
             **extra)
    print(f"mpc baseline: horizon {horizon}, {len(plants)} plants x {len(setpoints)} set-points -> {path}")
    return path


MARGIN_DELAYS = tuple(range(9))
MARGIN_GAINS = (0.25, 0.35, 0.5, 0.7, 1.4, 2.0, 2.8, 4.0)
MARGIN_SIGMAS = (0.01, 0.02, 0.05, 0.1)


def margins(args, agent, cwd):
    """--margins: dead time (0 .. 8 sample periods), loop gain (0.25 .. 4) and sensor noise (sigma up to 0.1) swept one axis at a time
    around the nominal loop, on every plant of --robust_test's plant set (or, with --margins_points P, of a P-per-parameter grid over
    the env's ensemble ranges), the step-response protocol of --robust_test, one launch for the trained agent and one for the prior
    controller alone (protocols.loop_sweep / loop_margins: every plant settles and the worst-plant ITAE stays within twice its
    nominal value).  Writes <cwd>/margins.npz -- perturb, plants, and per controller (prefix agent_ / prior_) summary, acceptable,
    cost, the four margins, sigma_slope and the per-plant margins -- and prints both delay margins side by side."""
    from . import protocols
    if "Stacking" in args.env:
        print("margins skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    n = int(args.margins_points)
    if n > 0:
        probe = gym_control.make_vec(args.env, 1, device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
        ranges = (probe.qww_Vrange, probe.qc_Vrange) if is_ph else (probe.a1_range, probe.a2_range, probe.Kp_range)
        probe.close()
        mesh = np.meshgrid(*[np.linspace(lo, hi, n) for lo, hi in ranges], indexing="ij")
        plants = np.stack([m.reshape(-1) for m in mesh], axis=1)
    grid = np.concatenate([protocols.perturbation_grid(delays=MARGIN_DELAYS), protocols.perturbation_grid(gains=MARGIN_GAINS),
                           protocols.perturbation_grid(sigmas=MARGIN_SIGMAS)])
    out, found = {}, {}
    for who, ag in (("agent", agent), ("prior", None)):
        env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
        fused = protocols._fused_policy(env, None, ag)
        if fused is None or not hasattr(env, "margin_supported") or not env.margin_supported(fused[0]):
            env.close()
            print(f"margins skipped for the {who}: the loop-perturbation sweep does not serve this env / actor (margin_supported)")
            continue
        res = protocols.loop_sweep(env, grid, agent=ag, plants=plants, setpoints=setpoints, steps=steps, band=band, tail=tail,
                                   seed=args.seed, want_pairs=True)
        env.close()
        m = protocols.loop_margins(res)
        found[who] = m
        out[f"{who}_summary"] = res["summary"]
        for k, v in m.items():
            out[f"{who}_{k}"] = np.asarray(v)
    if not found:
        return None
    path = os.path.join(cwd, "margins.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, perturb=grid, plants=plants, setpoints=np.asarray(setpoints, dtype=np.float64), steps=steps, band=band, tail=tail,
             cost_name="itae", factor=2.0, metric_names=np.asarray(protocols.METRIC_NAMES), **out)
    side = "  ".join(f"{who} {found[who]['delay_margin']:g}" for who in ("agent", "prior") if who in found)
    print(f"margins: {len(grid)} loop perturbations x {len(plants)} plants -> {path}")
    print(f"delay margin (sample periods, every plant settles and worst-plant ITAE <= 2 x nominal): {side}")
    return path


def select_policy(args, evaluator, cwd):
    """--select_policy: every actor the evaluator kept (--checkpoints M: the last M evaluated ones and the nominal-best one) under the
    step-response protocol of --robust_test on every plant of its plant set (or, with --select_points P, of a P-per-parameter grid
    over the env's ensemble ranges), in ONE launch (protocols.policy_sweep), and the choice by worst-plant ITAE next to the choice a
    plant-mean ranking makes (protocols.select_policy).  Writes <cwd>/policy_sweep.npz -- summary, plants, the cost table (mean_cost,
    worst_cost, worst_plant, settled, fit, order), best_index, nominal_index and the training step and evaluation return of each
    snapshot -- and <cwd>/actor_robust.pth, the chosen actor's state_dict; actor.pth is not touched.  Prints both choices."""
    from . import protocols
    if "Stacking" in args.env:
        print("policy selection skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    policies, snaps = evaluator.snapshot_policies() if evaluator is not None else (None, [])
    if policies is None:
        print("policy selection skipped: no snapshots the fused evaluation serves (--checkpoints M with M > 0, actor widths 64 / 128)")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    n = int(args.select_points)
    if n > 0:
        probe = gym_control.make_vec(args.env, 1, device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
        ranges = (probe.qww_Vrange, probe.qc_Vrange) if is_ph else (probe.a1_range, probe.a2_range, probe.Kp_range)
        probe.close()
        mesh = np.meshgrid(*[np.linspace(lo, hi, n) for lo, hi in ranges], indexing="ij")
        plants = np.stack([m.reshape(-1) for m in mesh], axis=1)
    env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
    if not hasattr(env, "policy_supported") or not env.policy_supported(policies):
        env.close()
        print("policy selection skipped: the policy sweep does not serve this env / actor (policy_supported)")
        return None
    res = protocols.policy_sweep(env, policies, plants=plants, setpoints=setpoints, steps=steps, band=band, tail=tail)
    env.close()
    sel = protocols.select_policy(res, cost="itae", robust="worst")
    best, nominal = sel["best_index"], sel["nominal_index"]
    os.makedirs(cwd, exist_ok=True)
    path = os.path.join(cwd, "policy_sweep.npz")
    np.savez(path, summary=res["summary"], plants=plants, setpoints=np.asarray(setpoints, dtype=np.float64), steps=steps, band=band,
             tail=tail, cost_name="itae", metric_names=np.asarray(protocols.METRIC_NAMES), best_index=best, nominal_index=nominal,
             snapshot_steps=np.asarray([s["step"] for s in snaps], dtype=np.int64),
             snapshot_returns=np.asarray([s["r_avg"] for s in snaps], dtype=np.float64),
             **{k: np.asarray(sel[k]) for k in ("cost", "mean_cost", "worst_cost", "worst_plant", "settled", "fit", "order")})
    torch.save(snaps[best]["state_dict"], os.path.join(cwd, "actor_robust.pth"))
    print(f"policy sweep: {len(snaps)} snapshots x {len(plants)} plants -> {path}")
    for who, j in (("robust  (worst-plant ITAE)", best), ("nominal (plant-mean ITAE) ", nominal)):
        print(f"  {who}: snapshot {j} of step {snaps[j]['step']}, worst-plant ITAE {sel['worst_cost'][j]:.6g}, mean ITAE "
              f"{sel['mean_cost'][j]:.6g}, {int(sel['settled'][j])} of {len(plants)} plants settled")
    return path


DISTURBANCE_LOADS = (-0.2, -0.1, 0.1, 0.2)
DISTURBANCE_MULTIPLIERS = (0.7, 0.85, 1.2, 1.5)


def disturbances(args, agent, cwd):
    """--disturbances: from step --disturbance_onset of every set-point segment to its end, a load on the controller's output (+-0.1,
    +-0.2 of the action range) or a step of one plant parameter (x 0.7 .. 1.5), one axis at a time around the nominal row, on every
    plant of --robust_test's plant set under the step-response protocol of --robust_test; one launch for the trained agent and one for
    the prior controller alone (protocols.disturbance_rejection / rejection_summary).  Writes <cwd>/disturbances.npz -- rows, plants
    and per controller (prefix agent_ / prior_) summary and the rejection summary -- and prints one line per row for each."""
    from . import protocols
    if "Stacking" in args.env:
        print("disturbances skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    onset = int(args.disturbance_onset) if int(getattr(args, "disturbance_onset", -1)) >= 0 else steps // 2
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    m = DISTURBANCE_MULTIPLIERS
    grid = protocols.disturbance_grid(onset, loads=DISTURBANCE_LOADS, m0=m, m1=m, m2=() if is_ph else m)
    out, found = {}, {}
    for who, ag in (("agent", agent), ("prior", None)):
        env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
        fused = protocols._fused_policy(env, None, ag)
        if fused is None or not hasattr(env, "disturbance_supported") or not env.disturbance_supported(fused[0]):
            env.close()
            print(f"disturbances skipped for the {who}: the disturbance sweep does not serve this env / actor (disturbance_supported)")
            continue
        res = protocols.disturbance_rejection(env, grid, agent=ag, plants=plants, setpoints=setpoints, steps=steps, band=band, tail=tail,
                                              want_pairs=True)
        env.close()
        found[who] = protocols.rejection_summary(res)
        out[f"{who}_summary"] = res["summary"]
        for k, v in found[who].items():
            out[f"{who}_{k}"] = np.asarray(v)
    if not found:
        return None
    path = os.path.join(cwd, "disturbances.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, rows=grid, plants=plants, setpoints=np.asarray(setpoints, dtype=np.float64), steps=steps, band=band, tail=tail,
             onset=onset, metric_names=np.asarray(protocols.METRIC_NAMES + protocols.DISTURB_ROW_NAMES), **out)
    print(f"disturbances: {len(grid)} rows x {len(plants)} plants, onset at step {onset} of {steps} -> {path}")
    for who, r in found.items():
        for p, row in enumerate(grid):
            print(f"{who} load {row[2]:+g} m ({row[3]:g}, {row[4]:g}, {row[5]:g}): worst peak {r['worst_peak'][p]:.4g}, recovery "
                  f"{r['worst_recovery'][p]:g} steps, IAE {r['worst_iae'][p]:.4g}, recovered {r['recovered'][p]:.2f}, |e0| {r['worst_e0'][p]:.3g}")
    return path


def actuator_rows(points, p_max_action=10.0):
    """The rows of --actuator: the all-off row, then per axis `points` values, one axis at a time (every other stage off), each halving
    or doubling from a mild one -- clamps [-c, c] from 1 down, rates from 1 per step down, dead-bands and actuator quanta from 1 / 256
    up, sensor quanta from 10 / 1024 up -- and the reference rig's row (protocols.rig_row) last.  float64 [2 + 5 * points, 6]."""
    from . import protocols
    q = max(int(points), 1)
    halves = [0.5 ** j for j in range(q)]
    fine = [2.0 ** j / 256 for j in range(q)]
    rows = [protocols.actuator_grid(limits=[(-c, c) for c in halves]), protocols.actuator_grid(rates=halves)[1:],
            protocols.actuator_grid(deadbands=fine)[1:], protocols.actuator_grid(qu=fine)[1:],
            protocols.actuator_grid(qy=[2.0 ** j * 10 / 1024 for j in range(q)])[1:], protocols.rig_row(p_max_action)[None]]
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def actuator(args, agent, cwd):
    """--actuator: the step-response protocol of --robust_test under a real actuator and sensor -- `actuator_rows(--actuator_points)`,
    one axis at a time around the ideal row, and the reference rig's row -- on every plant of --robust_test's plant set; one launch for
    the trained agent and one for the prior controller alone (protocols.actuator_sweep / actuator_summary).  Writes
    <cwd>/actuator_sweep.npz -- rows, plants and per controller (prefix agent_ / prior_) summary and the actuator summary -- and prints
    one line per row for each."""
    from . import protocols
    if "Stacking" in args.env:
        print("actuator sweep skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    grid = actuator_rows(getattr(args, "actuator_points", 4))
    out, found = {}, {}
    for who, ag in (("agent", agent), ("prior", None)):
        env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
        fused = protocols._fused_policy(env, None, ag)
        if fused is None or not hasattr(env, "actuator_supported") or not env.actuator_supported(fused[0]):
            env.close()
            print(f"actuator sweep skipped for the {who}: the actuator sweep does not serve this env / actor (actuator_supported)")
            continue
        res = protocols.actuator_sweep(env, grid, agent=ag, plants=plants, setpoints=setpoints, steps=steps, band=band, tail=tail,
                                       want_pairs=True)
        env.close()
        found[who] = protocols.actuator_summary(res)
        out[f"{who}_summary"] = res["summary"]
        for k, v in found[who].items():
            out[f"{who}_{k}"] = np.asarray(v)
    if not found:
        return None
    path = os.path.join(cwd, "actuator_sweep.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, rows=grid, plants=plants, setpoints=np.asarray(setpoints, dtype=np.float64), steps=steps, band=band, tail=tail,
             metric_names=np.asarray(protocols.METRIC_NAMES + protocols.ACT_ROW_NAMES), **out)
    print(f"actuator sweep: {len(grid)} rows x {len(plants)} plants -> {path}")
    for who, r in found.items():
        for p, row in enumerate(grid):
            print(f"{who} clamp [{row[0]:g}, {row[1]:g}] rate {row[2]:g} dead-band {row[3]:g} qu {row[4]:.4g} qy {row[5]:.4g}: worst ITAE x "
                  f"{r['itae_ratio'][p]:.3g}, limit cycle {r['limit_cycle'][p]:.2f}, reversals {r['reversals'][p]:g}")
        print(f"{who} tolerated without a limit cycle: " + ", ".join(f"{k[:-10]} {r[k]:.4g}" for k in sorted(r) if k.endswith("_tolerated")))
    return path


def bode(args, agent, cwd):
    """--bode: under the step-response protocol of --robust_test, on every plant of its plant set, a sinusoid of --bode_amplitude at
    --bode_points frequencies -- whole numbers of cycles in the second half of every set-point segment, the first half letting the loop
    reach its periodic state -- once at the set-point (the complementary sensitivity T) and once in front of the actuator (the loop
    transfer function L and the sensitivity S); one launch for the trained agent and one for the prior controller alone
    (protocols.frequency_sweep / frequency_response / stability_margins).  Writes <cwd>/frequency_response.npz -- rows, omega, plants
    and per controller (prefix agent_ / prior_) T, L, S, the fundamental's variance share and the margins per segment and plant -- and
    prints the worst plant's margins of both side by side."""
    from . import protocols
    if "Stacking" in args.env:
        print("bode skipped: the step-response protocol is defined on the Integrator observation, not on Stacking frames")
        return None
    is_ph = "NonLinearWaterTank" not in args.env
    setpoints = protocols.PH_SETPOINTS if is_ph else protocols.WT_SETPOINTS
    steps, band, tail = (50 if is_ph else 500), 0.05, 10
    onset = steps // 2
    window = steps - onset
    overrides = {} if is_ph else {"reward_type": args.reward_type}
    if args.env_zero_noise:
        overrides["noise_scale"] = 0.
    plants = np.asarray(protocols.PH_PARAM_GRID if is_ph else protocols.WT_ROBUST_PLANTS, dtype=np.float64)
    top = max((window - 1) // 2, 1)                        # below the Nyquist rate, where nothing is excited
    cycles = np.unique(np.rint(np.geomspace(1, top, max(int(getattr(args, "bode_points", 12)), 1))))
    amplitude = float(getattr(args, "bode_amplitude", 0.05))
    m = np.concatenate([cycles, cycles])
    point = np.repeat([protocols.FREQ_POINTS["setpoint"], protocols.FREQ_POINTS["load"]], len(cycles))
    rows, wave = protocols.excitation_grid(m, amplitude, point, steps, onset)
    out, found = {}, {}
    for who, ag in (("agent", agent), ("prior", None)):
        env = gym_control.make_vec(args.env, len(plants), device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
        fused = protocols._fused_policy(env, None, ag)
        if fused is None or not hasattr(env, "frequency_supported") or not env.frequency_supported(fused[0]):
            env.close()
            print(f"bode skipped for the {who}: the frequency-response sweep does not serve this env / actor (frequency_supported)")
            continue
        res = protocols.frequency_sweep(env, rows, wave, agent=ag, plants=plants, setpoints=setpoints, steps=steps, band=band, tail=tail)
        env.close()
        fr = protocols.frequency_response(res)
        found[who] = protocols.stability_margins(fr)
        omega = fr["omega"]
        out[f"{who}_pairs"] = res["pairs"]
        for k in ("T", "L", "S", "share"):
            out[f"{who}_{k}"] = fr[k]
        for k, v in found[who].items():
            out[f"{who}_{k}"] = v
    if not found:
        return None
    path = os.path.join(cwd, "frequency_response.npz")
    os.makedirs(cwd, exist_ok=True)
    np.savez(path, rows=rows, cycles=m, omega=omega, plants=plants, setpoints=np.asarray(setpoints, dtype=np.float64), steps=steps, band=band,
             tail=tail, onset=onset, amplitude=amplitude, metric_names=np.asarray(protocols.METRIC_NAMES + protocols.FREQ_ROW_NAMES), **out)
    print(f"bode: {len(rows)} rows ({len(cycles)} frequencies x set-point, load) x {len(plants)} plants, amplitude {amplitude:g}, "
          f"window {window} of {steps} steps -> {path}")
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (a margin no plant's grid brackets: NaN)
        worst = {who: (np.nanmin(r["gain_margin"]), np.nanmin(r["phase_margin"]), np.nanmax(r["peak_S"]), np.nanmin(r["bandwidth"]))
                 for who, r in found.items()}
    for j, (name, unit) in enumerate((("gain margin", ""), ("phase margin", " deg"), ("peak |S|", ""), ("bandwidth", " rad/sample"))):
        side = ", ".join(f"{who} {worst[who][j]:.4g}{unit}" for who in worst)
        print(f"worst plant {name}: {side}")
    return path


def apply_prior_K(env, path):
    """--prior_K FILE.npz: FILE's best_gain (the env's sign: a = -obs @ K) becomes the env's K -- and that of its clones (the
    evaluation env of an off-policy run) -- before the residual agent reads it."""
    K = np.asarray(np.load(path, allow_pickle=False)["best_gain"], dtype=np.float64).reshape(-1)
    old = np.asarray(env.K, dtype=np.float64).reshape(-1)
    if K.shape != old.shape or not np.isfinite(K).all():
        raise ValueError(f"--prior_K: best_gain {K.tolist()} must be {old.size} finite numbers")
    env.K = K.copy()
    if "P_control_K" in getattr(env, "_ctor", {}):
        env._ctor["P_control_K"] = K.copy()
    print(f"prior gain K = {K.tolist()} from {path} (built-in: {old.tolist()})")


BAND_LANES, BAND_BINS, BAND_QUANTILES = 1024, 128, (0.05, 0.25, 0.5, 0.75, 0.95)


def response_band(args, agent, cwd, policy, setpoints, steps, overrides):
    """The other half of --robust_test: the same protocol under the same policy on BAND_LANES lanes whose plants the reset draws
    from the env's registered ensemble ranges, reduced per step across the lanes (protocols.step_response_band: one group, one
    launch where the fused kernel serves the agent).  Writes <cwd>/response_band.npz: mean / std / min / max [4, T] in the row
    order `signals`, count, hist [T, BAND_BINS] of the controlled output with its `edges`, `quantiles` [T, 5] at
    `quantile_levels`, setpoints, steps."""
    from . import protocols
    is_ph = "NonLinearWaterTank" not in args.env
    env = gym_control.make_vec(args.env, BAND_LANES, device=args.device, state_mode=args.state_dtype, seed=args.seed, **overrides)
    b = protocols.step_response_band(env, agent=agent, policy=policy, setpoints=setpoints, steps=steps,
                                     hist=(BAND_BINS, 0.0, 14.0 if is_ph else 10.0))
    env.close()
    path = os.path.join(cwd, "response_band.npz")
    rows = {k: np.stack([b[k][name][:, 0] for name in protocols.BAND_SIGNALS]) for k in ("mean", "std", "min", "max")}
    np.savez(path, signals=np.asarray(protocols.BAND_SIGNALS), count=b["count"], hist=b["hist"][:, 0], edges=b["edges"],
             quantile_levels=np.asarray(BAND_QUANTILES), quantiles=protocols.band_quantiles(b["hist"][:, 0], b["edges"], BAND_QUANTILES),
             setpoints=np.asarray(setpoints, dtype=np.float64), steps=steps, **rows)
    print(f"response band: {BAND_LANES} plants x {len(setpoints)} set-points -> {path}")
    return path


def main(argv=None):
    args = build_parser().parse_args(argv)
    assert args.test_render_times % args.target_step == 0 or args.num_envs > 1, "Must be an integer multiple"
    dp = pdist.init_from_env(device=args.device) if args.num_envs > 1 else None
    if dp is not None and args.device.startswith("cuda"):
        args.device = f"cuda:{dp.local_rank}"
        torch.cuda.set_device(dp.local_rank)
    print(f"Agent: {args.algo}, Env: {args.env}, Seed: {args.seed}, lanes/GPU: {args.num_envs}")
    env = make_env(args, dp)
    if args.prior_K:
        apply_prior_K(env, args.prior_K)
    kargs, _ = prepare_train(args, env)
    kargs.agent.dp = dp
    algo = args.algo.lower()
    K = getattr(env, "K", None)
    kargs.residual_kwargs = {"init_K": np.asarray(K).reshape(-1, 1)} if ("residual" in algo and K is not None) else {}
    kargs.Modular_kwargs = {"integrator_dim": env.n_integrator} if ("modular" in algo and hasattr(env, "n_integrator")) else {}
    kargs.if_residual = hasattr(kargs.agent, "init_actor_zero")   # the reference sets True and crashes for TD3
    agent, _ = train_and_evaluate(kargs)
    if dp is None or dp.rank == 0:   # the replicas are identical: rank 0 alone writes the run directory
        save_dir = os.path.join(kargs.cwd, "final_model")
        os.makedirs(save_dir, exist_ok=True)
        agent.save_load_model(save_dir, if_save=True)
        with open(os.path.join(kargs.cwd, "args.txt"), "w") as f:
            f.write(str(args))
        print(f"Finish Training and Saved in {kargs.cwd}")
        robust_path = None
        if args.robust_test:
            robust_path = robust_test(args, agent, kargs.cwd)
        if args.identify:
            identify(args, kargs.cwd)
        if args.tune_prior > 0:
            tune_prior(args, kargs.cwd)
        if args.mpc_baseline > 0:
            mpc_baseline(args, kargs.cwd, robust_path)
        if args.margins:
            margins(args, agent, kargs.cwd)
        if args.disturbances:
            disturbances(args, agent, kargs.cwd)
        if args.actuator:
            actuator(args, agent, kargs.cwd)
        if args.bode:
            bode(args, agent, kargs.cwd)
        if args.select_policy:
            select_policy(args, getattr(kargs, "evaluator", None), kargs.cwd)
    return agent


if __name__ == "__main__":
    main()
