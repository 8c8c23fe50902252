"""Test helper: the fused PPO optimizer step as a CHAIN -- K steps, each reading the packed images, Adam moments, step counter and
row cursor the previous one left -- recorded step by step and held to a float64 replay.  Shared by tests/test_ppo_chain_cpu.py
(synthetic recordings, numpy alone) and tests/test_gpu_ppo_chain.py (recordings of the kernels), so that the checker the GPU
test relies on is itself tested: clean recordings pass with room to spare, every fault of FAULTS trips the assertion named for it.

The argument is transitive.  tests/test_gpu_ppo_sweep.py pins ONE pime_ppo_minibatch_grad on freshly packed weights to the
float64 oracle.  Here, step k's gradient must equal, bit for bit, a fresh object's single gradient at the chain's own pre-step
weights and the same index row (deterministic routes); step k's parameters and moments must equal the float64 Adam replay of the
kernel's OWN gradient within replay_bounds (so an element whose gradient is rounding noise, which Adam turns into a
full step of either sign, is held as tightly as any other); counters, critic scale, loss sums and packed images are held per step.
Only step 0 -- ppo_cases' own vetted minibatch -- is compared with the oracle's gradient, so no kink margin has to be
re-established along the trajectory.

A recording (what the GPU test's recorder and `synthesise` produce):
  {"layout": [(net, key, shape)] in flat order, "n_act": flat elements of the actor, "deterministic": bool,
   "image_map": int [n, 2] (forward / transposed image position of every flat element, negative: in no image) or None,
   "steps": [{"k": 0-based Adam step, "row": table row, "before" / "after": state, "grad", "scale", "images", "repack",
              "fresh_grad"}]}
  state  = {"param", "exp_avg", "exp_avg_sq" float32 [n], "step_count" float, "arrival" int (the optimizer's arrival word),
            "loss_sums" float32 [6], "cursor" int}
  images = [(forward, transposed) of the actor, of the critic] after the step; "repack": the same from a re-pack of the after-state
           parameters on a twin object.

The bounds.  Adam: `replay_bounds` below -- td3_cases.replay_bounds, derived there from the float32 operation count, with one
correction; the PPO kernels (adam_kernel of
csrc/ppo_train.hip and the slab reduction of csrc/ppo_fused.hip) form the update with the same operations as td3_cases.adam_f32.
loss_sums[0, 1, 2, 4]: the bars of tests/test_gpu_ppo_fused.py and the sweep on each step's INCREMENT.  loss_sums[3] accumulates
the step's scale: one float32 addition, so the increment is within 2^-23 of the accumulated value of the scale (half an ulp of
the sum, and the subtraction that forms the increment is exact or rounds once more).  critic_scale: rtol 3e-6, the sweep's bar."""
import collections

import numpy as np

import ppo_cases as PC
import ppo_oracle as P
import td3_cases as TD

K = 4
B = 293
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, clip=PC.RATIO_CLIP, lam=PC.LAMBDA_ENTROPY)
SCALE_RTOL = 3e-6
SUM_BARS = {0: (2e-4, 1e-3), 1: (2e-4, 1e-3), 2: (2e-4, 0.0), 4: (3e-4, 0.0)}   # rtol, atol / sqrt(B)

# fault -> the assertion of check_chain it must trip
FAULTS = collections.OrderedDict([
    ("counter_plus_one_at_step_2", "counters"),
    ("counter_not_advanced", "counters"),
    ("moments_of_step_1_not_written", "adam"),
    ("exp_avg_sq_from_previous_gradient", "adam"),
    ("stale_images_gradient", "gradient_fresh"),        # step 2's gradient taken at step 1's pre-step weights
    ("cursor_stuck", "counters"),                       # step 2 uses row 1 again
    ("cursor_reset", "counters"),                       # step 3 uses row 0
    ("row_not_updated", "adam"),                        # one row of one hidden weight keeps its value
    ("row_takes_neighbours_update", "adam"),            # image-map slip
    ("critic_scaled_with_previous_rows_scale", "gradient_fresh"),
    ("a_std_log_skipped", "frozen_or_absent"),
    ("adam_applied_twice", "adam"),
    ("loss_sums_overwritten", "loss_sums"),
    ("bias_corrections_swapped", "adam"),
    ("eps_inside_sqrt", "adam"),
    ("forward_image_stale", "images"),
])
# the faults that only the bit-equality of the two gradients shows: not demanded of the split pipeline (float atomics)
BIT_EQUALITY_FAULTS = ("stale_images_gradient",)
# cursor faults move the row a step reads, so the two gradients differ as well
ALSO_TRIPS = {"cursor_stuck": "gradient_fresh", "cursor_reset": "gradient_fresh"}


class ChainError(AssertionError):
    def __init__(self, failed):
        self.failed = collections.OrderedDict(failed)   # assertion name -> first message
        super().__init__("; ".join(f"[{k}] {v}" for k, v in self.failed.items()))


# ------------------------------------------------------------------------------------------------------------------ inputs
def chain_specs():
    """ppo_cases.per_route_shapes() and four more, all at B = 293 (property_cases' batch: a second workgroup of the LDS-resident
    kernels, a ragged 16-tile): the bench's nets (the pair kernel with alternating actor / critic order), the modular actor at
    widths 64 and 256, the stacked observation at width 256."""
    out = [s._replace(B=B) for s in PC.per_route_shapes()]
    for s in (PC.spec("modular", 3, 1, 128, B), PC.spec("modular", 4, 1, 64, B), PC.spec("modular", 4, 1, 256, B),
              PC.spec("plain", 30, 0, 256, B)):
        if s not in out:
            out.append(s)
    return out


def b3_chain_specs(forced16=False):
    """Under PIME_GRAD_BF16X3=1 (child processes; forced16: with PIME_MLP16=1): ppo_cases.b3_per_route_shapes at B = 293 -- one spec
    per (route, widths, actor kind, which nets run a B3 kernel and re-split their bf16 planes after every step)."""
    return [s._replace(B=B) for s in PC.b3_per_route_shapes(forced16)]


def deterministic(s):
    """False on the split pipeline, whose gradient sums are float atomics (tests/test_gpu_mlp16.py)."""
    return s.route[0] != "split"


def index_table(case, rows=K):
    """[rows, B]: row 0 is the case's own vetted index list; the others are drawn with the generator's rule (position p names a
    table row of combination p mod 10) from a seed derived from the spec, and positions 7 and 17 repeat the row before."""
    s = case.spec
    rng = np.random.RandomState([s.aw, s.cw, s.D, s.Di, s.B, int(s.kind == "ppo"), 4177])
    out = [np.array(case.idx)]
    for _ in range(1, rows):
        row = PC._pick(rng, np.arange(s.B)).astype(np.int64)
        for pos in (7, 17):
            if pos < s.B:
                row[pos] = out[-1][pos]
        out.append(row)
    return np.stack(out)


def layout(spec):
    """[(net, key)] in the order of the flat parameter tensor (torch's named_parameters: a module's own parameters before its
    submodules'): a_std_log, the actor's layers (weight, bias), the critic's."""
    names = P.MODULAR_LAYERS if spec.kind == "modular" else P.PLAIN_LAYERS
    out = [("act", "a_std_log")] + [("act", f"{n}.{p}") for n in names for p in ("weight", "bias")]
    return out + [("cri", f"{n}.{p}") for n in P.CRITIC_LAYERS for p in ("weight", "bias")]


def shaped_layout(spec, nets):
    act, cri = nets
    return [(net, key, tuple((act if net == "act" else cri)[key].shape)) for net, key in layout(spec)]


def flatten(lay, act, cri, dtype=np.float32):
    return np.concatenate([np.asarray((act if net == "act" else cri)[key], dtype=dtype).reshape(-1) for net, key, _ in lay])


def unflatten(lay, flat):
    act, cri, o = {}, {}, 0
    for net, key, shape in lay:
        n = int(np.prod(shape))
        (act if net == "act" else cri)[key] = flat[o:o + n].reshape(shape)
        o += n
    assert o == flat.size
    return act, cri


def slices(lay):
    out, o = {}, 0
    for net, key, shape in lay:
        n = int(np.prod(shape))
        out[f"{net}.{key}"] = slice(o, o + n)
        o += n
    return out


def n_actor(lay):
    return sum(int(np.prod(shape)) for net, _, shape in lay if net == "act")


def batch_rows(case, row):
    return tuple(t[row] for t in case.table)


def oracle_at(case, lay, param, row, hyper, dt=np.float64):
    """ppo_oracle.gradients at the flat parameters `param` on the table rows `row`."""
    act, cri = unflatten(lay, np.asarray(param))
    s = case.spec
    return P.gradients(act, cri, PC.okind(s.kind), s.Di, batch_rows(case, row), hyper["clip"], hyper["lam"], dt)


# ----------------------------------------------------------------------------------------------------------------- checker
def dp_replay_bounds(rep, exp_avg_before, grad, lr, betas=(0.9, 0.999)):
    """replay_bounds for the data-parallel step form (pime_adam_step_dp), where the gradient the replay takes -- the kernel's
    unscaled critic gradient times the float64 scale recomputed from dp_moments -- is not the float32 number the device steps on:
    the device rounds sqrt(var) to float32, the scale to float32 and the product g * scale to float32, three roundings of 2^-24,
    so its gradient is within e = 2^-22 relative of the replay's.  What that adds, with b1, b2 the betas:
      exp_avg     m' = m + (g - m)(1 - b1):  (1 - b1) e |g|.
      exp_avg_sq  v' = v b2 + g g (1 - b2):  2 e (1 - b2) g^2.
      param       the update u = step_size m' / (sqrt(v') / sqrt(bc2) + eps).  From m': step_size sqrt(bc2) (1 - b1) e |g| / sqrt(v')
                  with sqrt(v') >= sqrt(1 - b2) |g| and sqrt(bc2) / bc1 <= 1 at every step, at most lr e (1 - b1) / sqrt(1 - b2)
                  = 3.2 e lr.  From v': |u| (dv' / 2 v') <= |u| e with |u| <= 3.2 lr (replay_bounds).  Together 6.4 e lr < 2e-6 lr."""
    b = replay_bounds(rep, exp_avg_before, grad, lr)
    e, g = 2.0 ** -22, np.abs(np.asarray(grad, dtype=np.float64))
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    return {"param": b["param"] + 2e-6 * lr, "exp_avg": b["exp_avg"] + (1 - b1) * e * g,
            "exp_avg_sq": b["exp_avg_sq"] + 2 * e * (1 - b2) * g * g}


def replay_bounds(rep, exp_avg_before, grad, lr):
    """td3_cases.replay_bounds with the bound of exp_avg_sq corrected.  v' = v b2 + g g (1 - b2) is four float32 roundings -- the
    products v b2, g g and (g g)(1 - b2), and the sum -- of 2^-24 relative each, on positive terms: to first order at most
    2^-24 (v b2 + 2 g g (1 - b2) + v') <= 3 x 2^-24 v'.  td3_cases' 2^-22 v' is that worst case with a third to spare, and float32
    numpy comes within 0.72 of it on the 200 000 elements of a width-256 case from step 2 on (at step 1, v = 0 and two roundings
    are left).  Every bound here is to hold with HALF of it to spare for a correct float32 implementation (the condition
    tests/test_ppo_chain_cpu.py asserts), as the two others do by their own derivation (the parameter's final subtraction alone
    takes 2^-24 |w'| of 2^-23 |w'|; exp_avg's three roundings are relative to different operands).  So: twice the worst case,
    6 x 2^-24 v' + 1e-37 (subnormals)."""
    b = TD.replay_bounds(rep, exp_avg_before, grad, lr)
    b["exp_avg_sq"] = 6.0 * 2.0 ** -24 * np.abs(rep["exp_avg_sq"]) + 1e-37
    return b


def adam_shares(before, after, grad, step, hyper, bounds=None, sel=None):
    """{"param" | "exp_avg" | "exp_avg_sq": largest |after - float64 replay| / bound} over the elements `sel`."""
    rep = TD.adam_replay(before["param"], before["exp_avg"], before["exp_avg_sq"], grad, step, hyper["lr"], hyper["betas"],
                         hyper["eps"])
    bnd = (bounds or replay_bounds)(rep, before["exp_avg"], grad, hyper["lr"])
    sel = slice(None) if sel is None else sel
    out = {}
    for key in ("param", "exp_avg", "exp_avg_sq"):
        err = np.abs(np.asarray(after[key], dtype=np.float64) - rep[key])
        e, b = err[sel], bnd[key][sel]
        with np.errstate(divide="ignore", invalid="ignore"):   # a gradient that is exactly 0 (a closed unit): bound 0, error 0
            out[key] = float(np.where(e == 0, 0.0, e / b).max()) if e.size else 0.0
    return out


def check_chain(rec, case, table, hyper=HYPER, oracle_step0=True):
    """One named assertion per property (module docstring); every one is evaluated on every step, then ChainError names the ones
    that failed.  Returns the largest used share of every bound.

      gradient_oracle   step 0 only: every gradient tensor within ppo_cases.BAR of case.mid, as in the sweep.
      gradient_fresh    the chain's gradient equals the fresh object's, array_equal.  On the split pipeline (float atomics) the
                        actor's tensors are held to each other at 2 BAR of the tensor's largest entry instead: each of the two is
                        within BAR of the same float64 value (the sweep's bar), so they are within 2 BAR of each other.
      adam              after-state against adam_replay of the before-state and the step's own gradient, within replay_bounds.
      counters          step_count k -> k + 1, the arrival word at 0, the cursor row -> row + 1.
      critic_scale      against 1 / (std(r_sum of the row) + 1e-5) in float64, rtol 3e-6.
      loss_sums         increments against the float64 oracle at the pre-step weights (SUM_BARS), [3] against the step's scale.
      frozen_or_absent  elements that the image map puts in no image (a_std_log) moved, and by Adam's step.
      images            the packed images equal the re-pack of the after-state parameters."""
    lay, steps = rec["layout"], rec["steps"]
    sl, n_act = slices(lay), rec["n_act"]
    failed, used = collections.OrderedDict(), {}

    def fail(name, msg):
        failed.setdefault(name, msg)

    def note(name, share):
        used[name] = max(used.get(name, 0.0), float(share))

    absent = None
    if rec.get("image_map") is not None:
        absent = np.flatnonzero((rec["image_map"] < 0).all(axis=1))
    for st in steps:
        k, row, bf, af, g = st["k"], st["row"], st["before"], st["after"], st["grad"]
        what = f"step {k}"
        assert np.isfinite(g).all() and all(np.isfinite(af[x]).all() for x in ("param", "exp_avg", "exp_avg_sq")), what
        # -- gradients
        if oracle_step0 and k == 0:
            assert case.mid is not None and np.array_equal(table[0], case.idx)
            for name, s_ in sl.items():
                net, key = name.split(".", 1)
                want = case.mid["ga" if net == "act" else "gc"][key].reshape(-1)
                err = np.abs(g[s_] - want).max() / np.abs(want).max()
                note("grad step 0 (bar 3e-4 of the largest entry)", err / PC.BAR)
                if not err <= PC.BAR:
                    fail("gradient_oracle", f"{what}: gradient of {name} {err:.2e} of the largest entry off the oracle")
        fresh = st.get("fresh_grad")
        if fresh is not None:
            for name, s_ in sl.items():
                if rec["deterministic"] or name.startswith("cri."):
                    if not np.array_equal(g[s_], fresh[s_]):
                        fail("gradient_fresh", f"{what}: gradient of {name} differs from a fresh object's at the same weights and row "
                                               f"(largest difference {np.abs(g[s_] - fresh[s_]).max():.2e})")
                else:
                    err = np.abs(g[s_].astype(np.float64) - fresh[s_]).max() / np.abs(fresh[s_]).max()
                    note("grad chain vs fresh, split pipeline (2 x bar)", err / (2 * PC.BAR))
                    if not err <= 2 * PC.BAR:
                        fail("gradient_fresh", f"{what}: gradient of {name} {err:.2e} of the largest entry off a fresh object's")
        # -- Adam
        sh = adam_shares(bf, af, g, k + 1, hyper)
        for key, v in sh.items():
            note(f"adam {key} (replay_bounds)", v)
            if not v <= 1.0:
                fail("adam", f"{what}: {key} is {v:.3g} x replay_bounds off the float64 replay of the step's own gradient")
        if absent is not None and absent.size:
            sh = adam_shares(bf, af, g, k + 1, hyper, sel=absent)
            moved = af["param"][absent] != bf["param"][absent]
            if not (max(sh.values()) <= 1.0 and moved.all()):
                fail("frozen_or_absent", f"{what}: flat elements {absent.tolist()} (in no packed image) do not follow Adam")
        # -- counters
        if not (bf["step_count"] == k and af["step_count"] == k + 1 and af["arrival"] == 0 and bf["cursor"] == row
                and af["cursor"] == row + 1):
            fail("counters", f"{what}: step count {bf['step_count']} -> {af['step_count']} (want {k} -> {k + 1}), arrival word "
                             f"{af['arrival']}, cursor {bf['cursor']} -> {af['cursor']} (want {row} -> {row + 1})")
        # -- scale and loss sums against the float64 oracle at the kernel's pre-step weights
        o = oracle_at(case, lay, bf["param"], table[row], hyper)
        err = abs(st["scale"] / o["scale"] - 1)
        note("critic_scale (rtol 3e-6)", err / SCALE_RTOL)
        if not err <= SCALE_RTOL:
            fail("critic_scale", f"{what}: critic_scale {st['scale']!r} against {o['scale']!r}")
        d = af["loss_sums"].astype(np.float64) - bf["loss_sums"].astype(np.float64)
        nb = len(table[row])
        want = {0: o["sums"][0], 1: o["sums"][1], 2: o["sums"][2], 4: o["sums"][2] * o["scale"]}
        for i, (rtol, at) in SUM_BARS.items():
            share = abs(d[i] - want[i]) / (at * nb ** 0.5 + rtol * abs(want[i]))
            note(f"loss_sums[{i}] increment (rtol {rtol:.0e}" + (", atol 1e-3 sqrt(B))" if at else ")"), share)
            if not share <= 1.0:
                fail("loss_sums", f"{what}: loss_sums[{i}] grew by {d[i]!r}, the oracle's sum is {want[i]!r}")
        share = abs(d[3] - float(st["scale"])) / (2.0 ** -23 * abs(float(af["loss_sums"][3])))
        note("loss_sums[3] increment (2^-23 of the sum)", share)
        if not share <= 1.0:
            fail("loss_sums", f"{what}: loss_sums[3] grew by {d[3]!r}, the step's scale is {st['scale']!r}")
        # -- images
        if st.get("images") is not None:
            for (gf, gb), (wf, wb), net in zip(st["images"], st["repack"], ("actor", "critic")):
                if not (np.array_equal(gf, wf) and np.array_equal(gb, wb)):
                    fail("images", f"{what}: the {net}'s packed images differ from a re-pack of the parameters "
                                   f"(forward equal: {np.array_equal(gf, wf)}, transposed equal: {np.array_equal(gb, wb)})")
    if failed:
        raise ChainError(failed)
    return used


def states_equal(a, b, keys=("param", "exp_avg", "exp_avg_sq", "step_count", "arrival", "cursor")):
    """The first key on which two states differ bit for bit, or None."""
    for key in keys:
        if not np.array_equal(np.asarray(a[key]), np.asarray(b[key])):
            return key
    return None


# ------------------------------------------------------------------------------------------------------------- synthesiser
def _adam32(p, m, v, g, step, hyper, g_for_v=None, swap_bc=False, eps_inside=False):
    """td3_cases.adam_f32 with the deviations the faults need (without any it IS adam_f32, which `synthesise` uses then)."""
    f = np.float32
    lr, b1, b2, eps = f(hyper["lr"]), f(hyper["betas"][0]), f(hyper["betas"][1]), f(hyper["eps"])
    c1, c2 = (b2, b1) if swap_bc else (b1, b2)
    step_size = lr / f(1.0 - float(c1) ** step)
    bc2_sqrt = f(np.sqrt(1.0 - float(c2) ** step))
    gv = g if g_for_v is None else g_for_v
    m2 = m + (g - m) * (f(1) - b1)
    v2 = v * b2 + gv * gv * (f(1) - b2)
    den = np.sqrt(v2 / (bc2_sqrt * bc2_sqrt) + eps) if eps_inside else np.sqrt(v2) / bc2_sqrt + eps
    out = {"param": p - step_size * (m2 / den), "exp_avg": m2, "exp_avg_sq": v2}
    assert all(x.dtype == f for x in out.values())
    return out


def _images(lay, param):
    """Synthetic packed images: the net's flat parameters as they are (forward) and reversed (transposed)."""
    n = n_actor(lay)
    return [(param[:n].copy(), param[:n][::-1].copy()), (param[n:].copy(), param[n:][::-1].copy())]


def synthesise(case, table, fault=None, hyper=HYPER):
    """A recording made on the CPU: ppo_oracle.gradients in float32 for the chain's and the fresh gradient, float32 numpy
    (td3_cases.adam_f32) for Adam, float32 accumulators for the loss sums -- what a correct kernel may do, so the shares that
    check_chain returns for it measure how much of every bound float32 itself takes.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    f = np.float32
    lay = shaped_layout(case.spec, case.nets)
    sl, n_act = slices(lay), n_actor(lay)
    p = flatten(lay, *case.nets)
    m, v = np.zeros_like(p), np.zeros_like(p)
    count, cursor, sums = 0, 0, np.zeros(6, dtype=f)
    i_asl = sl["act.a_std_log"]
    hidden = sl["cri.net.2.weight"]
    cw = case.spec.cw

    def two_rows(g):
        """The two rows of the critic's second hidden weight with the largest gradients (a closed ReLU unit's row has none, and
        Adam leaves it where it is)."""
        a, b = np.argsort(np.abs(g[hidden]).reshape(cw, cw).max(axis=1))[-2:]
        return (slice(hidden.start + a * cw, hidden.start + (a + 1) * cw), slice(hidden.start + b * cw, hidden.start + (b + 1) * cw))

    imap = np.zeros((p.size, 2), dtype=np.int64)
    imap[i_asl] = -1
    steps, g_prev, befores = [], None, []

    def gradient(param, row, scale_row=None):
        o = oracle_at(case, lay, param, table[row], hyper, f)
        g = flatten(lay, o["ga"], o["gc"])
        if scale_row is not None:   # the critic's part under another row's scale
            other = P.critic_pass(unflatten(lay, param)[1], *[batch_rows(case, table[scale_row])[i] for i in (0, 4)], dt=f)["scale"]
            g[n_act:] = g[n_act:] / f(o["scale"]) * f(other)
        return g, o

    for k in range(len(table)):
        if fault == "cursor_reset" and k == 3:
            cursor = 0
        before = dict(param=p.copy(), exp_avg=m.copy(), exp_avg_sq=v.copy(), step_count=float(count), arrival=0,
                      loss_sums=sums.copy(), cursor=cursor)
        befores.append(before)
        row = cursor
        g_fresh, o_fresh = gradient(p, k)
        if fault == "stale_images_gradient" and k == 2:
            g, o = gradient(befores[1]["param"], row)
        elif fault == "critic_scaled_with_previous_rows_scale" and k == 2:
            g, o = gradient(p, row, scale_row=row - 1)
        elif row != k:
            g, o = gradient(p, row)
        else:
            g, o = g_fresh.copy(), o_fresh
        step = count + 1 + (fault == "counter_plus_one_at_step_2" and k == 2)
        if fault in (None, "counter_plus_one_at_step_2", "counter_not_advanced", "cursor_stuck", "cursor_reset",
                     "stale_images_gradient", "critic_scaled_with_previous_rows_scale", "loss_sums_overwritten",
                     "forward_image_stale", "a_std_log_skipped", "row_not_updated", "row_takes_neighbours_update",
                     "moments_of_step_1_not_written", "adam_applied_twice"):
            new = TD.adam_f32(p, m, v, g, step, hyper["lr"], hyper["betas"], hyper["eps"])
            same = _adam32(p, m, v, g, step, hyper)
            assert all(np.array_equal(new[x], same[x]) for x in same)
        else:
            new = _adam32(p, m, v, g, step, hyper,
                          g_for_v=g_prev if (fault == "exp_avg_sq_from_previous_gradient" and k >= 1) else None,
                          swap_bc=fault == "bias_corrections_swapped", eps_inside=fault == "eps_inside_sqrt")
        if fault == "adam_applied_twice" and k == 1:
            new = TD.adam_f32(new["param"], new["exp_avg"], new["exp_avg_sq"], g, step, hyper["lr"], hyper["betas"], hyper["eps"])
        p2, m2, v2 = new["param"].copy(), new["exp_avg"], new["exp_avg_sq"]
        if fault == "moments_of_step_1_not_written" and k == 1:
            m2, v2 = m, v
        if fault == "row_not_updated" and k == 1:
            row3, _ = two_rows(g)
            p2[row3] = p[row3]
        if fault == "row_takes_neighbours_update" and k == 1:
            row3, row4 = two_rows(g)
            p2[row3] = p[row3] + (p2[row4] - p[row4])
        if fault == "a_std_log_skipped":
            p2[i_asl] = p[i_asl]
        scale = f(o["scale"])
        inc = np.array([o["sums"][0], o["sums"][1], o["sums"][2], scale, f(o["sums"][2]) * scale, 0], dtype=f)
        sums = inc.copy() if fault == "loss_sums_overwritten" else (sums + inc).astype(f)
        sums[5] = sums[2]
        count = int(step) - (fault == "counter_not_advanced" and k == 1)
        cursor = row + 1 - (fault == "cursor_stuck" and k == 1)
        images = _images(lay, p2)
        if fault == "forward_image_stale" and k == 1:
            images[0] = (_images(lay, p)[0][0], images[0][1])
        g_prev = g
        p, m, v = p2, m2, v2
        after = dict(param=p.copy(), exp_avg=m.copy(), exp_avg_sq=v.copy(), step_count=float(count), arrival=0,
                     loss_sums=sums.copy(), cursor=cursor)
        steps.append(dict(k=k, row=k, before=before, after=after, grad=g, scale=float(scale), images=images,
                          repack=_images(lay, p), fresh_grad=g_fresh))
    return {"layout": lay, "n_act": n_act, "deterministic": deterministic(case.spec), "image_map": imap, "steps": steps}
